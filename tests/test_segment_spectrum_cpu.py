"""The segment-size fixtures of tests/segment_spectrum.py, proven on the CPU before a GPU sees them: for every single-leaf fixture
(size x live docs x norms) and every multi-leaf index the oracle's hit counts and doc sets are those of the plain-numpy set algebra,
the rows of the tie fixture are the expected rows in full, the statistics leaf is the one the fixtures name, and the query set
reaches the shapes it claims to reach (a short row, an empty row, a leaf that gives nothing to a non-empty row, a k-th place cut
through a tie that spans two leaves, k above the whole index's max_doc, a conjunction whose only match is doc 0 of a one-doc
leaf)."""
import numpy as np
import pytest

import segment_spectrum as ss


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _check_sets(oracle, leaves, what):
    """Every query of the set, k = the index's max_doc (no row is cut): totals and doc sets against the numpy reference.
    Returns [(query, reference docs, oracle row)]."""
    osr = oracle.Searcher([leaf.oracle_segment(oracle) for leaf in leaves])
    assert oracle.lib().orc_searcher_stats_leaf(osr._h) == ss.stats_leaf(leaves), what
    k = sum(leaf.max_doc for leaf in leaves)
    rows = ss.oracle_rows(oracle, osr, ss.ALL_QUERIES, k)
    out = []
    for q, (d, s, total) in zip(ss.ALL_QUERIES, rows):
        want = ss.ref_docs(leaves, q)
        assert total == want.size, (what, q, total, want.size)
        assert d.size == want.size and (np.sort(d) == want).all(), (what, q)
        assert np.isfinite(s).all() and (np.diff(s) <= 0).all(), (what, q)
        assert (np.diff(d)[np.diff(s) == 0] > 0).all(), (what, q, "equal scores not in doc order")
        out.append((q, want, (d, s, total)))
    assert len(rows) == len(ss.ALL_QUERIES)
    return osr, out


def test_sizes_are_the_ones_named():
    assert ss.SIZES == [n + d for n in (2, 32, 64, 128, 192, 256, 1024, 8192) for d in (-1, 0, 1)]
    for n in ss.SIZES:
        leaf = ss.Leaf(n)
        dfs = [int(x) for x in leaf.seg.terms["doc_freq"]]
        assert dfs[ss.EVERY] == dfs[ss.CONST] == n and dfs[ss.FIRST] == dfs[ss.LAST] == 1 and dfs[ss.EVEN] == (n + 1) // 2
        assert dfs[ss.ABSENT] == dfs[ss.FILLER] == 0 and (dfs[ss.SOMETIMES] > 0) == (n % 3 != 0) and 1 <= dfs[ss.FIFTH] <= n
        assert leaf.lists[ss.LAST][0][0] == n - 1 and leaf.lists[ss.FIRST][0][0] == 0
        assert np.unique(leaf.norms).size <= 64
        raw = ss.Leaf(n, "raw")
        assert np.unique(raw.norms).size == min(n, 70)   # 65 or more distinct bytes (raw mode) wherever max_doc allows it
        assert (np.unique(raw.norms).size >= 65) == (n >= 65)
        for live in ss.LIVE:
            lv = ss.Leaf(n, live=live)
            assert (lv.live_docs is None) == (live == "none")
            if lv.live_docs is not None:
                bits = np.unpackbits(lv.live_docs.view(np.uint8), bitorder="little")
                assert (bits[:n] == lv.alive).all() and not bits[n:].any() and lv.live_docs.size == (n + 63) // 64
        assert not ss.Leaf(n, live="all").alive.any() and ss.Leaf(n, live="last").alive.sum() == n - 1 == ss.Leaf(n, live="first").alive.sum()
    assert any(n % 3 == 0 for n in ss.SIZES) and any(n % 3 for n in ss.SIZES)


@pytest.mark.parametrize("max_doc", ss.SIZES)
def test_single_leaf_fixtures(oracle, max_doc):
    """Every live variant and norm kind of one size: the oracle's totals and doc sets are the reference's; at every k of the GPU
    module a row holds min(k, total) docs."""
    for norms in ss.NORMS:
        for live in ss.LIVE:
            leaf = ss.Leaf(max_doc, norms, live)
            osr, rows = _check_sets(oracle, [leaf], (max_doc, norms, live))
            if live == "all":
                assert all(want.size == 0 for _, want, _ in rows)
            if norms == "rank":
                for k in ss.KS:
                    for q, (d, s, total), (_, want, _) in zip(ss.ALL_QUERIES, ss.oracle_rows(oracle, osr, ss.ALL_QUERIES, k), rows):
                        assert total == want.size and d.size == min(k, total), (max_doc, live, k, q)


@pytest.mark.parametrize("name", list(ss.INDEXES))
def test_multi_leaf_indexes(oracle, name):
    leaves = ss.INDEXES[name]()
    bases = np.cumsum([0] + [leaf.max_doc for leaf in leaves])
    assert [leaf.doc_base for leaf in leaves] == bases[:-1].tolist()
    _check_sets(oracle, leaves, name)


def test_index_shapes():
    for shuffled in (False, True):
        leaves = ss.many(shuffled)
        sizes = [leaf.max_doc for leaf in leaves]
        assert sorted(sizes) == ss.SIZES and (sizes == ss.SIZES) != shuffled
        assert sum(leaf.live == "all" for leaf in leaves) == 1 and sum(leaf.hollow for leaf in leaves) == 1
        assert {leaf.live for leaf in leaves} == set(ss.LIVE)
        hollow = [leaf for leaf in leaves if leaf.hollow][0]
        assert not hollow.has[ss.QUERIED].any() and hollow.has[ss.FILLER].all()
    assert np.unique(ss.many(True, "raw")[ss.stats_leaf(ss.many(True, "raw"))].norms).size >= 65
    leaves = ss.tail()
    sizes = [leaf.max_doc for leaf in leaves]
    assert len(leaves) == 41 and sizes[17] == 50_000 and all(1 <= n <= 200 for n in sizes[:17] + sizes[18:]) and {1, 200} <= set(sizes)
    assert any(leaf.live == "all" for leaf in leaves)
    leaves = ss.twins()
    sizes = [leaf.max_doc for leaf in leaves]
    assert sizes.count(max(sizes)) == 2 and sizes.index(max(sizes)) == ss.TWINS_STATS_LEAF == ss.stats_leaf(leaves)
    leaves = ss.ties()
    assert len(leaves) == 24 and all(leaf.max_doc == 64 and (leaf.norms == ss.TIES_BYTE).all() for leaf in leaves)
    assert sum(leaf.max_doc for leaf in ss.crumbs()) < min(k for k in ss.KS if k > 10)


def test_twins_take_their_statistics_from_the_first_twin(oracle):
    """The first of the two largest leaves gives the statistics, and the choice shows in the scores: with the second twin's
    statistics FIFTH scores other bits."""
    leaves = ss.twins()
    osr = oracle.Searcher([leaf.oracle_segment(oracle) for leaf in leaves])
    assert oracle.lib().orc_searcher_stats_leaf(osr._h) == ss.TWINS_STATS_LEAF
    d, s, _ = osr.search(oracle.OP_TERM, [ss.FIFTH], 10, tie_mode=oracle.TIE_CANONICAL)
    second = [i for i, leaf in enumerate(leaves) if leaf.max_doc == 1024][1]
    other = oracle.Searcher([leaf.oracle_segment(oracle) for leaf in leaves])
    other.override_statistics(leaves[second].oracle_segment(oracle), sum(leaf.max_doc for leaf in leaves))
    d2, s2, _ = other.search(oracle.OP_TERM, [ss.FIFTH], 10, tie_mode=oracle.TIE_CANONICAL)
    assert (s.view(np.int32) != s2.view(np.int32)).any()


def test_ties_rows_in_full(oracle):
    """1536 docs that score alike: the merged row is the lowest global doc ids, ascending; the band of PLATEAU first, in doc order
    across the leaf boundary, then its freq-1 docs in doc order."""
    leaves = ss.ties()
    osr = oracle.Searcher([leaf.oracle_segment(oracle) for leaf in leaves])
    for k in ss.TIES_KS:
        d, s, total = osr.search(oracle.OP_TERM, [ss.CONST], k, tie_mode=oracle.TIE_CANONICAL)
        assert total == ss.TIES_LEAVES * ss.TIES_DOCS == 1536 and d.tolist() == list(range(k)) and np.unique(s).size == 1
        assert (ss.ref_ties_row(leaves, ss.CONST, k) == d).all()
    for k in ss.PLATEAU_KS:
        d, s, total = osr.search(oracle.OP_TERM, [ss.PLATEAU], k, tie_mode=oracle.TIE_CANONICAL)
        want = ss.ref_ties_row(leaves, ss.PLATEAU, k)
        assert (d == want).all(), (k, d, want)
        band = min(k, ss.PLATEAU_HI - ss.PLATEAU_LO)
        assert d[:band].tolist() == list(range(ss.PLATEAU_LO, ss.PLATEAU_LO + band)) and np.unique(s[:band]).size == 1
        assert k <= band or (s[band] < s[0] and np.unique(s[band:]).size == 1)
    # the conjunction and the disjunction of the two every-doc terms tie as well (CONST + an EVERY of seeded freqs does not)
    for op in (oracle.OP_AND, oracle.OP_OR):
        d, s, total = osr.search(op, [ss.CONST, ss.CONST], 129, tie_mode=oracle.TIE_CANONICAL)
        assert d.tolist() == list(range(129)) and total == 1536


def test_the_query_set_reaches_what_it_claims(oracle):
    # a row with fewer than k hits, a row with none, k above the whole index's max_doc: a three-doc leaf at k = 10
    leaf = ss.Leaf(3)
    osr = oracle.Searcher([leaf.oracle_segment(oracle)])
    rows = ss.oracle_rows(oracle, osr, ss.ALL_QUERIES, 10)
    assert any(0 < d.size < 10 for d, _, _ in rows) and any(total == 0 for _, _, total in rows) and 10 > leaf.max_doc
    for name in ("crumbs", "tail"):
        leaves = ss.INDEXES[name]()
        osr = oracle.Searcher([x.oracle_segment(oracle) for x in leaves])
        rows = ss.oracle_rows(oracle, osr, ss.ALL_QUERIES, 300)
        assert any(0 < d.size < 300 for d, _, _ in rows) and any(total == 0 for _, _, total in rows)
    assert sum(x.max_doc for x in ss.crumbs()) < 300
    # a leaf that contributes nothing to a non-empty row: by having no match (deleted, hollow) and by losing every place
    for name in ("many-shuffled", "tail", "crumbs"):
        leaves = ss.INDEXES[name]()
        osr = oracle.Searcher([x.oracle_segment(oracle) for x in leaves])
        d, s, total = osr.search(oracle.OP_TERM, [ss.EVERY], 300, tie_mode=oracle.TIE_CANONICAL)
        got = set(ss.leaf_of(leaves, d).tolist())
        assert d.size and len(got) < len(leaves)
        dead = [i for i, x in enumerate(leaves) if x.live == "all" or x.hollow]
        assert dead and not got & set(dead)
        if name != "crumbs":
            assert any(i not in got and ss.ref_leaf_docs(x, ss.TERMS[ss.EVERY]).size for i, x in enumerate(leaves))
    # a k-th place cut through a tie that spans two leaves
    leaves = ss.ties()
    osr = oracle.Searcher([x.oracle_segment(oracle) for x in leaves])
    for term, k in ((ss.PLATEAU, 30), (ss.CONST, 100)):
        d, s, _ = osr.search(oracle.OP_TERM, [term], k + 1, tie_mode=oracle.TIE_CANONICAL)
        assert s[k - 1] == s[k]
        wide, ws, _ = osr.search(oracle.OP_TERM, [term], 1536, tie_mode=oracle.TIE_CANONICAL)
        tied = wide[ws == s[k]]
        assert np.unique(ss.leaf_of(leaves, tied)).size >= 2 and tied[0] <= d[k - 1] < d[k] <= tied[-1]
    d, s, _ = osr.search(oracle.OP_TERM, [ss.PLATEAU], 30, tie_mode=oracle.TIE_CANONICAL)
    assert set(ss.leaf_of(leaves, d).tolist()) == {3, 4}
    # an AND whose only match is doc 0 of a one-doc leaf
    q = ss.Query(must=(ss.FIRST, ss.LAST))
    assert q in ss.ANDS
    assert ss.ref_docs([ss.Leaf(1)], q).tolist() == [0] and ss.ref_docs([ss.Leaf(2)], q).size == 0
    leaves = ss.crumbs()
    want = ss.ref_docs(leaves, q)
    ones = [x.doc_base for x in leaves if x.max_doc == 1 and x.alive[0]]
    assert want.tolist() == ones and len(ones) >= 1
    osr = oracle.Searcher([x.oracle_segment(oracle) for x in leaves])
    d, _, total = osr.search(oracle.OP_AND, [ss.FIRST, ss.LAST], 10, tie_mode=oracle.TIE_CANONICAL)
    assert sorted(d.tolist()) == ones and total == len(ones)


@pytest.mark.parametrize("max_doc", ss.POSITION_SIZES)
def test_tiny_positions_segments(oracle, max_doc):
    """The phrase fixtures: both files are written, phrases match where the planted prefix says they must, the absent term matches
    nowhere."""
    postings, norms, doc_count, sum_ttf = ss.positions_postings(max_doc)
    ix = oracle.PositionsIndex(max_doc, postings)
    assert not postings[4] and [d for d, _ in postings[3]] == [max_doc - 1]
    for terms, slop in ss.PHRASES:
        for k in ss.PHRASE_KS:
            d, s, total = ix.phrase_search(terms, k, norms, max_doc, doc_count, sum_ttf, slop=slop)
            assert d.size == min(k, total) and np.isfinite(s).all()
            if 4 in terms:
                assert total == 0
    for terms in ([0, 1], [0, 1, 2], [0, 0]):
        d, _, total = ix.phrase_search(terms, max_doc, norms, max_doc, doc_count, sum_ttf)
        assert {0, max_doc - 1} <= set(d.tolist()) and total >= min(2, max_doc)
    d, _, total = ix.phrase_search([0, 3], 10, norms, max_doc, doc_count, sum_ttf)
    assert d.tolist() == [max_doc - 1] and total == 1
    ix.close()
