"""The fixtures of tests/or_spectrum.py, proven on the CPU before a GPU sees them: every list has the property it is named for (read
back from the built `.doc` bytes with the oracle, BP128 and legacy), and for every query of the four families the oracle's rows are
those of the numpy reference - hit sets by set algebra, scores for the exact families A to C as f32 clause-order sums of the oracle's
per-term scores, bit for bit; family D inside oracle/parity.py's heap-order rule against the same sums."""
import numpy as np
import pytest

import or_spectrum as os_
from or_spectrum import (ABOVE_1K, ABOVE_256, ABOVE_4K, ABSENT, BELOW_1K, BELOW_256, BELOW_4K, BIG_FREQ, BLOCK, CONST, COPY, DF_127, EDGE_1K, EDGE_256,
                         FREQ11_DENSE, FREQ11_SPARSE, FROM_0, FROM_1, FROM_127, FROM_128, MAX_DOC, SPAN, TWIN_A, TWIN_B, WINDOWS, Query)

VARIANTS = [("rank", "none", 1), ("rank", "seeded", 1), ("raw", "none", 0), ("raw", "seeded", 1), ("none", "seeded", 0), ("rank", "none", 0)]
CPU_KS = (1, 10, 129, 300)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _blocks(docs):
    """[(first doc, last doc)] of the list's FullBlocks."""
    return [(int(docs[b * BLOCK]), int(docs[b * BLOCK + BLOCK - 1])) for b in range(docs.size // BLOCK)]


def _edges(max_doc, W):
    return list(range(W, max_doc, W))


def _decoded(oracle, leaf):
    seg = leaf.oracle_segment(oracle)
    return [seg.decode_term(leaf.seg.terms[t]) for t in range(os_.N_TERMS)]


def test_the_leaves_are_the_ones_named():
    assert MAX_DOC == 8 * 1024 + 37 == 32 * 256 + 37 == 2 * 4096 + 37
    assert os_.BIG_MAX_DOC == 129 * 256 + 1            # 129 whole windows of 256 docs, and one more that holds a single doc
    assert 1024 * 129 > 131072 >= 64 * 130             # 1024 queries: two windows per item; 64 queries: one
    items = (65 + 7) // 8 * 8                          # 130 windows in twos, rounded up to a workgroup's eight wavefronts
    assert items == 72 and 2 * (items - 1) >= 130      # the last items start past the last window
    assert [os_.dense_bound(MAX_DOC, W) for W in WINDOWS] == [2058, 515, 129]
    for W in WINDOWS:
        b = os_.dense_bound(MAX_DOC, W)
        assert b * W >= 64 * MAX_DOC > (b - 1) * W
    leaf = os_.Leaf()
    df = [d.size for d, _ in leaf.lists]
    assert (df[BELOW_256], df[ABOVE_256], df[BELOW_1K], df[ABOVE_1K], df[BELOW_4K], df[ABOVE_4K]) == (2057, 2058, 514, 515, 128, 129)
    assert df[DF_127] == 127 and df[ABSENT] == 0 and df[os_.FIRST_OF_WINDOW] == df[os_.LAST_DOC] == 1
    assert leaf.lists[os_.FIRST_OF_WINDOW][0][0] == 1024 and leaf.lists[os_.LAST_DOC][0][0] == MAX_DOC - 1
    assert (leaf.lists[COPY][0] == leaf.lists[FROM_1][0]).all() and (leaf.lists[COPY][1] == leaf.lists[FROM_1][1]).all()
    assert df[TWIN_A] == df[TWIN_B] >= 2058 and (leaf.lists[TWIN_A][0] != leaf.lists[TWIN_B][0]).any()
    assert [df[t] for t in os_.FIVE_DENSE] == sorted((df[t] for t in os_.FIVE_DENSE), reverse=True) and len({df[t] for t in os_.FIVE_DENSE}) == 5
    assert all(df[t] >= 2058 for t in os_.FIVE_DENSE)
    want = {0, MAX_DOC - 1} | {w + d for w in range(1024, MAX_DOC, 1024) for d in (-1, 0, 1)}
    assert set(leaf.lists[EDGE_1K][0].tolist()) == want and len(want) == 26
    want = {0, MAX_DOC - 1} | {w + d for w in range(256, MAX_DOC, 256) if w % 1024 for d in (-1, 0, 1)}
    assert set(leaf.lists[EDGE_256][0].tolist()) == want and len(want) == 74
    for kind, lo, hi in (("rank", 2, 64), ("raw", 65, 256)):
        nb = os_.Leaf(norms=kind).norms
        assert lo <= np.unique(nb).size <= hi and (nb[os_.CONST_LO:os_.CONST_HI] == os_.TIE_BYTE).all()
    assert os_.Leaf(norms="none").norms is None
    big = os_.Leaf(os_.BIG_MAX_DOC)
    assert {33023, 33024} <= set(big.lists[EDGE_256][0].tolist()) and big.lists[EDGE_256][0][-1] == 33024 == os_.BIG_MAX_DOC - 1
    assert all(big.lists[t][0].size < os_.dense_bound(os_.BIG_MAX_DOC, 4096) for t in os_.SPARSE_POOL)
    assert all(leaf.lists[t][0].size < BLOCK for t in os_.SPARSE_POOL)
    for W in WINDOWS:
        lo, hi = os_.PAIRS[W]
        assert big.lists[lo][0].size + 1 == big.lists[hi][0].size == os_.dense_bound(os_.BIG_MAX_DOC, W)
        assert not os_.eligible(big, lo, W) and os_.eligible(big, hi, W)


@pytest.mark.parametrize("version", os_.VERSIONS)
def test_blocks_against_every_window_edge(oracle, version):
    """The `.doc` bytes decode to the input lists, and the FullBlocks of the alignment lists sit against every window edge as named."""
    leaf = os_.Leaf(version=version)
    assert leaf.oracle_segment(oracle).version == version
    dec = _decoded(oracle, leaf)
    for t, (d, f) in enumerate(leaf.lists):
        assert (dec[t][0] == d).all() and (dec[t][1] == f).all(), os_.NAMES[t]
    blocks = {t: _blocks(dec[t][0]) for t in os_.FROM}
    for W in WINDOWS:
        for w1 in _edges(MAX_DOC, W):
            fits = w1 + BLOCK <= MAX_DOC     # behind the last edge, 8192, only the 37 docs of the VInt tails follow
            assert (w1 - BLOCK, w1 - 1) in blocks[FROM_0] and ((w1, w1 + BLOCK - 1) in blocks[FROM_0]) == fits   # ends on w1 - 1 | starts on w1
            assert (w1 - BLOCK + 1, w1) in blocks[FROM_1]                                                      # ends on w1
            assert ((w1 - 1, w1 + BLOCK - 2) in blocks[FROM_127]) == fits                                      # starts on w1 - 1
            assert (w1 - BLOCK, w1 - 1) in blocks[FROM_128] and ((w1, w1 + BLOCK - 1) in blocks[FROM_128]) == fits
        assert sum(w1 + BLOCK <= MAX_DOC for w1 in _edges(MAX_DOC, W)) == len(_edges(MAX_DOC, W)) - 1
    assert [leaf.tail_n(t) for t in os_.FROM] == [37, 36, 38, 37]
    assert [leaf.tail_n(t) for t in os_.TAILS] == [0, 1, 127]
    for t, (src, tail_n) in os_.TAILS.items():
        n = leaf.lists[t][0].size
        assert n >= 2058 and n // BLOCK >= 1 and (leaf.lists[t][0] == leaf.lists[src][0][:n]).all()
    assert [leaf.tail_n(t) for t in (os_.DF_128, os_.DF_129, DF_127)] == [0, 1, 127] and leaf.lists[DF_127][0].size // BLOCK == 0
    first, last = _blocks(dec[SPAN][0])[0]
    assert (first, last) == (200, 200 + 5 * 127) and first < 256 and last >= 768                               # crosses 256, 512 and 768
    assert np.isin(dec[SPAN][0], np.arange(256, 512)).sum() > 0 and all(os_.eligible(leaf, SPAN, W) for W in WINDOWS)


def test_dense_eligibility_and_selection():
    leaf = os_.Leaf()
    always = set(os_.FROM) | set(os_.TAILS) | {SPAN, ABOVE_256, TWIN_A, TWIN_B, COPY, FREQ11_DENSE}
    want = {256: always, 1024: always | {BELOW_256, ABOVE_1K}, 4096: always | {BELOW_256, ABOVE_1K, BELOW_1K, ABOVE_4K, FREQ11_SPARSE, BIG_FREQ, CONST, os_.STRETCH_129}}
    for W in WINDOWS:
        assert {t for t in os_.ALL_TERMS if os_.eligible(leaf, t, W)} == want[W], W
        lo, hi = os_.PAIRS[W]
        assert not os_.eligible(leaf, lo, W) and os_.eligible(leaf, hi, W) and leaf.lists[lo][0].size >= BLOCK
    assert not any(os_.eligible(leaf, t, 256) for t in os_.STRETCHES) and sum(n for _, n in os_.STRETCHES.values()) < os_.dense_bound(MAX_DOC, 256)
    pick = lambda s, W=1024, m=4: os_.dense_choice(leaf, s, W, m)   # noqa: E731
    assert pick((EDGE_1K, DF_127, os_.STRETCH_64)) == [] and pick((EDGE_1K, FROM_1, DF_127)) == [1]
    assert pick((FROM_0, FROM_1, FROM_127, FROM_128)) == [0, 1, 2, 3]
    assert pick((FROM_128, FROM_0, EDGE_1K, FROM_1, os_.TAIL_0, FROM_127)) == [1, 3, 4, 5]      # the fifth longest goes through a run
    assert pick((TWIN_B, TWIN_A, FROM_0, FROM_1, FROM_127, SPAN)) == [0, 2, 3, 4]               # the tie goes to the earlier clause
    assert pick((TWIN_B, TWIN_A, FROM_0, FROM_1, FROM_127, SPAN), m=1) == [2]
    assert pick((ABSENT, FROM_0)) == [0]                                                        # an absent clause takes no position
    n_dense = sorted({len(os_.dense_choice(leaf, q.should, W)) for q in os_.FAMILY_A for W in WINDOWS})
    assert n_dense == [0, 1, 2, 3, 4]
    assert max(sum(os_.eligible(leaf, t, 1024) for t in q.should) for q in os_.FAMILY_A) >= 5
    at15, at16 = [q for q in os_.FAMILY_B if len(q.should) == 17 and q.should.count(FROM_0) == 1]
    assert at15.should.index(FROM_0) == 15 and at16.should.index(FROM_0) == 16
    assert pick(at15.should) == [15] and pick(at16.should) == []                                # the mask is 16 bits wide


def test_stretches_per_window():
    leaf = os_.Leaf()
    for W in WINDOWS:
        for t, (first, n) in os_.STRETCHES.items():
            d = leaf.lists[t][0]
            per_window = np.bincount(d // W, minlength=MAX_DOC // W + 1)
            assert d.size == n and sorted(per_window[per_window > 0].tolist()) == [n] and (np.diff(d) == 1).all(), (W, os_.NAMES[t])
        assert (np.bincount(leaf.lists[FROM_0][0] // W)[:-1] == W).all() and np.bincount(leaf.lists[FROM_0][0] // W)[-1] == 37
    ends = {t: int(leaf.lists[t][0][-1]) for t in os_.STRETCHES}
    assert (ends[os_.STRETCH_64] + 1) % 1024 == 0 and (ends[os_.STRETCH_129] + 1) % 256 == 0
    assert sorted(n for _, n in os_.STRETCHES.values()) == [63, 64, 65, 128, 129]
    at = {}
    for name, fam in (("A", os_.FAMILY_A), ("B", os_.FAMILY_B), ("D", os_.FAMILY_D)):
        for q in fam:
            for i, t in enumerate(q.should):
                if t in os_.STRETCHES and ABSENT not in q.should[:i]:
                    at.setdefault(name, set()).add(i)
    assert {7, 8} <= at["A"] and {8, 15, 16, 63} <= at["B"] and {8, 15, 16, 63} <= at["D"]
    assert os_.OR_PREFETCH == 8


@pytest.mark.parametrize("version", os_.VERSIONS)
def test_ballot_mixing_freqs(oracle, version):
    leaf = os_.Leaf(version=version)
    dec = _decoded(oracle, leaf)
    for t, tail_eleven in ((FREQ11_DENSE, False), (FREQ11_SPARSE, True)):
        f = dec[t][1]
        nb = f.size // BLOCK
        kinds = set()
        for b in range(nb):
            blk = f[b * BLOCK:(b + 1) * BLOCK]
            kinds.add(b % 3)
            if b % 3 == 0:
                assert blk.max() <= 7
            elif b % 3 == 1:
                assert blk.max() == os_.SCORE_TABLE_FREQS
            else:
                assert (blk == 11).sum() == 1 and np.sort(blk)[-2] == 10 and (blk > 11).sum() == 0
        assert kinds == {0, 1, 2}
        tail = f[nb * BLOCK:]
        assert tail.size > 0 and ((tail == 11).sum() == 1 and tail.max() == 11 if tail_eleven else tail.max() <= 10)
    assert all(os_.eligible(leaf, FREQ11_DENSE, W) for W in WINDOWS)
    assert [os_.eligible(leaf, FREQ11_SPARSE, W) for W in WINDOWS] == [False, False, True]
    f = dec[BIG_FREQ][1]
    assert f.size == 200 and f[5] == (1 << 20) + 3 and f[150] == 1 << 21 and 5 < BLOCK <= 150 and (np.delete(f, [5, 150]) <= 10).all()
    others = [t for t in os_.ALL_TERMS if t not in (FREQ11_DENSE, FREQ11_SPARSE, BIG_FREQ) and dec[t][1].size]
    assert all(dec[t][1].max() <= os_.SCORE_TABLE_FREQS for t in others)


@pytest.mark.parametrize("norms", os_.NORMS)
def test_const_ties_across_a_window_edge(oracle, norms):
    leaf = os_.Leaf(norms=norms)
    docs, sc = os_.OrRef(oracle, leaf).clause(CONST)
    assert docs.tolist() == list(range(900, 1201)) and np.unique(sc.view(np.int32)).size == 1 and sc[0] > 0
    osr = oracle.Searcher([leaf.oracle_segment(oracle)])
    for k in os_.KS:
        d, s, total = os_.oracle_rows(oracle, osr, [Query(should=(CONST, ABSENT))], k)[0]
        assert total == 301 and d.tolist() == list(range(900, 900 + k))     # every k cuts the tie; from 125 docs on, past the edge 1024
    assert 900 + 64 < 1024 < 900 + 128 and 300 < 301


def test_the_seeded_mask_deletes_what_it_claims():
    for max_doc in (MAX_DOC,):
        leaf = os_.Leaf(max_doc, live="seeded")
        assert not leaf.alive[list(os_.DELETED_AT_EDGES)].any() and not leaf.alive[leaf.only_dense_doc]
        assert all((e + 1) % 256 == 0 or e % 256 == 0 for e in os_.DELETED_AT_EDGES)
        for w1 in (256, 1024, 4096):
            assert w1 - 1 in os_.DELETED_AT_EDGES and w1 in os_.DELETED_AT_EDGES
        holders = [t for t in os_.ALL_TERMS if leaf.has[t, leaf.only_dense_doc]]
        assert FROM_0 in holders and all(os_.eligible(leaf, t, os_.DEFAULT_W) for t in holders)
        assert 0.8 < leaf.alive.mean() < 0.9
        bits = np.unpackbits(leaf.live_docs.view(np.uint8), bitorder="little")
        assert (bits[:max_doc] == leaf.alive).all() and not bits[max_doc:].any() and leaf.live_docs.size == (max_doc + 63) // 64
        assert leaf.alive[[1022, 1025]].any()
    assert os_.Leaf().live_docs is None and os_.Leaf().alive.all()


def test_the_families_are_the_ones_named():
    leaf = os_.Leaf()
    for name, fam in os_.EXACT.items():
        assert not any(os_.is_heap_order(q) for q in fam), name       # nothing exact is judged by tolerance
        assert all(len(q.should) + len(q.must_not) <= 64 and len(q.should) >= 2 for q in fam), name
    assert all(os_.is_heap_order(q, leaf) for q in os_.FAMILY_D)
    assert all(10 <= len(q.should) <= 16 and not q.must_not for q in os_.FAMILY_D10)
    assert all(len(q.should) >= 17 or q.must_not for q in os_.FAMILY_D17)
    assert {len(q.should) for q in os_.FAMILY_A} >= set(range(2, 10)) - {5, 7} and max(len(q.should) for q in os_.FAMILY_A) == 9
    assert all(q.msm >= 2 for q in os_.FAMILY_B)
    for n in (10, 16, 17, 33, 63, 64):
        assert {2, n, n + 1} <= {q.msm for q in os_.FAMILY_B if len(q.should) == n}, n
    assert {len(q.must_not) for q in os_.FAMILY_C[:len(os_.FAMILY_A)]} == {1, 2, 3}
    assert [q.should for q in os_.FAMILY_C[:len(os_.FAMILY_A)]] == [q.should for q in os_.FAMILY_A]
    assert sum(len(q.should) + len(q.must_not) == 64 and q.msm == 2 for q in os_.FAMILY_C) >= 2
    assert any(q.must_not and q.msm >= 2 for q in os_.FAMILY_C)
    queries, rows = os_.mixed()
    assert sorted(i for r in rows.values() for i in r) == list(range(len(queries))) == list(range(sum(len(f) for f in os_.EXACT.values())))
    assert all([queries[i] for i in rows[name]] == fam for name, fam in os_.EXACT.items())
    assert len(os_.cycled(1024)) == 1024 and len(queries) < 512


def _hit_counts(leaf, queries):
    return [os_.ref_docs(leaf, q).size for q in queries]


def test_set_algebra_hit_counts():
    """Counts that can be told without any list in hand."""
    leaf = os_.Leaf()
    n = lambda **kw: os_.ref_docs(leaf, Query(**kw)).size   # noqa: E731
    assert n(should=(FROM_1, EDGE_1K), must_not=(FROM_0,)) == 0                       # every doc prohibited
    assert n(should=(FROM_0, FROM_1, FROM_127), must_not=(EDGE_1K,)) == MAX_DOC - 26
    assert n(should=(os_.FIRST_OF_WINDOW, os_.STRETCH_65), must_not=(EDGE_1K,)) == 65  # doc 1024 is prohibited; 25 docs only MUST_NOT holds
    assert n(should=(EDGE_1K,) * 12, msm=12) == 26 and n(should=(EDGE_1K,) * 12, msm=13) == 0
    assert n(should=(os_.FIRST_OF_WINDOW, os_.LAST_DOC), msm=2) == 0
    for c in (10, 16, 17, 33, 63, 64):
        s = os_._fill(c, {}, os_.DENSE_POOL)
        held_by_all = 25 if c >= len(os_.DENSE_POOL) else None     # EDGE_1K without doc 0
        assert n(should=s, msm=c) == held_by_all and n(should=s, msm=c + 1) == 0 and n(should=s, msm=2) == MAX_DOC   # (doc 0: FROM_0 twice)
    seeded = os_.Leaf(live="seeded")
    assert os_.ref_docs(seeded, Query(should=(FROM_0, ABSENT))).size == int(seeded.alive.sum()) < MAX_DOC
    assert leaf_counts_differ(leaf, seeded)


def leaf_counts_differ(a, b):
    return sum(x != y for x, y in zip(_hit_counts(a, os_.FAMILY_A), _hit_counts(b, os_.FAMILY_A))) > len(os_.FAMILY_A) // 2


@pytest.mark.parametrize("norms,live,version", VARIANTS, ids=["%s-%s-v%d" % v for v in VARIANTS])
def test_oracle_rows_are_the_numpy_rows(oracle, norms, live, version):
    """Families A to C: the oracle's disjunction scorer against set algebra and clause-order f32 sums, bit for bit. Family D: the
    numpy clause-order sums pass the heap-order rule against the oracle's rows, doc sets and hit counts exact."""
    from oracle import parity
    leaf = os_.Leaf(norms=norms, live=live, version=version)
    ref = os_.OrRef(oracle, leaf)
    filled = 0
    for k in CPU_KS:
        for name, fam in os_.EXACT.items():
            for q, (d, s, total) in zip(fam, os_.oracle_rows(oracle, ref.osr, fam, k)):
                wd, ws, wt = ref.row(q, k)
                assert total == wt == os_.ref_docs(leaf, q).size, (name, q, k, total, wt)
                assert d.size == wd.size == min(k, wt) and (d == wd).all(), (name, q, k, d[:8], wd[:8])
                assert (s.view(np.int32) == ws.view(np.int32)).all(), (name, q, k)
                filled += d.size
        for q, (d, s, total) in zip(os_.FAMILY_D, os_.oracle_rows(oracle, ref.osr, os_.FAMILY_D, k)):
            gd, gs, gt = ref.row(q, k)
            row_d = np.concatenate([gd, np.full(k - gd.size, -1, np.int32)])
            row_s = np.concatenate([gs, np.zeros(k - gs.size, np.float32)])
            assert total == os_.ref_docs(leaf, q).size and np.isin(d, os_.ref_docs(leaf, q)).all(), (q, k)
            parity.check_heap_order_row(ref.osr, oracle.OP_OR, list(q.should), row_d, row_s, gt, d, s, d.size, total, rtol=1e-5, what=str((q, k)))
    assert filled > 0


def test_the_big_leaf_rows(oracle):
    """The 33025-doc leaf of the two-windows-per-item plan: the same families over lists rebuilt for it."""
    leaf = os_.Leaf(os_.BIG_MAX_DOC)
    ref = os_.OrRef(oracle, leaf)
    queries, _ = os_.mixed()
    last = 0
    for q, (d, s, total) in zip(queries, os_.oracle_rows(oracle, ref.osr, queries, 10)):
        wd, ws, wt = ref.row(q, 10)
        assert total == wt and (d == wd).all() and (s.view(np.int32) == ws.view(np.int32)).all(), q
        last += int(np.isin(os_.ref_docs(leaf, q), (33023, 33024)).sum())
    assert last > 20     # the docs on either side of the last window's edge are hits of many queries
