"""The fixtures of tests/lazy_spectrum.py, proven on the CPU before a GPU sees them: every list sits on the side of its threshold
it is named for, the planted freqs move their docs' scores and their docs are in the top-k, the ladder's brackets hold a sharp
(query, k) each, the ties tie, the floor brackets hold - and for every query the oracle's rows are those of the numpy reference
LazyRef: hit sets and totals by set algebra, scores within 1e-5 of the float64 sums of the oracle's per-term scores."""
import numpy as np
import pytest

import lazy_spectrum as lz
from lazy_spectrum import (ABOVE_BM, ABSENT, BELOW_BM, CONST, D0, DS, EDGE_LZ, EDGE_W, FREQ_TOUCH, FREQS, LADDER_Q, MAX_DOC, NIB_OFF, NIB_ON, STEP, TIE_LZ,
                           WINDOW)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def main():
    return lz.Leaf()


@pytest.fixture(scope="module")
def ref(oracle, main):
    return lz.LazyRef(oracle, main)


def _steps(docs):
    return np.bincount(np.asarray(docs) // STEP, minlength=MAX_DOC // STEP + 1)


def test_the_leaves_and_thresholds_are_the_ones_named(main):
    assert MAX_DOC == 147_493 == 9 * WINDOW + 37 and MAX_DOC % 32 == 5 and -(-MAX_DOC // WINDOW) == 10
    assert lz.bitmap_bound(MAX_DOC) == 2305 and lz.bitmap_bound(MAX_DOC, 256) == 1024 and lz.nibble_bound(MAX_DOC) == 1153
    assert 1153 * 128 >= MAX_DOC > 1152 * 128
    assert [lz.bitmap_bound(n) for n in lz.SMALL] == [1024, 1024, 1024] and lz.SMALL == (STEP, WINDOW, WINDOW + 1)
    df = main.df
    assert (df(BELOW_BM), df(ABOVE_BM), df(NIB_OFF), df(NIB_ON)) == (2304, 2305, 1152, 1153)
    dfs = [df(t) for t in DS]
    assert dfs == sorted(dfs, reverse=True) and len(set(dfs)) == 8 and min(dfs) >= 2305 and dfs[7] < dfs[6] < 2305 + 400
    idfs = [lz.idf(n, MAX_DOC) for n in dfs]
    assert idfs == sorted(idfs)
    for t in (DS[6], DS[7]):                                  # about 36 docs per 2048: together they fit the cells with room to spare
        assert _steps(main.lists[t][0]).max() < 80
    assert df(ABSENT) == 0 and df(lz.LAST_DOC) == df(lz.FIRST_OF_WINDOW) == 1
    assert main.lists[lz.LAST_DOC][0][0] == MAX_DOC - 1 and main.lists[lz.FIRST_OF_WINDOW][0][0] == WINDOW
    assert df(lz.EVERY) == MAX_DOC and all(df(t) == 3 for t in lz.RARES)
    assert all(df(t) >= 2305 for t in (FREQS, EDGE_LZ, TIE_LZ)) and all(df(t) < 1024 for t in lz.FILLS + lz.ANCHS + (EDGE_W, CONST, FREQ_TOUCH))
    nb = main.norms
    assert 25 <= np.unique(nb).size <= 64 and {lz.SHORT, lz.LONG} <= set(nb.tolist())           # rank mode
    assert lz.norm_cache(lz.SHORT) < 0.33 and lz.norm_cache(lz.LONG) > 200                      # one token | 16384 of them
    assert (nb[main.built.background] == lz.LONG).all() and main.built.background.size == lz.N_BACKGROUND
    in_steps = np.isin(main.built.background // STEP, lz.RESERVED_STEPS)
    assert not in_steps.any()
    for t in lz.FILLS + (NIB_OFF, NIB_ON):
        assert np.isin(main.lists[t][0], main.built.background).all()
    assert main.alive.all() and main.live_docs is None
    one = lz.Leaf(live="one")
    assert (~one.alive).sum() == 1 and one.live_docs.size == (MAX_DOC + 63) // 64
    for n in lz.SMALL:
        small = lz.Leaf(n)
        present = [t for t in range(lz.N_TERMS) if small.df(t)]
        assert all(small.df(t) == main.df(t) for t in present if t not in (EDGE_W, lz.EVERY) + DS[:6]) and NIB_OFF in present and NIB_ON in present
        assert all(small.df(t) == n0 for t, n0 in zip(DS, lz.D_DFS) if t in present)             # (MAIN adds the ladder's postings to D0 .. D5)
        assert (BELOW_BM in present) == (n >= 2305) and small.lists[lz.LAST_DOC][0][0] == n - 1
        assert (small.df(lz.FIRST_OF_WINDOW) == 1) == (n > WINDOW)
        qs = lz.small_queries(small)
        assert [len(small.lazy_terms(q)) for q in qs][:3] == [0, 1, 2] and all(len(q.should) == 10 for q in qs)


@pytest.mark.parametrize("version", lz.VERSIONS)
def test_the_doc_bytes_decode_to_the_lists(oracle, version):
    leaf = lz.Leaf(version=version)
    seg = leaf.oracle_segment(oracle)
    assert seg.version == version
    for t, (d, f) in enumerate(leaf.lists):
        got = seg.decode_term(leaf.seg.terms[t])
        assert (got[0] == d).all() and (got[1] == f).all(), lz.NAMES[t]


def test_stretches_splits_and_edges(main):
    for t, (first, n) in lz.STRETCHES.items():
        d = main.lists[t][0]
        assert d.size == n and d[0] == first and (np.diff(d) == 1).all() and d[0] // STEP == d[-1] // STEP, lz.NAMES[t]
        assert d[0] // STEP in lz.RESERVED_STEPS
    assert sorted(n for t, (_, n) in lz.STRETCHES.items() if t not in (lz.STRETCH_512B, lz.STRETCH_513B)) == [63, 64, 65, 128, 129, 512, 513]
    assert (main.lists[lz.STRETCH_64][0][-1] + 1) % STEP == 0 and (main.lists[lz.STRETCH_129][0][-1] + 1) % WINDOW == 0
    assert main.lists[lz.STRETCH_65][0][0] % STEP == 0
    # what a step holds of each bail query's walked clauses: 512 | 513 and 1024 | 1025, and nothing else in those steps
    for cells, (fits, bails) in lz.BAIL_Q.items():
        for q, most in ((fits, cells), (bails, cells + 1)):
            assert main.lazy_terms(q) == [D0]
            walked = np.unique(np.concatenate([main.lists[t][0] for t in q.should if t != D0]))
            assert _steps(walked).max() == most and (_steps(walked) > lz.DEFAULT_CELLS // 4).sum() == 1, (cells, most)
    d = main.lists[lz.SPLIT][0]
    assert d.size == 513 and (np.diff(d) == 1).all() and _steps(d)[[29, 30]].tolist() == [256, 257] and 29 // 8 == 30 // 8
    a, b = main.lists[lz.SPLIT2_A][0], main.lists[lz.SPLIT2_B][0]
    assert a.size == b.size == 400 and a[0] // STEP == a[-1] // STEP == 40 and b[0] // STEP == b[-1] // STEP == 41 and 40 // 8 == 41 // 8
    assert 400 <= lz.DEFAULT_CELLS < 800                                                       # each step fits, the two together do not
    # run lanes (positions among the walked clauses) 7 | 8 - either side of the prefetched heads -, 13 as the last of 14 and 15 as
    # the last of 16, for every stretch of 63 .. 129
    at = {}
    for q in lz.FAMILIES["stretch"]:
        lanes = main.run_lanes(q)
        assert len(lanes) + len(main.lazy_terms(q)) == len(q.should) and sorted(lanes.values()) == list(range(len(lanes)))
        for i, t in enumerate(q.should):
            if t in lz.LONG_RUNS:
                at.setdefault(t, set()).add((lanes[i], len(lanes)))
    assert all(at[t] >= {(7, 9), (8, 9), (13, 14), (15, 16), (7, 11), (8, 11)} for t in lz.LONG_RUNS) and set(at) == set(lz.LONG_RUNS), at
    assert lz.LZ_PREFETCH == 8 and all(n >= 63 for _, n in (lz.STRETCHES[t] for t in lz.LONG_RUNS))
    assert main.run_lanes(lz.Query(should=(D0, lz.FILL_0, lz.FILL_1))) == {1: 0, 2: 1}            # a lazy clause in front shifts the lanes
    want = {0, MAX_DOC - 1} | {w + o for w in range(STEP, MAX_DOC, STEP) for o in (-1, 0, 1)}
    assert set(main.lists[EDGE_W][0].tolist()) == want == set(main.built.edges.tolist()) and len(want) == 2 + 3 * 72
    assert {w + o for w in range(WINDOW, MAX_DOC, WINDOW) for o in (-1, 0, 1)} <= want
    assert np.isin(main.built.edges, main.lists[EDGE_LZ][0]).all()
    f = dict(zip(*[a.tolist() for a in main.lists[EDGE_LZ]]))
    assert min(f[d] for d in want) >= 12 and max(f[d] for d in main.lists[EDGE_LZ][0].tolist() if d not in want) <= 10


def test_how_many_clauses_are_lazy(main):
    lazy = lambda q, ob=0: len(main.lazy_terms(q, ob))   # noqa: E731
    assert [lazy(q) for q in lz.FAMILIES["dense"]] == [0, 1, 4, 5, 6, 6, 6, 6, 1, 1, 6]
    assert [len(q.should) for q in lz.FAMILIES["dense"]][7] == 16 and lz.LZ_MAX_LAZY == 6
    seven, eight = lz.FAMILIES["dense"][5], lz.FAMILIES["dense"][6]
    assert main.lazy_terms(seven) == list(DS[:6]) and main.lazy_terms(eight) == list(DS[:6])     # the seventh and eighth densest are walked
    assert [lazy(q) for q in lz.FAMILIES["bounds"]] == [1, 0, 1, 0] and [lazy(q, 256) for q in lz.FAMILIES["bounds"]] == [2, 2, 2, 2]
    assert lazy(lz.FREQS_Q["nibble"]) == 1 and lazy(lz.FREQS_Q["general"]) == 1 and lazy(lz.FREQS_Q["general"], 256) == 3
    assert main.df(NIB_OFF) < lz.nibble_bound(MAX_DOC) <= main.df(NIB_ON)                         # under or_bitmaps = 256: all_nib is false
    assert lazy(LADDER_Q) == 6 and lazy(lz.FLOOR_Q) == 1 and lz.FLOOR_Q.should.count(lz.EVERY) == 6
    assert all(10 <= len(q.should) <= 16 for q in lz.ALL_QUERIES + [lz.FLOOR_Q] + [q for pair in lz.BAIL_Q.values() for q in pair])
    live = lambda q: sum(main.df(t) > 0 for t in q.should)   # noqa: E731
    assert all(live(q) >= 10 for q in lz.ALL_QUERIES)
    dup = lz.FAMILIES["absent"]
    assert dup[2].should.count(EDGE_W) == 2 and dup[3].should.count(BELOW_BM) == 3 and dup[4].should.count(lz.FILL_0) == 2 and ABSENT in dup[0].should
    assert len(lz.EIGHT) == len(set(lz.EIGHT)) == 8


def test_planted_freqs_matter(ref, main):
    """Every planted doc is in the top-64 of both FREQS queries, and its score moves by more than 1e-4 relative when the posting's
    freq is replaced by what a wrong read gives: the nibble's 15, the clamped byte, another entry of the overflow list."""
    b = main.built
    assert sorted({f for f, _ in b.freq_docs}) == list(lz.PLANTED_FREQS) and len(b.freq_docs) == 14
    lists = dict(zip(*[a.tolist() for a in main.lists[FREQS]]))
    over = sorted({f for f in lz.PLANTED_FREQS if f >= 255})
    assert (main.lists[FREQS][1] >= 255).sum() == 6 and over == [255, 256, 5000]
    for (f, where), doc in b.freq_docs.items():
        assert lists[doc] == f and main.norms[doc] == lz.LONG
        assert main.has[FREQ_TOUCH, doc] == (where == "touched")
        held = [t for t in range(lz.N_TERMS) if main.has[t, doc] and t != lz.EVERY]
        assert held == ([FREQS, FREQ_TOUCH] if where == "touched" else [FREQS])
    assert main.lazy_terms(lz.FREQS_Q["nibble"]) == [FREQS] and FREQ_TOUCH not in main.lazy_terms(lz.FREQS_Q["general"], 256)
    for name, q in lz.FREQS_Q.items():
        docs, sc = ref.ranking(q)
        for (f, where), doc in b.freq_docs.items():
            rank = int(np.flatnonzero(docs == doc)[0])
            assert rank < 64, (name, f, where, rank)
            wrong = ([15] if f != 15 and f >= 14 and f <= 16 else []) + ([min(f, 255)] if f > 255 else []) + ([o for o in over if o != f] if f >= 255 else [])
            if f == 254:
                wrong = [255]
            assert wrong or f == 15
            for w in wrong:
                moved = abs(ref.score_with(q, doc, FREQS, w) / sc[rank] - 1.0)
                assert moved > lz.SHARP, (name, f, where, w, moved)
        assert ref.is_sharp(q, 2) and set(docs[:2].tolist()) == {b.freq_docs[(5000, "touched")], b.freq_docs[(5000, "lazy")]}


def test_the_ladder_brackets(ref, main):
    """For every m a sharp (LADDER_Q, k): the k-th score lies strictly between the sums of the m - 1 and of the m largest clause maxima
    of the six lazy lists, HI_m is in, MID_m and LO_m (the same m lists) are out."""
    b = main.built
    assert main.lazy_terms(LADDER_Q) == list(DS[:6])
    maxima = sorted((ref.clause_max(t) for t in DS[:6]), reverse=True)
    docs, sc = ref.ranking(LADDER_Q)
    rank = {int(d): i for i, d in enumerate(docs[:4096].tolist())}
    ks = lz.ladder_ks(ref)
    assert sorted(ks.values(), reverse=True) == [ks[m] for m in range(1, 7)] and len(set(ks.values())) == 6 and max(ks.values()) <= 128
    for m in range(1, 7):
        hi, mid, lo = (b.ladder[(kind, m)] for kind in ("hi", "mid", "lo"))
        for doc, freq, byte in ((hi, 10, lz.SHORT), (mid, 1, lz.SHORT), (lo, 1, lz.LONG)):
            held = [t for t in range(lz.N_TERMS) if main.has[t, doc] and t != lz.EVERY]
            assert held == list(DS[6 - m:6]) and main.norms[doc] == byte                      # m lazy lists, no walked clause
            assert all(main.lists[t][1][np.searchsorted(main.lists[t][0], doc)] == freq for t in held)
            in_hi_half = freq / (freq + lz.norm_cache(byte)) >= 0.72                           # BITMAP_HI_CUT
            assert in_hi_half == (byte == lz.SHORT)
        k = ks[m]
        kth = sc[k - 1]
        assert sum(maxima[:m - 1]) < kth < sum(maxima[:m]), (m, k, kth)
        assert ref.is_sharp(LADDER_Q, k), (m, k, ref.gap(LADDER_Q, k))
        assert abs(sc[rank[hi]] / sum(maxima[:m]) - 1.0) < 1e-6                                # HI_m scores the m largest maxima
        assert rank[hi] < k and rank.get(mid, 1 << 30) >= k and rank.get(lo, 1 << 30) >= k, (m, k)
        assert sc[rank[hi]] > kth * (1 + lz.SHARP)
    for q in lz.FAMILIES["ladder"][1:]:                                                        # the same docs whatever the clause order
        assert set(ref.row(q, ks[1])[0][:ks[6]].tolist()) == set(docs[:ks[6]].tolist())


def test_ties(oracle, ref, main):
    docs, s = ref.clause(CONST)
    assert docs.tolist() == list(range(lz.CONST_LO, lz.CONST_HI)) and docs.size == 300 and np.unique(s.view(np.int32)).size == 1
    assert lz.CONST_LO < WINDOW - 128 and WINDOW < lz.CONST_HI and (main.norms[docs] == lz.TIE_BYTE).all()
    d2, s2 = ref.clause(TIE_LZ)
    assert np.unique(s2[np.isin(d2, docs)].view(np.int32)).size == 1 and main.lazy_terms(lz.TIE_Q["both"]) == [TIE_LZ]
    for q in lz.TIE_Q.values():
        held = main.has[list(q.should)][:, docs].sum(axis=0)
        assert (held == held[0]).all() and held[0] <= 2                                        # at most two addends: order-free in f32
        for k, row in zip(lz.TIE_KS, [lz.oracle_rows(oracle, ref.osr, [q], k)[0] for k in lz.TIE_KS]):
            assert row[0].tolist() == list(range(lz.CONST_LO, lz.CONST_LO + k)) and np.unique(row[1].view(np.int32)).size == 1
            assert ref.row(q, k)[0].tolist() == row[0].tolist()


def test_the_floor_brackets(ref, main):
    q, n = lz.FLOOR_Q, len(lz.FLOOR_Q.should)
    bound = sum(lz.idf(main.df(t), MAX_DOC) * (lz.K1 + 1.0) for t in q.should)
    _, sc = ref.ranking(q)
    assert sc[lz.FLOOR_K["hi"] - 1] > 1.01 * bound * n / 8192                                 # above n * 2^17 steps whatever the exponent
    assert sc[lz.FLOOR_K["lo"] - 1] < 0.99 * bound * n / 16384                                # below them
    assert sc.size == MAX_DOC and ref.is_sharp(q, lz.FLOOR_K["hi"])


def test_sharp_rows_are_common(ref):
    sharp = sum(ref.is_sharp(q, k) for q in lz.ALL_QUERIES for k in lz.KS)
    assert sharp >= len(lz.ALL_QUERIES) * len(lz.KS) // 3
    edge = ref.ranking(lz.EDGE_Q["lazy"])[0][:128]
    assert np.isin(edge, ref.leaf.built.edges).all() and {0, MAX_DOC - 1, WINDOW - 1, WINDOW, WINDOW + 1, 9 * WINDOW} <= set(edge.tolist())


def _check_rows(oracle, ref, queries, ks):
    from oracle import parity
    leaf = ref.leaf
    for k in ks:
        for q, (d, s, total) in zip(queries, lz.oracle_rows(oracle, ref.osr, queries, k)):
            hits = lz.ref_docs(leaf, q)
            rd, rs, rt = ref.row(q, k)
            assert total == rt == hits.size and d.size == rd.size == min(k, rt) and np.isin(d, hits).all(), (q, k)
            # LazyRef's row passes the heap-order rule against the oracle's: scores within 1e-5, docs exchanged only inside the band
            row_d = np.concatenate([rd, np.full(k - rd.size, -1, np.int32)])
            row_s = np.concatenate([rs.astype(np.float32), np.zeros(k - rs.size, np.float32)])
            differing = parity.check_heap_order_row(ref.osr, oracle.OP_OR, list(q.should), row_d, row_s, rt, d, s, d.size, total, rtol=1e-5, what=str((q, k)))
            np.testing.assert_allclose(np.sort(s.astype(np.float64))[::-1], rs, rtol=1e-5, atol=0)
            if ref.is_sharp(q, k):
                assert differing == 0 and set(d.tolist()) == set(rd.tolist()), (q, k)
            at = ref.separated(q, k)
            assert (d[at] == rd[at]).all(), (q, k)


@pytest.mark.parametrize("version", lz.VERSIONS)
def test_oracle_rows_are_the_numpy_rows(oracle, version):
    ref = lz.LazyRef(oracle, lz.Leaf(version=version))
    extra = [lz.FLOOR_Q] + [q for pair in lz.BAIL_Q.values() for q in pair]
    _check_rows(oracle, ref, lz.ALL_QUERIES + extra, lz.KS if version else (10, 128))
    _check_rows(oracle, ref, [LADDER_Q], sorted(lz.ladder_ks(ref).values()) + list(lz.FLOOR_K.values()))


@pytest.mark.parametrize("max_doc", lz.SMALL)
def test_the_small_leaves(oracle, max_doc):
    leaf = lz.Leaf(max_doc)
    ref = lz.LazyRef(oracle, leaf)
    _check_rows(oracle, ref, lz.small_queries(leaf), (1, 10, 128))


def test_the_long_leaf(oracle):
    """253 windows: alone a query is cut into 256 items of one window (the pilot launch needs 64 of them, k_premerge_items 256);
    among 300 rows into 128 items of two windows (neither). Two lists just above the bitmap bound, eight sparse ones below it."""
    assert lz.LONG_MAX_DOC == 4_128_805 == 252 * WINDOW + 37 and lz.bitmap_bound(lz.LONG_MAX_DOC) == 64_513
    assert lz.long_plan(1) == (256, 1) and lz.long_plan(lz.LONG_BATCH) == (128, 2) and lz.long_plan(8192, MAX_DOC) == (8, 2)
    leaf = lz.LongLeaf()
    assert 64_513 <= leaf.df(lz.LONG_L1) < leaf.df(lz.LONG_L0) < 64_513 + 300 and all(leaf.df(t) == 62 for t in lz.LONG_SPARSE)
    assert [len(leaf.lazy_terms(q)) for q in lz.LONG_QUERIES] == [2, 1, 0, 1] and all(len(q.should) >= 10 for q in lz.LONG_QUERIES)
    assert leaf.has[:, lz.LONG_MAX_DOC - 1].sum() == 2 and np.unique(leaf.top // WINDOW).size >= 8
    ref = lz.LazyRef(oracle, leaf)
    _check_rows(oracle, ref, lz.LONG_QUERIES, (10, 128))
    for q in lz.LONG_QUERIES:
        assert ref.is_sharp(q, 10) and np.isin(ref.row(q, 10)[0], leaf.top).all()


def test_the_splits_are_sharp_on_either_side_of_their_edge(ref, main):
    """SPLIT and SPLIT2: sharp rows at k = 10, 64 and 100 that hold docs below and above the step edge / of both steps."""
    one, two = lz.FAMILIES["split"][:2]
    assert one.should[:2] == (D0, lz.SPLIT) and two.should[:3] == (D0, lz.SPLIT2_A, lz.SPLIT2_B)
    for k in (10, 64, 100):
        d = ref.row(one, k)[0]
        d = d[np.isin(d, main.lists[lz.SPLIT][0])]
        assert ref.is_sharp(one, k) and (d < lz.SPLIT_AT).sum() >= 5 and (d >= lz.SPLIT_AT).sum() >= 5, k
        d = ref.row(two, k)[0]
        assert ref.is_sharp(two, k) and np.isin(d, main.lists[lz.SPLIT2_A][0]).sum() >= 5 and np.isin(d, main.lists[lz.SPLIT2_B][0]).sum() >= 5, k
