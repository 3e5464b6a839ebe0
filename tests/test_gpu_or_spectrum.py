"""Parity at every edge of the clause-order disjunction kernels (`-m gpu`): k_score_terms and k_or_windows answer every OR of fewer
than ten clauses, every OR with MUST_NOT clauses or min_should_match > 1, every OR of 17 to 64 clauses, every OR on a leaf with
deleted docs, with raw or no norms, or at k > 128 - and DisjunctionMaxQuery and BoostingQuery run on the same body. The fixtures of
tests/or_spectrum.py put a posting on either side of each threshold that code branches on: clause position 7 | 8 (the prefetched
run heads), dense selection (four per query, the first 16 clauses, `df * W >= 64 * max_doc`, ties to the earlier clause), a dense
block ending on w1 - 1 | w1 and starting on w1 - 1 | w1, a block across several windows, 63 | 64 | 65 | 128 | 129 run entries of
one clause in one window, runs that end on the last doc of a window / of the leaf, doc_freq 1 | 127 | 128 | 129, VInt tails of
0 | 1 | 127 behind dense blocks, a freq of 10 | 11 in one lane of a block, the 37-doc last window at W = 256 / 1024 / 4096, one | two
windows per item, k 64 | 65 and 128 | 129, BP128 | legacy, and the per-doc counter at min_should_match 2 / n / n + 1.

Everything goes through GpuIndexSearcher.search_batch and the C ABI, against the oracle: doc ids, score bits, -1 padding and hit
counts exact for the families A to C, hit counts also against the numpy set algebra; family D (ten or more clauses,
min_should_match <= 1: the reference sums in heap order) under oracle/parity.py's rule at rtol 1e-5. Each family runs in a batch of
its own and A + B + C dealt into one batch - so that plain queries run in the MUST_NOT / min_should_match instantiations - with
byte-identical rows. tests/test_or_spectrum_cpu.py proves the fixtures and the oracle's rows on the CPU.

Contexts: one module-scoped Context(profile_kernels=True) per knob set, created on first use. Under or_window_docs = 4096 a launch
without min_should_match runs 4096-doc windows; one with it (family B, the mixed batch) carries a counter byte per doc, and
search_or_group narrows its windows to the 3328 docs that fit a CU's LDS - before this module existed such a launch failed with
"invalid argument"."""
import numpy as np
import pytest

import or_spectrum as os_
from boosting_ref import BoostingRef, Positive
from boosting_ref import check_row as check_boosting_row
from dismax_ref import DismaxRef
from dismax_ref import check_row as check_dismax_row
from test_gpu_norm_spectrum import _assert_row

pytestmark = pytest.mark.gpu

KNOBS = {"default": {}, "w256": dict(or_window_docs=256), "w4096": dict(or_window_docs=4096), "run-only": dict(or_dense_clauses=-1),
         "dense1": dict(or_dense_clauses=1), "no-wide": dict(or_wide=-1)}
# (knobs, norms, live, .doc version): rank norms without deletions - where clauses are dense - under every knob set; every other
# value of every axis at least once, with deletions and legacy blocks at all three window widths
COMBOS = [(name, "rank", "none", 1) for name in KNOBS] + [
    ("default", "raw", "none", 1), ("default", "none", "none", 1), ("default", "rank", "seeded", 1), ("default", "rank", "none", 0),
    ("w256", "rank", "seeded", 0), ("w256", "raw", "seeded", 1), ("w4096", "rank", "none", 0), ("w4096", "none", "seeded", 0),
    ("w4096", "rank", "seeded", 1), ("run-only", "rank", "seeded", 0), ("dense1", "rank", "none", 0), ("no-wide", "raw", "none", 0)]


@pytest.fixture(scope="module")
def ctxs():
    import rucene_amd
    made = {}

    def get(name):
        if name not in made:
            made[name] = rucene_amd.Context(profile_kernels=True, **KNOBS[name])
        return made[name]
    yield get
    for c in made.values():
        c.close()


_searchers, _rows = {}, {}


def _osr(oracle, leaf):
    if leaf.key not in _searchers:
        _searchers[leaf.key] = oracle.Searcher([leaf.oracle_segment(oracle)])
    return _searchers[leaf.key]


def _want(oracle, leaf, queries, k):
    """The oracle's rows and the set algebra's hit counts, computed once per (leaf, query, k) and shared by every test."""
    missing = [q for q in dict.fromkeys(queries) if (leaf.key, q, k) not in _rows]
    if missing:
        for q, row in zip(missing, os_.oracle_rows(oracle, _osr(oracle, leaf), missing, k)):
            for a in row[:2]:
                a.setflags(write=False)
            _rows[(leaf.key, q, k)] = (row, os_.ref_docs(leaf, q))
    return [_rows[(leaf.key, q, k)] for q in queries]


def _gpu_leaf(fx):
    import rucene_amd
    return rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, doc_base=0, live_docs=fx.live_docs, sum_total_term_freq=fx.sttf)


def _gpu_query(q):
    import rucene_amd
    T = rucene_amd.TermQuery
    return rucene_amd.BooleanQuery.build([], [T(t) for t in q.should], must_nots=[T(t) for t in q.must_not], min_should_match=q.msm)


def _search(g, queries, k):
    hits, totals = g.search_batch([_gpu_query(q) for q in queries], k)
    assert hits.shape == (len(queries), k) and len(totals) == len(queries)
    return hits, totals


def _check_exact(oracle, leaf, queries, hits, totals, k, what):
    """Doc ids, score bits, -1 in the unused slots and the hit count, as the oracle has them; the hit count as the set algebra has it."""
    for i, (q, (want, docs)) in enumerate(zip(queries, _want(oracle, leaf, queries, k))):
        assert not os_.is_heap_order(q)
        _assert_row(hits[i], totals[i], want, (what, k, i, q))
        assert totals[i] == docs.size, (what, k, i, q, "hit count against the set algebra")


def _check_heap_order(oracle, leaf, queries, hits, totals, k, what):
    from oracle import parity
    osr = _osr(oracle, leaf)
    for i, (q, ((d, s, total), docs)) in enumerate(zip(queries, _want(oracle, leaf, queries, k))):
        assert os_.is_heap_order(q, leaf)
        parity.check_heap_order_row(osr, oracle.OP_OR, list(q.should), hits[i]["doc"], hits[i]["score"], totals[i], d, s, d.size, total, rtol=1e-5,
                                    min_should_match=q.msm, what="%s k %d %s" % (what, k, q))
        np.testing.assert_allclose(hits[i]["score"][:d.size], s, rtol=1e-5, atol=0)
        assert totals[i] == docs.size and np.isin(hits[i]["doc"][:d.size], docs).all(), (what, k, i, q, "against the set algebra")


def _same_rows(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.asarray(a[1]).tolist() == np.asarray(b[1]).tolist()


def _launches(c, *names):
    st = c.kernel_stats()
    return [st[n]["launches"] if n in st else 0 for n in names]


# ---- the families, knob set by knob set ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs,norms,live,version", COMBOS, ids=["%s-%s-%s-v%d" % c for c in COMBOS])
def test_families(ctxs, oracle, knobs, norms, live, version):
    """A, B, C and D each in a batch of its own and A + B + C dealt into one, at k in {1, 10, 64, 65, 128, 129, 300}: every row
    against the oracle, and the mixed batch's rows byte for byte those of the separate batches."""
    import rucene_amd
    fx = os_.Leaf(os_.MAX_DOC, norms, live, version)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(knobs))
    both, at = os_.mixed()
    try:
        for k in os_.KS:
            what = (knobs, norms, live, version)
            apart = {}
            for name, fam in os_.EXACT.items():
                apart[name] = _search(g, fam, k)
                _check_exact(oracle, fx, fam, *apart[name], k, what + (name,))
            hits, totals = _search(g, os_.FAMILY_D, k)
            _check_heap_order(oracle, fx, os_.FAMILY_D, hits, totals, k, what + ("D",))
            hits, totals = _search(g, both, k)
            for name in os_.EXACT:
                assert _same_rows((hits[at[name]], totals[at[name]]), apart[name]), (what, k, name, "mixed batch against its own")
    finally:
        leaf.segment.close()


@pytest.mark.parametrize("live,version", [("none", 1), ("seeded", 1), ("none", 0)], ids=["v1", "deletions", "legacy"])
def test_dense_blocks_and_runs_give_the_same_rows(ctxs, oracle, live, version):
    """Under rank norms the default context decodes up to four clauses per query inside the window kernel, or_dense_clauses = 1 one,
    or_dense_clauses = -1 sends every clause through a run: the rows of A, B and C are the same bytes."""
    import rucene_amd
    fx = os_.Leaf(os_.MAX_DOC, "rank", live, version)
    both, _ = os_.mixed()
    rows = {}
    for knobs in ("default", "run-only", "dense1"):
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(knobs))
        try:
            rows[knobs] = {k: _search(g, both, k) for k in (10, 65, 129)}
        finally:
            leaf.segment.close()
    for k, got in rows["default"].items():
        _check_exact(oracle, fx, both, *got, k, ("default", live, version))
        assert _same_rows(got, rows["run-only"][k]) and _same_rows(got, rows["dense1"][k]), (k, live, version)


# ---- two windows per item -----------------------------------------------------------------------------------------------------------
def test_two_windows_per_item(ctxs, oracle):
    """33025 docs in 256-doc windows, 1024 queries: 1024 * 130 windows > 131072 items, so every item walks two windows, the last
    window holds one doc and the last items of a query start behind it. The rows are the oracle's, and those of the same queries in
    batches of 64 (one window per item)."""
    import rucene_amd
    fx = os_.Leaf(os_.BIG_MAX_DOC)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("w256"))
    queries = os_.cycled(1024)
    assert len(queries) * ((fx.max_doc + 255) // 256) > 131072 >= 64 * ((fx.max_doc + 255) // 256)
    try:
        for k in (10, 129):
            hits, totals = _search(g, queries, k)
            _check_exact(oracle, fx, queries, hits, totals, k, "two windows per item")
            for lo in range(0, 1024, 64):
                assert _same_rows(_search(g, queries[lo:lo + 64], k), (hits[lo:lo + 64], totals[lo:lo + 64])), (k, lo, "one window per item")
    finally:
        leaf.segment.close()


# ---- which kernel answered ----------------------------------------------------------------------------------------------------------
FORCED = [("default", "rank", "none", 10, False), ("no-wide", "rank", "none", 10, True), ("default", "raw", "none", 10, True),
          ("default", "none", "none", 10, True), ("default", "rank", "seeded", 10, True), ("default", "rank", "none", 129, True)]


@pytest.mark.parametrize("knobs,norms,live,k,forced", FORCED, ids=["%s-%s-%s-k%d-%s" % c for c in FORCED])
def test_the_clause_order_kernels_answered(ctxs, oracle, knobs, norms, live, k, forced):
    """From the kernel statistics: A, B, C and the disjunctions of 17 and more clauses (or with MUST_NOT clauses) launch
    k_score_terms and k_or_windows and neither k_or_wide nor k_or_lazy, whatever the context; the disjunctions of 10 to 16 clauses
    do so once or_wide = -1, raw or no norms, deleted docs or k = 129 force them there - and not before."""
    import rucene_amd
    c = ctxs(knobs)
    fx = os_.Leaf(os_.MAX_DOC, norms, live)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    names = ("k_score_terms", "k_or_windows", "k_or_wide", "k_or_lazy")
    try:
        for what, fam in list(os_.EXACT.items()) + [("D17", os_.FAMILY_D17)] + ([("D10", os_.FAMILY_D10)] if forced else []):
            c.kernel_stats_reset()
            _search(g, fam, k)
            score, windows, wide, lazy = _launches(c, *names)
            assert score > 0 and windows > 0 and wide == 0 and lazy == 0, (what, dict(zip(names, (score, windows, wide, lazy))))
        if not forced:
            c.kernel_stats_reset()
            hits, totals = _search(g, os_.FAMILY_D10, k)
            _check_heap_order(oracle, fx, os_.FAMILY_D10, hits, totals, k, "not forced")
            score, windows, wide, lazy = _launches(c, *names)
            assert wide + lazy > 0, dict(zip(names, (score, windows, wide, lazy)))
    finally:
        leaf.segment.close()


# ---- the same edges through k_or_windows_max and k_or_windows_dem ------------------------------------------------------------------
EDGE_SETS = [(os_.EDGE_1K, os_.EDGE_256), (os_.FROM_0, os_.FROM_1, os_.FROM_127, os_.FROM_128), (os_.EDGE_1K, os_.FROM_1, os_.TAIL_0, os_.TAIL_1, os_.TAIL_127),
             (os_.SPAN, os_.EDGE_256, os_.FROM_127), tuple(os_.STRETCHES), (os_.FROM_0,) + tuple(os_.STRETCHES) + (os_.EDGE_1K, os_.EDGE_256),
             (os_.EDGE_1K, os_.EDGE_256, os_.DF_127, os_.BELOW_4K, os_.FIRST_OF_WINDOW, os_.LAST_DOC, os_.BIG_FREQ, os_.STRETCH_129, os_.STRETCH_64),
             (os_.CONST, os_.ABSENT), (os_.FREQ11_DENSE, os_.FREQ11_SPARSE, os_.FROM_128)]
DISMAX_TIES = (0.0, 0.25)
BOOST = 0.5


@pytest.mark.parametrize("knobs", ["default", "w256"])
@pytest.mark.parametrize("norms,live,version", [("rank", "none", 1), ("rank", "seeded", 0), ("raw", "none", 1)], ids=["rank", "rank-deletions-legacy", "raw"])
def test_edges_through_dismax_and_boosting(ctxs, oracle, knobs, norms, live, version):
    """The window-edge, block-alignment and stretch lists as the disjuncts of a DisjunctionMaxQuery (tie 0 and 0.25, fewer than ten
    disjuncts: exact) and as the positive side of a BoostingQuery that EDGE_1K demotes, against tests/dismax_ref.py and
    tests/boosting_ref.py. k_or_windows_max and k_or_windows_dem share the body of k_or_windows with narrower windows."""
    import rucene_amd
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    assert all(len(s) < 10 for s in EDGE_SETS)
    c = ctxs(knobs)
    fx = os_.Leaf(os_.MAX_DOC, norms, live, version)
    dref, bref = DismaxRef(oracle, [fx], _osr(oracle, fx)), BoostingRef(oracle, [fx], _osr(oracle, fx))
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    dismax = [(s, tie) for s in EDGE_SETS for tie in DISMAX_TIES]
    boosting = [Positive("or", s) for s in EDGE_SETS] + [Positive("or", EDGE_SETS[1], must_not=(os_.EDGE_256,)), Positive("or", EDGE_SETS[4], msm=2)]
    try:
        for k in (10, 65, 129):
            c.kernel_stats_reset()
            hits, totals = g.search_batch([rucene_amd.DisjunctionMaxQuery([T(t) for t in s], tie) for s, tie in dismax], k)
            assert _launches(c, "k_or_windows_max")[0] > 0
            for i, (s, tie) in enumerate(dismax):
                check_dismax_row(hits[i], totals[i], dref, s, tie, True, (knobs, norms, live, k, s, tie))
            c.kernel_stats_reset()
            hits, totals = g.search_batch([rucene_amd.BoostingQuery(B.build([], [T(t) for t in p.terms], must_nots=[T(t) for t in p.must_not],
                                                                            min_should_match=p.msm), T(os_.EDGE_1K), BOOST) for p in boosting], k)
            assert _launches(c, "k_or_windows_dem")[0] > 0
            for i, p in enumerate(boosting):
                check_boosting_row(hits[i], totals[i], bref, p, (os_.EDGE_1K,), BOOST, True, (knobs, norms, live, k, p))
    finally:
        leaf.segment.close()
