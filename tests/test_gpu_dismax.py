"""DisjunctionMaxQuery over term clauses on the GPU (`-m gpu`): RGPU_OP_DISMAX through the public mirrors and the C ABI, against rows
composed from the oracle's own per-clause scorers (tests/dismax_ref.py; tests/test_dismax_cpu.py proves that composition on the CPU).

The fixtures are those of tests/segment_spectrum.py. A row is checked on doc ids, score bits, -1 padding and the hit count, all exact,
wherever fewer than ten disjuncts have a scorer in the leaf (the reference's SimpleQueue: clause order) or the tie-breaker is 0 (the
maximum is order-free). With ten or more present and tie > 0 the reference sums in DisiPriorityQueue order and pins a score no
tighter than 1e-5 relative (README.md states the same for OR): those rows are asked for with k >= the hit count on the leaves of up
to 257 docs (k = 300, no k-th band exists) - equal doc sets, exact hit counts, scores within rtol 1e-5 - and, where k is below the hit
count (larger leaves, many leaves), under the same tolerance with the k-th band written out (dismax_ref.check_row).

Contexts: one module-scoped Context(profile_kernels=True) under default knobs; or_window_docs is a context knob, so the 256-doc
windows and the 4096-doc request (which the dismax group narrows until its launch fits a CU's LDS) have a module-scoped context
each, created on first use. The kernel-statistics test opens a fresh one."""
import os
import subprocess

import numpy as np
import pytest

import segment_spectrum as ss
from dismax_ref import DismaxRef, check_row

pytestmark = pytest.mark.gpu

TIES = (0.0, 0.1, 1.0)
KS = (1, 10, 129)
K_ALL = 300   # above every hit count of the leaves of up to 257 docs
E, F, L, V, Q5, A, S, C = ss.EVERY, ss.FIRST, ss.LAST, ss.EVEN, ss.FIFTH, ss.ABSENT, ss.SOMETIMES, ss.CONST
CLAUSE_SETS = {"one": (Q5,), "two": (V, Q5), "twice": (Q5, Q5), "nine": (E, F, L, V, Q5, A, S, C, V),
               "ten-present": (E, F, L, V, Q5, C, E, V, Q5, C), "twelve-present": (E, F, L, V, Q5, C, E, V, Q5, C, F, L),
               "twelve-absent-repeats": (F, L, Q5, A, V, A, F, A, C, A, E, A), "all-absent": (A, A)}
QUERIES = [(c, tie) for c in CLAUSE_SETS.values() for tie in TIES]
KNOBS = {"default": {}, "w256": dict(or_window_docs=256), "w4096": dict(or_window_docs=4096)}
SINGLE = [(n, norms, live) for n in (1, 64, 129, 257, 1025, 8193) for norms in ss.NORMS for live in ("none", "seeded", "all")]


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


def _gpu_leaf(fx):
    import rucene_amd
    return rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, doc_base=fx.doc_base, live_docs=fx.live_docs,
                                 sum_total_term_freq=fx.sttf)


def _dq(clauses, tie):
    import rucene_amd
    return rucene_amd.DisjunctionMaxQuery([rucene_amd.TermQuery(t) for t in clauses], tie)


def _exact(ref, clauses, tie):
    return tie == 0.0 or ref.present(clauses) < 10


def _check_batch(g, ref, k, what):
    hits, totals = g.search_batch([_dq(c, tie) for c, tie in QUERIES], k)
    assert hits.shape == (len(QUERIES), k) and len(totals) == len(QUERIES)
    for i, (c, tie) in enumerate(QUERIES):
        check_row(hits[i], totals[i], ref, c, tie, _exact(ref, c, tie), (what, k, c, tie))


def test_the_clause_sets_are_the_ones_named():
    fx = ss.Leaf(257)
    present = {name: sum(1 for t in c if fx.lists[t][0].size > 0) for name, c in CLAUSE_SETS.items()}
    assert present == {"one": 1, "two": 2, "twice": 2, "nine": 8, "ten-present": 10, "twelve-present": 12, "twelve-absent-repeats": 7, "all-absent": 0}
    assert [len(c) for c in CLAUSE_SETS.values()] == [1, 2, 2, 9, 10, 12, 12, 2]
    assert all(ss.Leaf(n).max_doc < K_ALL for n in (1, 64, 129, 257))


# ---- one leaf -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc,norms,live", SINGLE, ids=["%d-%s-%s" % c for c in SINGLE])
def test_single_leaf(ctxs, oracle, max_doc, norms, live):
    """Every clause set at every tie-breaker in one batch, k in {1, 10, 129} (two passes) and, on the leaves of up to 257 docs, 300
    (every hit: the rows of ten and more present disjuncts compare as whole doc sets); default knobs and 256-doc windows, and on the
    8193-doc leaves a request for 4096-doc windows."""
    import rucene_amd
    fx = ss.Leaf(max_doc, norms, live)
    ref = DismaxRef(oracle, [fx])
    ks = KS + ((K_ALL,) if max_doc <= 257 else ())
    for name in ["default", "w256"] + (["w4096"] if max_doc == 8193 else []):
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(name))
        try:
            for k in ks:
                _check_batch(g, ref, k, (max_doc, norms, live, name))
        finally:
            leaf.segment.close()


# ---- many leaves --------------------------------------------------------------------------------------------------------------------
def _small_index():
    """Five leaves of 548 docs in all, one of them hollow (no disjunct has a scorer there): every hit of every query fits k = 600."""
    leaves = [ss.Leaf(129, "rank", "seeded", salt=4), ss.Leaf(257, "rank", "none", salt=2), ss.Leaf(65, "rank", "none", salt=2, hollow=True),
              ss.Leaf(33, "rank", "last", salt=4), ss.Leaf(64, "rank", "first", salt=4)]
    base = 0
    for leaf in leaves:
        leaf.doc_base = base
        base += leaf.max_doc
    assert base == 548 and ss.stats_leaf(leaves) == 1
    return leaves


MULTI = {"many-shuffled": (lambda: ss.many(True), (10, 129)), "twins": (ss.twins, (10, 129)), "small-whole-rows": (_small_index, (10, 129, 600))}


@pytest.mark.parametrize("index", sorted(MULTI))
def test_multi_leaf(ctxs, oracle, index):
    """Leaves of every size at once / two equally large leaves / five small ones: the number of disjuncts with a scorer differs from
    leaf to leaf (a hollow leaf, SOMETIMES absent wherever max_doc is a multiple of 3), every leaf scores with the statistics leaf's
    weights, and the per-leaf rows merge under the canonical tie rule. On the small index k = 600 is above every hit count: the rows
    of ten and more present disjuncts with tie > 0 compare as whole doc sets there, as on the single leaves."""
    import rucene_amd
    leaves = MULTI[index][0]()
    ref = DismaxRef(oracle, leaves)
    if index == "small-whole-rows":
        assert max(ref.rows(c, 0.0)[2] for c in CLAUSE_SETS.values()) < 600 and ref.present(CLAUSE_SETS["twelve-present"]) == 12
    per_leaf = {tuple(sum(1 for t in c if leaf.lists[t][0].size > 0) for leaf in leaves) for c in CLAUSE_SETS.values()}
    assert any(len(set(p)) > 1 for p in per_leaf)
    gl = [_gpu_leaf(fx) for fx in leaves]
    g = rucene_amd.GpuIndexSearcher(gl, ctx=ctxs("default"))
    try:
        for k in MULTI[index][1]:
            _check_batch(g, ref, k, (index,))
    finally:
        for leaf in gl:
            leaf.segment.close()


# ---- mixed batches ------------------------------------------------------------------------------------------------------------------
def test_mixed_batch(ctxs, oracle):
    """Dismax queries between TERM, AND, OR and >= 10-clause OR queries of one search_batch: a group of their own - the other rows are
    byte for byte those of the same batch without them, the dismax rows are the ones they are alone."""
    import rucene_amd
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    fx = ss.Leaf(1025, "rank", "none")
    ref = DismaxRef(oracle, [fx])
    others = [B.build([T(t) for t in q.must], [T(t) for t in q.should]) for q in ss.TERMS + ss.ANDS + ss.ORS + ss.WIDE]
    mixed, where_other, where_dismax = [], [], []
    for i, q in enumerate(others):
        if i % 2 == 0 and i // 2 < len(QUERIES):
            where_dismax.append(len(mixed))
            mixed.append(_dq(*QUERIES[i // 2]))
        where_other.append(len(mixed))
        mixed.append(q)
    for j in range(len(where_dismax), len(QUERIES)):
        where_dismax.append(len(mixed))
        mixed.append(_dq(*QUERIES[j]))
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("default"))
    try:
        for k in (10, 129):
            plain_h, plain_t = g.search_batch(others, k)
            hits, totals = g.search_batch(mixed, k)
            assert hits[where_other].tobytes() == plain_h.tobytes() and totals[where_other].tolist() == plain_t.tolist(), k
            assert plain_t.sum() > 0
            for j, (c, tie) in enumerate(QUERIES):
                i = where_dismax[j]
                check_row(hits[i], totals[i], ref, c, tie, _exact(ref, c, tie), ("mixed", k, c, tie))
    finally:
        leaf.segment.close()


# ---- which kernel -------------------------------------------------------------------------------------------------------------------
def _launches(c, name):
    st = c.kernel_stats()
    return st[name]["launches"] if name in st else 0


def test_kernel_statistics(oracle):
    """A dismax batch runs k_score_terms + k_or_windows_max and neither of the heap-order kernels, even with 12 disjuncts on the
    8193-doc rank-mode leaf without deletions (where a 12-clause OR query takes k_or_lazy / k_or_wide); a plain OR batch never
    launches k_or_windows_max."""
    import rucene_amd
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    fx = ss.Leaf(8193, "rank", "none")
    ref = DismaxRef(oracle, [fx])
    c = rucene_amd.Context(profile_kernels=True)
    try:
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
        twelve = CLAUSE_SETS["twelve-present"]
        g.search_batch([B.build([], [T(V), T(Q5)]), B.build([], [T(t) for t in twelve])], 10)
        assert _launches(c, "k_or_windows_max") == 0
        assert _launches(c, "k_or_windows") > 0 and _launches(c, "k_or_lazy") + _launches(c, "k_or_wide") > 0
        c.kernel_stats_reset()
        batch = [(twelve, 0.1), (twelve, 0.0), (CLAUSE_SETS["two"], 0.1)]
        hits, totals = g.search_batch([_dq(*q) for q in batch], 10)
        assert _launches(c, "k_or_windows_max") == 1 and _launches(c, "k_score_terms") == 1
        assert _launches(c, "k_or_lazy") == 0 and _launches(c, "k_or_wide") == 0 and _launches(c, "k_or_windows") == 0
        for i, (cl, tie) in enumerate(batch):
            check_row(hits[i], totals[i], ref, cl, tie, _exact(ref, cl, tie), ("statistics", cl, tie))
        leaf.segment.close()
    finally:
        c.close()


# ---- the C ABI's refusals -----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals(ctxs, oracle):
    import torch
    import rucene_amd
    T, D = rucene_amd.TermQuery, rucene_amd.DisjunctionMaxQuery
    fx = ss.Leaf(257, "rank", "seeded")
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("default"))
    try:
        qs, ts = g.pack([D([T(V), T(Q5)], 0.1)], leaf)
        assert qs["op"][0] == 3

        def status(op=None, tie=None):
            q = qs.copy()
            if op is not None:
                q["op"][0] = op
            if tie is not None:
                q["n_must_not"][0] = int(np.float32(tie).view(np.int32))
            with pytest.raises(rucene_amd.RgpuError) as e:
                leaf.segment.search_batch(q, ts, 10)
            return e.value.status
        assert status(tie=np.nan) == -2 and status(tie=np.inf) == -2 and status(tie=-np.inf) == -2      # IllegalArgument
        assert status(op=3 | (2 << 8)) == -2           # a min_should_match byte
        assert status(op=3 | (1 << 16)) == -2          # an optional-SHOULD byte
        assert status(op=3 | (1 << 24)) == -2 and status(op=4) == -2
        p = g._planner(leaf)
        with pytest.raises(rucene_amd.RgpuError) as e:
            p.plan_batch([3], [2], [V, Q5], [0])
        assert e.value.status == -5                    # UnsupportedOperation
        with pytest.raises(rucene_amd.RgpuError) as e:
            p.plan_uniform(3, np.array([[V, Q5]]))
        assert e.value.status == -5
        d_hits = torch.empty((1, 10), dtype=torch.int64, device="cuda")
        d_tot = torch.empty((1,), dtype=torch.int64, device="cuda")
        with pytest.raises(rucene_amd.RgpuError) as e:
            p.search_uniform_device(leaf.segment, 3, np.array([[V, Q5]], dtype=np.int64), 10, d_hits.data_ptr(), d_tot.data_ptr())
        assert e.value.status == -5
        # QueryRescorer with a dismax second pass is not served: UnsupportedOperation, the first-pass rows untouched
        first, _ = g.search_batch([T(V)], 10)
        with pytest.raises(rucene_amd.RgpuError) as e:
            g.rescore_batch(first, [D([T(V), T(Q5)], 0.1)])
        assert e.value.status == -5
        # a refused call leaves the segment as it was: the query itself is served
        ref = DismaxRef(oracle, [fx])
        hits, totals = leaf.segment.search_batch(qs, ts, 10)
        check_row(hits[0], totals[0], ref, (V, Q5), 0.1, True, "after the refusals")
    finally:
        leaf.segment.close()


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------
def test_cpp_demo_rows_equal_the_python_mirror(ctxs, oracle, tmp_path):
    """tests/cpp/dismax_demo.cpp: rucene::DisjunctionMaxQuery through csrc/host/gpu_index_searcher.hpp on the 1025-doc rank-mode leaf -
    the lines it prints are the Python mirror's rows (which the tests above hold against the oracle)."""
    import rucene_amd
    T, D = rucene_amd.TermQuery, rucene_amd.DisjunctionMaxQuery
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "dismax_demo")
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "cpp", "dismax_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    fx = ss.Leaf(1025, "rank", "none")
    for name, blob in (("doc", fx.seg.doc_bytes), ("norms", fx.norms), ("terms", np.ascontiguousarray(fx.seg.terms, dtype=rucene_amd.TERM_STATE_DTYPE))):
        (tmp_path / (name + ".bin")).write_bytes(np.asarray(blob).tobytes())
    out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.max_doc), str(fx.sttf)], text=True).strip().splitlines()
    queries = [D([T(4)], 0.5), D([T(3), T(4)], 0.0), T(6), D([T(4), T(4)], 0.1), D([T(t) for t in (0, 1, 2, 3, 4, 5, 6, 7, 3)], 0.1),
               D([T(t) for t in (1, 2, 4, 5, 6, 5, 1, 2, 4, 5, 5, 5)], 1.0), D([T(5), T(5)], 0.1)]
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("default"))
    try:
        hits, totals = g.search_batch(queries, 10)
    finally:
        leaf.segment.close()
    assert len(out) == len(queries) + 1
    for i, line in enumerate(out):
        j = i if i < len(queries) else 1              # the last line: queries[1] through search() and a collector
        parts = line.split()
        assert parts[0] == "dismax" and int(parts[1]) == i and int(parts[2]) == totals[j], line
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        n = min(10, int(totals[j]))
        assert [x[0] for x in got] == hits[j]["doc"][:n].tolist(), line
        assert [x[1] for x in got] == hits[j]["score"][:n].view(np.uint32).tolist(), line
    assert totals[6] == 0 and totals[1] > 10
    ref = DismaxRef(oracle, [fx])
    check_row(hits[4], totals[4], ref, (0, 1, 2, 3, 4, 5, 6, 7, 3), 0.1, True, "the demo's nine-clause query")
