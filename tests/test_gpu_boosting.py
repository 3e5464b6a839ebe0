"""BoostingQuery on the GPU (`-m gpu`): demoting clauses (RGPU_NOT_WITH_DEMOTE) through the Python mirror and the C ABI, against rows
composed from the oracle (tests/boosting_ref.py; tests/test_boosting_cpu.py proves that composition on the CPU).

The fixtures are those of tests/segment_spectrum.py. Doc ids, score bits, -1 padding and hit counts are exact everywhere, except for
positives of ten and more present SHOULD clauses: the reference sums those in heap order and README.md states 1e-5 relative, so they
are asked for only with k at or above the hit count on the leaves of up to 257 docs - whole doc sets and hit counts exact, scores
within rtol 1e-5.

Contexts: one module-scoped Context(profile_kernels=True) per knob set - default, and_bitmaps=-1 with or_bitmaps=-1 (every demoting
clause is walked or compared, never asked through a doc bitmap), or_window_docs=256 - created on first use; rows are byte-identical
across them. The kernel-statistics test opens a fresh one."""
import numpy as np
import pytest

import segment_spectrum as ss
from boosting_ref import BoostingRef, Positive, check_row, hollow_leaves_with_positive_docs

pytestmark = pytest.mark.gpu

E, F, L, V, Q5, A, S, C = ss.EVERY, ss.FIRST, ss.LAST, ss.EVEN, ss.FIFTH, ss.ABSENT, ss.SOMETIMES, ss.CONST
BOOSTS = (0.5, 0.1, float(np.nextafter(np.float32(1), np.float32(0))))
POSITIVES = [Positive("term", (Q5,)), Positive("term", (E,)), Positive("and", (V, Q5)), Positive("and", (E, V, C)), Positive("or", (F, L, Q5)),
             Positive("or", (V, Q5, S), msm=2), Positive("or", (E, L, V, Q5, A, S, C, V, Q5), must_not=(F,))]
NEGATIVES = [(F,), (L,), (V,), (Q5,), (E,), (A,), (A, Q5), (V, Q5), (S,)]
QUERIES = [(p, n, b) for p in POSITIVES for n in NEGATIVES for b in BOOSTS]
WIDE_POSITIVES = [Positive("or", (E, F, L, V, Q5, C, E, V, Q5, C)), Positive("or", (E, F, L, V, Q5, C, E, V, Q5, C, F, L), must_not=(S,))]
KS = (1, 10, 129)
K_ALL = 300   # above every hit count of the leaves of up to 257 docs
KNOBS = {"default": {}, "no-bitmaps": dict(and_bitmaps=-1, or_bitmaps=-1), "w256": dict(or_window_docs=256)}
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


def _positive_query(p):
    import rucene_amd
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    if p.op == "term":
        return T(p.terms[0])
    if p.op == "and":
        return B.build([T(t) for t in p.terms], [], must_nots=[T(t) for t in p.must_not])
    return B.build([], [T(t) for t in p.terms], must_nots=[T(t) for t in p.must_not], min_should_match=p.msm)


def _bq(p, negative, boost):
    import rucene_amd
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    neg = T(negative[0]) if len(negative) == 1 else B.build([], [T(t) for t in negative])
    return rucene_amd.BoostingQuery(_positive_query(p), neg, boost)


def _check_batch(g, ref, queries, k, what, exact=True):
    hits, totals = g.search_batch([_bq(*q) for q in queries], k)
    assert hits.shape == (len(queries), k) and len(totals) == len(queries)
    for i, (p, n, b) in enumerate(queries):
        check_row(hits[i], totals[i], ref, p, n, b, exact, (what, k, p, n, b))
    return hits, totals


def test_the_fixture_shapes_are_the_ones_named():
    fx = ss.Leaf(1025)
    min_df = 512                                       # doc bitmaps are built for lists of 512 docs and more (segment_spectrum.py)
    assert fx.lists[V][0].size >= min_df > fx.lists[Q5][0].size and ss.Leaf(8193).lists[Q5][0].size >= min_df
    assert fx.lists[F][0].size == 1 and fx.lists[L][0].size == 1 and fx.lists[A][0].size == 0
    assert all(ss.Leaf(n).max_doc < K_ALL for n in (1, 64, 129, 257))
    small = ss.Leaf(257)
    assert [sum(1 for t in p.terms if small.lists[t][0].size > 0) for p in WIDE_POSITIVES] == [10, 12]
    assert max(sum(1 for t in p.terms if small.lists[t][0].size > 0) for p in POSITIVES) < 10


# ---- one leaf -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc,norms,live", SINGLE, ids=["%d-%s-%s" % c for c in SINGLE])
def test_single_leaf(ctxs, oracle, max_doc, norms, live):
    """Every positive x negative x boost in one batch, k in {1, 10, 129} (two passes) and, on the leaves of up to 257 docs, 300; under
    default knobs against the reference, and byte for byte the same rows without doc bitmaps and with 256-doc windows."""
    import rucene_amd
    fx = ss.Leaf(max_doc, norms, live)
    ref = BoostingRef(oracle, [fx])
    ks = KS + ((K_ALL,) if max_doc <= 257 else ())
    first = {}
    for name in KNOBS:
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(name))
        try:
            for k in ks:
                if name == "default":
                    hits, totals = _check_batch(g, ref, QUERIES, k, (max_doc, norms, live))
                    first[k] = (hits.tobytes(), totals.tolist())
                else:
                    hits, totals = g.search_batch([_bq(*q) for q in QUERIES], k)
                    assert (hits.tobytes(), totals.tolist()) == first[k], (name, k)
        finally:
            leaf.segment.close()


def test_a_demotion_that_changes_membership(ctxs, oracle):
    """(EVERY) demoted by EVEN at 0.1 on the 1025-doc leaf: the even docs fall behind the odd ones, so the top 10 holds odd docs only
    and differs from the positive's own row, which holds an even doc."""
    import rucene_amd
    fx = ss.Leaf(1025, "rank", "none")
    ref = BoostingRef(oracle, [fx])
    p = Positive("term", (E,))
    own_d, own_s, own_t = ref.positive(p)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("default"))
    try:
        for k in (10, 129):
            hits, totals = g.search_batch([_bq(p, (V,), 0.1), _positive_query(p)], k)
            check_row(hits[0], totals[0], ref, p, (V,), 0.1, True, ("membership", k))
            assert (hits[1]["doc"] == own_d[:k]).all() and totals[1] == own_t == totals[0]
            assert (own_d[:k] % 2 == 0).any(), "the positive's own row holds an even doc"
            assert (hits[0]["doc"] % 2 == 1).all(), "demotion moved every even doc out of the top k"
            assert hits[0]["doc"].tolist() != hits[1]["doc"].tolist()
    finally:
        leaf.segment.close()


@pytest.mark.parametrize("max_doc,live", [(n, lv) for n in (64, 129, 257) for lv in ("none", "seeded")])
def test_positives_of_ten_and_more_present_should_clauses(ctxs, oracle, max_doc, live):
    import rucene_amd
    fx = ss.Leaf(max_doc, "rank", live)
    ref = BoostingRef(oracle, [fx])
    queries = [(p, n, b) for p in WIDE_POSITIVES for n in NEGATIVES for b in BOOSTS[:2]]
    assert all(ref.present(p) >= 10 for p in WIDE_POSITIVES) and max(ref.positive(p)[2] for p in WIDE_POSITIVES) <= K_ALL
    for name in KNOBS:
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(name))
        try:
            _check_batch(g, ref, queries, K_ALL, (max_doc, live, name), exact=False)
        finally:
            leaf.segment.close()


# ---- many leaves --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ["many-shuffled", "twins"])
def test_multi_leaf(ctxs, oracle, index):
    """A negative of SOMETIMES: the leaves whose max_doc is a multiple of 3, and the hollow one, have no negative scorer and contribute
    nothing although the positives match docs there; the others merge under the canonical rule with the statistics leaf's weights."""
    import rucene_amd
    leaves = ss.many(True) if index == "many-shuffled" else ss.twins()
    ref = BoostingRef(oracle, leaves)
    queries = [(p, n, b) for p in POSITIVES for n in ((S,), (S, A), (S, F)) for b in BOOSTS[:2]]
    dropped = hollow_leaves_with_positive_docs(leaves, Positive("term", (E,)), (S,))
    assert dropped and all(leaves[i].max_doc % 3 == 0 for i in dropped)
    assert ref.rows(Positive("term", (E,)), (S,), 0.5)[2] < ref.positive(Positive("term", (E,)))[2]
    if index == "many-shuffled":
        assert any(leaf.hollow for leaf in leaves)
    # (S, F): FIRST has a posting in every leaf that is not hollow, so the multiples of 3 come back - and only SOMETIMES went missing there
    assert ref.rows(Positive("term", (E,)), (S, F), 0.5)[2] > ref.rows(Positive("term", (E,)), (S,), 0.5)[2]
    gl = [_gpu_leaf(fx) for fx in leaves]
    g = rucene_amd.GpuIndexSearcher(gl, ctx=ctxs("default"))
    try:
        for k in (10, 129):
            hits, totals = _check_batch(g, ref, queries, k, (index,))
            for i, q in enumerate(queries):
                if q[1] == (S,):
                    docs = hits[i]["doc"][hits[i]["doc"] >= 0]
                    assert not set(ss.leaf_of(leaves, docs).tolist()) & set(dropped), (index, k, q)
    finally:
        for leaf in gl:
            leaf.segment.close()


# ---- mixed batches and which kernel -------------------------------------------------------------------------------------------------
def _launches(c, name):
    st = c.kernel_stats()
    return st[name]["launches"] if name in st else 0


def test_mixed_batch_and_kernel_statistics(oracle):
    """Boosting queries between TERM, AND + MUST_NOT, OR, >= 10-clause OR and dismax queries of one search_batch: groups of their own
    (k_search_and_dem / k_or_windows_dem in the kernel statistics) - the other rows are byte for byte those of the same batch without
    them, which launches neither."""
    import rucene_amd
    T, B, D = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery
    fx = ss.Leaf(1025, "rank", "none")
    ref = BoostingRef(oracle, [fx])
    others = [B.build([T(t) for t in q.must], [T(t) for t in q.should], must_nots=[T(t) for t in q.must_not])
              for q in ss.TERMS + ss.ANDS + ss.NOTS + ss.ORS + ss.WIDE]
    others += [D([T(V), T(Q5)], 0.1), D([T(E), T(F), T(S)], 0.0)]
    boosting = [q for q in QUERIES if q[2] == 0.5]
    mixed, where_other, where_boosting = [], [], []
    for i, q in enumerate(others):
        if i < len(boosting):
            where_boosting.append(len(mixed))
            mixed.append(_bq(*boosting[i]))
        where_other.append(len(mixed))
        mixed.append(q)
    for j in range(len(where_boosting), len(boosting)):
        where_boosting.append(len(mixed))
        mixed.append(_bq(*boosting[j]))
    c = rucene_amd.Context(profile_kernels=True)
    try:
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
        for k in (10, 129):
            c.kernel_stats_reset()
            plain_h, plain_t = g.search_batch(others, k)
            assert _launches(c, "k_search_and_dem") == 0 and _launches(c, "k_or_windows_dem") == 0
            assert _launches(c, "k_search_and") > 0 and _launches(c, "k_or_windows") > 0 and _launches(c, "k_or_windows_max") > 0
            c.kernel_stats_reset()
            hits, totals = g.search_batch(mixed, k)
            passes = (k + 127) // 128
            assert _launches(c, "k_search_and_dem") == passes and _launches(c, "k_or_windows_dem") == passes
            assert hits[where_other].tobytes() == plain_h.tobytes() and totals[where_other].tolist() == plain_t.tolist(), k
            assert plain_t.sum() > 0
            for j, (p, n, b) in enumerate(boosting):
                i = where_boosting[j]
                check_row(hits[i], totals[i], ref, p, n, b, True, ("mixed", k, p, n, b))
        # a batch of TERM positives with demoting clauses alone never takes the TERM kernel
        c.kernel_stats_reset()
        g.search_batch([_bq(Positive("term", (E,)), (V,), 0.5), _bq(Positive("term", (Q5,)), (F,), 0.5)], 10)
        assert _launches(c, "k_search_and_dem") == 1 and _launches(c, "k_search_term") == 0 and _launches(c, "k_search_and") == 0
        leaf.segment.close()
    finally:
        c.close()


# ---- the C ABI's argument checks ----------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks(ctxs, oracle):
    import rucene_amd
    T, B, Bo = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.BoostingQuery
    nwd = rucene_amd.not_with_demote
    fx = ss.Leaf(257, "rank", "seeded")
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("default"))
    try:
        qs, ts = g.pack([Bo(B.build([T(V), T(E)], []), B.build([], [T(Q5), T(S)]), 0.5)], leaf)
        assert qs["op"][0] == 1 and qs["n_terms"][0] == 2 and qs["n_must_not"][0] == nwd(0, 2) and ts.size == 4

        def status(q=None, t=None):
            with pytest.raises(rucene_amd.RgpuError) as e:
                leaf.segment.search_batch(qs if q is None else q, ts if t is None else t, 10)
            return e.value.status

        def with_boost(b, at=(2, 3)):
            t = ts.copy()
            for i in at:
                t["weight"][i] = b
            return t

        def with_query(**fields):
            q = qs.copy()
            for name, v in fields.items():
                q[name][0] = v
            return q
        for b in (0.0, 1.0, -0.5, np.nan, np.inf):
            assert status(t=with_boost(b)) == -2, b                          # IllegalArgument
        assert status(t=with_boost(0.25, at=(3,))) == -2                     # differing boosts within one query
        assert status(q=with_query(n_must_not=nwd(0, 2) | (1 << 16))) == -2  # bits 16 and up
        assert status(q=with_query(n_must_not=nwd(0, 2) | (1 << 31) - (1 << 32))) == -2
        many_q, many_t = qs.copy(), np.concatenate([ts[:2]] + [ts[2:3]] * 63)
        many_q["n_must_not"][0] = nwd(0, 63)                                 # 2 + 63 clauses: over RGPU_MAX_QUERY_TERMS
        assert status(q=many_q, t=many_t) == -2
        many_q["n_must_not"][0] = nwd(33, 30)
        assert status(q=many_q, t=many_t) == -2
        many_q["n_must_not"][0] = nwd(65, 0)                                 # as before this field had a second byte
        assert status(q=many_q, t=many_t) == -2
        assert status(q=with_query(n_must_not=nwd(0, 3))) == -2              # the clause range leaves terms[]
        # demoting clauses with optional / nested clauses: UnsupportedOperation
        assert status(q=with_query(op=0 | (1 << 16), n_terms=1, n_must_not=nwd(0, 2))) == -5                     # RGPU_OP_WITH_SHOULD(TERM, 1)
        assert status(q=with_query(op=0 | (1 << 16) | (1 << 24), n_terms=1, n_must_not=nwd(0, 2))) == -5        # ... | SHOULD_REQUIRED
        four = np.concatenate([ts[:2], ts[:1], ts[2:]])
        assert status(q=with_query(op=0 | (2 << 16) | (1 << 25), n_terms=1, n_must_not=nwd(0, 2)), t=four) == -5  # ... | NESTED_MUST
        # the planner and the rescorer
        p = g._planner(leaf)
        with pytest.raises(rucene_amd.RgpuError) as e:
            p.plan_batch([1], [2], [V, E, Q5, S], [nwd(0, 2)])
        assert e.value.status == -5
        with pytest.raises(rucene_amd.RgpuError) as e:
            p.plan_batch([0, 2], [1, 2], [V, E, Q5, S, F], [0, nwd(1, 1)])
        assert e.value.status == -5
        first, _ = g.search_batch([T(V)], 10)
        with pytest.raises(rucene_amd.RgpuError) as e:
            g.rescore_batch(first, [Bo(T(E), T(Q5), 0.5)])
        assert e.value.status == -5
        # a refused call leaves the segment as it was: the query itself is served, and so is a boost next to the interval's lower end
        ref = BoostingRef(oracle, [fx])
        hits, totals = leaf.segment.search_batch(qs, ts, 10)
        check_row(hits[0], totals[0], ref, Positive("and", (V, E)), (Q5, S), 0.5, True, "after the refusals")
        tiny = float(np.finfo(np.float32).tiny)
        hits, totals = leaf.segment.search_batch(qs, with_boost(tiny), 10)
        check_row(hits[0], totals[0], ref, Positive("and", (V, E)), (Q5, S), tiny, True, "the smallest normal f32 as the boost")
    finally:
        leaf.segment.close()


# ---- record and merge ---------------------------------------------------------------------------------------------------------------
def test_record_and_merge(ctxs, oracle):
    """rgpu_search_batch_record_device per leaf, then rgpu_merge_records_device: the rows of search_batch over both leaves."""
    import torch
    import rucene_amd
    from rucene_amd import _lib as gpu
    leaves = [ss.Leaf(1025, "rank", "seeded", salt=1), ss.Leaf(129, "rank", "none", salt=1, doc_base=1025)]
    ref = BoostingRef(oracle, leaves)
    queries = [q for q in QUERIES if q[2] == 0.1]
    nq = len(queries)
    ctx = ctxs("default")
    gl = [_gpu_leaf(fx) for fx in leaves]
    g = rucene_amd.GpuIndexSearcher(gl, ctx=ctx)
    try:
        for k in (10, 129):
            rec = gpu.record_bytes(nq, k)
            recv = torch.zeros((2 * rec,), dtype=torch.uint8, device="cuda")
            for r, leaf in enumerate(gl):
                qs, ts = g.pack([_bq(*q) for q in queries], leaf)
                leaf.segment.search_batch_record_device(qs, ts, k, recv.data_ptr() + r * rec)
            hits = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
            totals = torch.zeros((nq,), dtype=torch.int64, device="cuda")
            ctx.merge_records_device(recv.data_ptr(), 2, nq, k, hits.data_ptr(), totals.data_ptr())
            ctx.synchronize()
            raw = recv.cpu().numpy()
            assert raw[rec - 8:rec].view(np.int64)[0] == 0 and raw[2 * rec - 8:].view(np.int64)[0] == 0    # both shards: status OK
            got = hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(nq, k)
            tot = totals.cpu().numpy()
            want_h, want_t = g.search_batch([_bq(*q) for q in queries], k)
            assert got.tobytes() == want_h.tobytes() and tot.tolist() == want_t.tolist(), k
            for i, (p, n, b) in enumerate(queries):
                check_row(got[i], tot[i], ref, p, n, b, True, ("record + merge", k, p, n, b))
    finally:
        for leaf in gl:
            leaf.segment.close()


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------
def test_cpp_demo_rows_equal_the_python_mirror(ctxs, oracle, tmp_path):
    """tests/cpp/boosting_demo.cpp: rucene::BoostingQuery through csrc/host/gpu_index_searcher.hpp on the 1025-doc rank-mode leaf - the
    lines it prints are the Python mirror's rows, which are the reference's."""
    import os
    import subprocess
    import rucene_amd
    T = rucene_amd.TermQuery
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "boosting_demo")
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "cpp", "boosting_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    fx = ss.Leaf(1025, "rank", "none")
    for name, blob in (("doc", fx.seg.doc_bytes), ("norms", fx.norms), ("terms", np.ascontiguousarray(fx.seg.terms, dtype=rucene_amd.TERM_STATE_DTYPE))):
        (tmp_path / (name + ".bin")).write_bytes(np.asarray(blob).tobytes())
    out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.max_doc), str(fx.sttf)], text=True).strip().splitlines()
    specs = [(Positive("term", (E,)), (V,), 0.1), (Positive("term", (Q5,)), (F,), 0.5), None, (Positive("and", (E, V, C)), (A, Q5), 0.5),
             (Positive("or", (V, Q5, S), msm=2), (E,), BOOSTS[2]), (Positive("or", (E, L, V, Q5, A, S, C, V, Q5), must_not=(F,)), (V, Q5), 0.1),
             (Positive("term", (E,)), (A,), 0.5)]
    queries = [T(S) if q is None else _bq(*q) for q in specs]
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("default"))
    try:
        hits, totals = g.search_batch(queries, 10)
    finally:
        leaf.segment.close()
    assert len(out) == len(queries) + 1
    for i, line in enumerate(out):
        j = i if i < len(queries) else 0              # the last line: queries[0] through search() and a collector
        parts = line.split()
        assert parts[0] == "boosting" and int(parts[1]) == i and int(parts[2]) == totals[j], line
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        n = min(10, int(totals[j]))
        assert [x[0] for x in got] == hits[j]["doc"][:n].tolist(), line
        assert [x[1] for x in got] == hits[j]["score"][:n].view(np.uint32).tolist(), line
    assert totals[6] == 0 and totals[0] > 10
    ref = BoostingRef(oracle, [fx])
    for i, q in enumerate(specs):
        if q is not None:
            check_row(hits[i], totals[i], ref, q[0], q[1], q[2], True, ("the demo's query", i))
