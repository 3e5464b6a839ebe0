"""Hit counts without scoring on the GPU (`-m gpu`): rgpu_count_batch against the numpy model of tests/count.py AND against the totals
of rgpu_search_batch / rgpu_search_batch_masked for the same arrays - every comparison exact - with the answering path read from
rgpu_kernel_stats; then the Python mirror and the C++ demo. Segments hold at most 3 W + 37 docs, W = COUNT_WINDOW_DOCS.

One rule is worth restating here because it is easy to get wrong: two present MUST_NOT clauses under min_should_match 2 exclude every
doc EITHER holds, not only the docs both hold - ReqNotScorer advance()s the prohibited DisjunctionSumScorer, and advance() never
looks at the count (disjunction_scorer.rs:75-89). That is what the oracle and
rgpu_search_batch report (tests/test_count_cpu.py), and counts equal those totals by contract."""
import os
import subprocess

import numpy as np
import pytest

import count as ct
import segment_spectrum as ss
from count import A, ABSENT, ALL, AND, B, C, CQ, EQ1, OR, T, W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KERNELS = ("k_count_lists", "k_count_windows", "k_count_emitted", "k_search_and(count candidates)")


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


def _sim_table(c):
    from rucene_amd import _lib as gpu
    _w, _idf, cache = gpu.bm25_compute_weight(1.2, 0.75, 1000, 1000, 60000, [10], 1.0)
    return c.sim_table(cache, 1.2)


def _segment(c, fx, alive=None, index_options=2, doc_bytes=None):
    import rucene_amd
    return rucene_amd.Segment(c, fx.seg.doc_bytes if doc_bytes is None else doc_bytes, fx.norms, fx.max_doc,
                              live_docs=None if alive is None else ss.live_words(alive), index_options=index_options)


def _launches(c):
    st = c.kernel_stats()
    return {k: (st[k]["launches"] if k in st else 0) for k in COUNT_KERNELS}


def _check(c, seg, fx, rows, alive=None, docset=None, terms=None, what=""):
    """counts == the model == the search's totals, row by row; -> the launches of the count kernels the call made"""
    from rucene_amd import _lib as gpu
    qs, ts = ct.pack(fx.terms if terms is None else terms, rows, gpu, sim_table=_sim_table(c))
    ds = None if docset is None else seg.docset_from_words(ss.live_words(docset))
    try:
        before = _launches(c)
        got = seg.count_batch(qs, ts, ds)
        after = _launches(c)
        _, totals = seg.search_batch(qs, ts, 1) if ds is None else seg.search_batch_masked(ds, qs, ts, 1)
    finally:
        if ds is not None:
            ds.close()
    mask = ct.mask_of(fx.max_doc, alive, docset)
    want = [ct.model_count(fx.has, fx.df, mask, q) for q in rows]
    assert got.dtype == np.int64
    for i, q in enumerate(rows):
        assert int(got[i]) == want[i] == int(totals[i]), (what, i, q, "count", int(got[i]), "model", want[i], "search", int(totals[i]))
    return {k: after[k] - before[k] for k in COUNT_KERNELS}


def _from_ss(q):
    if q.must:
        return CQ("term" if len(q.must) == 1 else "and", tuple(q.must), tuple(q.must_not))
    return CQ("or", tuple(q.should), tuple(q.must_not), q.msm)


class _SsLeaf:
    """a segment_spectrum.Leaf with the fields _check reads"""

    def __init__(self, max_doc):
        self.leaf = ss.Leaf(max_doc, "rank", "none")
        self.seg, self.norms, self.max_doc, self.has, self.terms = self.leaf.seg, self.leaf.norms, max_doc, self.leaf.has, self.leaf.seg.terms
        self.df = np.array([d.size for d, _ in self.leaf.lists])


# ---- windows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc", [1, 63, 64, 65, W - 1, W, W + 1])
def test_segment_sizes(ctx, max_doc):
    """the vocabulary of tests/segment_spectrum.py (every doc, doc 0, the last doc, every second, a fifth, absent ...) on leaves on both
    sides of a live word and of a window, plain, under deletions and under a set"""
    fx = _SsLeaf(max_doc)
    rows = [_from_ss(q) for q in ss.TERMS + ss.ANDS + ss.ORS + ss.NOTS + ss.MSM2 if bool(q.must) != bool(q.should) and not q.filt]
    rows += [OR(ss.EVERY, ss.EVEN, ss.FIFTH, msm=2), OR(ss.FIRST, ss.LAST, ss.EVEN, nots=(ss.FIFTH,)), T(ss.EVERY, nots=(ss.EVEN,))]
    for name in ("none", "first-deleted", "last-deleted", "seeded-deleted", "set", "set-under-deletions"):
        alive, docset = ct.masks(max_doc)[name]
        seg = _segment(ctx, fx, alive)
        try:
            _check(ctx, seg, fx, rows, alive, docset, what=(max_doc, name))
        finally:
            seg.close()


@pytest.mark.parametrize("per_item", [1, 2, 1000])
def test_window_edges_and_windows_per_item(monkeypatch, per_item):
    """every edge list of the WINDOW leaf (max_doc 2 W + 37: a short last window) through k_count_windows, with 1, 2 and all windows per
    work item (RGPU_COUNT_WINDOWS_PER_ITEM, read when the context is made)"""
    import rucene_amd
    monkeypatch.setenv("RGPU_COUNT_WINDOWS_PER_ITEM", str(per_item))
    c = rucene_amd.Context(profile_kernels=True)
    try:
        fx = ct.window_leaf()
        for name in ("none", "seeded-deleted", "set-under-deletions"):
            alive, docset = ct.masks(fx.max_doc)[name]
            seg = _segment(c, fx, alive)
            try:
                ran = _check(c, seg, fx, ct.WINDOW_ROWS, alive, docset, what=(per_item, name))
                assert ran["k_count_windows"] == 1 and ran["k_count_lists"] == 0 and ran["k_count_emitted"] == 0, ran
            finally:
                seg.close()
    finally:
        c.close()


@pytest.mark.parametrize("n_rows", [2047, 2048, 2049])
def test_many_rows(ctx, n_rows):
    fx = ct.window_leaf()
    some = [OR(A, B), OR(ct.EDGE, ct.SPARSE, ABSENT), T(C, nots=(A,)), OR(A, B, C, msm=2), OR(ct.SLAST, ct.S0)]
    rows = [some[i % len(some)] for i in range(n_rows)]
    seg = _segment(ctx, fx)
    try:
        ran = _check(ctx, seg, fx, rows, what=n_rows)
        assert ran["k_count_windows"] == 1
    finally:
        seg.close()


# ---- thresholds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["none", "seeded-deleted", "set"])
def test_thresholds(ctx, mask):
    """msm 0 | 1 | 2 | n | n + 1; a repeated term counted twice; 63 | 64 clauses that all hold one doc under msm 64; MUST_NOT with one
    present clause, with two under msm 2, with one present and one absent; every doc prohibited; an OR of MUST_NOT clauses only; every
    SHOULD clause absent"""
    fx = ct.window_leaf()
    alive, docset = ct.masks(fx.max_doc)[mask]
    seg = _segment(ctx, fx, alive)
    try:
        ran = _check(ctx, seg, fx, ct.THRESHOLD_ROWS, alive, docset, what=mask)
        assert ran["k_count_windows"] == 1 and ran["k_count_emitted"] == 0, ran
    finally:
        seg.close()


# ---- conjunctions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["none", "seeded-deleted", "set", "set-under-deletions"])
def test_conjunctions(ctx, mask):
    """2 and 3 clauses, an absent MUST, +a -a, +a +a, a tail-only and a singleton lead, equal doc_freqs, MUST_NOT clauses - plain, under
    deletions and under a set: k_search_and in emit mode, then k_count_emitted"""
    fx = ct.window_leaf()
    alive, docset = ct.masks(fx.max_doc)[mask]
    seg = _segment(ctx, fx, alive)
    try:
        ran = _check(ctx, seg, fx, ct.CONJ_ROWS, alive, docset, what=mask)
        assert ran["k_count_emitted"] == 1 and ran["k_search_and(count candidates)"] == 1 and ran["k_count_windows"] == 0, ran
    finally:
        seg.close()


def test_a_conjunction_needs_a_similarity_table():
    import rucene_amd
    from rucene_amd import _lib as gpu
    c = rucene_amd.Context()
    try:
        fx = ct.window_leaf()
        seg = _segment(c, fx)
        try:
            qs, ts = ct.pack(fx.terms, [OR(A, B), AND(A, C)], gpu)
            with pytest.raises(rucene_amd.RgpuError) as e:
                seg.count_batch(qs, ts)
            assert e.value.status == -1
            assert seg.count_batch(qs[:1], ts).tolist() == [ct.model_count(fx.has, fx.df, np.ones(fx.max_doc, bool), OR(A, B))]   # the union needs none
        finally:
            seg.close()
    finally:
        c.close()


# ---- TERM ------------------------------------------------------------------------------------------------------------------------------
def test_doc_freq_rows_launch_nothing(ctx):
    fx = ct.window_leaf()
    seg = _segment(ctx, fx)
    try:
        _check(ctx, seg, fx, ct.WINDOW_ROWS[:3])      # (the terms are prepared and the searches' kernels have run once)
        before = {k: v["launches"] for k, v in ctx.kernel_stats().items()}
        from rucene_amd import _lib as gpu
        qs, ts = ct.pack(fx.terms, ct.TERM_ROWS + [AND(A, ABSENT), OR(ABSENT, ABSENT)], gpu, sim_table=_sim_table(ctx))
        got = seg.count_batch(qs, ts)
        assert {k: v["launches"] for k, v in ctx.kernel_stats().items()} == before        # DOC_FREQ and ZERO rows alone: the host knows
        every = np.ones(fx.max_doc, bool)
        assert got.tolist() == [ct.model_count(fx.has, fx.df, every, q) for q in ct.TERM_ROWS] + [0, 0]
        ran = _check(ctx, seg, fx, ct.TERM_ROWS)
        assert not any(ran.values()), ran
    finally:
        seg.close()


@pytest.mark.parametrize("mask", ["first-deleted", "last-deleted", "seeded-deleted", "all-deleted", "set", "set-under-deletions"])
def test_list_rows(ctx, mask):
    fx = ct.window_leaf()
    alive, docset = ct.masks(fx.max_doc)[mask]
    seg = _segment(ctx, fx, alive)
    try:
        ran = _check(ctx, seg, fx, ct.TERM_ROWS, alive, docset, what=mask)
        assert ran["k_count_lists"] == 1 and ran["k_count_windows"] == 0 and ran["k_count_emitted"] == 0, ran
    finally:
        seg.close()


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
def test_masks(ctx):
    """the empty set (every row ZERO: nothing launched), every doc, a set under deletions; a set of another segment is refused"""
    import rucene_amd
    from rucene_amd import _lib as gpu
    fx = ct.window_leaf()
    rows = ct.WINDOW_ROWS[-6:] + ct.CONJ_ROWS[:4] + ct.TERM_ROWS[:4] + ct.THRESHOLD_ROWS[:5]
    for name in ("empty-set", "every-doc-set", "set-under-deletions"):
        alive, docset = ct.masks(fx.max_doc)[name]
        seg = _segment(ctx, fx, alive)
        try:
            ran = _check(ctx, seg, fx, rows, alive, docset, what=name)
            assert (not any(ran.values())) == (name == "empty-set"), (name, ran)
        finally:
            seg.close()
    seg, other = _segment(ctx, fx), _segment(ctx, fx)
    try:
        foreign = other.docset_from_words(ss.live_words(np.ones(fx.max_doc, bool)))
        qs, ts = ct.pack(fx.terms, rows, gpu, sim_table=_sim_table(ctx))
        out = np.full(len(rows), -7, np.int64)
        rc = gpu.lib().rgpu_count_batch(seg._h, foreign._h, qs.ctypes.data, qs.size, ts.ctypes.data, ts.size, out.ctypes.data)
        assert rc == -2 and (out == -7).all()
        foreign.close()
    finally:
        seg.close()
        other.close()


# ---- bitmaps ---------------------------------------------------------------------------------------------------------------------------
def test_decoded_and_bitmap_clauses_agree(ctx):
    """the same union rows before any doc bitmap exists (every clause decoded) and after a search has built them (TermBitmap::memb read)"""
    from rucene_amd import _lib as gpu
    fx = ct.window_leaf()
    rows = [OR(A, C), OR(A, B, C, ALL), OR(C, ct.SPARSE, nots=(A,)), T(ALL, nots=(C,)), OR(A, C, ct.EDGE, ct.TAIL127, nots=(ALL,)), CQ("dismax", (C, A))]
    for name in ("none", "seeded-deleted"):
        alive, docset = ct.masks(fx.max_doc)[name]
        seg = _segment(ctx, fx, alive)
        try:
            qs, ts = ct.pack(fx.terms, rows, gpu, sim_table=_sim_table(ctx))
            first = seg.count_batch(qs, ts)
            assert seg.footprint()["doc_bitmap_bytes"] == 0
            aq, at = ct.pack(fx.terms, [AND(A, C), AND(B, ALL), AND(A, C, ALL)], gpu, sim_table=_sim_table(ctx))
            seg.search_batch(aq, at, 10)      # conjunctions of dense clauses: the search builds their doc bitmaps
            assert seg.footprint()["doc_bitmap_bytes"] > 0
            ran = _check(ctx, seg, fx, rows, alive, what=name)
            assert ran["k_count_windows"] == 1
            assert seg.count_batch(qs, ts).tolist() == first.tolist()
        finally:
            seg.close()


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["none", "seeded-deleted"])
def test_dismax_optional_and_demoting_clauses(ctx, mask):
    fx = ct.window_leaf()
    alive, docset = ct.masks(fx.max_doc)[mask]
    seg = _segment(ctx, fx, alive)
    try:
        _check(ctx, seg, fx, ct.ABI_ROWS, alive, what=mask)
    finally:
        seg.close()


def test_refusals(ctx):
    import rucene_amd
    from rucene_amd import _lib as gpu
    fx = ct.window_leaf()
    seg = _segment(ctx, fx)
    try:
        base = [CQ("and", (A, C), opt=(B, EQ1)), OR(A, B, C)]
        qs, ts = ct.pack(fx.terms, base, gpu, sim_table=_sim_table(ctx))
        seg.count_batch(qs, ts)
        before = {k: v["launches"] for k, v in ctx.kernel_stats().items()}

        def refused(row, field, value):
            q2 = qs.copy()
            q2[row][field] = value
            out = np.full(2, -7, np.int64)
            rc = gpu.lib().rgpu_count_batch(seg._h, None, q2.ctypes.data, q2.size, ts.ctypes.data, ts.size, out.ctypes.data)
            assert (out == -7).all()
            with pytest.raises(rucene_amd.RgpuError) as e:     # the same row is refused by the search with the same code, or served
                seg.search_batch(q2, ts, 1)
            assert e.value.status == rc or rc == -5
            return rc
        assert refused(1, "n_terms", 70) == -2 and refused(1, "first_term", int(ts.size) - 2) == -2 and refused(1, "n_must_not", 1 << 16) == -2
        assert refused(1, "op", 7) == -2 and refused(0, "op", gpu.OP_AND | (2 << 8)) == -2 and refused(1, "op", gpu.OP_OR | (1 << 16)) == -2
        assert refused(1, "op", gpu.OP_DISMAX | (1 << 8)) == -2
        out = np.full(2, -7, np.int64)
        for op in (gpu.OP_AND | (2 << 16) | gpu.OP_SHOULD_REQUIRED, gpu.OP_AND | (2 << 16) | gpu.OP_NESTED_MUST):
            q2 = qs.copy()
            q2[0]["op"] = op
            assert gpu.lib().rgpu_count_batch(seg._h, None, q2.ctypes.data, q2.size, ts.ctypes.data, ts.size, out.ctypes.data) == -5 and (out == -7).all()
        assert {k: v["launches"] for k, v in ctx.kernel_stats().items()} == before     # nothing was launched
    finally:
        seg.close()


@pytest.mark.parametrize("variant", ["raw-norms", "no-norms", "legacy", "docs-only"])
def test_norm_modes_formats_and_a_docs_only_field(ctx, oracle, variant):
    norms = {"raw-norms": "raw", "no-norms": "none"}.get(variant, "rank")
    fx = ct.window_leaf(version=0 if variant == "legacy" else 1, norms=norms)
    terms, doc_bytes, index_options = fx.terms, None, 2
    if variant == "docs-only":
        w = oracle.Writer(fx.max_doc, version=1, write_freqs=False)
        terms = np.zeros(len(fx.lists), dtype=oracle.TERM_STATE_DTYPE)
        terms["skip_offset"], terms["singleton_doc_id"] = -1, -1
        for t, (d, _) in enumerate(fx.lists):
            if d.size:
                terms[t] = w.write_term(d, np.ones_like(d))
        doc_bytes = np.frombuffer(bytes(w.close()), np.uint8).copy()
        terms["total_term_freq"] = -1
        index_options = 1
    rows = ct.WINDOW_ROWS + ct.THRESHOLD_ROWS[:8] + ct.CONJ_ROWS + ct.TERM_ROWS
    for name in ("none", "seeded-deleted"):
        alive, docset = ct.masks(fx.max_doc)[name]
        seg = _segment(ctx, fx, alive, index_options=index_options, doc_bytes=doc_bytes)
        try:
            _check(ctx, seg, fx, rows, alive, terms=terms, what=(variant, name))
        finally:
            seg.close()


# ---- mirrors ---------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(ctx):
    """four leaves, one of which lacks a case's terms; the two no-launch shortcuts; grouped doc-set rows; a _RequiredSet row; the
    fallback hook receiving a phrase and a span query"""
    import rucene_amd as ra
    lists = ct.window_lists()
    hollow = [(np.zeros(0, np.int32), np.zeros(0, np.int32)) if t in (A, B) else lists[t] for t in range(len(lists))]
    leaves_fx = [ct.Leaf(ct.MAX_DOC, lists), ct.Leaf(ct.MAX_DOC, hollow), ct.Leaf(ct.MAX_DOC, lists), ct.Leaf(ct.MAX_DOC, lists)]
    TQ, BQ = ra.TermQuery, ra.BooleanQuery
    queries = [(TQ(A), T(A)), (BQ.build([TQ(A), TQ(C)], []), AND(A, C)), (BQ.build([], [TQ(A), TQ(B), TQ(C)], min_should_match=2), OR(A, B, C, msm=2)),
               (BQ.build([], [TQ(A), TQ(B)], must_nots=[TQ(C)]), OR(A, B, nots=(C,))), (BQ.build([TQ(C)], [], must_nots=[TQ(A)]), T(C, nots=(A,))),
               (ra.DisjunctionMaxQuery([TQ(A), TQ(ct.SPARSE)], 0.1), CQ("dismax", (A, ct.SPARSE))), (TQ(ABSENT), T(ABSENT))]
    for deleted in (False, True):
        alives = [ct.seeded(ct.MAX_DOC, 10 + i) if deleted else None for i in range(4)]
        base, leaves = 0, []
        for fx, alive in zip(leaves_fx, alives):
            s = fx.seg
            leaves.append(ra.LeafReader(s.doc_bytes, fx.norms, fx.max_doc, s.terms, doc_base=base, live_docs=None if alive is None else ss.live_words(alive),
                                        sum_total_term_freq=fx.sttf))
            base += fx.max_doc
        searcher = ra.GpuIndexSearcher(leaves, ctx=ctx, required_sets=True)
        masks = [np.ones(ct.MAX_DOC, bool) if a is None else a for a in alives]
        want = lambda q, extra=None: sum(ct.model_count(fx.has, fx.df, m if extra is None else m & extra[i], q) for i, (fx, m) in enumerate(zip(leaves_fx, masks)))
        got = searcher.count_batch([q for q, _ in queries])
        assert got.dtype == np.int64 and got.tolist() == [want(cq) for _, cq in queries], deleted
        _, totals = searcher.search_batch([q for q, _ in queries], 1)
        assert got.tolist() == np.asarray(totals).tolist()
        # the shortcuts: no GPU call at all
        before = {k: v["launches"] for k, v in ctx.kernel_stats().items()}
        assert searcher.count(ra.MatchAllDocsQuery()) == sum(int(m.sum()) for m in masks)
        if not deleted:
            assert searcher.count(TQ(A)) == want(T(A)) == 3 * 700
        assert {k: v["launches"] for k, v in ctx.kernel_stats().items()} == before
        assert searcher.count(queries[2][0]) == want(queries[2][1])
        # doc-set rows, grouped by their combination of sets; a row whose only required clause is a set matches all of it
        f1, f2 = searcher.cache_filter(TQ(C)), searcher.cache_filter(TQ(EQ1))
        in_c, in_e = [fx.has[C] for fx in leaves_fx], [fx.has[EQ1] for fx in leaves_fx]
        grouped = [BQ.build([TQ(A)], [], filters=[f1]), BQ.build([], [TQ(A), TQ(B)], must_nots=[f2]), BQ.build([TQ(A)], [TQ(B)], filters=[f1]),
                   BQ.build([], [TQ(A), TQ(B)], filters=[f1]), TQ(A)]
        got = searcher.count_batch(grouped)
        not_e = [~m for m in in_e]
        assert got.tolist() == [want(T(A), in_c), want(OR(A, B), not_e), want(T(A), in_c), sum(int((m & c).sum()) for m, c in zip(masks, in_c)), want(T(A))]
        _, totals = searcher.search_batch(grouped, 1)
        assert got.tolist() == np.asarray(totals).tolist()
        # what the GPU path refuses goes to the hook
        seen = []
        phrase, span = ra.PhraseQuery([A, B]), ra.SpanNearQuery([ra.SpanTermQuery(A), ra.SpanTermQuery(B)], 0, True)
        for q in (phrase, span):
            with pytest.raises(ra.RgpuError) as e:
                searcher.count(q)
            assert e.value.status == -5
        searcher.cpu_count_fallback = lambda q: seen.append(q) or 41
        assert searcher.count(phrase) == 41 and searcher.count(span) == 41 and seen == [phrase, span]


def test_cpp_demo(tmp_path):
    """tests/cpp/count_demo.cpp: count / count_many of the C++ mirror over two WINDOW leaves (one with deletions), held against the model"""
    fx = ct.window_leaf()
    alives = [None, ct.seeded(fx.max_doc, 20)]
    args = [str(tmp_path), "2"]
    for i, alive in enumerate(alives):
        d = tmp_path / ("leaf%d" % i)
        d.mkdir()
        (d / "doc.bin").write_bytes(np.ascontiguousarray(fx.seg.doc_bytes, np.uint8).tobytes())
        (d / "norms.bin").write_bytes(fx.norms.tobytes())
        (d / "terms.bin").write_bytes(np.ascontiguousarray(fx.terms).tobytes())
        (d / "live.bin").write_bytes(b"" if alive is None else ss.live_words(alive).tobytes())
        args += [str(fx.max_doc), str(fx.sttf)]
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "count_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "count_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("count_demo OK"), out.stdout
    rows = [T(A), AND(A, C), OR(A, B, C, msm=2), OR(A, B, nots=(C,)), T(C, nots=(A,)), OR(ct.EDGE, ct.SPARSE, ct.SLAST, ABSENT), T(ABSENT)]
    masks = [np.ones(fx.max_doc, bool) if a is None else a for a in alives]
    want = [sum(ct.model_count(fx.has, fx.df, m, q) for m in masks) for q in rows] + [sum(int(m.sum()) for m in masks)]
    got = [int(line.split()[2]) for line in out.stdout.splitlines() if line.startswith("count ")]
    assert got == want, out.stdout
