"""Doc sets on the GPU through the C ABI (`-m gpu`): construction and round trip, rgpu_docset_collect_batch against the numpy
reference of tests/docset.py, rgpu_docset_combine, and the masked search entry points - bit for bit against rgpu_search_batch on a
twin segment uploaded with live AND set, and against the oracle on those live docs under the rules the existing suite applies
(exact; disjunctions of ten or more clauses with min_should_match <= 1 under oracle/parity.py's rule, on tests/or_spectrum.py's
fixtures). tests/test_docset_cpu.py proves on the CPU that a search on fewer live docs IS the filtered query."""
import numpy as np
import pytest

import docset as ds
import or_spectrum as os_
import segment_spectrum as ss
from test_gpu_norm_spectrum import _assert_row
from test_gpu_segment_spectrum import _check_rows, _gpu_query, _is_wide

pytestmark = pytest.mark.gpu

LIVE = ("none", "seeded")


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


def _sim_table(c):
    """any similarity table: collecting a conjunction runs the search's conjunction kernel, which loads its lead's table"""
    from rucene_amd import _lib as gpu
    _w, _idf, cache = gpu.bm25_compute_weight(1.2, 0.75, 1000, 1000, 60000, [10], 1.0)
    return c.sim_table(cache, 1.2)


def _segment(c, fx, live_docs="own", index_options=2, doc_bytes=None):
    import rucene_amd
    return rucene_amd.Segment(c, fx.seg.doc_bytes if doc_bytes is None else doc_bytes, fx.norms, fx.max_doc,
                              live_docs=fx.live_docs if isinstance(live_docs, str) else live_docs, index_options=index_options)


def _words(mask):
    return ss.live_words(mask)


def _same_rows(a, b, what):
    assert a[0]["doc"].tolist() == b[0]["doc"].tolist(), (what, "docs")
    assert a[0]["score"].view(np.int32).tolist() == b[0]["score"].view(np.int32).tolist(), (what, "score bits")
    assert np.asarray(a[1]).tolist() == np.asarray(b[1]).tolist(), (what, "totals")


# ---- construction and round trip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc", [1, 63, 64, 65, 127, 128, 129, 8193])
def test_construction_and_round_trip(ctx, max_doc):
    import rucene_amd
    fx = ss.Leaf(max_doc, "rank", "none")
    seg = _segment(ctx, fx)
    try:
        n_words = (max_doc + 63) // 64
        first, last = np.zeros(max_doc, bool), np.zeros(max_doc, bool)
        first[0], last[-1] = True, True
        rng = np.random.default_rng([max_doc, 70])
        some = rng.random(max_doc) < 0.4
        for name, m in (("empty", np.zeros(max_doc, bool)), ("full", np.ones(max_doc, bool)), ("first", first), ("last", last), ("some", some)):
            a = seg.docset_from_words(_words(m))
            ids = np.flatnonzero(m).astype(np.int32)
            shuffled = rng.permutation(np.concatenate([ids, ids[::2], ids[:1]]))     # unsorted, with repeats
            b = seg.docset_from_docs(shuffled)
            for s in (a, b):
                w = s.words()
                assert w.size == n_words and (w == _words(m)).all(), (max_doc, name)
                assert s.cardinality == int(m.sum()) and s.nbytes >= 8 * n_words, (max_doc, name)
            a.close()
            b.close()
        if max_doc % 64:   # (a whole last word has no bit past max_doc to set)
            bad = _words(np.ones(max_doc, bool)).copy()
            bad[-1] |= np.uint64(1) << np.uint64(max_doc % 64)
            with pytest.raises(rucene_amd.RgpuError) as e:
                seg.docset_from_words(bad)
            assert e.value.status == -2
            bad[-1] = np.uint64(1) << np.uint64(63)
            with pytest.raises(rucene_amd.RgpuError) as e:
                seg.docset_from_words(bad)
            assert e.value.status == -2
        for docs in ([0, max_doc], [-1], [max_doc - 1, 2**31 - 1, 0]):
            with pytest.raises(rucene_amd.RgpuError) as e:
                seg.docset_from_docs(np.array(docs, np.int32))
            assert e.value.status == -2, docs
        assert seg.docset_from_docs(np.zeros(0, np.int32)).cardinality == 0
        assert "doc_bitmap_bytes" in seg.footprint()   # (doc sets are not part of the segment's footprint: rgpu_docset_bytes)
    finally:
        seg.close()


# ---- collect_batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("live", LIVE)
@pytest.mark.parametrize("fmt", ["bp128", "legacy", "docs-only"])
def test_collect_batch_against_the_numpy_reference(ctx, oracle, fmt, live):
    """TERM over lists of 1, 127, 128, 129, 2176, 2304 postings and one that holds every second doc; AND of two and three clauses
    (the lead first / last, a clause absent, a dense clause, a repeated term); OR of 1, 9, 10 and 16 clauses; each with 0, 1 and 2
    MUST_NOT clauses - both .doc formats and a docs-only field, with and without deletions: deleted docs stay in the set."""
    import rucene_amd
    from rucene_amd import _lib as gpu
    fx = ds.collect_leaf(0 if fmt == "legacy" else 1)
    alive = None if live == "none" else ds.seeded_alive(fx.max_doc)
    terms, doc_bytes, index_options = fx.terms, fx.seg.doc_bytes, 2
    if fmt == "docs-only":
        doc_bytes, terms = ds.collect_docs_only(oracle)
        index_options = 1
    seg = rucene_amd.Segment(ctx, doc_bytes, fx.norms, fx.max_doc, live_docs=None if alive is None else _words(alive), index_options=index_options)
    try:
        table = _sim_table(ctx)
        ctx.kernel_stats_reset()
        for name, queries, as_and in (("all", ds.COLLECT_QUERIES, False), ("one-clause conjunctions", ds.COLLECT_TERMS, True)):
            qs, ts = ds.pack(terms, queries, gpu, sim_table=table, as_and=as_and)
            sets = seg.docset_collect_batch(qs, ts)
            assert len(sets) == len(queries)
            for q, s in zip(queries, sets):
                want = ds.ref_set(fx.has, q)
                got = s.words()
                assert (got == _words(want)).all(), (fmt, live, name, q, "docs differing", np.flatnonzero(np.unpackbits(got.view(np.uint8), bitorder="little")[:fx.max_doc] != want)[:10])
                assert s.cardinality == int(want.sum()), (fmt, live, name, q)
            if alive is not None:   # deleted docs stay in the set
                dense = sets[queries.index(ss.Query(must=(ds.DENSE,)))]
                assert dense.cardinality == fx.lists[ds.DENSE][0].size > int((fx.has[ds.DENSE] & alive).sum())
            for s in sets:
                s.close()
        st = ctx.kernel_stats()
        for kernel in ("k_docset_lists", "k_docset_from_emitted", "k_docset_combine"):
            assert kernel in st and st[kernel]["launches"] > 0, (kernel, sorted(st))
    finally:
        seg.close()


def test_collect_batch_refusals(ctx):
    import rucene_amd
    from rucene_amd import _lib as gpu
    fx = ds.collect_leaf(1)
    seg = _segment(ctx, fx, live_docs=None)
    try:
        table = _sim_table(ctx)
        base = [ss.Query(must=(ds.DF129, ds.MID)), ss.Query(should=(ds.R[0], ds.R[1], ds.R[2]))]
        qs, ts = ds.pack(fx.terms, base, gpu, sim_table=table)
        for s in seg.docset_collect_batch(qs, ts):
            s.close()

        def refused(change):
            q2 = qs.copy()
            change(q2)
            with pytest.raises(rucene_amd.RgpuError) as e:
                seg.docset_collect_batch(q2, ts)
            return e.value.status

        def set_(row, field, value):
            def go(q):
                q[row][field] = value
            return go
        assert refused(set_(1, "op", gpu.OP_DISMAX)) == -5                                   # another op
        assert refused(set_(1, "op", gpu.OP_OR | (2 << 8))) == -5                            # min_should_match >= 2
        assert refused(set_(0, "n_must_not", gpu.not_with_demote(0, 1))) == -5               # a demote byte
        assert refused(set_(0, "op", gpu.OP_AND | (1 << 16))) == -5                          # RGPU_OP_WITH_SHOULD
        assert refused(set_(0, "op", gpu.OP_AND | (1 << 16) | gpu.OP_SHOULD_REQUIRED)) == -5
        assert refused(set_(0, "op", gpu.OP_AND | (2 << 16) | gpu.OP_NESTED_MUST)) == -5
        assert refused(set_(0, "n_terms", 70)) == -2 and refused(set_(1, "first_term", 4)) == -2
    finally:
        seg.close()


# ---- combine --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc", [65, 8193])
def test_combine(ctx, max_doc):
    fx = ss.Leaf(max_doc, "rank", "none")
    seg = _segment(ctx, fx)
    try:
        rng = np.random.default_rng([max_doc, 71])
        masks = [rng.random(max_doc) < p for p in (0.7, 0.6, 0.8, 0.3, 0.2)]
        sets = [seg.docset_from_words(_words(m)) for m in masks]
        for n_all in range(4):
            for n_none in range(3):
                want = np.ones(max_doc, bool)
                for m in masks[:n_all]:
                    want &= m
                for m in masks[3:3 + n_none]:
                    want &= ~m
                got = seg.docset_combine(sets[:n_all], sets[3:3 + n_none])
                w = got.words()
                assert (w == _words(want)).all() and got.cardinality == int(want.sum()), (max_doc, n_all, n_none)
                assert int(w[-1]) >> (max_doc % 64) == 0   # n_all = 0: the tail bits past max_doc stay clear
                got.close()
        # more operands than one launch takes on a side
        many = [seg.docset_from_words(_words(rng.random(max_doc) < 0.97)) for _ in range(19)]
        want = np.ones(max_doc, bool)
        for s in many[:18]:
            want &= np.unpackbits(s.words().view(np.uint8), bitorder="little")[:max_doc].astype(bool)
        got = seg.docset_combine(many[:18], [many[18]])
        want &= ~np.unpackbits(many[18].words().view(np.uint8), bitorder="little")[:max_doc].astype(bool)
        assert (got.words() == _words(want)).all() and got.cardinality == int(want.sum())
    finally:
        seg.close()


# ---- masked parity ----------------------------------------------------------------------------------------------------------------
class _Masked:
    """One fixture leaf on the GPU, a doc set on it, and its twin: the same files uploaded with live AND set"""

    def __init__(self, c, oracle, fx, mask):
        import rucene_amd
        self.fx, self.mask = fx, mask
        self.leaf = rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, live_docs=fx.live_docs, sum_total_term_freq=fx.sttf)
        self.g = rucene_amd.GpuIndexSearcher([self.leaf], ctx=c)
        self.seg = self.leaf.segment
        self.set = self.seg.docset_from_words(_words(mask))
        self.alive = fx.alive & mask
        self.twin = rucene_amd.Segment(c, fx.seg.doc_bytes, fx.norms, fx.max_doc, live_docs=_words(self.alive))
        self.osr = oracle.Searcher([oracle.Segment(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, live_docs=_words(self.alive), sum_total_term_freq=fx.sttf)])

    def both(self, queries, k, what):
        """masked on the leaf, unmasked on the twin: the same rows bit for bit"""
        qs, ts = self.g.pack(queries, self.leaf)
        got = self.seg.search_batch_masked(self.set, qs, ts, k)
        _same_rows(got, self.twin.search_batch(qs, ts, k), what)
        return got

    def close(self):
        self.twin.close()
        self.seg.close()


def _kind_queries(kind):
    """-> (mirror query objects, the ss.Query records the oracle is asked with, or None where only the twin is compared)"""
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    plain = {"TERM": ss.TERMS, "AND": ss.ANDS, "OR < 10": ss.ORS, "OR >= 10": ss.WIDE, "min_should_match 2": ss.MSM2, "MUST_NOT terms": ss.NOTS,
             "FILTER terms": ss.FILTERS}
    if kind in plain:
        return [_gpu_query(q) for q in plain[kind]], plain[kind]
    if kind == "WITH_SHOULD":
        return [Bq.build([T(ss.EVEN)], [T(ss.FIFTH), T(ss.SOMETIMES)]), Bq.build([T(ss.EVERY), T(ss.EVEN)], [T(ss.LAST)], must_nots=[T(ss.FIRST)]),
                Bq.build([T(ss.CONST)], [T(ss.ABSENT), T(ss.FIFTH)])], None
    if kind == "SHOULD_REQUIRED":
        return [Bq.build([T(ss.EVERY), Bq.build([], [T(ss.EVEN), T(ss.FIFTH)])], []), Bq.build([T(ss.FIFTH), Bq.build([], [T(ss.LAST), T(ss.SOMETIMES), T(ss.ABSENT)])], [])], None
    if kind == "NESTED_MUST":
        return [Bq.build([T(ss.EVERY), Bq.build([T(ss.EVEN), T(ss.FIFTH)], [])], []), Bq.build([T(ss.FIFTH), Bq.build([T(ss.EVERY), T(ss.CONST)], [])], [])], None
    if kind == "DISMAX":
        return [rucene_amd.DisjunctionMaxQuery([T(ss.EVEN), T(ss.FIFTH), T(ss.LAST)], 0.3), rucene_amd.DisjunctionMaxQuery([T(ss.EVERY), T(ss.ABSENT)], 0.0)], None
    assert kind == "NOT_WITH_DEMOTE"
    return [rucene_amd.BoostingQuery.build(T(ss.EVERY), T(ss.EVEN), 0.5),
            rucene_amd.BoostingQuery.build(Bq.build([], [T(ss.EVEN), T(ss.FIFTH)], must_nots=[T(ss.SOMETIMES)]), Bq.build([], [T(ss.FIRST), T(ss.LAST)]), 0.25),
            rucene_amd.BoostingQuery.build(Bq.build([T(ss.EVERY), T(ss.FIFTH)], []), T(ss.EVEN), 0.75)], None


KINDS = ["TERM", "AND", "OR < 10", "OR >= 10", "min_should_match 2", "WITH_SHOULD", "SHOULD_REQUIRED", "NESTED_MUST", "DISMAX", "NOT_WITH_DEMOTE",
         "MUST_NOT terms", "FILTER terms"]


@pytest.mark.parametrize("live", LIVE)
@pytest.mark.parametrize("kind", KINDS)
def test_masked_parity_per_op_kind(ctx, oracle, kind, live):
    """Every op and flag rgpu_search_batch accepts, masked by a seeded half of an 8193-doc leaf: the twin's rows bit for bit at
    k = 10 and 129; the oracle's rows on live AND set where the oracle takes the query in one call."""
    fx = ss.Leaf(8193, "rank", live)
    m = _Masked(ctx, oracle, fx, ds.mask_of("half", fx.max_doc, fx.alive))
    try:
        queries, records = _kind_queries(kind)
        for k in (10, 129):
            hits, totals = m.both(queries, k, (kind, live, k))
            assert totals.sum() > 0 and totals.max() < fx.max_doc
            if records is not None and kind != "OR >= 10":
                _check_rows(oracle, m.osr, records, hits, totals, k, (kind, live, k))
                assert totals.tolist() == [int(m.mask[ss.ref_leaf_docs(fx, q)].sum()) for q in records], (kind, live, k, "hit counts against the set algebra")
    finally:
        m.close()


SWEEP = [(n, live, mask) for n in ds.SWEEP_SIZES for live in LIVE for mask in ds.MASKS]


@pytest.mark.parametrize("max_doc,live,mask", SWEEP, ids=["%d-%s-%s" % c for c in SWEEP])
def test_masked_parity_sweep(ctx, oracle, max_doc, live, mask):
    """Leaves of 1, 64, 65 and 8193 docs, with and without deletions, masked by nothing, everything, one doc, a seeded half and the
    complement of the live docs, at k = 1, 10, 128, 129 and 300: every query of tests/segment_spectrum.py in one batch, the twin's
    rows bit for bit; the oracle's rows on live AND set (the disjunctions of ten or more clauses are held against the oracle in
    test_masked_wide_disjunctions_against_the_oracle)."""
    fx = ss.Leaf(max_doc, "rank", live)
    m = _Masked(ctx, oracle, fx, ds.mask_of(mask, max_doc, fx.alive))
    try:
        queries = [_gpu_query(q) for q in ss.ALL_QUERIES]
        exact = [i for i, q in enumerate(ss.ALL_QUERIES) if not _is_wide(q)]
        ref_totals = [int(m.mask[ss.ref_leaf_docs(fx, q)].sum()) for q in ss.ALL_QUERIES]
        for k in ds.SWEEP_KS:
            hits, totals = m.both(queries, k, (max_doc, live, mask, k))
            assert totals.tolist() == ref_totals, (max_doc, live, mask, k, "hit counts against the set algebra")
            _check_rows(oracle, m.osr, [ss.ALL_QUERIES[i] for i in exact], hits[exact], totals[exact], k, (max_doc, live, mask, k))
        if mask in ("empty", "not-live"):
            assert not any(ref_totals)   # nothing left
    finally:
        m.close()


@pytest.mark.parametrize("live", LIVE)
@pytest.mark.parametrize("mask", ["full", "half"])
def test_masked_wide_disjunctions_against_the_oracle(ctx, oracle, mask, live):
    """Disjunctions of ten or more clauses with min_should_match <= 1 (the reference sums them in heap order): family D of
    tests/or_spectrum.py, masked, against the twin bit for bit and against the oracle on live AND set under oracle/parity.py's rule."""
    from oracle import parity
    fx = os_.Leaf(os_.MAX_DOC, "rank", live)
    m = _Masked(ctx, oracle, fx, ds.mask_of(mask, fx.max_doc, fx.alive))
    try:
        queries = [_gpu_query(q) for q in os_.FAMILY_D]
        for k in (10, 128, 129):
            hits, totals = m.both(queries, k, ("family D", live, mask, k))
            want = os_.oracle_rows(oracle, m.osr, os_.FAMILY_D, k)
            for i, (q, (d, s, total)) in enumerate(zip(os_.FAMILY_D, want)):
                assert os_.is_heap_order(q, fx)
                parity.check_heap_order_row(m.osr, oracle.OP_OR, list(q.should), hits[i]["doc"], hits[i]["score"], totals[i], d, s, d.size, total, rtol=1e-5,
                                            min_should_match=q.msm, what="family D %s %s k %d %s" % (live, mask, k, q))
                np.testing.assert_allclose(hits[i]["score"][:d.size], s, rtol=1e-5, atol=0)
                assert totals[i] == int(m.mask[os_.ref_docs(fx, q)].sum())
    finally:
        m.close()


# ---- isolation, no behaviour change, lifetime ---------------------------------------------------------------------------------------
def _device_rows(nq, k):
    import torch
    return torch.full((nq, k), -3, dtype=torch.int64, device="cuda"), torch.full((nq,), -3, dtype=torch.int64, device="cuda")


def _host_rows(hits, totals, k):
    from rucene_amd import _lib as gpu
    return hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(-1, k), totals.cpu().numpy()


@pytest.mark.parametrize("deferred", [False, True], ids=["default", "or_deferred"])
def test_isolation_across_streams(oracle, deferred):
    """ONE segment, no synchronisation in between: masked by A on stream 1, masked by B on stream 2, unmasked on stream 1. After one
    sync all three row sets are what the blocking calls return. On a context opened with or_deferred = 1 the masked batches are
    disjunctions of ten or more clauses (what that knob defers when unmasked) and an unmasked deferred batch runs before them."""
    import torch
    import rucene_amd
    c = rucene_amd.Context(or_deferred=deferred)
    try:
        # (deletions keep the fixed-point disjunction kernels, the ones whose flags are looked at later, from running at all: the
        # deferred case needs a leaf without them)
        fx = ss.Leaf(8193, "rank", "none" if deferred else "seeded")
        leaf = rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, live_docs=fx.live_docs, sum_total_term_freq=fx.sttf)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
        seg = leaf.segment
        rng = np.random.default_rng(72)
        a = seg.docset_from_words(_words(rng.random(fx.max_doc) < 0.5))
        b = seg.docset_from_words(_words(rng.random(fx.max_doc) < 0.2))
        records = ss.WIDE if deferred else ss.TERMS + ss.ANDS + ss.ORS + ss.NOTS
        k = 10
        qs, ts = g.pack([_gpu_query(q) for q in records], leaf)
        want = [seg.search_batch_masked(a, qs, ts, k), seg.search_batch_masked(b, qs, ts, k), seg.search_batch(qs, ts, k)]
        assert want[0][1].tolist() != want[1][1].tolist() != want[2][1].tolist()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = [_device_rows(len(records), k) for _ in range(4)]
        torch.cuda.synchronize()
        if deferred:   # an unmasked batch whose look at its flags is still pending when the first mask is installed
            seg.search_batch_device(qs, ts, k, outs[3][0].data_ptr(), outs[3][1].data_ptr(), stream=s1.cuda_stream)
        seg.search_batch_device_masked(a, qs, ts, k, outs[0][0].data_ptr(), outs[0][1].data_ptr(), stream=s1.cuda_stream)
        seg.search_batch_device_masked(b, qs, ts, k, outs[1][0].data_ptr(), outs[1][1].data_ptr(), stream=s2.cuda_stream)
        seg.search_batch_device(qs, ts, k, outs[2][0].data_ptr(), outs[2][1].data_ptr(), stream=s1.cuda_stream)
        c.synchronize()
        torch.cuda.synchronize()
        for i in range(3):
            _same_rows(_host_rows(*outs[i], k), want[i], ("stream order", deferred, i))
        if deferred:
            _same_rows(_host_rows(*outs[3], k), want[2], ("the deferred batch in front", deferred))
        seg.close()
    finally:
        c.close()


def test_unmasked_calls_run_what_they_ran(oracle):
    """On a context that has built and used doc sets, an unmasked single-term batch through the planner's fused call still takes the
    one-pass path (fused_term_batches) and launches the kernels it launches on a fresh context."""
    import torch
    import rucene_amd
    from rucene_amd import _lib as gpu
    fx = ss.Leaf(8193, "rank", "none")
    ids = np.array(ss.QUERIED, np.int64).reshape(-1, 1)
    k = 10
    seen = []
    for use_docsets in (False, True):
        c = rucene_amd.Context(profile_kernels=True)
        try:
            leaf = rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, sum_total_term_freq=fx.sttf)
            g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
            if use_docsets:
                qs, ts = g.pack([_gpu_query(q) for q in ss.TERMS + ss.ANDS + ss.ORS], leaf)
                half = leaf.segment.docset_from_words(_words(ds.mask_of("half", fx.max_doc, fx.alive)))
                made = leaf.segment.docset_collect_batch(qs[:len(ss.TERMS) + len(ss.ANDS)], ts)
                both = leaf.segment.docset_combine([half], [made[ss.FIFTH]])
                for s in (half, both, made[ss.EVEN]):
                    leaf.segment.search_batch_masked(s, qs, ts, k)
            hits, totals = _device_rows(ids.shape[0], k)
            torch.cuda.synchronize()
            for _ in range(2):   # the first call prepares the terms and builds the sketches (the full path)
                g.search_uniform_device(gpu.OP_TERM, ids, leaf, k, hits.data_ptr(), totals.data_ptr())
                c.synchronize()
            c.kernel_stats_reset()
            g.search_uniform_device(gpu.OP_TERM, ids, leaf, k, hits.data_ptr(), totals.data_ptr())
            c.synchronize()
            st = c.kernel_stats()
            seen.append((sorted(n for n, v in st.items() if v["launches"] > 0), st["fused_term_batches"]["launches"], _host_rows(hits, totals, k)))
            leaf.segment.close()
        finally:
            c.close()
    assert seen[0][1] == seen[1][1] == 1, (seen[0][1], seen[1][1])
    assert seen[0][0] == seen[1][0] and not any(n.startswith("k_docset") for n in seen[1][0]), (seen[0][0], seen[1][0])
    _same_rows(seen[0][2], seen[1][2], "fused single-term rows")
    osr = oracle.Searcher([fx.oracle_segment(oracle)])
    for i, t in enumerate(ss.QUERIED):
        _assert_row(seen[1][2][0][i], seen[1][2][1][i], osr.search(oracle.OP_TERM, [t], k, tie_mode=oracle.TIE_CANONICAL), ("fused", t))


def test_lifetime(ctx):
    """A set of segment 1 used with segment 2 is IllegalArgument (the segments are told apart by uid: same files, same size).
    rgpu_docset_free right after an enqueue-only masked call waits for it: the rows are intact."""
    import torch
    import rucene_amd
    fx = ss.Leaf(8193, "rank", "seeded")
    leaf = rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, live_docs=fx.live_docs, sum_total_term_freq=fx.sttf)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    seg1 = leaf.segment
    seg2 = _segment(ctx, fx)
    try:
        m = ds.mask_of("half", fx.max_doc, fx.alive)
        s1 = seg1.docset_from_words(_words(m))
        s2 = seg2.docset_from_words(_words(m))
        qs, ts = g.pack([_gpu_query(q) for q in ss.TERMS + ss.ANDS + ss.ORS], leaf)
        k = 10
        for call in (lambda: seg2.search_batch_masked(s1, qs, ts, k), lambda: seg1.docset_combine([s1, s2]), lambda: seg2.docset_combine([], [s1]),
                     lambda: seg1.search_batch_device_masked(s2, qs, ts, k, 8, 8)):
            with pytest.raises(rucene_amd.RgpuError) as e:
                call()
            assert e.value.status == -2
        want = seg1.search_batch_masked(s1, qs, ts, k)
        _same_rows(seg2.search_batch_masked(s2, qs, ts, k), want, "the same files, the same mask")
        stream = torch.cuda.Stream()
        hits, totals = _device_rows(qs.size, k)
        torch.cuda.synchronize()
        seg1.search_batch_device_masked(s1, qs, ts, k, hits.data_ptr(), totals.data_ptr(), stream=stream.cuda_stream)
        s1.close()   # returns when the masked search has finished reading the set
        _same_rows(_host_rows(hits, totals, k), want, "rows behind rgpu_docset_free")
    finally:
        seg2.close()
        seg1.close()
