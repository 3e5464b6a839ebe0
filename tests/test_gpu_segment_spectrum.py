"""Parity over segment sizes from one doc up, and over many leaves (`-m gpu`). The decisions the library takes by segment size - the
norm-rank table built from however few norm bytes exist, the 64-doc rounding of live-docs words, the guards next to two-docs-per-lane
loads, disjunction windows wider than the whole segment, chunk frontiers and sketches of lists that are one block or a VInt tail
alone, a merge over rows that are nearly all -1 - are met here from the small side: the fixtures of tests/segment_spectrum.py
(max_doc 1 .. 8193 on both sides of every word, block and chunk edge; live docs none / seeded / last / first / all deleted;
rank-mode, raw-mode and no norms) one leaf at a time, and as indexes of up to 41 leaves (every size at once, a large leaf among
forty flushed ones, two equally large leaves, 1536 docs that tie, fewer docs than k).

Doc bitmaps are built for lists of 1024 docs and more, whatever the knobs, and a conjunction's membership bits for lists of 512 and
more: their 32-doc word rounding is met at max_doc 1023, 1024, 1025, 8191, 8192, 8193 and 50 000 only, and on smaller leaves
or_bitmaps = -1 and and_bitmaps = -1 run what the default runs.
test_kernels_reached asserts from the kernel statistics which disjunction kernel answers at which size.

Everything goes through the public mirrors and the C ABI on one module-scoped Context, against the oracle: doc ids, hit counts and
score bits exact, disjunctions of ten or more clauses under oracle/parity.py's rule at rtol 1e-5; hit counts also against the numpy
set algebra of the fixtures. tests/test_segment_spectrum_cpu.py proves the fixtures on the CPU. The "raw" norms pass is run from
max_doc 65 up: below that a leaf cannot hold 65 distinct bytes and would be a second rank-mode leaf.

Phrases are searched on single tiny leaves only: the oracle's phrase_search takes one leaf's files and cannot be told another
leaf's statistics, so multi-leaf phrases have no reference here."""
import numpy as np
import pytest

import segment_spectrum as ss
from test_gpu_norm_spectrum import _assert_row, _run_term
from test_gpu_parity import _check_against_oracle, _check_not_queries

pytestmark = pytest.mark.gpu

KNOBS = {"small-items-no-and-bitmaps": dict(blocks_per_item=3, and_blocks_per_item=1, or_window_docs=256, and_bitmaps=-1),
         "no-or-bitmaps": dict(or_bitmaps=-1)}
GROUP_KS = (10, 129)   # the group-by-group passes; the mixed batch runs at every k of ss.KS
SINGLE = [(n, norms, live) for n in ss.SIZES for norms in ss.NORMS for live in ss.LIVE if norms != "raw" or n >= 65]


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


def _gpu_leaf(fx):
    import rucene_amd
    return rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, doc_base=fx.doc_base, live_docs=fx.live_docs,
                                 sum_total_term_freq=fx.sttf)


def _gpu_query(q):
    import rucene_amd
    T = rucene_amd.TermQuery
    return rucene_amd.BooleanQuery.build([T(t) for t in q.must], [T(t) for t in q.should], filters=[T(t) for t in q.filt],
                                         must_nots=[T(t) for t in q.must_not], min_should_match=q.msm)


def _is_wide(q):
    return len(q.should) >= 10 and q.msm <= 1


def _check_rows(oracle, osr, queries, hits, totals, k, what):
    """Every row of a batch against the oracle: exact, but for the disjunctions the reference sums in heap order."""
    from oracle import parity
    want = ss.oracle_rows(oracle, osr, queries, k)
    assert hits.shape == (len(queries), k) and len(totals) == len(queries)
    for i, q in enumerate(queries):
        if _is_wide(q):
            d, s, total = want[i]
            parity.check_heap_order_row(osr, oracle.OP_OR, list(q.should), hits[i]["doc"], hits[i]["score"], totals[i], d, s, d.size, total,
                                        rtol=1e-5, what="%s %s" % (what, q))
            np.testing.assert_allclose(hits[i]["score"][:d.size], s, rtol=1e-5, atol=0)
        else:
            _assert_row(hits[i], totals[i], want[i], (what, q))


def _check_searcher(oracle, osr, g, leaves, what):
    """Every query kind through GpuIndexSearcher.search_batch: all of them mixed into one batch at every k of ss.KS (every row
    compared, hit counts also against numpy); at GROUP_KS also group by group through the helpers of tests/test_gpu_parity.py, and
    the FILTER and min_should_match rows in a batch of their own."""
    ref_totals = [ss.ref_docs(leaves, q).size for q in ss.ALL_QUERIES]
    mixed = [_gpu_query(q) for q in ss.ALL_QUERIES]
    rest = ss.FILTERS + ss.MSM2
    for k in ss.KS:
        hits, totals = g.search_batch(mixed, k)
        _check_rows(oracle, osr, ss.ALL_QUERIES, hits, totals, k, (what, k, "mixed"))
        assert totals.tolist() == ref_totals, (what, k, "hit counts against the set algebra")
    for k in GROUP_KS:
        _check_against_oracle(oracle, osr, g, [ss.spec(oracle, q) for q in ss.EXACT], k)
        _check_against_oracle(oracle, osr, g, [ss.spec(oracle, q) for q in ss.WIDE], k, exact=False)
        _check_not_queries(oracle, osr, g, [ss.not_spec(oracle, q) for q in ss.NOTS], k)
        hits, totals = g.search_batch([_gpu_query(q) for q in rest], k)
        _check_rows(oracle, osr, rest, hits, totals, k, (what, k, "filters, min_should_match"))


# ---- one leaf -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc,norms,live", SINGLE, ids=["%d-%s-%s" % c for c in SINGLE])
def test_single_leaf(ctx, oracle, max_doc, norms, live):
    """One size, one kind of norms, one live-docs variant: decode_terms bit-exact (the absent terms in the call), TERM through
    search_batch, the fused plan-and-search call and the two-call device path, AND / OR / MUST_NOT / FILTER / min_should_match,
    mixed and separately, k in {1, 10, 128, 129, 300}: k exceeds max_doc for most sizes, the unused slots hold doc -1."""
    import rucene_amd
    fx = ss.Leaf(max_doc, norms, live)
    what = (max_doc, norms, live)
    osr = oracle.Searcher([fx.oracle_segment(oracle)])
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    try:
        docs, freqs = leaf.segment.decode_terms(fx.seg.terms)
        assert fx.seg.terms.size == ss.N_TERMS and fx.seg.terms["doc_freq"][ss.ABSENT] == 0
        assert (docs == np.concatenate([d for d, _ in fx.lists])).all() and (freqs == np.concatenate([f for _, f in fx.lists])).all(), what
        for k in ss.KS:
            want = ss.oracle_rows(oracle, osr, ss.TERMS, k)
            for fused in (True, False):
                rows, totals = _run_term(g, leaf, ss.QUERIED, k, fused)
                for t in ss.QUERIED:
                    _assert_row(rows[t], totals[t], want[t], (what, k, "fused" if fused else "two calls", t))
                    assert totals[t] == int((fx.has[t] & fx.alive).sum())
        _check_searcher(oracle, osr, g, [fx], what)
    finally:
        leaf.segment.close()


def _launched(c, *names):
    st = c.kernel_stats()
    return [n in st and st[n]["launches"] > 0 for n in names]


REACH = [(33, "rank", "none", 10, "default", "wide"), (129, "rank", "none", 10, "default", "wide"), (1023, "rank", "none", 128, "default", "wide"),
         (1024, "rank", "none", 10, "default", "lazy"), (8193, "rank", "none", 128, "default", "lazy"), (1024, "rank", "none", 10, "no-or-bitmaps", "wide"),
         (8193, "rank", "none", 10, "no-or-bitmaps", "wide"), (129, "rank", "seeded", 10, "default", "windows"), (129, "raw", "none", 10, "default", "windows"),
         (129, "none", "none", 10, "default", "windows"), (129, "rank", "none", 129, "default", "windows"), (8193, "rank", "last", 10, "default", "windows")]


@pytest.mark.parametrize("max_doc,norms,live,k,knobs,kernel", REACH, ids=["%d-%s-%s-k%d-%s-%s" % c for c in REACH])
def test_kernels_reached(oracle, max_doc, norms, live, k, knobs, kernel):
    """Which kernel answers the disjunctions of ten and more clauses on a small leaf, from the kernel statistics. The fixed-point
    kernels take a leaf with rank-mode norms, no deleted docs and k <= 128: k_or_wide while no clause has a doc bitmap (every list
    below 1024 docs, or or_bitmaps = -1), k_or_lazy and k_bitmap_build once the every-doc lists reach 1024 docs; deleted docs, raw
    or no norms, or k above 128 leave the clause-order window kernel alone. The rows are checked as everywhere else; a TERM batch
    launches k_search_term; no list below 1024 docs gets a full bitmap and none below 512 a conjunction's membership bits."""
    import rucene_amd
    ctx2 = rucene_amd.Context(profile_kernels=True, **(KNOBS[knobs] if knobs != "default" else {}))
    try:
        fx = ss.Leaf(max_doc, norms, live)
        osr = oracle.Searcher([fx.oracle_segment(oracle)])
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx2)
        _run_term(g, leaf, ss.QUERIED, k, True)
        ctx2.kernel_stats_reset()
        rows, totals = _run_term(g, leaf, ss.QUERIED, k, True)
        st = ctx2.kernel_stats()
        print(max_doc, norms, live, k, knobs, "TERM:", {n: v["launches"] for n, v in st.items() if v["launches"]})
        assert _launched(ctx2, "k_search_term")[0]
        ctx2.kernel_stats_reset()
        _check_against_oracle(oracle, osr, g, [ss.spec(oracle, q) for q in ss.WIDE], k, exact=False)
        st = ctx2.kernel_stats()
        print(max_doc, norms, live, k, knobs, "OR >= 10:", {n: v["launches"] for n, v in st.items() if v["launches"]})
        lazy, wide, windows, built = _launched(ctx2, "k_or_lazy", "k_or_wide", "k_or_windows", "k_bitmap_build")
        if kernel == "lazy":
            assert lazy and built, (lazy, wide, windows, built)
        elif kernel == "wide":
            assert wide and not lazy and not built, (lazy, wide, windows, built)
        else:
            assert windows and not lazy and not wide and not built, (lazy, wide, windows, built)
        # conjunctions and short disjunctions: no full bitmap for a list below 1024 docs, no membership bits (the bits alone, for a
        # conjunction's clauses) for one below 512
        ctx2.kernel_stats_reset()
        _check_against_oracle(oracle, osr, g, [ss.spec(oracle, q) for q in ss.ANDS + ss.ORS], k)
        st = ctx2.kernel_stats()
        print(max_doc, norms, live, k, knobs, "AND, OR < 10:", {n: v["launches"] for n, v in st.items() if v["launches"]})
        assert _launched(ctx2, "k_search_and")[0] and _launched(ctx2, "k_or_windows")[0]
        built, memb = _launched(ctx2, "k_bitmap_build", "k_bitmap_memb")
        assert not (built and max_doc < 1024) and not (memb and max_doc < 512), (built, memb)
        if max_doc == 1023 and knobs == "default":
            assert memb   # EVERY (1023 docs) and EVEN (512) behind a sparser lead: membership bits, no full bitmap
        leaf.segment.close()
    finally:
        ctx2.close()


# ---- many leaves --------------------------------------------------------------------------------------------------------------------
def _open(oracle, name, ctx):
    import rucene_amd
    fxs = ss.INDEXES[name]()
    osr = oracle.Searcher([fx.oracle_segment(oracle) for fx in fxs])
    assert oracle.lib().orc_searcher_stats_leaf(osr._h) == ss.stats_leaf(fxs)
    g = rucene_amd.GpuIndexSearcher([_gpu_leaf(fx) for fx in fxs], ctx=ctx)
    return fxs, osr, g


def _close(g):
    for leaf in g.leaves:
        leaf.segment.close()


@pytest.mark.parametrize("name", list(ss.INDEXES))
def test_multi_leaf_search(ctx, oracle, name):
    """The same query kinds through GpuIndexSearcher(leaves): per-leaf rows merged on the device, doc ids carry the doc base, the
    statistics are those of the first largest leaf."""
    fxs, osr, g = _open(oracle, name, ctx)
    try:
        _check_searcher(oracle, osr, g, fxs, name)
    finally:
        _close(g)


def test_twins_score_with_the_first_twin(ctx, oracle):
    """Two equally large leaves: the first of them is the statistics leaf (searcher.rs:306-363), in the oracle and in the mirror;
    FIFTH has another doc_freq in the second twin, so the other choice gives other score bits."""
    fxs, osr, g = _open(oracle, "twins", ctx)
    try:
        assert oracle.lib().orc_searcher_stats_leaf(osr._h) == ss.TWINS_STATS_LEAF == g._stats_leaf
        twin = [i for i, fx in enumerate(fxs) if fx.max_doc == fxs[ss.TWINS_STATS_LEAF].max_doc]
        assert twin == [ss.TWINS_STATS_LEAF, 3] and g.term_statistics(ss.FIFTH) == fxs[twin[0]].lists[ss.FIFTH][0].size != fxs[twin[1]].lists[ss.FIFTH][0].size
        for k in (1, 10, 129):
            _check_against_oracle(oracle, osr, g, [ss.spec(oracle, q) for q in ss.EXACT], k)
    finally:
        _close(g)


def test_ties_rows_in_full(ctx, oracle):
    """24 leaves of 64 docs that all score alike: the merged row is the lowest global doc ids in ascending order, at k = 1, 10, 100
    and 129; a band of equal scores across a leaf boundary is cut by doc id."""
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    fxs, osr, g = _open(oracle, "ties", ctx)
    try:
        for term, ks in ((ss.CONST, ss.TIES_KS), (ss.PLATEAU, ss.PLATEAU_KS)):
            for k in ks:
                hits, totals = g.search_batch([T(term), Bq.build([T(term), T(ss.CONST)], []), Bq.build([], [T(term), T(ss.CONST)])], k)
                want = ss.ref_ties_row(fxs, term, k)
                assert (hits[0]["doc"] == want).all(), (term, k, hits[0]["doc"], want)
                assert (hits[1]["doc"] == want).all(), (term, k, "AND", hits[1]["doc"], want)   # CONST adds the same to every doc
                if term == ss.CONST:
                    assert hits[0]["doc"].tolist() == list(range(k)) == hits[2]["doc"].tolist() and np.unique(hits[0]["score"]).size == 1
                    assert totals.tolist() == [1536, 1536, 1536]
                _assert_row(hits[0], totals[0], osr.search(oracle.OP_TERM, [term], k, tie_mode=oracle.TIE_CANONICAL), ("ties", term, k))
                _assert_row(hits[1], totals[1], osr.search(oracle.OP_AND, [term, ss.CONST], k, tie_mode=oracle.TIE_CANONICAL), ("ties AND", term, k))
                _assert_row(hits[2], totals[2], osr.search(oracle.OP_OR, [term, ss.CONST], k, tie_mode=oracle.TIE_CANONICAL), ("ties OR", term, k))
    finally:
        _close(g)


@pytest.mark.parametrize("name", list(ss.INDEXES))
def test_multi_leaf_sharded_call_with_a_world_of_one(ctx, oracle, name):
    """rgpu_search_batch_sharded leaf by leaf in a world of one: the local search's rows; merged over the leaves, the oracle's."""
    import torch
    from rucene_amd import _lib as gpu
    fxs, osr, g = _open(oracle, name, ctx)
    comm = gpu.Comm(ctx, 1, 0, gpu.comm_unique_id())
    try:
        batch = ss.EXACT + ss.WIDE
        queries = [_gpu_query(q) for q in batch]
        for k in (10, 129):
            per_leaf = []
            for leaf in g.leaves:
                qs, ts = g.pack(queries, leaf)
                want_h, want_t = leaf.segment.search_batch(qs, ts, k)
                dh = torch.full((len(queries), k), -3, dtype=torch.int64, device="cuda")
                dt = torch.full((len(queries),), -3, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                comm.search_batch_sharded(leaf.segment, qs, ts, k, dh.data_ptr(), dt.data_ptr())
                ctx.synchronize()
                got = dh.cpu().numpy().view(gpu.HIT_DTYPE).reshape(len(queries), k)
                assert (got["doc"] == want_h["doc"]).all() and (got["score"].view(np.int32) == want_h["score"].view(np.int32)).all(), (name, k, leaf.doc_base)
                assert (dt.cpu().numpy() == want_t).all() and (comm.status() == 0).all(), (name, k, leaf.doc_base)
                per_leaf.append((got.copy(), dt.cpu().numpy()))
            hits, totals = per_leaf[0] if len(per_leaf) == 1 else g._merge_leaves(per_leaf, len(queries), k)
            _check_rows(oracle, osr, batch, hits, totals, k, (name, "sharded", k))
    finally:
        comm.close()
        _close(g)


@pytest.mark.parametrize("name", list(ss.INDEXES))
def test_multi_leaf_rescoring(ctx, oracle, name):
    """QueryRescorer across all the leaves (one call per leaf, the last one finishes): per row the oracle's Searcher.rescore."""
    fxs, osr, g = _open(oracle, name, ctx)
    try:
        first = [ss.TERMS[ss.EVERY], ss.TERMS[ss.CONST], ss.TERMS[ss.LAST], ss.TERMS[ss.ABSENT], ss.ORS[2], ss.ANDS[1], ss.ORS[0], ss.TERMS[ss.FIFTH]]
        second = [ss.TERMS[ss.EVEN], ss.ORS[1], ss.ANDS[0], ss.TERMS[ss.EVERY], ss.TERMS[ss.ABSENT], ss.TERMS[ss.FIRST], ss.ORS[6], ss.ANDS[7]]
        gq = [_gpu_query(q) for q in second]
        for k in (10, 100):
            hits, totals = g.search_batch([_gpu_query(q) for q in first], k)
            _check_rows(oracle, osr, first, hits, totals, k, (name, "first pass", k))
            for mode in range(5):
                for window, qw, rw in ((k, 1.0, 1.0), (7, 1.3, 0.25)):
                    got = g.rescore_batch(hits, gq, query_weight=qw, rescore_weight=rw, mode=mode, window_size=window)
                    for i, q in enumerate(second):
                        op, tids = ss.spec(oracle, q)
                        n = int((hits[i]["doc"] >= 0).sum())
                        wd, ws = osr.rescore(op, tids, hits[i]["doc"][:n], hits[i]["score"][:n], window, qw, rw, mode)
                        assert (got[i]["doc"][:n] == wd).all() and (got[i]["doc"][n:] == -1).all(), (name, k, mode, window, i, got[i]["doc"][:n], wd)
                        assert (got[i]["score"][:n].view(np.int32) == ws.view(np.int32)).all(), (name, k, mode, window, i)
    finally:
        _close(g)


# ---- work-partitioning knobs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("name", ["many-shuffled", "many-raw"])
def test_work_partitioning_knobs_on_many_leaves(oracle, name, knobs):
    """Small work items, 256-doc disjunction windows, no conjunction bitmaps / no disjunction bitmaps, on leaves that are mostly
    smaller than one window. (Only the leaves of 1023 docs and more hold lists long enough for a bitmap or membership bits: for the
    others the bitmap knobs change nothing, the item and window sizes do.)"""
    import rucene_amd
    ctx2 = rucene_amd.Context(profile_kernels=True, **KNOBS[knobs])
    try:
        fxs, osr, g = _open(oracle, name, ctx2)
        try:
            _check_searcher(oracle, osr, g, fxs, (name, knobs))
        finally:
            _close(g)
    finally:
        ctx2.close()


# ---- tiny positions segments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc", ss.POSITION_SIZES)
def test_phrases_on_tiny_segments(ctx, oracle, max_doc):
    """Exact and slop-2 phrases of two and three terms (a repeated term, an absent term) on leaves of 1, 2, 64, 129 and 257 docs."""
    import rucene_amd
    from rucene_amd import _lib as gpu
    postings, norms, doc_count, sum_ttf = ss.positions_postings(max_doc)
    ix = oracle.PositionsIndex(max_doc, postings)
    doc_bytes, pos_bytes = ix.files()
    n = len(postings)
    terms = np.zeros(n, dtype=gpu.TERM_STATE_DTYPE)
    tpos = np.zeros(n, dtype=gpu.TERM_POSITIONS_DTYPE)
    for t in range(n):
        st = ix.term_state(t)
        terms[t] = (st["doc_start_fp"], st["skip_offset"], st["total_term_freq"], st["doc_freq"], st["singleton_doc_id"])
        tpos[t]["pos_start_fp"], tpos[t]["last_pos_block_offset"] = st["pos_start_fp"], st["last_pos_block_offset"]
    leaf = rucene_amd.LeafReader(np.frombuffer(doc_bytes, np.uint8), norms, max_doc, terms, doc_count=doc_count, sum_total_term_freq=sum_ttf, index_options=3)
    leaf.pos_bytes, leaf.term_positions = np.frombuffer(pos_bytes, np.uint8), tpos
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    try:
        queries = [rucene_amd.PhraseQuery(t, slop=sl) for t, sl in ss.PHRASES]
        matched = 0
        for k in ss.PHRASE_KS:
            hits, totals = g.search_phrase_batch(queries, k)
            for i, q in enumerate(queries):
                want = ix.phrase_search(q.terms, k, norms, max_doc, doc_count, sum_ttf, slop=q.slop)
                _assert_row(hits[i], totals[i], want, (max_doc, "phrase", q.terms, q.slop, k))
                matched += want[2]
        assert matched >= len(ss.PHRASES)
    finally:
        leaf.segment.close()
        ix.close()
