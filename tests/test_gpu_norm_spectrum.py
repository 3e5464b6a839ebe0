"""Parity over the whole norm-byte range (`-m gpu`), in both norm storage modes. rgpu_segment_upload keeps a segment of at most 64
distinct norm bytes in RANK mode (ranks in HBM, the LDS score table, 6-bit rank frontier words, chunk frontiers, sketches, the
pruned TERM kernels, k_or_wide / k_or_lazy) and any other segment in RAW mode, where another set of kernels and code paths answers
the same queries. The fixtures of tests/norm_spectrum.py (one byte, {0, 255}, exactly 64 bytes with ranks 0..63 used, 65 bytes,
all 256) are run through every query kind: every row against the oracle bit for bit (doc ids, score bits, totals; disjunctions of
ten or more clauses under oracle/parity.py's rule at rtol 1e-5), planted rows also against a float64 ranking computed in numpy.
tests/test_norm_spectrum_cpu.py proves the fixtures' expectations on the CPU."""
import os

import numpy as np
import pytest

import norm_spectrum as ns
from test_gpu_parity import _check_against_oracle, _check_nested_rows, _check_not_queries, _conjunction_with_a_nested_child

pytestmark = pytest.mark.gpu

TERM_KS = [1, 10, 64, 65, 128]   # through the device calls; 300 goes through search_batch (passes of 128)
ALL_TERMS = list(range(ns.N_TERMS))
OR10 = [ns.PLANTED, ns.CROSSED, ns.ZERO_FRONT, ns.ZERO_DEEP, ns.SPARSE, ns.BELOW_DENSITY, ns.ABOVE_DENSITY, ns.BITMAP, ns.RANDOM0 + 2, ns.RANDOM0 + 3]
PHRASE_SPECTRA = ("rank64", "raw65", "all256")

_oracles = {}


def _osr(oracle, name, version=1):
    if (name, version) not in _oracles:
        _oracles[(name, version)] = oracle.Searcher([ns.spectrum(name, version).oracle_segment(oracle)])
    return _oracles[(name, version)]


_term_rows = {}


def _term_want(oracle, name, version, term, k):
    key = (name, version, term, k)
    if key not in _term_rows:
        _term_rows[key] = _osr(oracle, name, version).search(oracle.OP_TERM, [term], k, tie_mode=oracle.TIE_CANONICAL)
    return _term_rows[key]


def _context(env=None, **cfg):
    import rucene_amd
    env = env or {}
    saved = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        return rucene_amd.Context(profile_kernels=True, **cfg)
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def _searcher(sp, ctx, live=None):
    import rucene_amd
    leaf = rucene_amd.LeafReader(sp.seg.doc_bytes, sp.seg.norms, ns.MAX_DOC, sp.seg.terms, live_docs=live, sum_total_term_freq=ns.STTF)
    return rucene_amd.GpuIndexSearcher([leaf], ctx=ctx), leaf


def _run_term(g, leaf, ids, k, fused):
    import torch
    from rucene_amd import _lib as gpu
    sel = np.asarray(ids, dtype=np.int64).reshape(-1, 1)
    nq = sel.shape[0]
    hits = torch.full((nq, k), -3, dtype=torch.int64, device="cuda")
    totals = torch.full((nq,), -3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    if fused:
        g.search_uniform_device(gpu.OP_TERM, sel, leaf, k, hits.data_ptr(), totals.data_ptr())
    else:
        qs, ts = g.pack_uniform(gpu.OP_TERM, sel, leaf)
        leaf.segment.search_batch_device(qs, ts, k, hits.data_ptr(), totals.data_ptr())
    g.ctx.synchronize()
    return hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(nq, k), totals.cpu().numpy()


def _assert_row(row, total, want, what):
    d, sc, tot = want
    assert total == tot, (what, "total", int(total), tot)
    missing = sorted(set(d.tolist()) - set(row["doc"].tolist()))
    assert (row["doc"][:d.size] == d).all() and (row["doc"][d.size:] == -1).all(), (what, "docs", "missing", missing[:10], row["doc"][:8], d[:8])
    assert (row["score"][:d.size].view(np.int32) == sc.view(np.int32)).all(), (what, "score bits")


def _assert_ranking(row, ranking, n, what):
    n = min(n, ranking.size)
    assert (row["doc"][:n] == ranking[:n]).all(), (what, "float64 ranking", row["doc"][:n], ranking[:n])


def _stats(ctx, *names):
    st = ctx.kernel_stats()
    return [n in st and st[n]["launches"] > 0 for n in names]


# ---- the mode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ns.SPECTRA)
def test_mode_is_what_the_table_says(oracle, name):
    """The storage mode, told from behaviour: in a rank spectrum a fused TERM batch on the planted list leaves most FullBlocks packed
    and a ten-clause disjunction runs k_or_lazy or k_or_wide; with 65 or more distinct bytes (no config switch) the TERM batch
    decodes every block and the disjunction runs the clause-order window kernel alone."""
    import rucene_amd
    sp = ns.spectrum(name)
    ctx = _context()
    try:
        g, leaf = _searcher(sp, ctx)
        nw = sp.n_winners(ns.PLANTED)
        _run_term(g, leaf, [ns.PLANTED], nw, True)  # (the first call prepares the term through the full path)
        rows, totals = _run_term(g, leaf, [ns.PLANTED], nw, True)
        c = ctx.last_search_counters()
        _assert_row(rows[0], totals[0], _term_want(oracle, name, 1, ns.PLANTED, nw), (name, "TERM"))
        print(name, "blocks_decoded", c["blocks_decoded"], "of", ns.PLANTED_BLOCKS)
        assert c["op"] == 0 and c["postings_covered"] == sp.lists[ns.PLANTED][0].size
        if sp.rank_mode:
            assert 0 < c["blocks_decoded"] < ns.PLANTED_BLOCKS // 2, c
        else:
            assert c["blocks_decoded"] == ns.PLANTED_BLOCKS, c
        _check_against_oracle(oracle, _osr(oracle, name), g, [(oracle.OP_OR, OR10)], 10, exact=False)
        lazy, wide, windows = _stats(ctx, "k_or_lazy", "k_or_wide", "k_or_windows")
        assert (lazy or wide) == sp.rank_mode and (sp.rank_mode or windows), (name, lazy, wide, windows)
        assert isinstance(g, rucene_amd.GpuIndexSearcher)
    finally:
        ctx.close()


# ---- TERM -----------------------------------------------------------------------------------------------------------------------
TERM_KNOBS = {"query-4": ({"RGPU_TERM_QUERY_WAVES": "4"}, 1), "query-2": ({"RGPU_TERM_QUERY_WAVES": "2"}, 1),
              "query-8": ({"RGPU_TERM_QUERY_WAVES": "8"}, 1), "query-no-sketch": ({"RGPU_TERM_SKETCH": "0"}, 1),
              "query-legacy": ({}, 0), "items-fold": ({"RGPU_TERM_KERNEL": "items", "RGPU_TERM_FOLD": "1"}, 1),
              "items-merge-launch": ({"RGPU_TERM_KERNEL": "items", "RGPU_TERM_FOLD": "0"}, 1),
              "items-no-sketch": ({"RGPU_TERM_KERNEL": "items", "RGPU_TERM_SKETCH": "0"}, 1),
              "items-legacy": ({"RGPU_TERM_KERNEL": "items"}, 0)}


@pytest.mark.parametrize("knobs", list(TERM_KNOBS))
@pytest.mark.parametrize("name", ns.SPECTRA)
def test_term_rows_every_kernel(oracle, name, knobs):
    """Every list of the spectrum as a TERM query: the query kernel at 2, 4 and 8 waves, the items kernel with the fold inside the
    launch and in a launch of its own, with and without sketches, BP128 and legacy .doc files; the fused call and the two-call path,
    k 1..128, and k 300 through search_batch. The planted rows also against the float64 ranking: a winner is in the top-k only
    because of its norm byte, so a block bound that under-states a rank loses it."""
    import rucene_amd
    env, version = TERM_KNOBS[knobs]
    sp = ns.spectrum(name, version)
    rank = {t: sp.ranking(t) for t in (ns.PLANTED, ns.CROSSED)}
    ctx = _context(env)
    try:
        g, leaf = _searcher(sp, ctx)
        ids = ALL_TERMS + [ns.PLANTED, ns.CROSSED]
        for k in TERM_KS:
            for fused in (True, False):
                rows, totals = _run_term(g, leaf, ids, k, fused)
                for j, t in enumerate(ids):
                    what = (name, knobs, k, "fused" if fused else "two calls", t)
                    if t in rank:
                        _assert_ranking(rows[j], rank[t], min(k, sp.n_winners(t) + 1), what)
                    _assert_row(rows[j], totals[j], _term_want(oracle, name, version, t, k), what)
        hits, totals = g.search_batch([rucene_amd.TermQuery(t) for t in ids], 300)
        for j, t in enumerate(ids):
            _assert_row(hits[j], totals[j], _term_want(oracle, name, version, t, 300), (name, knobs, 300, t))
        if "items" in knobs:
            assert not _stats(ctx, "term_query_launches")[0]
        elif sp.rank_mode:
            assert _stats(ctx, "term_query_launches")[0]
    finally:
        ctx.close()


# ---- AND ------------------------------------------------------------------------------------------------------------------------
AND_SPECS = [[ns.PLANTED, ns.EVERY_DOC], [ns.CROSSED, ns.EVERY_DOC], [ns.PLANTED, ns.BITMAP], [ns.SPARSE, ns.PLANTED, ns.EVERY_DOC],
             [ns.BITMAP, ns.HALF, ns.EVERY_DOC, ns.PLANTED], [ns.SINGLETON, ns.EVERY_DOC], [ns.RANDOM0 + 3, ns.HALF, ns.EVERY_DOC],
             [ns.PLANTED, ns.CROSSED], [ns.HALF, ns.EVERY_DOC, ns.BITMAP, ns.ABOVE_DENSITY, ns.BELOW_DENSITY], [ns.ZERO_FRONT, ns.EVERY_DOC],
             [ns.ZERO_DEEP, ns.HALF, ns.EVERY_DOC], [ns.ABSENT, ns.EVERY_DOC], [ns.HALF, ns.EVERY_DOC], [ns.BELOW_DENSITY, ns.HALF],
             [ns.CROSSED, ns.HALF, ns.BITMAP], [ns.RANDOM0 + 2, ns.EVERY_DOC, ns.HALF]]


@pytest.mark.parametrize("and_bitmaps", [0, -1], ids=["bitmaps", "no-bitmaps"])
@pytest.mark.parametrize("name", ns.SPECTRA)
def test_conjunctions(oracle, name, and_bitmaps):
    """2 to 5 clauses mixing the planted lists, bitmap clauses (df above 1 doc in 64), sparse clauses and the every-doc list; leads of
    one posting, one block and hundreds of blocks; with and without the conjunction's doc bitmaps."""
    sp = ns.spectrum(name)
    osr = _osr(oracle, name)
    extra = lambda docs: sp.term_score_f64(ns.EVERY_DOC, docs)   # noqa: E731
    ctx = _context(and_bitmaps=and_bitmaps)
    try:
        g, leaf = _searcher(sp, ctx)
        specs = [(oracle.OP_AND, s) for s in AND_SPECS]
        for k in (1, 7, 8, 10, 100, 300):
            _check_against_oracle(oracle, osr, g, specs, k)
        import rucene_amd
        T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
        for t in (ns.PLANTED, ns.CROSSED):
            nw = sp.n_winners(t)
            hits, _ = g.search_batch([Bq.build([T(t), T(ns.EVERY_DOC)], [])], nw)
            _assert_ranking(hits[0], sp.ranking(t, extra=extra), nw, (name, "AND", t))
    finally:
        ctx.close()


# ---- OR -------------------------------------------------------------------------------------------------------------------------
OR_SPECS = [[ns.PLANTED, ns.EVERY_DOC], [ns.CROSSED, ns.SPARSE], [ns.ZERO_FRONT, ns.SINGLETON, ns.RANDOM0 + 2], [ns.ZERO_DEEP, ns.BELOW_DENSITY, ns.ABOVE_DENSITY],
            [ns.PLANTED, ns.CROSSED, ns.ZERO_FRONT, ns.ZERO_DEEP, ns.SPARSE, ns.BELOW_DENSITY, ns.ABOVE_DENSITY, ns.BITMAP, ns.ABSENT],
            [ns.HALF, ns.BITMAP, ns.EVERY_DOC], [ns.ZERO_FRONT, ns.ZERO_DEEP], [ns.SINGLETON, ns.ABSENT], [ns.PLANTED, ns.CROSSED]]


@pytest.mark.parametrize("name", ns.SPECTRA)
def test_disjunctions_below_ten_clauses(oracle, name):
    """2 to 9 SHOULD clauses (the clause-order kernel): bit for bit. The planted list next to the every-doc list ranks its winners
    by the float64 sums."""
    import rucene_amd
    sp = ns.spectrum(name)
    extra = lambda docs: sp.term_score_f64(ns.EVERY_DOC, docs)   # noqa: E731
    ctx = _context()
    try:
        g, leaf = _searcher(sp, ctx)
        for k in (1, 10, 100, 300):
            _check_against_oracle(oracle, _osr(oracle, name), g, [(oracle.OP_OR, s) for s in OR_SPECS], k)
        T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
        nw = sp.n_winners(ns.PLANTED)
        hits, _ = g.search_batch([Bq.build([], [T(ns.PLANTED), T(ns.EVERY_DOC)])], nw)
        _assert_ranking(hits[0], sp.ranking(ns.PLANTED, extra=extra), nw, (name, "OR"))
    finally:
        ctx.close()


WIDE_SPECS = [OR10, [ns.SINGLETON, ns.RANDOM0 + 2, ns.RANDOM0 + 3] + [ns.ZERO_FRONT] * 7,   # rare terms next to the byte-0 list: the top-k
              [ns.SINGLETON, ns.RANDOM0 + 4] + [ns.ZERO_DEEP] * 9,                           # reaches down into totals near 1e-17
              OR10 + [ns.HALF, ns.EVERY_DOC], [ns.EVERY_DOC] * 10, list(range(ns.RANDOM0, ns.RANDOM0 + 10)),
              [ns.PLANTED] * 5 + [ns.CROSSED] * 5, [ns.ZERO_FRONT, ns.ZERO_DEEP] * 5 + [ns.ABSENT]]


@pytest.mark.parametrize("knobs", [dict(), dict(or_bitmaps=-1), dict(or_wide=-1)], ids=["k_or_lazy", "k_or_wide", "k_or_windows"])
@pytest.mark.parametrize("name", ns.SPECTRA)
def test_disjunctions_of_ten_or_more_clauses(oracle, name, knobs):
    """Ten and more SHOULD clauses under oracle/parity.py's rule: through k_or_lazy (dense clauses met through their doc bitmaps),
    k_or_wide (or_bitmaps = -1) and the clause-order window kernel (or_wide = -1, and whatever the knobs in raw mode); the byte-0
    lists next to rare terms take the top-k down to totals near 1e-17 (the fixed-point floor and its redo in f32)."""
    sp = ns.spectrum(name)
    ctx = _context(**knobs)
    try:
        g, leaf = _searcher(sp, ctx)
        _check_against_oracle(oracle, _osr(oracle, name), g, [(oracle.OP_OR, OR10)], 10, exact=False)
        lazy, wide, windows = _stats(ctx, "k_or_lazy", "k_or_wide", "k_or_windows")
        if "or_wide" in knobs or not sp.rank_mode:
            assert windows and not lazy and not wide, (name, knobs, lazy, wide, windows)
        elif "or_bitmaps" in knobs:
            assert wide and not lazy, (name, knobs, lazy, wide, windows)
        else:
            assert lazy, (name, knobs, lazy, wide, windows)
        for k in (1, 10, 100, 300):
            _check_against_oracle(oracle, _osr(oracle, name), g, [(oracle.OP_OR, s) for s in WIDE_SPECS], k, exact=False)
    finally:
        ctx.close()


# ---- MUST + SHOULD, MUST_NOT, FILTER, min_should_match, a nested disjunction ---------------------------------------------------------
@pytest.mark.parametrize("name", ns.SPECTRA)
def test_boolean_trees(oracle, name):
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    sp = ns.spectrum(name)
    osr = _osr(oracle, name)
    ctx = _context()
    try:
        g, leaf = _searcher(sp, ctx)
        # MUST + SHOULD [+ MUST_NOT]: ReqOptScorer with its skip rule
        opt = [([ns.PLANTED], [ns.EVERY_DOC], []), ([ns.CROSSED, ns.EVERY_DOC], [ns.HALF, ns.BITMAP], []), ([ns.HALF], [ns.PLANTED, ns.ZERO_FRONT], [ns.BITMAP]),
               ([ns.ZERO_DEEP], [ns.HALF], []), ([ns.EVERY_DOC], [ns.ZERO_FRONT, ns.SINGLETON], []), ([ns.BITMAP, ns.HALF], [ns.ABSENT, ns.SPARSE], [ns.BELOW_DENSITY]),
               ([ns.RANDOM0 + 3], [ns.EVERY_DOC, ns.HALF], [])]
        queries = [Bq.build([T(t) for t in m], [T(t) for t in s], must_nots=[T(t) for t in n]) for m, s, n in opt]
        for k in (10, 100, 300):
            hits, totals = g.search_batch(queries, k)
            for i, (m, s, n) in enumerate(opt):
                want = osr.search_opt(oracle.OP_AND if len(m) > 1 else oracle.OP_TERM, m, s, k, must_not_ids=n)
                _assert_row(hits[i], totals[i], want, (name, "MUST+SHOULD", k, opt[i]))
        # MUST_NOT
        nots = [(oracle.OP_TERM, [ns.PLANTED], [ns.HALF]), (oracle.OP_TERM, [ns.EVERY_DOC], [ns.HALF, ns.BITMAP]), (oracle.OP_AND, [ns.HALF, ns.EVERY_DOC], [ns.PLANTED]),
                (oracle.OP_OR, [ns.PLANTED, ns.CROSSED, ns.SPARSE], [ns.BITMAP]), (oracle.OP_OR, [ns.ZERO_FRONT, ns.ZERO_DEEP], [ns.HALF, ns.ABSENT]),
                (oracle.OP_TERM, [ns.ZERO_DEEP], [ns.SINGLETON]), (oracle.OP_AND, [ns.BITMAP, ns.HALF], [ns.ABOVE_DENSITY, ns.SPARSE])]
        for k in (10, 100):
            _check_not_queries(oracle, osr, g, nots, k)
        # FILTER: required, weight 0
        filt = [([ns.PLANTED], [ns.EVERY_DOC]), ([ns.HALF, ns.BITMAP], [ns.EVERY_DOC]), ([], [ns.ZERO_DEEP, ns.EVERY_DOC]), ([ns.ZERO_FRONT], [ns.HALF]),
                ([ns.EVERY_DOC], [ns.CROSSED])]
        fq = [Bq.build([T(t) for t in m], [], filters=[T(t) for t in f]) for m, f in filt]
        for k in (10, 100):
            hits, totals = g.search_batch(fq, k)
            for i, (m, f) in enumerate(filt):
                want = osr.search(oracle.OP_AND, m + f, k, tie_mode=oracle.TIE_CANONICAL, boosts=[1.0] * len(m) + [0.0] * len(f))
                _assert_row(hits[i], totals[i], want, (name, "FILTER", k, filt[i]))
        # min_should_match (clause-order sums, bit-exact past ten clauses too)
        msm = [([ns.PLANTED, ns.HALF, ns.BITMAP], 2, []), ([ns.EVERY_DOC, ns.ZERO_FRONT, ns.ZERO_DEEP, ns.HALF], 2, [ns.BITMAP]), (OR10 + [ns.HALF, ns.EVERY_DOC], 3, []),
               ([ns.HALF, ns.EVERY_DOC, ns.BITMAP, ns.CROSSED], 3, []), ([ns.SINGLETON, ns.EVERY_DOC], 2, [])]
        mq = [Bq.build([], [T(t) for t in p], must_nots=[T(t) for t in n], min_should_match=m) for p, m, n in msm]
        offs = np.concatenate([[0], np.cumsum([len(p) for p, _, _ in msm])]).astype(np.int32)
        noffs = np.concatenate([[0], np.cumsum([len(n) for _, _, n in msm])]).astype(np.int32)
        tids = np.concatenate([np.asarray(p, np.int64) for p, _, _ in msm])
        nids = np.concatenate([np.asarray(n, np.int64) for _, _, n in msm])
        for k in (10, 100):
            hits, totals = g.search_batch(mq, k)
            cd, cs, cc, ct, _, _ = osr.search_batch(np.full(len(msm), oracle.OP_OR, np.int32), offs, tids, k, tie_mode=oracle.TIE_CANONICAL, threads=4,
                                                    not_offsets=noffs, not_ids=nids, min_should_match=np.asarray([m for _, m, _ in msm], np.int32))
            for i in range(len(msm)):
                n = int(cc[i])
                _assert_row(hits[i], totals[i], (cd[i, :n], cs[i, :n], ct[i]), (name, "min_should_match", k, msm[i]))
        # "+a +(b c)": a disjunction under MUST, rows put together from the oracle's scorers child by child
        df = lambda t: int(sp.seg.terms[t]["doc_freq"])   # noqa: E731
        docs_of = lambda t: sp.lists[t][0]                # noqa: E731
        cases = [([ns.PLANTED], [ns.HALF, ns.EVERY_DOC], [], 1), ([ns.HALF], [ns.ZERO_FRONT, ns.PLANTED], [], 0), ([ns.BITMAP, ns.EVERY_DOC], [ns.CROSSED, ns.SPARSE], [ns.HALF], 2),
                 ([ns.ZERO_DEEP], [ns.BITMAP, ns.HALF], [], 1)]
        for k in (10, 100):
            nq, expect = [], []
            for musts, shoulds, mn, at in cases:
                clauses = [T(t) for t in musts]
                clauses.insert(at, Bq.build([], [T(t) for t in shoulds]))
                nq.append(Bq.build(clauses, [], must_nots=[T(t) for t in mn]))
                expect.append(_conjunction_with_a_nested_child(oracle, osr, docs_of, df, musts, shoulds, True, mn, at, k))
            assert sum(e[0] for e in expect) > 1000
            _check_nested_rows(g, nq, expect, cases, k)
    finally:
        ctx.close()


# ---- phrases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deletions", [False, True], ids=["all-live", "deletions"])
@pytest.mark.parametrize("name", PHRASE_SPECTRA)
def test_exact_and_sloppy_phrases(oracle, name, deletions):
    """Two- and three-term phrases, slop 0 and 2, over a positions field with the spectrum's norms (search_phrase.hpp selects between
    ranks and raw bytes in three places), with and without deleted docs."""
    import rucene_amd
    sp = ns.spectrum(name)
    seg, phrases, doc_count, sum_ttf = sp.positions()
    live = None
    if deletions:
        alive = np.random.default_rng(3).random(ns.MAX_DOC) < 0.7
        live = np.packbits(alive, bitorder="little")
        live = np.concatenate([live, np.zeros((-live.size) % 8, np.uint8)]).view(np.uint64)
    ctx = _context()
    try:
        leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
        leaf.live_docs, leaf.doc_count, leaf.sum_total_term_freq = live, doc_count, sum_ttf
        ix = oracle.PositionsIndex.from_files(seg.doc_bytes, seg.pos_bytes, seg.terms, leaf.term_positions)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        queries = [rucene_amd.PhraseQuery(t, slop=sl) for t, sl in phrases]
        matched = 0
        for k in (10, 100, 300):
            hits, totals = g.search_phrase_batch(queries, k)
            for i, q in enumerate(queries):
                want = ix.phrase_search(q.terms, k, sp.norms, ns.MAX_DOC, doc_count, sum_ttf, slop=q.slop, live_docs=live)
                _assert_row(hits[i], totals[i], want, (name, "phrase", q.terms, q.slop, k))
                matched += want[2]
        assert matched > 1000
        ix.close()
    finally:
        ctx.close()


# ---- the rescorer, k above 128, live docs, the sharded call -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rank64", "raw65"])
def test_rescorer_large_k_live_docs_and_the_sharded_call(oracle, name):
    import torch
    import rucene_amd
    from rucene_amd import _lib as gpu
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    sp = ns.spectrum(name)
    osr = _osr(oracle, name)
    ctx = _context()
    try:
        g, leaf = _searcher(sp, ctx)
        # QueryRescorer: first passes of k = 100, every mode
        first = [T(ns.PLANTED), T(ns.ZERO_DEEP), Bq.build([], [T(ns.CROSSED), T(ns.HALF)]), Bq.build([T(ns.HALF), T(ns.EVERY_DOC)], [])]
        seconds = [(oracle.OP_TERM, [ns.EVERY_DOC]), (oracle.OP_OR, [ns.HALF, ns.BITMAP]), (oracle.OP_AND, [ns.EVERY_DOC, ns.HALF]), (oracle.OP_TERM, [ns.ZERO_FRONT])]
        gq = [T(t[0]) if op == oracle.OP_TERM else (Bq.build([T(x) for x in t], []) if op == oracle.OP_AND else Bq.build([], [T(x) for x in t])) for op, t in seconds]
        hits, totals = g.search_batch(first, 100)
        for mode in range(5):
            for window, qw, rw in ((100, 1.0, 1.0), (37, 1.3, 0.25)):
                got = g.rescore_batch(hits, gq, query_weight=qw, rescore_weight=rw, mode=mode, window_size=window)
                for i, (op, tids) in enumerate(seconds):
                    n = int((hits[i]["doc"] >= 0).sum())
                    wd, ws = osr.rescore(op, tids, hits[i]["doc"][:n], hits[i]["score"][:n], window, qw, rw, mode)
                    assert (got[i]["doc"][:n] == wd).all() and (got[i]["doc"][n:] == -1).all(), (name, mode, window, i)
                    assert (got[i]["score"][:n].view(np.int32) == ws.view(np.int32)).all(), (name, mode, window, i)
        # k above 128: passes
        specs = [(oracle.OP_TERM, [t]) for t in (ns.PLANTED, ns.CROSSED, ns.ZERO_FRONT, ns.ZERO_DEEP, ns.EVERY_DOC, ns.RANDOM0 + 4)]
        specs += [(oracle.OP_AND, [ns.PLANTED, ns.EVERY_DOC]), (oracle.OP_AND, [ns.HALF, ns.BITMAP, ns.EVERY_DOC]), (oracle.OP_OR, [ns.ZERO_DEEP, ns.SPARSE]),
                  (oracle.OP_OR, [ns.PLANTED, ns.CROSSED, ns.HALF])]
        for k in (129, 300, 1000):
            _check_against_oracle(oracle, osr, g, specs, k)
            _check_against_oracle(oracle, osr, g, [(oracle.OP_OR, OR10), (oracle.OP_OR, WIDE_SPECS[1])], k, exact=False)
        # the sharded call in a world of one: the local search's rows, which are the oracle's
        queries = [T(ns.PLANTED), T(ns.ZERO_DEEP), Bq.build([T(ns.CROSSED), T(ns.EVERY_DOC)], []), Bq.build([], [T(ns.PLANTED), T(ns.SPARSE), T(ns.ZERO_FRONT)]),
                   Bq.build([], [T(t) for t in OR10])]
        packed = g.pack(queries, leaf)
        comm = gpu.Comm(ctx, 1, 0, gpu.comm_unique_id())
        for k in (10, 100):
            want_h, want_t = leaf.segment.search_batch(packed[0], packed[1], k)
            dh = torch.zeros((len(queries), k), dtype=torch.int64, device="cuda")
            dt = torch.zeros((len(queries),), dtype=torch.int64, device="cuda")
            comm.search_batch_sharded(leaf.segment, packed[0], packed[1], k, dh.data_ptr(), dt.data_ptr())
            ctx.synchronize()
            got = dh.cpu().numpy().view(gpu.HIT_DTYPE).reshape(len(queries), k)
            assert (got["doc"] == want_h["doc"]).all() and (got["score"].view(np.int32) == want_h["score"].view(np.int32)).all(), (name, k)
            assert (dt.cpu().numpy() == want_t).all() and (comm.status() == 0).all()
            for i, (op, tids) in enumerate([(oracle.OP_TERM, [ns.PLANTED]), (oracle.OP_TERM, [ns.ZERO_DEEP]), (oracle.OP_AND, [ns.CROSSED, ns.EVERY_DOC]),
                                            (oracle.OP_OR, [ns.PLANTED, ns.SPARSE, ns.ZERO_FRONT])]):
                _assert_row(got[i], dt.cpu().numpy()[i], osr.search(op, tids, k, tie_mode=oracle.TIE_CANONICAL), (name, "sharded", k, i))
        comm.close()
        leaf.segment.close()
        # live docs: the best winner of the planted list deleted (the next one moves up), and every third doc besides
        top = int(sp.ranking(ns.PLANTED)[0])
        alive = np.ones(ns.MAX_DOC, bool)
        alive[np.setdiff1d(np.arange(0, ns.MAX_DOC, 3), sp.plants[ns.PLANTED][1])] = False
        alive[top] = False
        live = np.packbits(alive, bitorder="little")
        live = np.concatenate([live, np.zeros((-live.size) % 8, np.uint8)]).view(np.uint64)
        osr_live = oracle.Searcher([sp.oracle_segment(oracle, live_docs=live)])
        g2, leaf2 = _searcher(sp, ctx, live=live)
        rank = sp.ranking(ns.PLANTED, live=sp.plants[ns.PLANTED][1] != top)
        for k in (1, 10, 128):
            for fused in (True, False):
                rows, totals = _run_term(g2, leaf2, ALL_TERMS, k, fused)
                _assert_ranking(rows[ns.PLANTED], rank, min(k, rank.size), (name, "live docs", k, fused))
                for t in ALL_TERMS:
                    _assert_row(rows[t], totals[t], osr_live.search(oracle.OP_TERM, [t], k, tie_mode=oracle.TIE_CANONICAL), (name, "live docs", k, fused, t))
        for k in (10, 300):
            _check_against_oracle(oracle, osr_live, g2, [(oracle.OP_AND, s) for s in AND_SPECS[:6]] + [(oracle.OP_OR, s) for s in OR_SPECS[:4]], k)
            _check_against_oracle(oracle, osr_live, g2, [(oracle.OP_OR, OR10)], k, exact=False)
    finally:
        ctx.close()


# ---- the config switch --------------------------------------------------------------------------------------------------------
def test_raw_norms_switch_gives_the_rows_of_rank_mode(oracle):
    """raw_norms=True on rank64 (raw bytes in HBM, no table, no pruning) against the default context on rank64 (ranks): the same rows
    bit for bit, below ten clauses and for TERM / AND; both against the oracle."""
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    sp = ns.spectrum("rank64")
    queries = [T(t) for t in ALL_TERMS] + [Bq.build([T(t) for t in s], []) for s in AND_SPECS] + [Bq.build([], [T(t) for t in s]) for s in OR_SPECS]
    queries += [Bq.build([T(ns.PLANTED)], [T(ns.EVERY_DOC)]), Bq.build([T(ns.HALF)], [], must_nots=[T(ns.BITMAP)])]
    specs = [(oracle.OP_TERM, [t]) for t in ALL_TERMS] + [(oracle.OP_AND, s) for s in AND_SPECS] + [(oracle.OP_OR, s) for s in OR_SPECS]
    rows = {}
    for raw in (False, True):
        ctx = _context(raw_norms=raw)
        try:
            g, leaf = _searcher(sp, ctx)
            for k in (10, 128, 300):
                rows[(raw, k)] = g.search_batch(queries, k)
                _check_against_oracle(oracle, _osr(oracle, "rank64"), g, specs, k)
            _run_term(g, leaf, [ns.PLANTED], 7, True)
            _run_term(g, leaf, [ns.PLANTED], 7, True)
            decoded = ctx.last_search_counters()["blocks_decoded"]
            assert (decoded == ns.PLANTED_BLOCKS) == raw, (raw, decoded)
        finally:
            ctx.close()
    for k in (10, 128, 300):
        (h0, t0), (h1, t1) = rows[(False, k)], rows[(True, k)]
        assert (t0 == t1).all() and (h0["doc"] == h1["doc"]).all() and (h0["score"].view(np.int32) == h1["score"].view(np.int32)).all(), k
