"""Work-item bounds (`-m gpu`): every kernel that cuts a posting list into work items walks each item with a loop of its own, and
an item that stops early is invisible to fixtures whose postings mostly tie (ties go to the lowest doc id, so the last blocks of a
long list rarely reach a top-k, and hit counts come from item bounds, not from what was scored). Here a long list of low,
equal-scoring background postings carries PLANTED postings of strictly distinct (freq, norm byte) scores at the blocks where an
item loop can go wrong: block 0, either side of 4096 blocks (64 chunks of 64 blocks: one 64-bit chunk mask) and of 8192, the last
full block and the VInt tail. The top-k is then exactly the planted set, in an order no truncated walk matches by luck. Every
row is checked twice: against the oracle, bit for bit, and against a float64 BM25 of the plants computed here in numpy (so a kernel
and an oracle that fail alike still fail)."""
import os

import numpy as np
import pytest

from norm_spectrum import _byte315_to_float, bm25_f64  # noqa: F401 (one copy, shared with the norm-spectrum fixtures)

pytestmark = pytest.mark.gpu

FULL_BLOCKS = 9000           # one item of the largest sizes spans three 4096-block windows
TAIL = 77                    # VInt tail: df is not a multiple of 128
DF = 128 * FULL_BLOCKS + TAIL
MAX_DOC = 1_200_000
BG_NORM = 100                # every background posting: freq 1, this norm byte
IN_BLOCK = 77                # a plant's position inside its block
# (block, freq, norm byte) of the winners, scores strictly distinct and NOT in doc order; "tail" = the VInt tail
WINNERS = [(0, 6, 124), (4095, 9, 120), (4096, 10, 124), (4097, 8, 120), (8191, 7, 124), (8192, 10, 120),
           (FULL_BLOCKS - 1, 9, 124), ("tail", 8, 124)]
LOSER = (2080, 3, 110)       # mid-chunk (chunk 32, lane 32): above the background, below every winner — pruned for k <= 8
OUT_OF_TABLE = 1000          # the out-of-table variant: the winner at block 4097 gets this freq (> SCORE_TABLE_FREQS)


def _pos(block):
    return 128 * FULL_BLOCKS + 40 if block == "tail" else 128 * block + IN_BLOCK


class Planted:
    """The segment: term 0 the planted list (winners' freqs inside the score table), term 1 the same docs with one winner's freq far
    above it, term 2 every doc of the segment at freq 1 (a dense clause for AND / OR), term 3 a short list through the plants (a
    SHOULD clause)."""

    def __init__(self):
        from rucene_amd import indexgen
        rng = np.random.default_rng(4096)
        self.docs = np.sort(rng.choice(MAX_DOC, size=DF, replace=False)).astype(np.int32)
        freqs = np.ones(DF, np.int32)
        self.norms = np.full(MAX_DOC, BG_NORM, np.uint8)
        plants = WINNERS + [LOSER]
        self.plant_pos = np.array([_pos(p[0]) for p in plants])
        self.plant_docs = self.docs[self.plant_pos]
        freqs[self.plant_pos] = [p[1] for p in plants]
        self.norms[self.plant_docs] = [p[2] for p in plants]
        self.freqs = freqs
        self.freqs_oot = freqs.copy()
        self.freqs_oot[_pos(4097)] = OUT_OF_TABLE
        dense = np.arange(MAX_DOC, dtype=np.int32)
        short = np.sort(np.concatenate([self.plant_docs, rng.choice(MAX_DOC, size=500, replace=False).astype(np.int32)]))
        short = np.unique(short)
        self.lists = [(self.docs, self.freqs), (self.docs, self.freqs_oot), (dense, np.ones(MAX_DOC, np.int32)),
                      (short, np.full(short.size, 2, np.int32))]
        self.seg = indexgen.build_explicit(MAX_DOC, self.lists, norms=self.norms)
        self.sttf = 3 * MAX_DOC
        self.avgdl = float(np.float32(self.sttf / MAX_DOC))
        # the winners must be strictly ordered with room to spare for f32 rounding, the loser below them all
        for freqs_ in (self.freqs, self.freqs_oot):
            s = bm25_f64(DF, MAX_DOC, self.avgdl, freqs_[self.plant_pos], self.norms[self.plant_docs])
            w = np.sort(s[:len(WINNERS)])
            assert (np.diff(w) > 1e-4 * w[1:]).all() and s[-1] < w[0] * (1 - 1e-4)
            bg = bm25_f64(DF, MAX_DOC, self.avgdl, 1, BG_NORM)
            assert s[-1] > bg * (1 + 1e-4)

    def ranking(self, term, live=None, norms=True, extra=None):
        """Planted docs of `term` (0 / 1) ranked by float64 BM25, ties to the lower doc; `extra(docs) -> float64` adds other
        clauses' scores; `live`: boolean mask over the plants (deleted plants leave)."""
        f = (self.freqs if term == 0 else self.freqs_oot)[self.plant_pos]
        s = bm25_f64(DF, MAX_DOC, self.avgdl, f, self.norms[self.plant_docs] if norms else None)
        if extra is not None:
            s = s + extra(self.plant_docs)
        docs = self.plant_docs
        if live is not None:
            s, docs = s[live], docs[live]
        order = np.lexsort((docs, -s))
        return docs[order]


@pytest.fixture(scope="module")
def planted():
    return Planted()


@pytest.fixture(scope="module")
def term_want(planted, oracle):
    """The oracle's TERM rows of the planted lists, once for the whole sweep."""
    seg = planted.seg
    osearcher = oracle.Searcher([oracle.Segment(seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sum_total_term_freq=planted.sttf)])
    return {(t, k): osearcher.search(oracle.OP_TERM, [t], k, tie_mode=oracle.TIE_CANONICAL) for t in (0, 1) for k in TERM_KS}


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
    assert (row["doc"][:d.size] == d).all() and (row["doc"][d.size:] == -1).all(), (what, "docs", "missing", missing[:10])
    assert (row["score"][:d.size].view(np.int32) == sc.view(np.int32)).all(), (what, "score bits")


def _assert_ranking(row, ranking, k, what):
    n = min(k, ranking.size)
    assert (row["doc"][:n] == ranking[:n]).all(), (what, "float64 ranking", row["doc"][:n], ranking[:n])


TERM_ITEM_SIZES = [0, 64, 96, 4095, 4096, 4097, 6000, 8192, 16384, 131072]
TERM_KS = [1, 10, 64, 128]


@pytest.mark.parametrize("fold", ["1", "0"], ids=["fold", "merge-launch"])
@pytest.mark.parametrize("bpi", TERM_ITEM_SIZES)
def test_term_items_of_any_size_reach_every_block(planted, term_want, bpi, fold):
    """Guards term_blocks_fast's chunk mask (one bit per 64-block chunk, 64 bits): an item of more than 4096 blocks must still visit
    every chunk behind the first 64. Plants at blocks 0, 4095-4097, 8191-8192, 8999 (the last full block) and in the VInt tail of a
    9000-block list, a pruned loser at block 2080; winners inside the score table (term 0, the pruned fast path) and one far above it
    (term 1: the in_table == false branch). Item sizes from 64 to 1 << 17 blocks, the library's own (0) and callers' non-powers of
    two, k 1..128, through the two-call path and the fused call, with the query's items folded inside the launch and in a launch of
    their own."""
    import rucene_amd
    seg = planted.seg
    want = term_want
    rank = {t: planted.ranking(t) for t in (0, 1)}
    ctx = _context({"RGPU_TERM_FOLD": fold}, blocks_per_item=bpi)
    try:
        leaf = rucene_amd.LeafReader(seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sum_total_term_freq=planted.sttf)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        for k in TERM_KS:
            for fused in (False, True):
                rows, totals = _run_term(g, leaf, [0, 1, 0], k, fused)
                for j, t in enumerate((0, 1, 0)):
                    what = (bpi, fold, k, "fused" if fused else "two calls", t)
                    assert totals[j] == DF, what
                    _assert_ranking(rows[j], rank[t], k if k <= len(WINNERS) else len(WINNERS), what)
                    _assert_row(rows[j], totals[j], want[(t, k)], what)
        assert ctx.kernel_stats()["fused_term_batches"]["launches"] >= len(TERM_KS)
    finally:
        ctx.close()


def test_term_item_size_range_is_checked_at_init():
    """Guards rgpu_init's range for rgpu_config.blocks_per_item: 0 (auto) .. 1 << 17 (the doubling loops' ceiling) are taken, a
    negative size or one above the ceiling is an ILLEGAL_ARGUMENT error, not a context whose items the kernels cannot cut."""
    import rucene_amd
    for bpi in (0, 1, 1 << 17):
        rucene_amd.Context(blocks_per_item=bpi).close()
    for bpi in (-1, (1 << 17) + 1, 1 << 30):
        with pytest.raises(rucene_amd.RgpuError) as e:
            rucene_amd.Context(blocks_per_item=bpi)
        assert e.value.status == -2, bpi


@pytest.mark.parametrize("bpi", [0, 4097, 8192, 131072])
def test_term_items_with_live_docs_and_without_norms(planted, oracle, bpi):
    """Guards stream_blocks as k_search_term's general path walks it (live docs; a field without norms): the same planted list, the
    top winner (block 4096) deleted so that the next one must move up, and again with no norms at all (scores by freq alone, ties to
    the lower doc). Item sizes up to 1 << 17 blocks, k 1..128, two-call and fused."""
    import rucene_amd
    seg = planted.seg
    top = int(planted.plant_docs[2])  # WINNERS[2]: block 4096, the best of term 0
    live = np.full((MAX_DOC + 63) // 64, ~np.uint64(0), dtype=np.uint64)
    live[-1] = np.uint64((1 << (MAX_DOC % 64 or 64)) - 1)
    live[top // 64] &= ~np.uint64(1 << (top % 64))
    keep = planted.plant_docs != top
    cases = [("live docs", seg.norms, live, planted.ranking(0, live=keep), DF - 1),
             ("no norms", None, None, planted.ranking(0, norms=False), DF)]
    ctx = _context(blocks_per_item=bpi)
    try:
        for what, norms, lv, rank, df_live in cases:
            oseg = oracle.Segment(seg.doc_bytes, norms, MAX_DOC, seg.terms, live_docs=lv, sum_total_term_freq=planted.sttf)
            osearcher = oracle.Searcher([oseg])
            leaf = rucene_amd.LeafReader(seg.doc_bytes, norms, MAX_DOC, seg.terms, live_docs=lv, sum_total_term_freq=planted.sttf)
            g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
            for k in TERM_KS:
                want = osearcher.search(oracle.OP_TERM, [0], k, tie_mode=oracle.TIE_CANONICAL)
                for fused in (False, True):
                    rows, totals = _run_term(g, leaf, [0], k, fused)
                    w = (what, bpi, k, fused)
                    assert totals[0] == df_live, w
                    if norms is not None:  # (without norms the plants tie with each other by freq; the oracle's row decides)
                        _assert_ranking(rows[0], rank, min(k, len(WINNERS) - 1), w)
                    _assert_row(rows[0], totals[0], want, w)
    finally:
        ctx.close()


def test_decode_terms_returns_every_item_of_a_long_list(planted):
    """Guards k_decode_terms' items (RGPU_DEC_BPI blocks each): every doc and freq of the 9000-block planted lists (and the dense
    1.2 M-doc list) against the arrays they were built from, so that a dropped item shows as missing postings."""
    import rucene_amd
    seg = planted.seg
    ctx = rucene_amd.Context()
    try:
        gseg = rucene_amd.Segment(ctx, seg.doc_bytes, seg.norms, MAX_DOC)
        docs, freqs = gseg.decode_terms(seg.terms[[0, 1, 2]])
        want_d = np.concatenate([planted.lists[t][0] for t in (0, 1, 2)])
        want_f = np.concatenate([planted.lists[t][1] for t in (0, 1, 2)])
        assert docs.size == want_d.size
        assert (docs == want_d).all(), np.flatnonzero(docs != want_d)[:10]
        assert (freqs == want_f).all(), np.flatnonzero(freqs != want_f)[:10]
    finally:
        ctx.close()


AND_ITEM_SIZES = [0, 1, 63, 64, 65, 72, 200, 5000]


@pytest.mark.parametrize("abpi", AND_ITEM_SIZES)
def test_and_lead_items_reach_every_block(planted, oracle, abpi):
    """Guards k_search_and's lead items and k_req_opt_scan's: the planted list leads (it is the shorter clause) and the dense clause
    holds every planted doc, so the AND top-k is the plants, ranked by their summed float64 scores. Lead item sizes of 1..5000 blocks
    and the library's own; with 1 block per item, a batch of 30 queries has 270 k items and search_pass doubles the size. A MUST +
    SHOULD query (planted MUST, short SHOULD through the plants) goes through the same cut."""
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    seg = planted.seg
    osearcher = oracle.Searcher([oracle.Segment(seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sum_total_term_freq=planted.sttf)])
    dense = lambda d: bm25_f64(MAX_DOC, MAX_DOC, planted.avgdl, 1, planted.norms[d])
    rank = {t: planted.ranking(t, extra=dense) for t in (0, 1)}
    ctx = _context(and_blocks_per_item=abpi)
    try:
        leaf = rucene_amd.LeafReader(seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sum_total_term_freq=planted.sttf)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        n_and = 30 if abpi == 1 else 2
        for k in (1, 10, 64):
            queries = [Bq.build([T(i % 2), T(2)], []) for i in range(n_and)]
            queries += [Bq.build([T(0)], [T(3)]), Bq.build([T(1), T(2)], [T(3)])]
            hits, totals = g.search_batch(queries, k)
            for i in range(n_and):
                t = i % 2
                w = ("AND", abpi, k, i)
                _assert_ranking(hits[i], rank[t], min(k, len(WINNERS)), w)
                _assert_row(hits[i], totals[i], osearcher.search(oracle.OP_AND, [t, 2], k, tie_mode=oracle.TIE_CANONICAL), w)
            _assert_row(hits[n_and], totals[n_and], osearcher.search_opt(oracle.OP_TERM, [0], [3], k), ("MUST+SHOULD", abpi, k))
            _assert_row(hits[n_and + 1], totals[n_and + 1], osearcher.search_opt(oracle.OP_AND, [1, 2], [3], k),
                        ("AND+SHOULD", abpi, k))
    finally:
        ctx.close()


def test_or_runs_reach_every_block(planted, oracle):
    """Guards k_score_terms' run items (32 blocks each, doubled past 1 M items; k_or_lazy reads the runs): a dense clause OR the
    planted list, and OR the out-of-table variant, k 1..128 — the top-k is the plants ranked by their summed float64 scores. (A batch
    past 1 048 576 run items would need ~3 700 distinct 9000-block lists: not built here.)"""
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    seg = planted.seg
    osearcher = oracle.Searcher([oracle.Segment(seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sum_total_term_freq=planted.sttf)])
    dense = lambda d: bm25_f64(MAX_DOC, MAX_DOC, planted.avgdl, 1, planted.norms[d])
    ctx = _context()
    try:
        leaf = rucene_amd.LeafReader(seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sum_total_term_freq=planted.sttf)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        specs = [[2, 0], [2, 1], [0, 2, 3]]
        for k in TERM_KS:
            hits, totals = g.search_batch([Bq.build([], [T(t) for t in s]) for s in specs], k)
            for i, s in enumerate(specs[:2]):
                _assert_ranking(hits[i], planted.ranking(s[1], extra=dense), min(k, len(WINNERS)), ("OR", s, k))
            for i, s in enumerate(specs):
                _assert_row(hits[i], totals[i], osearcher.search(oracle.OP_OR, s, k, tie_mode=oracle.TIE_CANONICAL), ("OR", s, k))
    finally:
        ctx.close()


def test_term_auto_item_size_doubled_past_4096_blocks(oracle):
    """Guards the library's own TERM item size (route: the item-count loops of search_pass and of the fused call double
    blocks_per_item up to 1 << 17 when a batch has more than 262 144 items; a list of at least 8 x the size keeps it). 40 000 queries
    on a 512-block list (8 items each) take the size to 1 << 17; one more query on a 66 000-block list then has items of 8192 blocks.
    Plants at blocks 4095-4097, 8191-8192, 40000, 65999 and the tail of that list, distinct scores; rows against the oracle (once
    per distinct term) and the float64 ranking, two-call and fused."""
    import rucene_amd
    from rucene_amd import indexgen
    nb_long, nb_short, nq_short = 66_000, 512, 40_000
    df_long = 128 * nb_long + 5
    max_doc = df_long + 1000
    docs = np.arange(df_long, dtype=np.int32)
    freqs = np.ones(df_long, np.int32)
    norms = np.full(max_doc, BG_NORM, np.uint8)
    plants = [(4095, 6, 124), (4096, 9, 120), (4097, 10, 124), (8191, 8, 120), (8192, 7, 124), (40_000, 10, 120),
              (nb_long - 1, 9, 124), (nb_long, 8, 124)]  # (the last: posting 2 of the tail)
    pos = np.array([128 * b + 2 for b, _, _ in plants])
    freqs[pos] = [p[1] for p in plants]
    norms[docs[pos]] = [p[2] for p in plants]
    short = np.arange(0, 2 * 128 * nb_short, 2, dtype=np.int32) + 1
    seg = indexgen.build_explicit(max_doc, [(docs, freqs), (short, np.ones(short.size, np.int32))], norms=norms)
    sttf = 3 * max_doc
    osearcher = oracle.Searcher([oracle.Segment(seg.doc_bytes, seg.norms, max_doc, seg.terms, sum_total_term_freq=sttf)])
    avgdl = float(np.float32(sttf / max_doc))
    s = bm25_f64(df_long, max_doc, avgdl, freqs[pos], norms[docs[pos]])
    rank = docs[pos][np.lexsort((docs[pos], -s))]
    ids = np.ones(nq_short + 1, np.int64)
    ids[nq_short // 2] = 0
    k = 10
    want = {t: osearcher.search(oracle.OP_TERM, [t], k, tie_mode=oracle.TIE_CANONICAL) for t in (0, 1)}
    ctx = _context()
    try:
        leaf = rucene_amd.LeafReader(seg.doc_bytes, seg.norms, max_doc, seg.terms, sum_total_term_freq=sttf)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        for fused in (False, True):
            rows, totals = _run_term(g, leaf, ids, k, fused)
            what = "fused" if fused else "two calls"
            _assert_ranking(rows[nq_short // 2], rank, len(plants), what)
            for t in (0, 1):
                sel = ids == t
                d, sc, tot = want[t]
                assert (totals[sel] == tot).all(), (what, t)
                assert (rows["doc"][sel] == d).all(), (what, t, np.flatnonzero(~(rows["doc"][sel] == d).all(axis=1))[:5])
                assert (rows["score"][sel].view(np.int32) == sc.view(np.int32)).all(), (what, t)
    finally:
        ctx.close()
