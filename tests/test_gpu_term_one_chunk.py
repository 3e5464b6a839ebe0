"""The one-chunk path of k_search_term_query (`-m gpu`; kernels/search_term_query.hpp): table-path lists of at most
RGPU_TERM_SHORT_BLOCKS FullBlocks — no chunk frontier, no queue, no lock: a ballot of survivors dealt to the waves by rank, a private
top-k per wave, the tail beside the blocks in wave W - 1, one merge. Through search_uniform_device, against the oracle bit for bit
(docs, score bits, totals; TIE_CANONICAL): every block count at which the deal changes (0, 1, 2, W - 1, W, W + 1, 4 W, 4 W + 1, 15,
16 — the first with a sketch —, 17, 63, 64, and 65 on the general path) with tails of 0, 1 and 127 postings, W 2 / 4 / 8, k 1 .. 128,
bp128 and legacy blocks; lists whose postings all tie, with the winners in block 0, in the last block, in the tail, and a k-th band
over the blocks of four waves; a freq outside the score table; the same rows under RGPU_TERM_SHORT_BLOCKS 0 / 15 / 64 and under the
work-item kernel; short lists off the table path; 200 enqueue-only calls of two layouts on two streams."""
import numpy as np
import pytest

from test_gpu_term_query import _assert_row, _context, _fused, _launches

pytestmark = pytest.mark.gpu

KS = [1, 10, 64, 65, 128]
MAX_DOC = 50_000
BLOCKS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 32, 33, 63, 64, 65]   # {W - 1, W, W + 1, 4 W, 4 W + 1} for W = 2, 4, 8 and the path's edges
TAILS = [0, 1, 127]


def _sizes_segment(version=1, seed=21):
    """one list per (block count, tail), a list of 300 blocks, and — (0, 0) — a term the leaf does not hold; freqs 1 .. 5 and 35
    norm values: few score levels, so ties with the threshold are the rule"""
    from rucene_amd import indexgen
    rng = np.random.default_rng(seed)
    sizes = [128 * nb + t for nb in BLOCKS for t in TAILS] + [128 * 300 + 9]
    lists = []
    for n in sizes:
        d = np.sort(rng.choice(MAX_DOC, size=n, replace=False)).astype(np.int32)
        lists.append((d, rng.integers(1, 6, size=n).astype(np.int32)))
    norms = rng.integers(90, 125, size=MAX_DOC).astype(np.uint8)
    seg = indexgen.build_explicit(MAX_DOC, lists, norms=norms, version=version)
    return seg, int(sum(int(f.sum()) for _, f in lists)), len(sizes)


class _Wanted:
    """the oracle's rows of every list of a segment, computed once per k and shared"""

    def __init__(self, oracle, seg, sttf, n, live=None, norms=True):
        self.oracle, self.n = oracle, n
        self.osr = oracle.Searcher([oracle.Segment(seg.doc_bytes, seg.norms if norms else None, MAX_DOC, seg.terms, live_docs=live, sum_total_term_freq=sttf)])
        self.rows = {}

    def __call__(self, k):
        if k not in self.rows:
            self.rows[k] = [self.osr.search(self.oracle.OP_TERM, [t], k, tie_mode=self.oracle.TIE_CANONICAL) for t in range(self.n)]
        return self.rows[k]


@pytest.fixture(scope="module")
def sized(oracle):
    out = {}
    for version in (1, 0):
        seg, sttf, n = _sizes_segment(version)
        out[version] = (seg, sttf, n, _Wanted(oracle, seg, sttf, n))
    return out


def _check_all(g, leaf, ids, k, wanted, what):
    rows, totals = _fused(g, leaf, ids, k)
    want = wanted(k)
    for j, t in enumerate(ids):
        _assert_row(rows[j], totals[j], want[int(t)], (what, k, j, int(t)))
    return rows, totals


def _gpu_leaf(ctx, seg, sttf, live=None, norms=True):
    import rucene_amd
    leaf = rucene_amd.LeafReader(seg.doc_bytes, seg.norms if norms else None, MAX_DOC, seg.terms, live_docs=live, sum_total_term_freq=sttf)
    return rucene_amd.GpuIndexSearcher([leaf], ctx=ctx), leaf


@pytest.mark.parametrize("version", [1, 0], ids=["bp128", "legacy"])
@pytest.mark.parametrize("waves", ["4", "2", "8"])
def test_block_counts_and_tails(sized, waves, version):
    seg, sttf, n, wanted = sized[version]
    ctx = _context({"RGPU_TERM_QUERY_WAVES": waves})
    try:
        g, leaf = _gpu_leaf(ctx, seg, sttf)
        ids = list(range(n)) + list(range(n - 1, -1, -1))
        _fused(g, leaf, ids, 10)   # (the first call prepares the terms through the full path and builds the sketches)
        n0 = _launches(ctx, "term_query_launches")
        for k in KS:
            _check_all(g, leaf, ids, k, wanted, ("sizes", waves, version))
        assert _launches(ctx, "term_query_launches") - n0 == len(KS)
    finally:
        ctx.close()


def _ties_segment(seed=33):
    """lists of 16 blocks + 40 postings (one chunk, four blocks per wave at W = 4) under one norm value, scores by freq alone:
    0: every posting ties — the k lowest docs win, all of block 0;  1: the winners (freq 3) are the last block's first postings;
    2: the winners are in the tail;  3: six clear winners (freq 5), then a band of freq 3 with three members in each of blocks
    0 .. 7 — a k-th band over the blocks of every wave;  4: a three-block list with one freq above the score table"""
    from rucene_amd import indexgen
    rng = np.random.default_rng(seed)
    n = 128 * 16 + 40
    lists = []
    for case in range(4):
        d = np.sort(rng.choice(MAX_DOC, size=n, replace=False)).astype(np.int32)
        f = np.ones(n, np.int32)
        if case == 1:
            f[128 * 15:128 * 15 + 12] = 3
        elif case == 2:
            f[128 * 16 + 5:128 * 16 + 17] = 3
        elif case == 3:
            for b in range(8):
                f[128 * b + rng.choice(128, size=3, replace=False)] = 3
            f[rng.choice(n, size=6, replace=False)] = 5
        lists.append((d, f))
    d = np.sort(rng.choice(MAX_DOC, size=128 * 3 + 11, replace=False)).astype(np.int32)
    f = rng.integers(1, 4, size=d.size).astype(np.int32)
    f[200] = 50
    lists.append((d, f))
    norms = np.full(MAX_DOC, 100, np.uint8)
    seg = indexgen.build_explicit(MAX_DOC, lists, norms=norms)
    return seg, int(sum(int(f.sum()) for _, f in lists)), len(lists), lists


@pytest.mark.parametrize("waves", ["4", "8"])
def test_ties_bands_and_a_freq_outside_the_table(oracle, waves):
    seg, sttf, n, lists = _ties_segment()
    wanted = _Wanted(oracle, seg, sttf, n)
    ctx = _context({"RGPU_TERM_QUERY_WAVES": waves})
    try:
        g, leaf = _gpu_leaf(ctx, seg, sttf)
        ids = list(range(n)) * 3
        _fused(g, leaf, ids, 10)
        for k in KS:
            rows, _ = _check_all(g, leaf, ids, k, wanted, ("ties", waves))
            m = min(k, 128)
            assert (rows[0]["doc"][:m] == lists[0][0][:m]).all()   # every posting ties: the lowest docs, block 0's
        rows, _ = _check_all(g, leaf, ids, 10, wanted, ("ties", waves))
        assert (rows[1]["doc"] == lists[1][0][128 * 15:128 * 15 + 10]).all()
        assert (rows[2]["doc"] == lists[2][0][128 * 16 + 5:128 * 16 + 15]).all()
        assert rows[4]["doc"][0] == lists[4][0][200]   # the freq of 50
    finally:
        ctx.close()


def test_identical_rows_across_settings(sized):
    """RGPU_TERM_SHORT_BLOCKS 0 (the path off) / 15 / 64 and the work-item kernel: the same rows, totals and postings_covered; what the
    kernel counts as requested covers every block it unpacked"""
    seg, sttf, n, wanted = sized[1]
    ids = list(range(n)) * 2
    seen = {}
    for name, env in (("0", {"RGPU_TERM_SHORT_BLOCKS": "0"}), ("15", {"RGPU_TERM_SHORT_BLOCKS": "15"}), ("64", {"RGPU_TERM_SHORT_BLOCKS": "64"}),
                      ("items", {"RGPU_TERM_KERNEL": "items"})):
        ctx = _context(env)
        try:
            g, leaf = _gpu_leaf(ctx, seg, sttf)
            _fused(g, leaf, ids, 10)
            for k in (10, 128):
                rows, totals = _check_all(g, leaf, ids, k, wanted, ("settings", name))
                c = ctx.last_search_counters()
                seen[(name, k)] = (rows.copy(), totals.copy(), c["postings_covered"])
                if name in ("0", "64"):
                    assert c["blocks_decoded"] > 0 and c["touched_bytes"] >= (128 + 18) * c["blocks_decoded"], (name, k, c)
            assert (_launches(ctx, "term_query_launches") > 0) == (name != "items")
        finally:
            ctx.close()
    for k in (10, 128):
        r0, t0, c0 = seen[("0", k)]
        for name in ("15", "64", "items"):
            r, t, c = seen[(name, k)]
            assert (r["doc"] == r0["doc"]).all() and (r["score"].view(np.int32) == r0["score"].view(np.int32)).all(), (name, k)
            assert (t == t0).all() and c == c0, (name, k, c, c0)


@pytest.mark.parametrize("case", ["live docs", "raw norms", "no norms"])
def test_short_lists_off_the_table_path(oracle, sized, case):
    seg, sttf, n, _ = sized[1]
    live, cfg, norms = None, {}, True
    if case == "live docs":
        alive = np.ones(MAX_DOC, bool)
        alive[::7] = False
        live = np.packbits(alive, bitorder="little")
        live = np.concatenate([live, np.zeros((-live.size) % 8, np.uint8)]).view(np.uint64)
    elif case == "raw norms":
        cfg["raw_norms"] = True
    else:
        norms = False
    wanted = _Wanted(oracle, seg, sttf, n, live=live, norms=norms)
    ctx = _context(**cfg)
    try:
        g, leaf = _gpu_leaf(ctx, seg, sttf, live=live, norms=norms)
        for k in (10, 65):
            _check_all(g, leaf, list(range(n)), k, wanted, case)
    finally:
        ctx.close()


def test_200_enqueue_only_calls_of_two_layouts_on_two_streams(sized):
    """No synchronize in between: a batch of short lists only and one mixed with long lists and absent ids alternate on two streams;
    every call's rows are compared on the device with the first call's of its layout."""
    import torch
    from rucene_amd import _lib as gpu
    seg, sttf, n, wanted = sized[1]
    short = [t for t in range(n - 1) if BLOCKS[t // len(TAILS)] <= 64 and (t // len(TAILS), t % len(TAILS)) != (0, 0)]
    batches = [np.array(short + short[::-1]), np.array([n - 1, 0, 5, n - 4, n - 3, n - 2, -1, n + 7, 20, n - 1, 0] + short[::3])]
    k = 10
    ctx = _context()
    try:
        g, leaf = _gpu_leaf(ctx, seg, sttf)
        first = []
        for b in range(2):
            rows, totals = _fused(g, leaf, batches[b], k)
            want = wanted(k)
            for j, t in enumerate(batches[b]):
                if 0 <= t < n:
                    _assert_row(rows[j], totals[j], want[int(t)], ("first", b, j))
                else:
                    assert totals[j] == 0 and (rows[j]["doc"] == -1).all()
            first.append((torch.from_numpy(rows.view(np.int64).copy()).cuda(), torch.from_numpy(totals.copy()).cuda()))
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [(torch.full((len(batches[i % 2]), k), -3, dtype=torch.int64, device="cuda"), torch.full((len(batches[i % 2]),), -3, dtype=torch.int64, device="cuda"))
                for i in range(200)]
        n0 = _launches(ctx, "term_query_launches")
        torch.cuda.synchronize()
        for i in range(200):
            b = i % 2
            sel = np.asarray(batches[b], dtype=np.int64).reshape(-1, 1)
            g.search_uniform_device(gpu.OP_TERM, sel, leaf, k, outs[i][0].data_ptr(), outs[i][1].data_ptr(), stream=streams[b].cuda_stream)
        ctx.synchronize()
        for s in streams:
            s.synchronize()
        same = torch.stack([(outs[i][0] == first[i % 2][0]).all() & (outs[i][1] == first[i % 2][1]).all() for i in range(200)])
        assert bool(same.all()), [i for i in range(200) if not bool(same[i])][:8]
        assert _launches(ctx, "term_query_launches") - n0 == 200
    finally:
        ctx.close()
