"""k_search_term_query (`-m gpu`): the fused single-term call's one-workgroup-per-query kernel (kernels/search_term_query.hpp) against
the oracle, bit for bit, and against the work-item kernel it replaces (RGPU_TERM_KERNEL=items). Cases: planted winners at the blocks
where a chunk or item loop can go wrong, a list whose candidates overflow the queue round after round, k 1..128, legacy (v0) and
docs-only fields, absent / df 1 / tail-only terms, deleted docs, raw norms, no norms, and many launches of alternating layouts."""
import os

import numpy as np
import pytest

from test_gpu_item_bounds import DF, MAX_DOC, WINNERS, Planted

pytestmark = pytest.mark.gpu

KS = [1, 10, 64, 100, 128]


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


def _fused(g, leaf, ids, k):
    import torch
    from rucene_amd import _lib as gpu
    sel = np.asarray(ids, dtype=np.int64).reshape(-1, 1)
    nq = sel.shape[0]
    hits = torch.full((nq, k), -3, dtype=torch.int64, device="cuda")
    totals = torch.full((nq,), -3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.search_uniform_device(gpu.OP_TERM, sel, leaf, k, hits.data_ptr(), totals.data_ptr())
    g.ctx.synchronize()
    return hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(nq, k), totals.cpu().numpy()


def _assert_row(row, total, want, what):
    d, sc, tot = want
    assert total == tot, (what, "total", int(total), tot)
    assert (row["doc"][:d.size] == d).all() and (row["doc"][d.size:] == -1).all(), (what, "docs", row["doc"][:8], d[:8])
    assert (row["score"][:d.size].view(np.int32) == sc.view(np.int32)).all(), (what, "score bits")


def _launches(ctx, name):
    st = ctx.kernel_stats()
    return st[name]["launches"] if name in st else 0


class _Leaf:
    """A segment on the GPU (searcher + leaf) and the oracle over the same bytes."""

    def __init__(self, ctx, oracle, doc_bytes, norms, max_doc, terms, sttf, live=None, **seg_kw):
        import rucene_amd
        self.leaf = rucene_amd.LeafReader(doc_bytes, norms, max_doc, terms, live_docs=live, sum_total_term_freq=sttf, **seg_kw)
        self.g = rucene_amd.GpuIndexSearcher([self.leaf], ctx=ctx)
        okw = {"has_freqs": False} if seg_kw.get("index_options") == 1 else {}
        self.osr = oracle.Searcher([oracle.Segment(doc_bytes, norms, max_doc, terms, live_docs=live, sum_total_term_freq=sttf, **okw)])


def _check(lf, oracle, ids, k, what):
    rows, totals = _fused(lf.g, lf.leaf, ids, k)
    for j, t in enumerate(ids):
        want = lf.osr.search(oracle.OP_TERM, [int(t)], k, tie_mode=oracle.TIE_CANONICAL)
        _assert_row(rows[j], totals[j], want, (what, k, j, int(t)))
    return rows, totals


@pytest.fixture(scope="module")
def planted():
    return Planted()


@pytest.mark.parametrize("waves", ["4", "2", "8"])
def test_planted_winners_every_k(planted, oracle, waves):
    """Plants at blocks 0, 4095-4097, 8191-8192, the last full block and the tail of a 9000-block list (term 0, inside the score
    table; term 1: one winner's freq above it), k 1..128, at every workgroup width: the oracle's rows, the float64 ranking of the
    plants, and the new kernel really ran."""
    seg = planted.seg
    ctx = _context({"RGPU_TERM_QUERY_WAVES": waves})
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, planted.sttf)
        rank = {t: planted.ranking(t) for t in (0, 1)}
        _fused(lf.g, lf.leaf, [0, 1], 10)  # (the first call prepares the terms through the full path)
        n0 = _launches(ctx, "term_query_launches")
        for k in KS:
            rows, totals = _check(lf, oracle, [0, 1, 0], k, ("planted", waves))
            for j, t in enumerate((0, 1, 0)):
                assert totals[j] == DF
                n = min(k, len(WINNERS))
                assert (rows[j]["doc"][:n] == rank[t][:n]).all(), (waves, k, t, rows[j]["doc"][:n], rank[t][:n])
        assert _launches(ctx, "term_query_launches") - n0 == len(KS)
    finally:
        ctx.close()


def _ramp_segment(levels=6, per_level=300, seed=11):
    """A list whose blocks' best postings rise level by level along the list (every block of a level ties with the others): without a
    starting threshold every queue round's candidates are beaten by the next round's, so the queue overflows round after round."""
    from rucene_amd import indexgen
    rng = np.random.default_rng(seed)
    nb = levels * per_level
    df = 128 * nb + 40
    max_doc = df + 5000
    docs = np.sort(rng.choice(max_doc, size=df, replace=False)).astype(np.int32)
    freqs = np.ones(df, np.int32)
    norms = np.full(max_doc, 100, np.uint8)
    plant = 128 * np.arange(nb) + 5
    freqs[plant] = 2 + np.arange(nb) // per_level  # 2 .. levels + 1: inside the table
    norms[docs[plant]] = 120
    short = np.sort(rng.choice(max_doc, size=3000, replace=False)).astype(np.int32)
    lists = [(docs, freqs), (short, np.ones(short.size, np.int32))]
    seg = indexgen.build_explicit(max_doc, lists, norms=norms)
    return seg, max_doc, int(freqs.sum() + short.size)


@pytest.mark.parametrize("sketch", ["1", "0"], ids=["sketch", "no-sketch"])
def test_ties_overflow_the_queue_in_rounds(oracle, sketch):
    """1800 blocks in six levels of 300 tying blocks each (plus a VInt tail): with and without block-max sketches, k 1..128, one query
    and a batch of many copies of it."""
    seg, max_doc, sttf = _ramp_segment()
    ctx = _context({"RGPU_TERM_SKETCH": sketch})
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, max_doc, seg.terms, sttf)
        for k in KS:
            _check(lf, oracle, [0, 1], k, ("ramp", sketch))
        _check(lf, oracle, [0] * 300 + [1] * 20, 10, ("ramp batch", sketch))
    finally:
        ctx.close()


def _edge_segment(version=1):
    """absent term, df 1, tail-only lists (2, 77, 127), exactly one block, one block + 1, a few blocks, a long list"""
    from rucene_amd import indexgen
    rng = np.random.default_rng(5)
    max_doc = 300_000
    sizes = [0, 1, 2, 77, 127, 128, 129, 1000, 128 * 64, 128 * 64 + 1, 150_000]
    lists = []
    for n in sizes:
        d = np.sort(rng.choice(max_doc, size=n, replace=False)).astype(np.int32)
        lists.append((d, rng.integers(1, 12, size=n).astype(np.int32)))
    norms = rng.integers(90, 125, size=max_doc).astype(np.uint8)
    seg = indexgen.build_explicit(max_doc, lists, norms=norms, version=version)
    return seg, max_doc, int(sum(f.sum() for _, f in lists)), len(sizes)


@pytest.mark.parametrize("version", [1, 0], ids=["bp128", "legacy"])
def test_absent_singleton_and_tail_only_terms(oracle, version):
    seg, max_doc, sttf, n = _edge_segment(version)
    ctx = _context()
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, max_doc, seg.terms, sttf)
        ids = list(range(n)) + list(range(n - 1, -1, -1))
        _fused(lf.g, lf.leaf, ids, 10)
        n0 = _launches(ctx, "term_query_launches")
        for k in KS:
            _check(lf, oracle, ids, k, ("edges", version))
        assert _launches(ctx, "term_query_launches") - n0 == len(KS)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["live docs", "raw norms", "no norms"])
def test_queries_off_the_table_path(oracle, case):
    """The waves stride over the list with stream_blocks: deleted docs (every 7th doc), raw norm bytes (no
    score table), a field without norms — k 1..128, the edge lists in one batch."""
    seg, max_doc, sttf, n = _edge_segment()
    live = None
    norms = seg.norms
    cfg = {}
    if case == "live docs":
        alive = np.ones(max_doc, bool)
        alive[::7] = False
        live = np.packbits(alive, bitorder="little")
        live = np.concatenate([live, np.zeros((-live.size) % 8, np.uint8)]).view(np.uint64)
    elif case == "raw norms":
        cfg["raw_norms"] = True
    else:
        norms = None
    ctx = _context(**cfg)
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, norms, max_doc, seg.terms, sttf, live=live)
        for k in KS:
            _check(lf, oracle, list(range(n)), k, case)
    finally:
        ctx.close()


def test_docs_only_field(oracle):
    """IndexOptions::Docs: a synthetic freq row of 1 per block, plain-delta tails"""
    import rucene_amd  # noqa: F401
    rng = np.random.default_rng(9)
    max_doc = 200_000
    sizes = [1, 50, 128, 129, 5000, 60_000]
    lists = [np.sort(rng.choice(max_doc, size=n, replace=False)).astype(np.int32) for n in sizes]
    norms = rng.integers(95, 125, size=max_doc).astype(np.uint8)
    w = oracle.Writer(max_doc, version=1, write_freqs=False)
    terms = np.array([w.write_term(d, np.ones_like(d)) for d in lists], dtype=oracle.TERM_STATE_DTYPE)
    doc_bytes = w.close()
    terms["total_term_freq"] = -1
    ctx = _context()
    try:
        lf = _Leaf(ctx, oracle, doc_bytes, norms, max_doc, terms, -1, index_options=1)
        for k in KS:
            _check(lf, oracle, list(range(len(sizes))), k, "docs only")
    finally:
        ctx.close()


def test_zipf_batches_match_items_kernel_across_launches(oracle):
    """A Zipf segment: batches of different layouts (long lists, short ones, mixed with absent ids, k 10 and 100) launched a few
    hundred times in alternation, every row against the oracle's once and against RGPU_TERM_KERNEL=items."""
    import rucene_amd
    from rucene_amd import indexgen
    seg = indexgen.build_zipf(1_000_000, 20_000)
    rng = np.random.default_rng(1)
    batches = [(np.arange(0, 64), 10), (rng.integers(0, 20_000, size=512), 10), (rng.integers(0, 200, size=200), 100),
               (np.concatenate([np.arange(40), rng.integers(5000, 20_000, size=100)]), 64)]
    ctx = _context()
    ctx_items = _context({"RGPU_TERM_KERNEL": "items"})
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, seg.max_doc, seg.terms, seg.sum_total_term_freq)
        g2 = rucene_amd.GpuIndexSearcher([rucene_amd.LeafReader.from_synthetic(seg)], ctx=ctx_items)
        first = [_check(lf, oracle, ids, k, ("zipf", b)) for b, (ids, k) in enumerate(batches)]
        for b, (ids, k) in enumerate(batches):
            rows, totals = _fused(g2, g2.leaves[0], ids, k)
            assert (rows["doc"] == first[b][0]["doc"]).all() and (rows["score"].view(np.int32) == first[b][0]["score"].view(np.int32)).all(), b
            assert (totals == first[b][1]).all(), b
        assert _launches(ctx_items, "term_query_launches") == 0
        for i in range(300):
            b = i % len(batches)
            ids, k = batches[b]
            rows, totals = _fused(lf.g, lf.leaf, ids, k)
            assert (rows["doc"] == first[b][0]["doc"]).all() and (rows["score"].view(np.int32) == first[b][0]["score"].view(np.int32)).all(), (i, b)
            assert (totals == first[b][1]).all(), (i, b)
    finally:
        ctx.close()
        ctx_items.close()
