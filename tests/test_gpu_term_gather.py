"""The block stage of k_search_term_query's gather (`-m gpu`; kernels/search_term_query.hpp, general path) at the sizes where it can
go wrong: as many surviving chunks as waves, one less, one more, two passes and one more; a queue exactly full and one entry over;
a queue that overflows round after round; equal top scores in every wave's chunks; the edge of a gather window. The cases are the
ones the dealt gather needs (-DRGPU_TERMQ_DEAL=1, DESIGN §3.y6: chunks dealt to the waves, queue entries reserved from one LDS
counter in whatever order the waves get there, a full round repeating its window with the chunks it queued marked done, a sort that
no longer gets its entries in block order) and hold for the stepped gather alike. Every row against the oracle bit for bit
(TIE_CANONICAL) and against a context opened with RGPU_TERM_KERNEL=items, at RGPU_TERM_QUERY_WAVES 2 / 4 / 8 and k 1 / 10 / 64 / 100 /
128. The CPU model of the dealt schedule is tests/test_term_gather_model_cpu.py."""
import numpy as np
import pytest

from test_gpu_term_query import KS, _Leaf, _assert_row, _context, _fused, _ramp_segment

pytestmark = pytest.mark.gpu

WAVES = ["2", "4", "8"]


class _Fixture:
    """A segment built once, and the oracle's answers over it, computed once per (term, k)."""

    def __init__(self, seg, max_doc, sttf):
        self.seg, self.max_doc, self.sttf = seg, max_doc, sttf
        self.want = {}

    def oracle_row(self, oracle, lf, t, k):
        if (t, k) not in self.want:
            self.want[(t, k)] = lf.osr.search(oracle.OP_TERM, [int(t)], k, tie_mode=oracle.TIE_CANONICAL)
        return self.want[(t, k)]


class _Pair:
    """The query kernel under `env` and the work-item kernel (RGPU_TERM_KERNEL=items) over one segment."""

    def __init__(self, fx, oracle, env):
        self.fx, self.oracle = fx, oracle
        self.ctx = _context(env)
        self.ctx_items = _context({**env, "RGPU_TERM_KERNEL": "items"})
        args = (fx.seg.doc_bytes, fx.seg.norms, fx.max_doc, fx.seg.terms, fx.sttf)
        self.lf = _Leaf(self.ctx, oracle, *args)
        self.items = _Leaf(self.ctx_items, oracle, *args)

    def check(self, ids, k, what):
        rows, totals = _fused(self.lf.g, self.lf.leaf, ids, k)
        for j, t in enumerate(ids):
            _assert_row(rows[j], totals[j], self.fx.oracle_row(self.oracle, self.lf, t, k), (what, k, j, int(t)))
        rows2, totals2 = _fused(self.items.g, self.items.leaf, ids, k)
        assert (rows2["doc"] == rows["doc"]).all() and (rows2["score"].view(np.int32) == rows["score"].view(np.int32)).all(), (what, k, "items")
        assert (totals2 == totals).all(), (what, k, "items totals")
        return rows, totals

    def close(self):
        st = self.ctx.kernel_stats()
        ran = st["term_query_launches"]["launches"] if "term_query_launches" in st else 0
        self.ctx.close()
        self.ctx_items.close()
        assert ran > 0  # the query kernel really ran


def _deal_cs(W):
    return [1, W - 1, W, W + 1, 2 * W, 2 * W + 1]


@pytest.fixture(scope="module")
def deal_edges():
    """Lists of 64 c + r blocks for every c the three widths ask for, r 0 / 1 / 63, with and without a 40-posting tail; freqs 1..11
    (11 lies above the score table: such a block has no bound and is always a candidate), random norms."""
    from rucene_amd import indexgen
    rng = np.random.default_rng(23)
    max_doc = 320_000
    cs = sorted({c for W in (2, 4, 8) for c in _deal_cs(W)})
    index, lists = {}, []
    for c in cs:
        for r in (0, 1, 63):
            for tail in (0, 40):
                n = 128 * (64 * c + r) + tail
                d = np.sort(rng.choice(max_doc, size=n, replace=False)).astype(np.int32)
                index[(c, r, tail)] = len(lists)
                lists.append((d, rng.integers(1, 12, size=n).astype(np.int32)))
    norms = rng.integers(90, 125, size=max_doc).astype(np.uint8)
    seg = indexgen.build_explicit(max_doc, lists, norms=norms)
    return _Fixture(seg, max_doc, int(sum(f.sum() for _, f in lists))), index


@pytest.mark.parametrize("waves", WAVES)
def test_deal_edges(deal_edges, oracle, waves):
    """One chunk per wave, one short of it, one more, two passes and two passes plus one — each with a whole last chunk, a last
    chunk of one block and one of 63; RGPU_TERM_SHORT_BLOCKS=0 sends the 64-block list through the general path too."""
    fx, index = deal_edges
    W = int(waves)
    ids = [index[(c, r, tail)] for c in sorted(set(_deal_cs(W))) for r in (0, 1, 63) for tail in (0, 40)]
    p = _Pair(fx, oracle, {"RGPU_TERM_QUERY_WAVES": waves, "RGPU_TERM_SHORT_BLOCKS": "0"})
    try:
        for k in KS:
            p.check(ids, k, ("deal edges", waves))
    finally:
        p.close()


CAPACITY_BLOCKS = [255, 256, 257, 319, 320, 321, 512, 513]


@pytest.fixture(scope="module")
def all_tying():
    """every block ties: one freq, one norm"""
    from rucene_amd import indexgen
    rng = np.random.default_rng(29)
    max_doc = 200_000
    lists = []
    for nb in CAPACITY_BLOCKS:
        d = np.sort(rng.choice(max_doc, size=128 * nb, replace=False)).astype(np.int32)
        lists.append((d, np.full(d.size, 3, np.int32)))
    seg = indexgen.build_explicit(max_doc, lists, norms=np.full(max_doc, 100, np.uint8))
    return _Fixture(seg, max_doc, int(sum(f.sum() for _, f in lists))), [d for d, _ in lists]


@pytest.mark.parametrize("waves", WAVES)
def test_queue_capacity(all_tying, oracle, waves):
    """Without a starting threshold the first gather's candidates are every block of the list: one short of the queue's 256 entries,
    exactly full, one over, and the same around 320 (five chunks) and 512. Every score ties, so the rows are the list's first k docs."""
    fx, docs = all_tying
    p = _Pair(fx, oracle, {"RGPU_TERM_QUERY_WAVES": waves, "RGPU_TERM_SKETCH": "0"})
    try:
        ids = list(range(len(CAPACITY_BLOCKS)))
        for k in KS:
            rows, _ = p.check(ids, k, ("capacity", waves))
            for j in ids:
                assert (rows[j]["doc"] == docs[j][:k]).all(), (waves, k, CAPACITY_BLOCKS[j])
    finally:
        p.close()


@pytest.fixture(scope="module", params=[(6, 300), (3, 70)], ids=["6x300", "3x70"])
def ramp(request):
    seg, max_doc, sttf = _ramp_segment(*request.param)
    return _Fixture(seg, max_doc, sttf)


@pytest.mark.parametrize("sketch", ["1", "0"], ids=["sketch", "no-sketch"])
@pytest.mark.parametrize("waves", WAVES)
def test_overflow_round_after_round(ramp, oracle, waves, sketch):
    """Levels of tying blocks that rise along the list: every round's candidates are beaten by the next level's, so the queue fills
    round after round and its window is repeated. The order in which the waves reserve their entries differs from launch to
    launch; the rows may not: one query, then a batch of 300 copies and 20 of the short list, launched 20 times."""
    p = _Pair(ramp, oracle, {"RGPU_TERM_QUERY_WAVES": waves, "RGPU_TERM_SKETCH": sketch})
    try:
        for k in KS:
            p.check([0, 1], k, ("ramp", waves, sketch))
        batch = [0] * 300 + [1] * 20
        first, totals = p.check(batch, 10, ("ramp batch", waves, sketch))
        for i in range(19):
            rows, tot = _fused(p.lf.g, p.lf.leaf, batch, 10)
            assert rows.tobytes() == first.tobytes() and (tot == totals).all(), (waves, sketch, i)
    finally:
        p.close()


def _ties_segment(W):
    """2 W + 1 chunks; in each, one block (the first, the middle, the last lane's in turn) holds one posting of the top score"""
    from rucene_amd import indexgen
    rng = np.random.default_rng(31 + W)
    n_chunks = 2 * W + 1
    nb = 64 * n_chunks
    max_doc = 3 * 128 * nb
    docs = np.sort(rng.choice(max_doc, size=128 * nb, replace=False)).astype(np.int32)
    freqs = np.ones(docs.size, np.int32)
    plant = np.array([128 * (64 * c + (0, 31, 63)[c % 3]) + 17 for c in range(n_chunks)])
    freqs[plant] = 5
    seg = indexgen.build_explicit(max_doc, [(docs, freqs)], norms=np.full(max_doc, 100, np.uint8))
    return _Fixture(seg, max_doc, int(freqs.sum())), docs[plant]


@pytest.mark.parametrize("sketch", ["1", "0"], ids=["sketch", "no-sketch"])
@pytest.mark.parametrize("waves", WAVES)
def test_ties_across_waves(oracle, waves, sketch):
    """Equal top scores in every wave's chunks: whatever order the waves queue them in, the lowest docs win (the sort's tie-break is the
    block, not the queue position), and past them the lowest doc of the rest."""
    W = int(waves)
    fx, winners = _ties_segment(W)
    p = _Pair(fx, oracle, {"RGPU_TERM_QUERY_WAVES": waves, "RGPU_TERM_SKETCH": sketch})
    try:
        for k in sorted({1, W, 2 * W, 2 * W + 1, 2 * W + 2} | set(KS)):
            rows, _ = p.check([0], k, ("ties", waves, sketch))
            n = min(k, winners.size)
            assert (rows[0]["doc"][:n] == winners[:n]).all(), (waves, sketch, k, rows[0]["doc"][:n], winners[:n])
    finally:
        p.close()


WINDOW_CHUNKS = 512  # TQ_CHUNK_UNROLL * 64 * W chunks at W = 2


@pytest.fixture(scope="module")
def window_edge():
    """512 * 64 + 3 * 64 + 5 blocks and a tail: at W = 2 one whole window, then a second of four chunks (the last partial). Levels of
    tying blocks rise along the list, so without a starting threshold the first window fills round after round and is repeated with
    its queued chunks marked done. Its last level is two chunks (128 entries, not a full round): the same round goes on into the
    second window, whose 197 blocks of a higher level no longer fit — that window is repeated too, with a map that must have been
    cleared. Winners are planted in chunks 0, 511, 512, 514 and in the tail."""
    from rucene_amd import indexgen
    rng = np.random.default_rng(37)
    nb = WINDOW_CHUNKS * 64 + 3 * 64 + 5
    df = 128 * nb + 40
    max_doc = df + df // 2
    docs = np.sort(rng.choice(max_doc, size=df, replace=False)).astype(np.int32)
    freqs = np.ones(df, np.int32)
    blocks = np.arange(nb)
    chunk = blocks // 64
    freqs[128 * blocks + 5] = 2 + np.minimum(chunk // 128, 3) + (chunk >= 510) + (chunk >= 512)  # levels 2 .. 5, 6 (chunks 510-511), 7
    plant = np.array([128 * (64 * 0 + 9) + 3, 128 * (64 * 511 + 63) + 127, 128 * (64 * 512) + 0, 128 * (64 * 514 + 4) + 77, df - 1])
    freqs[plant] = [10, 9, 10, 8, 9]
    norms = np.full(max_doc, 100, np.uint8)
    seg = indexgen.build_explicit(max_doc, [(docs, freqs)], norms=norms)
    return _Fixture(seg, max_doc, int(freqs.sum())), docs[plant]


@pytest.mark.parametrize("sketch", ["1", "0"], ids=["sketch", "no-sketch"])
@pytest.mark.parametrize("waves", WAVES)
def test_window_edge_and_done_cleared(window_edge, oracle, waves, sketch):
    fx, winners = window_edge
    p = _Pair(fx, oracle, {"RGPU_TERM_QUERY_WAVES": waves, "RGPU_TERM_SKETCH": sketch})
    try:
        for k in KS:
            rows, _ = p.check([0], k, ("window edge", waves, sketch))
            if k >= winners.size:
                assert set(winners.tolist()) == set(rows[0]["doc"][:winners.size].tolist()), (waves, sketch, k)
    finally:
        p.close()
