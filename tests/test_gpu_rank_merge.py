"""group_offer2 (`-m gpu`; kernels/search_term.hpp: the level cut in front of the list's lock, the insertions behind it, and — in a
-DRGPU_TERM_RANK_MERGE=1 build — the rank merge): blocks that offer exactly 0, 1, 2, 3, 16, 17, 64 and 128 entering
keys to the shared top-k, ties across blocks and across waves, lists of 1, 2, 15, 16, 17 and 65 blocks, a tail and a singleton,
k 1 / 10 / 64 / 100 — through the fused single-term call (k_search_term_query) and through RGPU_TERM_KERNEL=items (k_search_term),
both against the oracle bit for bit: doc ids, score bits, totals.

How a block offers exactly n keys whatever the order the waves get to it: every doc of these lists has the same norm, so the score
rises with the freq alone. An "exact" list is 66 blocks: 65 carriers, each with ONE posting of freq 2 among postings of freq 1,
and one hot block with n postings of freq 3..5. The list has a block-max sketch (16 blocks or more), whose threshold for k <= 64 is
the carriers' score at the largest doc id: under it — or under a list already full of carriers' keys — the hot block's n keys enter
and no other key of the block does; a carrier offers its one key, or none once k smaller docs tie with it."""
import numpy as np
import pytest

from test_gpu_term_query import _Leaf, _assert_row, _context, _fused, _launches

pytestmark = pytest.mark.gpu

KS = [1, 10, 64, 100]
NS = [0, 1, 2, 3, 16, 17, 64, 128]
LENGTHS = [1, 2, 15, 16, 17, 65]  # FullBlocks (+ a VInt tail each)
FLAT = 9000     # docs [0, FLAT) carry one norm byte: the exact lists live there
MAX_DOC = 12000


def _exact_list(rng, n, tail):
    """66 blocks + `tail` postings; block 40 is the hot one"""
    nb, hot = 66, 40
    df = 128 * nb + tail
    docs = np.sort(rng.choice(FLAT, size=df, replace=False)).astype(np.int32)
    freqs = np.ones(df, np.int32)
    for b in range(nb):
        if b != hot:
            freqs[128 * b + int(rng.integers(0, 128))] = 2  # a carrier's one better posting, anywhere in the block
    at = 128 * hot + rng.choice(128, size=n, replace=False)
    freqs[at] = rng.integers(3, 6, size=n)  # few distinct scores: the candidates tie among themselves, doc ascending decides
    return docs, freqs


def _segment():
    from rucene_amd import indexgen
    rng = np.random.default_rng(20)
    norms = np.full(MAX_DOC, 100, np.uint8)
    norms[FLAT:] = rng.integers(90, 125, size=MAX_DOC - FLAT)
    lists = [_exact_list(rng, n, tail=37 if i % 2 else 0) for i, n in enumerate(NS)]
    names = ["exact %d" % n for n in NS]
    for nb in LENGTHS:  # mixed norms, freqs 1..12 (some beyond the score table), a tail behind the blocks
        df = 128 * nb + 50
        d = np.sort(rng.choice(MAX_DOC, size=df, replace=False)).astype(np.int32)
        lists.append((d, rng.integers(1, 13, size=df).astype(np.int32)))
        names.append("%d blocks" % nb)
    for nb in (2, 17):  # one score everywhere: every block ties with every other, across the waves of a workgroup
        d = np.sort(rng.choice(FLAT, size=128 * nb, replace=False)).astype(np.int32)
        lists.append((d, np.full(d.size, 2, np.int32)))
        names.append("all ties, %d blocks" % nb)
    d = np.sort(rng.choice(MAX_DOC, size=77, replace=False)).astype(np.int32)
    lists.append((d, rng.integers(1, 6, size=77).astype(np.int32)))
    names.append("tail only")
    lists.append((np.array([4321], np.int32), np.array([3], np.int32)))
    names.append("singleton")
    seg = indexgen.build_explicit(MAX_DOC, lists, norms=norms)
    return seg, int(sum(int(f.sum()) for _, f in lists)), names


@pytest.fixture(scope="module")
def world(oracle):
    """the segment, and the oracle's rows for every (term, k), computed once"""
    seg, sttf, names = _segment()
    osr = oracle.Searcher([oracle.Segment(seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sum_total_term_freq=sttf)])
    want = {(t, k): osr.search(oracle.OP_TERM, [t], k, tie_mode=oracle.TIE_CANONICAL) for t in range(len(names)) for k in KS}
    return seg, sttf, names, want


def _assert_batch(rows, totals, ids, k, want, what):
    for j, t in enumerate(ids):
        _assert_row(rows[j], totals[j], want[(int(t), k)], (what, k, j, int(t)))


def test_the_hot_blocks_hold_what_they_should(world):
    """the oracle's own rows: exactly n postings score above the carriers', whose 65 ties follow in doc order"""
    _, _, names, want = world
    for t, n in enumerate(NS):
        d, sc, _ = want[(t, 100)]
        if n >= 100:
            assert np.unique(sc).size <= 3, names[t]  # freqs 3..5 only
            continue
        levels = np.unique(sc)  # ascending: [freq 1,] the carriers' freq 2, the hot freqs
        carrier = levels[1] if n + 65 < 100 else levels[0]
        assert int((sc > carrier).sum()) == n, names[t]
        ties = d[sc == carrier]
        assert ties.size == min(65, 100 - min(n, 100)) and (np.diff(ties) > 0).all(), names[t]


@pytest.mark.parametrize("kernel", ["query", "items"])
@pytest.mark.parametrize("k", KS)
def test_every_list_one_batch(world, oracle, kernel, k):
    """every list in one batch (one workgroup each, forwards and backwards), and the launch count of the kernel that ran"""
    seg, sttf, names, want = world
    ctx = _context({"RGPU_TERM_KERNEL": "items"} if kernel == "items" else None)
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sttf)
        ids = list(range(len(names))) + list(range(len(names) - 1, -1, -1))
        _fused(lf.g, lf.leaf, ids, k)  # (the first call prepares the terms through the full path)
        n0 = _launches(ctx, "term_query_launches")
        rows, totals = _fused(lf.g, lf.leaf, ids, k)
        _assert_batch(rows, totals, ids, k, want, kernel)
        assert _launches(ctx, "term_query_launches") - n0 == (1 if kernel == "query" else 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("waves", ["2", "8"])
def test_other_workgroup_widths(world, oracle, waves):
    """two and eight waves share the list: who meets the hot block first changes, the rows do not"""
    seg, sttf, names, want = world
    ctx = _context({"RGPU_TERM_QUERY_WAVES": waves})
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sttf)
        ids = list(range(len(names)))
        for k in KS:
            rows, totals = _fused(lf.g, lf.leaf, ids, k)
            _assert_batch(rows, totals, ids, k, want, ("waves", waves))
    finally:
        ctx.close()


def test_no_sketch_every_block_offered(world, oracle):
    """without block-max sketches the lists start from an empty top-k: the first blocks offer all 128 keys, later ones a few"""
    seg, sttf, names, want = world
    ctx = _context({"RGPU_TERM_SKETCH": "0"})
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sttf)
        ids = list(range(len(names)))
        for k in KS:
            rows, totals = _fused(lf.g, lf.leaf, ids, k)
            _assert_batch(rows, totals, ids, k, want, "no sketch")
    finally:
        ctx.close()


def test_fifty_calls_alternating_two_streams(world, oracle):
    """two streams, two batches of different layout, 50 calls in alternation without a wait in between"""
    import torch
    from rucene_amd import _lib as gpu
    seg, sttf, names, want = world
    k = 10
    ctx = _context()
    try:
        lf = _Leaf(ctx, oracle, seg.doc_bytes, seg.norms, MAX_DOC, seg.terms, sttf)
        nt = len(names)
        batches = [np.array(list(range(nt)) * 3, dtype=np.int64).reshape(-1, 1),
                   np.array(list(range(nt - 1, -1, -1)) + list(range(len(NS))) * 5, dtype=np.int64).reshape(-1, 1)]
        for b in batches:
            _fused(lf.g, lf.leaf, b[:, 0], k)  # terms prepared
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        hits = [torch.full((b.shape[0], k), -3, dtype=torch.int64, device="cuda") for b in batches]
        totals = [torch.full((b.shape[0],), -3, dtype=torch.int64, device="cuda") for b in batches]
        torch.cuda.synchronize()
        n0 = _launches(ctx, "term_query_launches")
        for i in range(50):
            j = i % 2
            lf.g.search_uniform_device(gpu.OP_TERM, batches[j], lf.leaf, k, hits[j].data_ptr(), totals[j].data_ptr(), streams[j].cuda_stream)
            if i in (24, 25):  # one look in the middle of the run, each lane once
                streams[j].synchronize()
                rows = hits[j].cpu().numpy().view(gpu.HIT_DTYPE).reshape(-1, k)
                _assert_batch(rows, totals[j].cpu().numpy(), batches[j][:, 0], k, want, ("mid", i))
        torch.cuda.synchronize()
        assert _launches(ctx, "term_query_launches") - n0 == 50
        for j in range(2):
            rows = hits[j].cpu().numpy().view(gpu.HIT_DTYPE).reshape(-1, k)
            _assert_batch(rows, totals[j].cpu().numpy(), batches[j][:, 0], k, want, ("end", j))
    finally:
        ctx.close()
