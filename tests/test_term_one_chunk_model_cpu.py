"""A numpy model of k_search_term_query's one-chunk path (kernels/search_term_query.hpp), checked against a plain sort (no GPU).

The model follows the kernel step by step: every block's bound against the floor gives the survivor mask; wave w takes the survivors
of rank w, w + W, ...; a wave keeps a private top-k with tau = max(its k-th best, floor), re-tests a block against tau before it
unpacks it, cuts a block with many candidates to its best score levels (term_level_cut) and inserts in lane order (posting 2 * lane
of every lane first, then 2 * lane + 1); wave W - 1 takes the tail first; one merge of the W lists (each at most 64 or 128 keys)
gives the row. It must drop no winner and keep the order, ties by doc ascending, for lists of 1..64 blocks plus a tail,
W 2 / 4 / 8, k 1 / 10 / 64 / 65 / 128, with scores of few levels, every posting tying, and a k-th band that straddles waves."""
import numpy as np
import pytest

LEVEL_CUT_MIN = 16   # RGPU_TERM_LEVEL_CUT_MIN
KS = [1, 10, 64, 65, 128]


def key_of(score, doc):
    """larger == better under (score desc, doc asc): the kernel's make_key with the score's order bits as an integer level"""
    return (int(score) << 32) | (0xFFFFFFFF - int(doc))


def key_doc(key):
    return 0xFFFFFFFF - (key & 0xFFFFFFFF)


def thr_of(tau, lo):
    """term_thr_of: the score a block must reach; strict when none of its docs (all above lo) can win a tie with tau's doc"""
    if tau == 0:
        return 0
    bits = tau >> 32
    return bits + 1 if key_doc(tau) <= lo + 1 else bits


class PrivateList:
    def __init__(self, k, floor):
        self.k, self.floor = k, floor
        self.cap = 128 if k > 64 else 64   # WaveTopK: one or two registers per lane
        self.keys = []                     # sorted descending
        self.tau = floor

    def insert_in_lane_order(self, keys):
        for x in keys:
            if x > self.tau:
                self.keys.append(x)
                self.keys.sort(reverse=True)
                del self.keys[self.cap:]
                kth = self.keys[self.k - 1] if len(self.keys) >= self.k else 0
                self.tau = max(kth, self.floor)

    def offer2(self, key0, key1):
        """wave_offer2: the level cut (narrow lists only), then posting 2 * lane of every lane, then 2 * lane + 1"""
        k = self.k
        cand = [x for x in key0 + key1 if x > self.tau]
        if self.cap == 64 and len(cand) > max(k, LEVEL_CUT_MIN):
            level, have = None, 0
            for lv in sorted({x >> 32 for x in key0 + key1 if x}, reverse=True):
                level = lv
                have += sum(1 for x in key0 + key1 if x and x >> 32 == lv)
                if have >= k:
                    break
            if have < k:
                level = 0
            key0 = [x if x >> 32 >= level else 0 for x in key0]
            key1 = [x if x >> 32 >= level else 0 for x in key1]
        self.insert_in_lane_order(key0)
        self.insert_in_lane_order(key1)


def one_chunk(blocks, tail, W, k, floor):
    """blocks: list of (docs[128], scores[128]); tail: (docs, scores) of fewer than 128 postings. Returns (keys of the row, blocks unpacked)."""
    bound = [int(s.max()) for _, s in blocks]
    lo = [-1] + [int(d[-1]) for d, _ in blocks[:-1]]
    pm = [b for b in range(len(blocks)) if bound[b] >= thr_of(floor, lo[b])]
    lists, unpacked = [], 0
    for w in range(W):
        mine = PrivateList(k, floor)
        if w == W - 1 and len(tail[0]):
            keys = [key_of(s, d) for d, s in zip(*tail)] + [0] * (128 - len(tail[0]))
            mine.offer2(keys[0::2], keys[1::2])
        for b in pm[w::W]:
            if bound[b] < thr_of(mine.tau, lo[b]):
                continue
            unpacked += 1
            docs, scores = blocks[b]
            if int(scores.max()) < thr_of(mine.tau, lo[b]):
                continue
            keys = [key_of(s, d) for d, s in zip(docs, scores)]
            mine.offer2(keys[0::2], keys[1::2])
        lists.append(mine.keys)
    cap = 128 if k > 64 else 64
    merged = []
    for lst in lists:   # topk_merge_sorted: the cap best of the union, sorted
        merged = sorted(merged + lst, reverse=True)[:cap]
    return merged[:k], unpacked


def plain(blocks, tail, k):
    keys = [key_of(s, d) for docs, scores in blocks + [tail] for d, s in zip(docs, scores)]
    return sorted(keys, reverse=True)[:k]


def make_list(rng, nblocks, tail_n, scores_of):
    n = 128 * nblocks + tail_n
    docs = np.sort(rng.choice(50_000, size=n, replace=False)).astype(np.int64)
    scores = scores_of(n, docs).astype(np.int64)
    blocks = [(docs[128 * b:128 * b + 128], scores[128 * b:128 * b + 128]) for b in range(nblocks)]
    return blocks, (docs[128 * nblocks:], scores[128 * nblocks:])


def few_levels(rng):
    return lambda n, docs: 1000 + rng.integers(0, 6, size=n)


def all_tie(rng):
    return lambda n, docs: np.full(n, 1234)


def band_across_waves(rng):
    """six clear winners, then a band of equal scores with three members in each of the first blocks — more members than any k <= 10
    leaves room for, in blocks that different waves own"""
    def f(n, docs):
        s = np.full(n, 1000)
        s[rng.choice(n, size=min(6, n), replace=False)] = 3000
        for b in range(min(8, n // 128)):
            s[128 * b + rng.choice(128, size=3, replace=False)] = 2000
        return s
    return f


def winners_last(rng):
    def f(n, docs):
        s = np.full(n, 1000)
        s[-12:] = 2000   # the last postings: the tail, or the last block of a list without one
        return s
    return f


def floors_of(blocks, tail, k):
    """no floor; the tightest valid sketch floor (the k-th best score, largest doc); a looser one"""
    keys = plain(blocks, tail, k)
    out = [0]
    if len(keys) >= k:
        out.append((keys[k - 1] >> 32) << 32)
        out.append(((keys[k - 1] >> 32) - 1) << 32)
    return out


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("shape", [few_levels, all_tie, band_across_waves, winners_last], ids=lambda f: f.__name__)
def test_one_chunk_model_equals_plain_sort(W, shape):
    rng = np.random.default_rng(100 * W + len(shape.__name__))
    sizes = [(nb, t) for nb in (1, 2, W - 1, W, W + 1, 4 * W, 4 * W + 1, 15, 16, 17, 63, 64) if nb >= 1 for t in (0, 1, 127)]
    sizes += [(int(nb), int(t)) for nb, t in zip(rng.integers(1, 65, size=6), rng.integers(0, 128, size=6))]
    for nb, t in sizes:
        blocks, tail = make_list(rng, nb, t, shape(rng))
        for k in KS:
            want = plain(blocks, tail, k)
            for floor in floors_of(blocks, tail, k):
                got, unpacked = one_chunk(blocks, tail, W, k, floor)
                assert got == want, (shape.__name__, W, nb, t, k, floor, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:4])
                assert unpacked <= nb


def test_private_thresholds_skip_blocks_but_no_winner():
    """every posting ties: the k lowest docs win, all in block 0 (one wave's); the other waves' blocks are losers, and a wave with a
    full list of its own skips its later blocks (strict test: their docs lie above its k-th best's doc)"""
    rng = np.random.default_rng(7)
    blocks, tail = make_list(rng, 16, 40, all_tie(rng))
    for W in (2, 4, 8):
        got, unpacked = one_chunk(blocks, tail, W, 10, 0)
        assert got == plain(blocks, tail, 10)
        assert [key_doc(x) for x in got] == [int(d) for d in blocks[0][0][:10]]
        assert unpacked == W   # every wave unpacks its first block only
