"""A numpy model of group_offer2 (kernels/search_term.hpp) — the level cut in front of the lock and the rank merge of variant
builds (RGPU_TERM_RANK_MERGE=1) — against the sequential topk_offer semantics (kernels/wave.hpp): one insertion per entering key,
in lane order, key0 before key1, the threshold rising on the way.

The list is 64 lanes of u64 keys, sorted descending, 0 == empty; a block offers two keys per lane. The merge ranks list and
candidates against each other and scatters once; ranks below k and the resulting threshold must be what the insertions leave,
whatever sits at ranks >= k. In front of the lock a block with many candidates is cut to its best score levels, as many as
cover k keys (cut_to_levels): the cut works with an older, lower threshold than the one found under the lock, and must not change
the outcome either."""
import numpy as np
import pytest

LANES = 64
MERGE_MIN, MERGE_MAX = 3, 16  # group_offer2 merges for n in [3, RGPU_TERM_RANK_MERGE_MAX]; other n keep the insertions
CUT_MIN = 16                  # RGPU_TERM_LEVEL_CUT_MIN: more than max(k, CUT_MIN) candidates are cut to score levels before the lock
NS = [0, 1, 2, 3, 16, 17, 64, 128]
KS = [1, 10, 64]


def make_key(score, doc):
    """wave.hpp make_key: larger == better under (score desc, doc asc)"""
    u = int(np.float32(score).view(np.uint32))
    o = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (o << 32) | (~int(doc) & 0xFFFFFFFF)


def offer_sequential(lst, key0, key1, k, floor):
    """topk_offer(key0) then topk_offer(key1): insertions in lane order, a key at or below the threshold of the moment is skipped"""
    t = list(lst)
    tau = max(t[k - 1], floor)
    for keys in (key0, key1):
        for x in keys:
            if x > tau:
                p = sum(1 for v in t if v > x)
                t = (t[:p] + [x] + t[p:])[:LANES]
                tau = max(t[k - 1], floor)
    return t, tau


def offer_rank_merge(lst, key0, key1, k, floor):
    """the kernel's arithmetic, lane-parallel: shift of every list key, list position + rank among the candidates of every candidate"""
    L = np.array(lst, dtype=np.uint64)
    tau = np.uint64(max(lst[k - 1], floor))
    c = np.concatenate([np.array(key0, dtype=np.uint64), np.array(key1, dtype=np.uint64)])
    cand = c[c > tau]
    shift = (cand[None, :] > L[:, None]).sum(axis=1)                 # per lane: candidates above its list key
    rank = (cand[None, :] > cand[:, None]).sum(axis=1)               # per candidate: candidates above it
    pos = (L[None, :] > cand[:, None]).sum(axis=1)                   # per candidate: list keys above it
    out = np.zeros(LANES + cand.size, dtype=np.uint64)
    written = np.zeros(LANES + cand.size, dtype=np.int64)
    np.add.at(written, np.arange(LANES) + shift, 1)
    np.add.at(written, pos + rank, 1)
    assert (written == 1).all(), "the scatter's targets are a permutation"
    out[np.arange(LANES) + shift] = L
    out[pos + rank] = cand
    t = [int(v) for v in out[:LANES]]                                # what lands at 64 or beyond is dropped
    return t, max(t[k - 1], floor), int(cand.size)


def cut_to_levels(key0, key1, k, stale_tau):
    """in front of the lock: with more than max(k, CUT_MIN) keys above the caller's threshold, score levels (a key's high word) are
    taken from the top until they cover k keys; keys below the last level are dropped"""
    both = list(key0) + list(key1)
    if sum(1 for x in both if x > stale_tau) <= max(k, CUT_MIN):
        return list(key0), list(key1)
    level, have = 0xFFFFFFFF, 0
    while have < k:
        t = max([x >> 32 for x in both if (x >> 32) < level] or [0])
        if t == 0:
            level = 0
            break
        have += sum(1 for x in both if (x >> 32) == t)
        level = t
    keep = [x if (x >> 32) >= level else 0 for x in both]
    return keep[:LANES], keep[LANES:]


def offer_dispatch(lst, key0, key1, k, floor, stale_tau=0, merge=True):
    """group_offer2: the cut in front of the lock, then (merge: variant builds) the merge for MERGE_MIN <= n <= MERGE_MAX entering keys,
    the insertions otherwise"""
    key0, key1 = cut_to_levels(key0, key1, k, stale_tau)
    tau = max(lst[k - 1], floor)
    assert stale_tau <= tau
    n = sum(1 for x in list(key0) + list(key1) if x > tau)
    if merge and MERGE_MIN <= n <= MERGE_MAX:
        return offer_rank_merge(lst, key0, key1, k, floor)[:2]
    return offer_sequential(lst, key0, key1, k, floor)


def _list(rng, fill, scores, doc0=1_000_000):
    """a sorted list with `fill` keys (docs above doc0: never a candidate's doc)"""
    docs = doc0 + 2 * rng.choice(50_000, size=fill, replace=False)  # even docs; a block's are odd: keys are unique
    keys = sorted((make_key(rng.choice(scores), d) for d in docs), reverse=True)
    return keys + [0] * (LANES - fill)


def _block(rng, n_valid, scores, doc_lo=0):
    """two keys per lane, docs ascending in posting order (lane i holds postings 2i, 2i+1), 0 where there is no posting"""
    docs = doc_lo + 2 * np.sort(rng.choice(25_000, size=128, replace=False)) + 1
    keys = [make_key(rng.choice(scores), d) for d in docs]
    drop = rng.choice(128, size=128 - n_valid, replace=False)
    for i in drop:
        keys[i] = 0
    return keys[0::2], keys[1::2]


def _compare(lst, key0, key1, k, floor, what):
    want, want_tau = offer_sequential(lst, key0, key1, k, floor)
    got, got_tau, n = offer_rank_merge(lst, key0, key1, k, floor)
    assert got[:k] == want[:k], (what, "ranks below k", n)
    assert got_tau == want_tau, (what, "threshold", n)
    assert all(a > b or (a == 0 and b == 0) for a, b in zip(got, got[1:])), (what, "the list stays sorted, keys unique")
    # the caller's threshold: nothing yet, the floor alone, the list's own (what the lock will find)
    for stale in sorted({0, floor, max(lst[k - 1], floor)}):
        for merge in (False, True):
            d, d_tau = offer_dispatch(lst, key0, key1, k, floor, stale, merge)
            assert d[:k] == want[:k] and d_tau == want_tau, (what, "dispatch", n, stale, merge)
    return n


def _with_n_entering(rng, n, k, fill, scores_low, scores_high):
    """a block of which exactly n keys pass the list's threshold: n keys from scores_high, 128 - n from scores_low"""
    lst = _list(rng, fill, scores_low[-1:] if fill else scores_low)
    docs = 2 * np.sort(rng.choice(25_000, size=128, replace=False)) + 1
    high = set(rng.choice(128, size=n, replace=False).tolist())
    keys = [make_key(rng.choice(scores_high) if i in high else rng.choice(scores_low[:-1]), d) for i, d in enumerate(docs)]
    return lst, keys[0::2], keys[1::2]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_exactly_n_entering_keys_into_a_full_list(n, k):
    """a full list of one score; n keys of the block score above it, the others below it"""
    rng = np.random.default_rng(1000 * n + k)
    low, high = [1.0, 1.5, 2.0], [3.0, 3.5, 4.0, 4.0, 5.0]
    lst, key0, key1 = _with_n_entering(rng, n, k, LANES, low, high)
    assert _compare(lst, key0, key1, k, 0, ("full", n, k)) == n


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fill", [0, 1, 9, 10, 63])
def test_empty_and_partly_filled_lists(fill, k):
    """below k keys the threshold is 0: every real key enters (up to 128 of them), and most leave again"""
    rng = np.random.default_rng(77 * fill + k)
    for n_valid in (0, 1, 2, 3, 16, 17, 64, 128):
        lst = _list(rng, fill, [2.0, 2.5, 3.0])
        key0, key1 = _block(rng, n_valid, [1.0, 2.0, 2.5, 3.0, 4.0])
        _compare(lst, key0, key1, k, 0, ("fill", fill, n_valid, k))


@pytest.mark.parametrize("k", KS)
def test_floor_above_the_kth_best(k):
    """a floor (the sketch's threshold, another wavefront's publication) above the list's own k-th best, and above every key"""
    rng = np.random.default_rng(5 + k)
    for fill in (0, k - 1, k, LANES):
        for floor_score in (2.25, 3.0, 9.0):
            lst = _list(rng, fill, [1.0, 2.0, 2.5])
            key0, key1 = _block(rng, 128, [1.0, 2.0, 2.25, 2.5, 3.0, 4.0])
            floor = make_key(floor_score, 0x7FFFFFFF)  # (score, largest doc id), as sketch_floor leaves it
            _compare(lst, key0, key1, k, floor, ("floor", fill, floor_score, k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n_valid", NS)
def test_all_equal_scores_doc_ascending_decides(n_valid, k):
    """one score everywhere: the smaller doc wins; the block's docs lie below, between and above the list's"""
    rng = np.random.default_rng(31 * n_valid + k)
    for fill in (0, k, LANES):
        for doc_lo in (0, 1_020_000, 2_000_000):
            lst = _list(rng, fill, [2.0])
            key0, key1 = _block(rng, n_valid, [2.0], doc_lo=doc_lo)
            _compare(lst, key0, key1, k, 0, ("ties", fill, doc_lo, n_valid, k))


@pytest.mark.parametrize("k", KS)
def test_random_sequences_of_blocks(k):
    """many blocks into one list, the merge's output fed back (ranks >= k hold whatever it left there), few distinct scores"""
    rng = np.random.default_rng(900 + k)
    scores = [0.5, 1.0, 1.0, 1.5, 2.0, 2.0, 2.5, 3.0]
    for trial in range(8):
        got = [0] * LANES
        want = [0] * LANES
        floor = 0 if trial % 2 == 0 else make_key(1.0, 0x7FFFFFFF)
        for b in range(24):
            key0, key1 = _block(rng, int(rng.choice([1, 2, 3, 5, 16, 17, 40, 128])), scores, doc_lo=60_000 * b)
            want, want_tau = offer_sequential(want, key0, key1, k, floor)
            n = sum(1 for x in key0 + key1 if x > max(got[k - 1], floor))
            if n:
                got, got_tau = offer_rank_merge(got, key0, key1, k, floor)[:2]
            else:
                got_tau = max(got[k - 1], floor)
            assert got[:k] == want[:k] and got_tau == want_tau, (trial, b, k)
