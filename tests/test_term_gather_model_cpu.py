"""Executable specification of the dealt block stage of k_search_term_query's gather (kernels/search_term_query.hpp, general path,
-DRGPU_TERMQ_DEAL=1) — a numpy model, no GPU code. The chunks that survive a window's test are dealt to the waves (wave w: cq[w], cq[w + W], ...); a chunk's
candidate blocks reserve queue entries from one shared counter, in whatever order the waves get there. A reservation that fits is
written and its chunk marked done; the first that does not fit sets q_end, leaves its chunk undone and stops its wave. The round
keeps [0, min(q_count, q_end)), sorts it by (bound desc, block asc) and drains it; a round that was full repeats the same window,
skipping the chunks marked done, with the threshold the drain reached. The model runs under many reservation orders — any
permutation of the surviving chunks, which covers every interleaving of the waves — and must show, whatever the order:
  the written entries are exactly [0, nq);  no block is queued twice;  every round completes at least one chunk (so there are at most
  as many rounds as chunk survivals: the kernel terminates);  the rows are the brute-force canonical top-k."""
import numpy as np
import pytest

from test_blockmax_model import _table, frontier_words
from test_term_queue_model import _bound, _term_blocks, sketch_floor, world  # noqa: F401  (world: the Zipf fixture)

ORDERS = 200


class _List:
    """One term's FullBlocks, with everything that does not depend on the schedule computed once."""

    def __init__(self, docs, freqs, ranks, table):
        self.nb = nb = docs.shape[0]
        self.table = table
        self.n_chunks = -(-nb // 64)
        words = frontier_words(freqs, ranks)
        self.words = words
        self.bounds = np.array([_bound(table, int(w)) for w in words.tolist()], dtype=np.int64)
        self.lo = np.concatenate([[-1], docs[:-1, -1]]).astype(np.int64)  # the doc in front of each block
        self.chunk_bound = np.full(self.n_chunks, 0xFFFFFFFF, dtype=np.int64)  # dir_sum: whole chunks only
        for c in range(nb // 64):
            ws = words[64 * c:64 * c + 64].astype(np.uint64)
            m = int((ws & np.uint64(15)).max())
            for f in range(1, 11):
                m |= int(((ws >> np.uint64(4 + 6 * (f - 1))) & np.uint64(63)).max()) << (4 + 6 * (f - 1))
            self.chunk_bound[c] = _bound(table, m)
        bits = table[ranks, np.minimum(freqs, 10)].view(np.uint32).astype(np.uint64)
        keys = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - docs.astype(np.uint64))
        self.keys = np.sort(keys, axis=1)  # per block, ascending
        flat = np.sort(keys.reshape(-1))[::-1]
        self.best = [int(x) for x in flat[:128].tolist()]  # brute force: keys are unique, larger is better (score desc, doc asc)

    def thr(self, tau, lo):
        """term_thr_of over an array of docs in front"""
        if tau == 0:
            return np.zeros_like(lo)
        bits, doc = tau >> 32, 0xFFFFFFFF - (tau & 0xFFFFFFFF)
        return bits + (doc <= lo + 1)


def deal_search(L, k, cap, W, window, order_of, floor=0, lag=0):
    """order_of(sizes) -> the order in which the window's surviving chunks (positions in cq; sizes[i] = candidates of cq[i]) reach
    the counter. Returns (hits, rounds) and asserts the schedule's invariants on the way."""
    top = []  # ascending, at most k keys
    tau = lambda: max(top[0] if len(top) == k else 0, floor)
    queued = set()
    cnext, rounds, survivals = 0, 0, 0
    done = set()  # chunks of the window at cnext whose blocks are queued
    while cnext < L.n_chunks:
        q_count, q_end, slots = 0, None, {}
        completed = 0
        full = False
        while cnext < L.n_chunks and not full:
            t = tau()
            wend = min(L.n_chunks, cnext + window)
            cs = np.arange(cnext, wend)
            cq = [int(c) for c in cs[L.chunk_bound[cs] >= L.thr(t, L.lo[64 * cs])].tolist() if c not in done]
            survivals += len(cq)
            cand = []
            for c in cq:
                b = np.arange(64 * c, min(L.nb, 64 * c + 64))
                cand.append(b[L.bounds[b] >= L.thr(t, L.lo[b])])
            stopped = set()
            for i in order_of([len(x) for x in cand]):
                if i % W in stopped:  # its wave met a full queue and takes no more chunks
                    continue
                n = len(cand[i])
                if n == 0:
                    done.add(cq[i])
                    completed += 1
                    continue
                at = q_count
                q_count += n
                if at + n <= cap:
                    for j, b in enumerate(cand[i].tolist()):
                        assert at + j not in slots
                        slots[at + j] = b
                    done.add(cq[i])
                    completed += 1
                else:
                    q_end = at if q_end is None else min(q_end, at)
                    stopped.add(i % W)
            full = q_end is not None
            if not full:
                done.clear()
                cnext = wend
        nq = min(q_count, q_end) if full else q_count
        assert sorted(slots) == list(range(nq)), (sorted(slots), nq)  # the written entries are exactly [0, nq)
        queue = list(slots.values())
        assert not (queued & set(queue)) and len(set(queue)) == len(queue)  # no block is queued twice
        queued |= set(queue)
        if full:
            assert completed >= 1 and nq >= 1  # progress: the reservation that got entry 0 fits
        if nq == 0:
            continue
        rounds += 1
        queue.sort(key=lambda b: (-int(L.bounds[b]), b))
        hist = []
        for b in queue:
            hist.append(tau())
            if L.bounds[b] < L.thr(hist[max(0, len(hist) - 1 - lag)], L.lo[b:b + 1])[0]:
                break
            if L.bounds[b] < L.thr(tau(), L.lo[b:b + 1])[0]:
                continue
            kb = L.keys[b]
            new = kb[np.searchsorted(kb, np.uint64(tau()), side="right"):]
            if new.size:
                top = sorted(top + [int(x) for x in new.tolist()])[-k:]
    assert rounds <= max(1, survivals)
    return top[::-1], rounds


def _orders(seed):
    """ORDERS seeded permutations and the three adversarial orders"""
    rng = np.random.default_rng(seed)
    out = [lambda s, r=np.random.default_rng(rng.integers(1 << 62)): r.permutation(len(s)).tolist() for _ in range(ORDERS)]
    out.append(lambda s: sorted(range(len(s)), key=lambda i: -s[i]))  # fullest chunk first
    out.append(lambda s: sorted(range(len(s)), key=lambda i: s[i]))   # fullest chunk last
    out.append(lambda s: list(range(len(s)))[::-1])                   # strictly reverse
    return out


def _run_all(L, k, cap, floors, seed, windows=(4096,), waves=(4,)):
    want = L.best[:k]
    most = 0
    for fl in floors:
        for window in windows:
            for W in waves:
                for order_of in _orders(seed):
                    hits, rounds = deal_search(L, k, cap, W, window, order_of, floor=fl)
                    assert hits == want[:len(hits)] and len(hits) == min(k, len(want), 128 * L.nb), (k, cap, fl, window, W)
                    most = max(most, rounds)
    return most


@pytest.fixture(scope="module")
def zipf_lists(oracle, world):  # noqa: F811
    seg, oseg, _ = world
    return {term: _List(*_term_blocks(seg, oseg, term)) for term in (0, 1, 3, 9, 40, 200)}


@pytest.mark.parametrize("term", [0, 1, 3, 9, 40, 200])
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("cap", [64, 256])
def test_zipf_terms_any_reservation_order(zipf_lists, term, k, cap):
    L = zipf_lists[term]
    floor = sketch_floor_of(L, k)
    # (one window holds these lists; a window of 3 chunks also moves the window edge and the done bits through them)
    most = _run_all(L, k, cap, (floor, 0), seed=1000 * term + k, windows=(4096, 3) if term in (0, 3) else (4096,))
    print("term %d k %d cap %d, %d FullBlocks: at most %d rounds" % (term, k, cap, L.nb, most))


def sketch_floor_of(L, k):
    return sketch_floor(L.table, L.words, k)


def _ramp(levels, per, seed=3):
    """test_term_queue_model's ramp of tying levels: every block's best posting ties within a level and the levels rise along the list"""
    rng = np.random.default_rng(seed)
    nb = levels * per
    docs = np.sort(rng.choice(10 * 128 * nb, size=128 * nb, replace=False)).astype(np.int64).reshape(nb, 128)
    freqs = np.ones((nb, 128), np.int64)
    freqs[:, 5] = 2 + np.arange(nb) // per
    ranks = np.zeros((nb, 128), np.int64)
    ranks[:, 5] = 3
    cache = np.array([1.5, 1.2, 1.0, 0.8], np.float32)
    return _List(docs, freqs, ranks, _table(2.0, 1.2, cache, np.arange(4)))


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("cap", [64, 256])
def test_ramp_overflows_round_after_round(k, cap):
    L = _ramp(6, 70)
    most = _run_all(L, k, cap, (0, sketch_floor_of(L, k)), seed=k + cap, windows=(4096, 2), waves=(2, 4, 8))
    assert most >= 2  # without a starting threshold the 420 tying-by-level blocks do not fit one round
    print("ramp k %d cap %d: at most %d rounds" % (k, cap, most))


def _all_tie(nb, seed=5):
    """every block ties: one freq, one norm"""
    rng = np.random.default_rng(seed)
    docs = np.sort(rng.choice(4 * 128 * nb, size=128 * nb, replace=False)).astype(np.int64).reshape(nb, 128)
    freqs = np.full((nb, 128), 2, np.int64)
    ranks = np.zeros((nb, 128), np.int64)
    return _List(docs, freqs, ranks, _table(2.0, 1.2, np.array([1.0], np.float32), np.arange(1)))


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("cap", [64, 256])
@pytest.mark.parametrize("over", [-1, 0, 1], ids=["one short", "exactly full", "one over"])
def test_queue_exactly_full_and_one_over(k, cap, over):
    """cap - 1, cap and cap + 1 tying blocks without a starting threshold: the first gather's candidates are every block. Exactly
    full is one round (q_end never set: q_count == cap fits); one over leaves a chunk for a second round whatever the order."""
    L = _all_tie(cap + over)
    for W in (2, 4, 8):
        for order_of in _orders(cap + over):
            hits, rounds = deal_search(L, k, cap, W, 4096, order_of)
            assert hits == L.best[:k]
            if over <= 0:
                assert rounds == 1
    # the rows are the first k docs: every score ties
    assert [0xFFFFFFFF - (h & 0xFFFFFFFF) for h in L.best[:k]] == sorted(0xFFFFFFFF - (int(x) & 0xFFFFFFFF) for x in L.keys.reshape(-1))[:k]
