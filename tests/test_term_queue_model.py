"""Executable specification of k_search_term_query's schedule (kernels/search_term_query.hpp) — a numpy model, no GPU code. One query:
rounds of (gather, sort, drain) over a queue of fixed capacity. The gather tests whole chunks of 64 blocks against their field-wise
maximum frontier word (strict when the doc in front of the chunk is at or past the threshold's doc), then the blocks of the chunks
that survive, and appends the blocks that may still enter, chunk by chunk, until the next chunk would not fit. The queue is sorted
by (bound desc, block asc) and popped in that order; the first pop that fails the threshold ends the round. A popped block is tested
again just before it is unpacked, against a threshold that may have risen meanwhile (`lag`: pops in flight). The model must return
the brute-force canonical top-k of the FullBlock postings (whose scores the oracle pins) for any capacity and lag, with and without
the sketch's starting threshold, and it reports per query the candidates per round and the blocks unpacked — the numbers behind
the queue capacity (256) and the workgroup width."""
import numpy as np
import pytest

from test_blockmax_model import _TopK, _key, _table, frontier_words

INT_MAX = 0x7FFFFFFF


def _thr(tau, lo):
    """term_thr_of: raw score bits a block's bound must reach; strict when no doc of the block (all > lo) can win a tie"""
    if tau == 0:
        return 0
    bits, doc = tau >> 32, 0xFFFFFFFF - (tau & 0xFFFFFFFF)
    return bits + 1 if doc <= lo + 1 else bits


def _bound(table, w):
    """term_bound_of: the largest table[rank_f][f] over f <= the word's largest freq (raw bits); all ones without a bound"""
    fmax = w & 15
    if fmax > 10:
        return 0xFFFFFFFF
    return max([int(table[(w >> (4 + 6 * (f - 1))) & 63, f].view(np.uint32)) for f in range(1, fmax + 1)] + [0])


def sketch_floor(table, words, k):
    """sketch_floor: the k-th best of the blocks' (largest freq, its largest rank) scores, as the key (score, largest doc id)"""
    s = []
    for w in words.tolist():
        f = w & 15
        if 1 <= f <= 10:
            s.append(int(table[(w >> (4 + 6 * (f - 1))) & 63, f].view(np.uint32)))
    if len(s) < k:
        return 0
    m = sorted(s, reverse=True)[k - 1]
    return _key(m, INT_MAX) if m else 0


def queue_search(docs, freqs, ranks, table, k, cap=256, floor=0, lag=0):
    nb = docs.shape[0]
    words = frontier_words(freqs, ranks)
    n_chunks = -(-nb // 64)
    chunk_words = [None] * n_chunks  # SegView::dir_sum: the field-wise maximum of a whole chunk's words (none for a partial chunk)
    for c in range(nb // 64):
        ws = words[64 * c:64 * c + 64].astype(np.uint64)
        m = int((ws & np.uint64(15)).max())
        for f in range(1, 11):
            m |= int(((ws >> np.uint64(4 + 6 * (f - 1))) & np.uint64(63)).max()) << (4 + 6 * (f - 1))
        chunk_words[c] = m
    bounds = [_bound(table, int(w)) for w in words.tolist()]
    lo_of = lambda b: -1 if b == 0 else int(docs[b - 1, -1])
    top = _TopK(k)
    tau = lambda: max(top.tau(), floor)
    cnext, rounds, unpacked = 0, [], 0
    while cnext < n_chunks:
        queue, full = [], False
        while cnext < n_chunks and not full:
            t = tau()
            window = [c for c in range(cnext, n_chunks)
                      if (_bound(table, chunk_words[c]) if chunk_words[c] is not None else 0xFFFFFFFF) >= _thr(t, lo_of(64 * c))]
            for c in window:
                cand = [b for b in range(64 * c, min(nb, 64 * c + 64)) if bounds[b] >= _thr(t, lo_of(b))]
                if len(queue) + len(cand) > cap:
                    cnext, full = c, True
                    break
                queue += cand
            if not full:
                cnext = n_chunks
        rounds.append(len(queue))
        queue.sort(key=lambda b: (-bounds[b], b))
        hist = []  # the threshold at every pop: a pop is tested with the one `lag` pops earlier (the list lags behind the pops in flight)
        for b in queue:
            hist.append(tau())
            if bounds[b] < _thr(hist[max(0, len(hist) - 1 - lag)], lo_of(b)):
                break
            if bounds[b] < _thr(tau(), lo_of(b)):  # the second test, just before the unpack
                continue
            unpacked += 1
            s = table[ranks[b], np.minimum(freqs[b], 10)].view(np.uint32)
            for d, sb in zip(docs[b].tolist(), s.tolist()):
                if _key(sb, d) > tau():
                    top.offer(_key(sb, d))
    hits = sorted(top.keys, reverse=True)
    return [(0xFFFFFFFF - (h & 0xFFFFFFFF), np.array([h >> 32], dtype=np.uint32).view(np.float32)[0]) for h in hits], rounds, unpacked


@pytest.fixture(scope="module")
def world(oracle):
    import __graft_entry__ as g
    g.build()
    from rucene_amd import indexgen
    seg = indexgen.build_zipf(300_000, 20_000, seed=17)
    oseg = oracle.Segment(seg.doc_bytes, seg.norms, seg.max_doc, seg.terms, sum_total_term_freq=seg.sum_total_term_freq)
    return seg, oseg, oracle.Searcher([oseg])


def _term_blocks(seg, oseg, term):
    import rucene_amd
    d, f = oseg.decode_term(seg.terms[term])
    nb = len(d) // 128
    docs, freqs = d[:nb * 128].reshape(nb, 128), f[:nb * 128].reshape(nb, 128)
    rank_to_norm = np.unique(seg.norms)
    ranks = np.searchsorted(rank_to_norm, seg.norms[docs])
    w, _, cache = rucene_amd.bm25_compute_weight(1.2, 0.75, seg.max_doc, seg.doc_count, seg.sum_total_term_freq,
                                                 [int(seg.terms[term]["doc_freq"])])
    return docs, freqs, ranks, _table(w, 1.2, np.asarray(cache, dtype=np.float32), rank_to_norm)


def _want(docs, freqs, ranks, table, k):
    scores = table[ranks, np.minimum(freqs, 10)]
    order = np.lexsort((docs.reshape(-1), -scores.reshape(-1)))[:k]
    return [(int(docs.reshape(-1)[i]), np.float32(scores.reshape(-1)[i])) for i in order]


@pytest.mark.parametrize("term", [0, 1, 3, 9, 40, 200])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_queue_schedule_is_exact(oracle, world, term, k):
    seg, oseg, searcher = world
    docs, freqs, ranks, table = _term_blocks(seg, oseg, term)
    od, os_, _ = searcher.search(oracle.OP_TERM, [term], 5, tie_mode=oracle.TIE_CANONICAL)
    best = dict(zip(docs.reshape(-1).tolist(), table[ranks, np.minimum(freqs, 10)].reshape(-1).tolist()))
    for dd, ss in zip(od.tolist(), os_.tolist()):
        if dd in best:
            assert np.float32(best[dd]) == np.float32(ss)  # the model's table scores are the oracle's, bit for bit
    want = _want(docs, freqs, ranks, table, k)
    floor = sketch_floor(table, frontier_words(freqs, ranks), k)
    report = []
    for cap in (64, 256):
        for fl in (floor, 0):
            for lag in (0, 16):
                hits, rounds, unpacked = queue_search(docs, freqs, ranks, table, k, cap=cap, floor=fl, lag=lag)
                assert [(h[0], np.float32(h[1])) for h in hits] == want, (cap, fl, lag)
                report.append((cap, bool(fl), lag, rounds[:6], unpacked))
    print("term %d k %d, %d FullBlocks: (cap, sketch, lag, candidates per round, unpacked) %s" % (term, k, docs.shape[0], report))


def test_ties_overflow_the_queue_in_rounds():
    """Every block's best posting ties within a level and the levels rise along the list: without a starting threshold every round
    fills the queue and the next round's blocks beat it; the answer is still the canonical top-k."""
    rng = np.random.default_rng(3)
    nb, per = 1200, 200
    docs = np.sort(rng.choice(10 * 128 * nb, size=128 * nb, replace=False)).astype(np.int64).reshape(nb, 128)
    freqs = np.ones((nb, 128), np.int64)
    freqs[:, 5] = 2 + np.arange(nb) // per
    ranks = np.zeros((nb, 128), np.int64)
    ranks[:, 5] = 3
    cache = np.array([1.5, 1.2, 1.0, 0.8], np.float32)  # shorter docs (higher rank) score higher: a monotone table
    table = _table(2.0, 1.2, cache, np.arange(4))
    for k in (1, 10, 128):
        want = _want(docs, freqs, ranks, table, k)
        for fl in (0, sketch_floor(table, frontier_words(freqs, ranks), k)):
            hits, rounds, unpacked = queue_search(docs, freqs, ranks, table, k, cap=64, floor=fl)
            assert [(h[0], np.float32(h[1])) for h in hits] == want
            if fl == 0:
                assert len(rounds) >= 3 and rounds[0] == 64, rounds
            print("ramp k %d sketch %s: candidates per round %s, unpacked %d" % (k, bool(fl), rounds, unpacked))
