"""Step and kernel times of rgpu_search_span_unordered_batch on the benchmark's positions corpus, k = 10:

  unordered-2   1024 two-clause unordered SpanNearQuerys at slop 2 (bench.py's pairs)
  ordered-2     the same pairs through rgpu_search_span_near_batch        } the yardsticks: code the unordered call does not touch,
  sloppy-2      the same pairs as sloppy PhraseQuerys at slop 2           } expected where scripts/measure_span_near.py measured them
  unordered-6   256 six-clause unordered queries at slop 24: k_span_unordered_lanes answers
  unordered-7   256 seven-clause ones: every candidate goes on to k_span_unordered, one wavefront each

Two warm-up steps, then the median of five timed regions of one blocking call each; kernel times from rgpu_kernel_stats.

Before a time is taken every row an unordered leg returns is compared with the model of tests/span_unordered.py (NearSpansUnordered
restated statement for statement), over the postings as rgpu_decode_terms / rgpu_decode_positions hand them out: every returned
hit must be a doc of the conjunction whose walk gives exactly the returned score bits and no better doc may be missing among the
checked ones; a row whose conjunction has at most FULL_ROW candidates is recomputed whole - total hits and the top k, doc ids and
score bits. (Whole rows over millions of candidates are not recomputed in Python; the figure printed says how many rows were.)
`python scripts/measure_span_unordered.py [out.json]`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rucene_amd  # noqa: E402
from rucene_amd import indexgen  # noqa: E402
import span_near as sn  # noqa: E402
import span_unordered as su  # noqa: E402

SEED_QUERIES = 0x527563656E65 ^ 0x51
DOCS, VOCAB, NQ, K, SLOP = int(os.environ.get("DOCS", 10_000_000)), 1_000_000, 1024, 10, 2
NQ_MANY, SLOP_MANY, FULL_ROW = 256, 24, int(os.environ.get("FULL_ROW", 3000))
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB, positions=True)
print("built in %.1f s" % (time.time() - t0), flush=True)
ranks = indexgen.log_uniform_ranks(2 * NQ, 1, 1000, SEED_QUERIES ^ 0xF2).reshape(-1, 2) - 1   # bench.py's pairs
many = {n: indexgen.log_uniform_ranks(n * NQ_MANY, 1, 200, SEED_QUERIES ^ (0xA0 + n)).reshape(-1, n) - 1 for n in (6, 7)}
S, N = rucene_amd.SpanTermQuery, rucene_amd.SpanNearQuery

ctx = rucene_amd.Context(profile_kernels=True)
leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)


def near(terms, slop, in_order):
    return g.pack_phrases([N([S(int(t)) for t in row], slop=slop, in_order=in_order) for row in terms], leaf)


_lists = {}


def postings_of(term):
    """(docs, offsets into positions, positions) of one term, decoded by the library's decode kernels; the last few are kept"""
    if term not in _lists:
        if len(_lists) >= 48:
            _lists.pop(next(iter(_lists)))
        state, ptrs = leaf.positions_state(int(term))
        docs, freqs = leaf.segment.decode_terms(state)
        _lists[term] = (docs, np.concatenate([[0], np.cumsum(freqs, dtype=np.int64)]), leaf.segment.decode_positions(state, ptrs))
    return _lists[term]


def lists_of(terms, doc):
    out = []
    for t in terms:
        docs, at, positions = postings_of(t)
        i = int(np.searchsorted(docs, doc))
        if i >= docs.size or docs[i] != doc:
            return None
        out.append(positions[at[i]:at[i + 1]].tolist())
    return out


def check_rows(name, terms, slop, hits, totals):
    """every returned row against the model (see the module docstring) -> (rows recomputed whole, hits checked)"""
    whole = checked = 0
    norms = np.asarray(seg.norms)
    for r, row in enumerate(terms):
        row = [int(t) for t in row]
        dfs = [int(leaf.terms[t]["doc_freq"]) for t in row]
        weight, cache = sn.weight_of(dfs, seg.max_doc, seg.doc_count, seg.sum_total_term_freq)
        got = [(int(d), np.float32(s)) for d, s in zip(hits[r]["doc"], hits[r]["score"]) if d >= 0]
        assert len(got) == min(K, int(totals[r])), (name, r, len(got), int(totals[r]))
        for doc, score in got:
            lists = lists_of(row, doc)
            assert lists is not None, (name, r, doc, "not a doc of the conjunction")
            hit, freq, _ = su.walk_reference(lists, slop)
            want = sn.score(weight, cache, freq, norms[doc])
            assert hit and want.view(np.int32) == score.view(np.int32), (name, r, row, doc, float(want), float(score))
            checked += 1
        assert got == sorted(got, key=lambda x: (-float(x[1]), x[0])), (name, r)
        if min(dfs) <= 40 * FULL_ROW:
            cand = postings_of(row[int(np.argmin(dfs))])[0]
            for t in row:
                docs_t = postings_of(t)[0]
                cand = cand[docs_t[np.minimum(np.searchsorted(docs_t, cand), docs_t.size - 1)] == cand]
                if cand.size == 0:
                    break
            if cand.size <= FULL_ROW:
                rows = []
                for doc in cand.tolist():
                    hit, freq, _ = su.walk_reference(lists_of(row, doc), slop)
                    if hit:
                        rows.append((doc, sn.score(weight, cache, freq, norms[doc])))
                rows.sort(key=lambda x: (-float(x[1]), x[0]))
                assert len(rows) == int(totals[r]), (name, r, len(rows), int(totals[r]))
                assert [(d, s.view(np.int32)) for d, s in rows[:K]] == [(d, s.view(np.int32)) for d, s in got], (name, r)
                whole += 1
    return whole, checked


try:
    out = {"docs": DOCS, "k": K, "date": time.strftime("%Y-%m-%d")}
    packed = {"unordered-2": near(ranks, SLOP, False), "ordered-2": near(ranks, SLOP, True),
              "sloppy-2": g.pack_phrases([rucene_amd.PhraseQuery([int(a), int(b)], slop=SLOP) for a, b in ranks], leaf),
              "unordered-6": near(many[6], SLOP_MANY, False), "unordered-7": near(many[7], SLOP_MANY, False)}
    calls = {"unordered-2": leaf.segment.search_span_unordered_batch, "ordered-2": leaf.segment.search_span_near_batch,
             "sloppy-2": leaf.segment.search_phrase_batch, "unordered-6": leaf.segment.search_span_unordered_batch,
             "unordered-7": leaf.segment.search_span_unordered_batch}
    models = {"unordered-2": (ranks, SLOP), "unordered-6": (many[6], SLOP_MANY), "unordered-7": (many[7], SLOP_MANY)}
    for name, args in packed.items():
        for _ in range(2):
            hits, totals = calls[name](*args, K)
        if name in models:
            t1 = time.time()
            whole, checked = check_rows(name, *models[name], hits, totals)
            print(name, "rows against the model: %d hits of %d rows, %d rows recomputed whole, in %.0f s" % (checked, len(totals), whole, time.time() - t1),
                  flush=True)
            out.setdefault("checked", {})[name] = {"hits": checked, "rows": int(len(totals)), "rows_recomputed_whole": whole}
        regions, walls = [], []
        for _ in range(5):
            ctx.kernel_stats_reset()
            t = time.perf_counter()
            hits, totals = calls[name](*args, K)
            walls.append(1e3 * (time.perf_counter() - t))
            regions.append({n: v["total_ms"] for n, v in ctx.kernel_stats().items() if v["launches"]})
        names = sorted({n for r in regions for n in r})
        med = {n: round(float(np.median([r.get(n, 0.0) for r in regions])), 4) for n in names}
        tot = float(np.median([sum(r.values()) for r in regions]))
        out[name] = {"kernels_ms_median": med, "kernels_ms_total_median": tot, "step_ms_median": float(np.median(walls)), "step_ms": walls,
                     "rows_with_hits": int((totals > 0).sum()), "hits": int(totals.sum())}
        print(name, "kernels %.3f ms, step %.3f ms (min %.3f, max %.3f)" % (tot, float(np.median(walls)), min(walls), max(walls)), med,
              "rows with hits", int((totals > 0).sum()), "hits", int(totals.sum()), flush=True)
    if len(sys.argv) > 1:   # optional: a file for the result tree
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    ctx.close()
print("done")
