"""Step and kernel times of rgpu_search_fields_batch on a two-field corpus, k = 10:

  fields   1024 queries (f0:a | f1:a) (f0:b | f1:b) - two dismax groups (tie 0.1) under SHOULD - on ONE segment of two fields: two
           Zipfian term sets over the same docs (indexgen.build_zipf with two seeds), field 1's postings spliced behind field 0's
           in one .doc file, each field with its own norms and statistics
  flat-or  the yardstick: rgpu_search_batch on the flat four-clause single-field OR a_0 a_1 b_0 b_1 over the same postings (the same
           file uploaded as a one-field segment). It is the nearest thing the library could run before and NOT the same query: one
           field's norms and weights, one sum, no maximum, and its dense clauses are decoded inside its window kernel.

Two warm-up steps, then the median of five timed regions of one blocking call each; per-launch times from rgpu_kernel_stats.
Before a time is taken the first rows of `fields` whose lists are short enough are recomputed in numpy from the postings as
rgpu_decode_terms hands them out (BM25 per clause with its field's norm byte and cache, the fold of include/rucene_gpu.h) and
compared bit for bit. `python scripts/measure_cross_field.py [out.json]`; DOCS / VOCAB in the environment size the corpus."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import _lib, indexgen  # noqa: E402

DOCS, VOCAB, NQ, K, TIE = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), 1024, 10, 0.1
K1, B = 1.2, 0.75
CHECK_ROWS, CHECK_POSTINGS = 6, 4_000_000

t0 = time.time()
segs = [indexgen.build_zipf(DOCS, VOCAB), indexgen.build_zipf(DOCS, VOCAB, seed=indexgen.DEFAULT_SEED ^ 0xF1E1D)]
print("built in %.1f s" % (time.time() - t0), flush=True)
a, b = segs[0].doc_bytes, segs[1].doc_bytes
header = int(segs[1].terms["doc_start_fp"][segs[1].terms["doc_freq"] >= 2].min())
assert header == int(segs[0].terms["doc_start_fp"][segs[0].terms["doc_freq"] >= 2].min())   # (the headers differ in the segment id alone)
doc = np.concatenate([a[:-16], b[header:-16], a[-16:]])   # one .doc file: field 0's postings, field 1's, the footer
terms = [segs[0].terms, segs[1].terms.copy()]
terms[1]["doc_start_fp"] += a.size - 16 - header
pairs = indexgen.log_uniform_ranks(2 * NQ, 1, 1000, 0x527563656E65 ^ 0xC7).reshape(-1, 2) - 1

ctx = rucene_amd.Context(profile_kernels=True)
seg2 = rucene_amd.Segment(ctx, doc, segs[0].norms, DOCS)     # two fields
assert seg2.attach_field(segs[1].norms) == 1
seg1 = rucene_amd.Segment(ctx, doc, segs[0].norms, DOCS)     # the same bytes as one field: the yardstick's


def weight(f, t, stats_of=None):
    s = segs[f if stats_of is None else stats_of]
    w, _, cache = _lib.bm25_compute_weight(K1, B, DOCS, s.doc_count, s.sum_total_term_freq, [int(terms[f][t]["doc_freq"])], 1.0)
    return w, cache


caches = [weight(f, 0)[1] for f in (0, 1)]
tables = [ctx.sim_table(c, K1) for c in caches]

# ---- the two batches -----------------------------------------------------------------------------------------------------------------
clauses = np.zeros(4 * NQ, _lib.FIELD_CLAUSE_DTYPE)
groups = np.zeros(2 * NQ, _lib.FIELD_GROUP_DTYPE)
queries = np.zeros(NQ, _lib.FIELDS_QUERY_DTYPE)
flat_terms = np.zeros(4 * NQ, _lib.QUERY_TERM_DTYPE)
flat_queries = np.zeros(NQ, _lib.QUERY_DTYPE)
for q, (ta, tb) in enumerate(pairs):
    for g, t in enumerate((int(ta), int(tb))):
        for f in (0, 1):
            c = clauses[4 * q + 2 * g + f]
            c["state"], c["weight"], c["sim_table"], c["field"] = terms[f][t], weight(f, t)[0], tables[f], f
            y = flat_terms[4 * q + 2 * g + f]
            y["state"], y["weight"], y["sim_table"] = terms[f][t], weight(f, t, stats_of=0)[0], tables[0]
        groups[2 * q + g] = (4 * q + 2 * g, 2, int(np.float32(TIE).view(np.uint32)), _lib.GROUP_DISMAX)
    queries[q] = (_lib.OCCUR_SHOULD, 2 * q, 2, 0, 0, 0)
    flat_queries[q] = (2, 4, 4 * q, 0)   # RGPU_OP_OR


def check_rows(hits, totals):
    """the first CHECK_ROWS rows whose four lists hold at most CHECK_POSTINGS postings, recomputed in numpy"""
    norms = [np.asarray(s.norms) for s in segs]
    done = 0
    for q, (ta, tb) in enumerate(pairs):
        if sum(int(terms[f][t]["doc_freq"]) for t in (ta, tb) for f in (0, 1)) > CHECK_POSTINGS:
            continue
        acc, count = np.zeros(DOCS, np.float32), np.zeros(DOCS, np.int8)
        for t in (int(ta), int(tb)):
            total, best, held = np.zeros(DOCS, np.float32), np.zeros(DOCS, np.float32), np.zeros(DOCS, bool)
            present = [f for f in (0, 1) if terms[f][t]["doc_freq"] > 0]
            for f in present:
                d, fr = seg2.decode_terms(terms[f][t]) if f == 0 else seg1.decode_terms(terms[f][t])
                w, cache = weight(f, t)
                wk = np.float32(np.float32(w) * np.float32(K1 + 1.0))
                fq = fr.astype(np.float32)
                s = ((wk * fq).astype(np.float32) / (fq + cache[norms[f][d]]).astype(np.float32)).astype(np.float32)
                first = ~held[d]
                total[d] = np.where(first, np.float32(0.0), total[d]) + s
                best[d] = np.where(first, s, np.maximum(best[d], s))
                held[d] = True
            gsc = best if len(present) == 1 else (best + ((total - best).astype(np.float32) * np.float32(TIE)).astype(np.float32)).astype(np.float32)
            acc = np.where(held, np.where(count == 0, np.float32(0.0) + gsc, acc + gsc), acc).astype(np.float32)
            count += held
        docs = np.flatnonzero(count > 0)
        o = np.lexsort((docs, -acc[docs].astype(np.float64)))[:K]
        n = min(K, docs.size)
        assert int(totals[q]) == docs.size, (q, int(totals[q]), docs.size)
        assert (hits[q]["doc"][:n] == docs[o]).all() and (hits[q]["doc"][n:] == -1).all(), (q, hits[q]["doc"], docs[o])
        assert (hits[q]["score"][:n].view(np.int32) == acc[docs][o].view(np.int32)).all(), (q, hits[q]["score"], acc[docs][o])
        done += 1
        if done == CHECK_ROWS:
            break
    return done


try:
    out = {"docs": DOCS, "vocab": VOCAB, "queries": NQ, "k": K, "date": time.strftime("%Y-%m-%d"),
           "postings": int(sum(int(terms[f][int(t)]["doc_freq"]) for row in pairs for t in row for f in (0, 1)))}
    calls = {"fields": lambda: seg2.search_fields_batch(queries, groups, clauses, K), "flat-or": lambda: seg1.search_batch(flat_queries, flat_terms, K)}
    for name, call in calls.items():
        for _ in range(2):
            hits, totals = call()
        if name == "fields":
            t1 = time.time()
            out["rows_recomputed"] = check_rows(hits, totals)
            print("fields: %d rows recomputed in numpy, bit-equal, in %.0f s" % (out["rows_recomputed"], time.time() - t1), flush=True)
        regions, walls = [], []
        for _ in range(5):
            ctx.kernel_stats_reset()
            t = time.perf_counter()
            hits, totals = call()
            walls.append(1e3 * (time.perf_counter() - t))
            regions.append({n: v["total_ms"] for n, v in ctx.kernel_stats().items() if v["launches"]})
        names = sorted({n for r in regions for n in r})
        med = {n: round(float(np.median([r.get(n, 0.0) for r in regions])), 4) for n in names}
        tot = float(np.median([sum(r.values()) for r in regions]))
        out[name] = {"kernels_ms_median": med, "kernels_ms_total_median": tot, "step_ms_median": float(np.median(walls)), "step_ms": walls,
                     "rows_with_hits": int((totals > 0).sum()), "hits": int(totals.sum())}
        print(name, "kernels %.3f ms, step %.3f ms (min %.3f, max %.3f)" % (tot, float(np.median(walls)), min(walls), max(walls)), med,
              "hits", int(totals.sum()), flush=True)
    out["ratio_step_fields_over_flat_or"] = out["fields"]["step_ms_median"] / out["flat-or"]["step_ms_median"]
    out["ratio_kernels_fields_over_flat_or"] = out["fields"]["kernels_ms_total_median"] / out["flat-or"]["kernels_ms_total_median"]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    seg1.close()
    seg2.close()
    ctx.close()
print("done")
