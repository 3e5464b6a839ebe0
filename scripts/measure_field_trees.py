"""Step and kernel times of rgpu_search_fields_tree_batch on a two-field corpus, k = 10. The corpus is
measure_cross_field.py's: two Zipfian term sets over the same 10 M docs, field 1's postings spliced behind field 0's in one .doc file,
each field with its own norms and statistics. 1024 query-string trees over the two fields, every word a sum group (f0:w f1:w):

  +a b rule   "+a b": ReqOptScorer under its sequential rule - k_fields_tree_windows leaves records, k_req_opt_scan walks them
  +a b add    the same batch on a context opened with req_opt_rule = -1: one pass, req + opt everywhere
  a b         "a b": two sum groups under SHOULD
  dismax-old  the yardstick: rgpu_search_fields_batch on the groups of `a b` written as DisjunctionMaxQuery at tie 1.0 under SHOULD -
              max + (sum - max) * 1.0, the nearest tree the old call serves (NOT the same scores)
  dismax-new  the batch of dismax-old through the new call: a batch both calls serve, byte-identical rows

Two warm-up steps, then the median of five timed regions of one blocking call each; per-launch times from rgpu_kernel_stats.
Before a time is taken the first rows of `+a b rule`, `+a b add` and `a b` whose lists are short enough are recomputed in numpy from
the postings as rgpu_decode_terms hands them out and compared bit for bit. `python scripts/measure_field_trees.py [out.json]`;
DOCS / VOCAB in the environment size the corpus."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import _lib, indexgen  # noqa: E402

DOCS, VOCAB, NQ, K = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), 1024, 10
K1, B = 1.2, 0.75
CHECK_ROWS, CHECK_POSTINGS = 4, 4_000_000

t0 = time.time()
segs = [indexgen.build_zipf(DOCS, VOCAB), indexgen.build_zipf(DOCS, VOCAB, seed=indexgen.DEFAULT_SEED ^ 0xF1E1D)]
print("built in %.1f s" % (time.time() - t0), flush=True)
a, b = segs[0].doc_bytes, segs[1].doc_bytes
header = int(segs[1].terms["doc_start_fp"][segs[1].terms["doc_freq"] >= 2].min())
assert header == int(segs[0].terms["doc_start_fp"][segs[0].terms["doc_freq"] >= 2].min())
doc = np.concatenate([a[:-16], b[header:-16], a[-16:]])
terms = [segs[0].terms, segs[1].terms.copy()]
terms[1]["doc_start_fp"] += a.size - 16 - header
pairs = indexgen.log_uniform_ranks(2 * NQ, 1, 1000, 0x527563656E65 ^ 0xC7).reshape(-1, 2) - 1
norms = [np.asarray(s.norms) for s in segs]


def weight(f, t):
    s = segs[f]
    w, _, cache = _lib.bm25_compute_weight(K1, B, DOCS, s.doc_count, s.sum_total_term_freq, [int(terms[f][t]["doc_freq"])], 1.0)
    return w, cache


class Side:
    """One context (a rule mode) with the two-field segment and the fields' sim tables"""

    def __init__(self, req_opt_rule):
        self.ctx = rucene_amd.Context(profile_kernels=True, req_opt_rule=req_opt_rule)
        self.seg = rucene_amd.Segment(self.ctx, doc, segs[0].norms, DOCS)
        assert self.seg.attach_field(segs[1].norms) == 1
        self.tables = [self.ctx.sim_table(weight(f, 0)[1], K1) for f in (0, 1)]

    def clauses(self):
        out = np.zeros(4 * NQ, _lib.FIELD_CLAUSE_DTYPE)
        for q, (ta, tb) in enumerate(pairs):
            for g, t in enumerate((int(ta), int(tb))):
                for f in (0, 1):
                    c = out[4 * q + 2 * g + f]
                    c["state"], c["weight"], c["sim_table"], c["field"] = terms[f][t], weight(f, t)[0], self.tables[f], f
        return out

    def close(self):
        self.seg.close()
        self.ctx.close()


def tree_batch(n_must, kind):
    groups = np.zeros(2 * NQ, _lib.FIELD_TREE_GROUP_DTYPE)
    queries = np.zeros(NQ, _lib.FIELDS_TREE_QUERY_DTYPE)
    one = int(np.float32(1.0).view(np.uint32))
    for q in range(NQ):
        for g in (0, 1):
            groups[2 * q + g] = (4 * q + 2 * g, 2, one, kind, 0, 0)
        queries[q] = (2 * q, n_must, 2 - n_must, 0, 0, 0)
    return queries, groups


def old_batch():
    groups = np.zeros(2 * NQ, _lib.FIELD_GROUP_DTYPE)
    queries = np.zeros(NQ, _lib.FIELDS_QUERY_DTYPE)
    one = int(np.float32(1.0).view(np.uint32))
    for q in range(NQ):
        for g in (0, 1):
            groups[2 * q + g] = (4 * q + 2 * g, 2, one, _lib.GROUP_DISMAX)
        queries[q] = (_lib.OCCUR_SHOULD, 2 * q, 2, 0, 0, 0)
    return queries, groups


def sum_group(t):
    """-> (held, 0.0f + s_0 + s_1 per doc) of the word's sum group"""
    total, held = np.zeros(DOCS, np.float32), np.zeros(DOCS, bool)
    for f in (0, 1):
        if terms[f][t]["doc_freq"] == 0:
            continue
        d, fr = plain.decode_terms(terms[f][t])   # (the same bytes uploaded as ONE field: a field-0 call reads any term's postings)
        w, cache = weight(f, t)
        wk = np.float32(np.float32(w) * np.float32(K1 + 1.0))
        fq = fr.astype(np.float32)
        s = ((wk * fq).astype(np.float32) / (fq + cache[norms[f][d]]).astype(np.float32)).astype(np.float32)
        total[d] = (np.where(held[d], total[d], np.float32(0.0)) + s).astype(np.float32)
        held[d] = True
    return held, total


def check_rows(hits, totals, n_must, rule):
    """the first CHECK_ROWS rows whose four lists hold at most CHECK_POSTINGS postings, recomputed in numpy"""
    done = 0
    for q, (ta, tb) in enumerate(pairs):
        if sum(int(terms[f][t]["doc_freq"]) for t in (ta, tb) for f in (0, 1)) > CHECK_POSTINGS:
            continue
        (ha, sa), (hb, sb) = sum_group(int(ta)), sum_group(int(tb))
        if n_must == 0:      # 0.0f + ga + gb over the groups on the doc
            docs = np.flatnonzero(ha | hb)
            acc = np.where(ha, np.float32(0.0) + sa, np.float32(0.0)).astype(np.float32)
            acc = np.where(hb, np.where(ha, acc + sb, np.float32(0.0) + sb), acc).astype(np.float32)
            final = acc[docs]
        else:                # req = ga as it is, opt = 0.0f + gb; the rule over the hits in doc order
            docs = np.flatnonzero(ha)
            req, opt = sa[docs], np.where(hb[docs], np.float32(0.0) + sb[docs], np.float32(0.0)).astype(np.float32)
            final = (req + opt).astype(np.float32)
            if rule:
                ssum, num = np.float32(0.0), 0
                for i in range(docs.size):
                    if num > 100 and np.float32(2.0) * req[i] < ssum / np.float32(num):
                        final[i] = req[i]
                    else:
                        ssum, num = np.float32(ssum + req[i]), num + 1
        o = np.lexsort((docs, -final.astype(np.float64)))[:K]
        n = min(K, docs.size)
        assert int(totals[q]) == docs.size, (q, int(totals[q]), docs.size)
        assert (hits[q]["doc"][:n] == docs[o]).all() and (hits[q]["doc"][n:] == -1).all(), (q, hits[q]["doc"], docs[o])
        assert (hits[q]["score"][:n].view(np.int32) == final[o].view(np.int32)).all(), (q, hits[q]["score"], final[o])
        done += 1
        if done == CHECK_ROWS:
            break
    return done


sides = {"rule": Side(0), "add": Side(-1)}
plain = rucene_amd.Segment(sides["rule"].ctx, doc, segs[0].norms, DOCS)
try:
    out = {"docs": DOCS, "vocab": VOCAB, "queries": NQ, "k": K, "date": time.strftime("%Y-%m-%d"),
           "postings": int(sum(int(terms[f][int(t)]["doc_freq"]) for row in pairs for t in row for f in (0, 1))),
           "lead_postings": int(sum(int(terms[f][int(row[0])]["doc_freq"]) for row in pairs for f in (0, 1)))}
    rule, add = sides["rule"], sides["add"]
    cl = {name: s.clauses() for name, s in sides.items()}
    must_q, sum_g = tree_batch(1, _lib.GROUP_SUM)
    should_q, _ = tree_batch(0, _lib.GROUP_SUM)
    dm_q, dm_g = tree_batch(0, _lib.GROUP_DISMAX)
    old_q, old_g = old_batch()
    calls = [("+a b rule", rule, lambda: rule.seg.search_fields_tree_batch(must_q, sum_g, cl["rule"], K), (1, True)),
             ("+a b add", add, lambda: add.seg.search_fields_tree_batch(must_q, sum_g, cl["add"], K), (1, False)),
             ("a b", rule, lambda: rule.seg.search_fields_tree_batch(should_q, sum_g, cl["rule"], K), (0, True)),
             ("dismax-old", rule, lambda: rule.seg.search_fields_batch(old_q, old_g, cl["rule"], K), None),
             ("dismax-new", rule, lambda: rule.seg.search_fields_tree_batch(dm_q, dm_g, cl["rule"], K), None)]
    kept = {}
    for name, side, call, check in calls:
        for _ in range(2):
            hits, totals = call()
        if check is not None:
            t1 = time.time()
            n = check_rows(hits, totals, *check)
            out.setdefault("rows_recomputed", {})[name] = n
            print("%s: %d rows recomputed in numpy, bit-equal, in %.0f s" % (name, n, time.time() - t1), flush=True)
        regions, walls = [], []
        for _ in range(5):
            side.ctx.kernel_stats_reset()
            t = time.perf_counter()
            hits, totals = call()
            walls.append(1e3 * (time.perf_counter() - t))
            regions.append({n: v["total_ms"] for n, v in side.ctx.kernel_stats().items() if v["launches"]})
        launches = {n: v["launches"] for n, v in side.ctx.kernel_stats().items() if v["launches"]}
        names = sorted({n for r in regions for n in r})
        med = {n: round(float(np.median([r.get(n, 0.0) for r in regions])), 4) for n in names}
        tot = float(np.median([sum(r.values()) for r in regions]))
        kept[name] = (hits.tobytes(), totals.copy())
        out[name] = {"kernels_ms_median": med, "kernels_ms_total_median": tot, "step_ms_median": float(np.median(walls)), "step_ms": walls,
                     "launches": launches, "rows_with_hits": int((totals > 0).sum()), "hits": int(totals.sum())}
        print(name, "kernels %.3f ms, step %.3f ms (min %.3f, max %.3f)" % (tot, float(np.median(walls)), min(walls), max(walls)), med, launches,
              "hits", int(totals.sum()), flush=True)
    assert kept["dismax-old"][0] == kept["dismax-new"][0] and (kept["dismax-old"][1] == kept["dismax-new"][1]).all()
    out["dismax_rows_identical"] = True
    scan = out["+a b rule"]["kernels_ms_median"].get("k_req_opt_scan", 0.0)
    out["share_k_req_opt_scan"] = scan / out["+a b rule"]["kernels_ms_total_median"]
    for name in ("+a b rule", "+a b add", "a b", "dismax-new"):
        out["ratio_step_%s_over_dismax_old" % name] = out[name]["step_ms_median"] / out["dismax-old"]["step_ms_median"]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    plain.close()
    for s in sides.values():
        s.close()
print("done")
