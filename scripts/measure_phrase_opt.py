"""Step and kernel times of rgpu_search_phrase_opt_batch for 1024 queries +a +b "a b" (the phrase boost), k = 10, on the benchmark's
10 M-doc positions corpus, beside the two nearest things the library could run before for the same pairs:

  phrase-bool     rgpu_search_phrase_bool_batch on +"a b": a DIFFERENT query - only the docs that hold the phrase are hits, nothing
                  is scored but the phrase; it shares the candidate conjunction, the match stage and k_phrase_bool_score
  and + rescore   rgpu_search_batch on +a +b, then rgpu_rescore_phrase_batch over its top k with "a b": a DIFFERENT query too - the
                  phrase re-ranks the first pass's ten hits, it does not lift a doc into them

Two warm-up steps, then the median of five timed regions of one blocking call each (min .. max beside it); per-launch times from
rgpu_kernel_stats, and the share of k_req_opt_join and k_req_opt_scan in the new call's kernel time.
`python scripts/measure_phrase_opt.py [out.json]`; DOCS / VOCAB in the environment size the corpus."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import _lib, indexgen  # noqa: E402

SEED_QUERIES = 0x527563656E65 ^ 0x51
DOCS, VOCAB, NQ, K = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), 1024, 10
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB, positions=True)
print("built in %.1f s" % (time.time() - t0), flush=True)
ctx = rucene_amd.Context(profile_kernels=True)
leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx, optional_phrases=True)
ranks = indexgen.log_uniform_ranks(2 * NQ, 1, 1000, SEED_QUERIES ^ 0xF5).reshape(-1, 2) - 1
T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
try:
    out = {"docs": DOCS, "vocab": VOCAB, "rows": NQ, "k": K, "date": time.strftime("%Y-%m-%d")}
    pairs = [(int(a), int(b)) for a, b in ranks]
    opt = g.pack_phrase_opt([B.build([T(a), T(b)], [P([a, b])]) for a, b in pairs], leaf)
    pbool = g.pack_phrase_bool([B([P([a, b])], [], 0) for a, b in pairs], leaf)
    and_qs, and_ts = g.pack([B.build([T(a), T(b)], []) for a, b in pairs], leaf)
    ph_qs, ph_ts = g.pack_phrases([P([a, b]) for a, b in pairs], leaf)
    req = np.zeros(NQ, dtype=_lib.RESCORE_REQUEST_DTYPE)
    req["query_weight"], req["rescore_weight"], req["mode"], req["window_size"] = 1.0, 1.0, _lib.RESCORE_TOTAL, K

    def and_rescore():
        hits, totals = leaf.segment.search_batch(and_qs, and_ts, K)
        return leaf.segment.rescore_phrase_batch(ph_qs, ph_ts, req, hits, finish=True), totals
    legs = {"phrase-opt": lambda: leaf.segment.search_phrase_opt_batch(*opt, K), "phrase-bool": lambda: leaf.segment.search_phrase_bool_batch(*pbool, K),
            "and + rescore": and_rescore}
    totals = {}
    for name, call in legs.items():
        for _ in range(2):
            res = call()
        regions, walls = [], []
        for _ in range(5):
            ctx.kernel_stats_reset()
            t = time.perf_counter()
            res = call()
            walls.append(1e3 * (time.perf_counter() - t))
            regions.append({n: v["total_ms"] for n, v in ctx.kernel_stats().items() if v["launches"]})
        totals[name] = res[1]
        names = sorted({n for r in regions for n in r})
        med = {n: round(float(np.median([r.get(n, 0.0) for r in regions])), 4) for n in names}
        tot = float(np.median([sum(r.values()) for r in regions]))
        out[name] = {"kernels_ms_median": med, "kernels_ms_total_median": tot, "step_ms_median": float(np.median(walls)), "step_ms_min": min(walls),
                     "step_ms_max": max(walls), "hits": int(res[1].sum())}
        print(name, "kernels %.3f ms, step %.3f ms (min %.3f, max %.3f), %d hits" % (tot, float(np.median(walls)), min(walls), max(walls), int(res[1].sum())),
              med, flush=True)
    # the conjunction's docs are the new call's hits; the phrase's docs are among them
    assert (totals["phrase-opt"] == totals["and + rescore"]).all() and (totals["phrase-bool"] <= totals["phrase-opt"]).all()
    mine = out["phrase-opt"]
    out["share_join"] = mine["kernels_ms_median"].get("k_req_opt_join", 0.0) / mine["kernels_ms_total_median"]
    out["share_scan"] = mine["kernels_ms_median"].get("k_req_opt_scan", 0.0) / mine["kernels_ms_total_median"]
    print("k_req_opt_join %.1f %%, k_req_opt_scan %.1f %% of the new call's kernel time" % (100 * out["share_join"], 100 * out["share_scan"]))
    if len(sys.argv) > 1:   # optional: a file for the result tree
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    ctx.close()
print("done")
