"""Kernel times of rgpu_search_phrase_or_batch for 1024 queries "a b" c (all SHOULD, k = 10) on the benchmark's positions corpus,
beside rgpu_search_phrase_batch for the same 1024 phrases alone: median of five regions, per launch name, from rgpu_kernel_stats
(DESIGN.md "BooleanQuery with exact phrase clauses under SHOULD"). The run-building kernels (k_phrase_run_*) stand side by side with
the same batch's k_phrase_match_lanes and k_or_windows. `python scripts/measure_phrase_or.py [out.json]`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import indexgen  # noqa: E402

SEED_QUERIES = 0x527563656E65 ^ 0x51
DOCS, VOCAB, NQ, K = 10_000_000, 1_000_000, 1024, 10
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB, positions=True)
print("built in %.1f s" % (time.time() - t0), flush=True)
ctx = rucene_amd.Context(profile_kernels=True)
leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
ranks = indexgen.log_uniform_ranks(3 * NQ, 1, 1000, SEED_QUERIES ^ 0xF3).reshape(-1, 3) - 1
T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
try:
    out = {"docs": DOCS, "rows": NQ, "k": K, "date": time.strftime("%Y-%m-%d")}
    phrases = [P([int(a), int(b)]) for a, b, _ in ranks]
    packed = g.pack_phrase_or([B.build([], [P([int(a), int(b)]), T(int(c))]) for a, b, c in ranks], leaf)
    qs, ts = g.pack_phrases(phrases, leaf)
    legs = {"phrase_or": lambda: leaf.segment.search_phrase_or_batch(*packed, K), "phrase": lambda: leaf.segment.search_phrase_batch(qs, ts, K)}
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
        med = {n: float(np.median([r.get(n, 0.0) for r in regions])) for n in names}
        tot = float(np.median([sum(r.values()) for r in regions]))
        out[name] = {"kernels_ms_median": med, "kernels_ms_total_median": tot, "wall_ms_median": float(np.median(walls)), "hits": int(res[1].sum())}
        print(name, "kernels %.3f ms, wall %.3f ms, %d hits" % (tot, float(np.median(walls)), int(res[1].sum())), med, flush=True)
    assert (totals["phrase_or"] >= totals["phrase"]).all(), "a SHOULD term can only add hits"
    po = out["phrase_or"]["kernels_ms_median"]
    out["run_building_ms"] = sum(v for n, v in po.items() if n.startswith("k_phrase_run_"))
    print("run building %.3f ms | k_phrase_match_lanes %.3f ms | k_or_windows %.3f ms" % (out["run_building_ms"], po.get("k_phrase_match_lanes", 0.0),
                                                                                          po.get("k_or_windows", 0.0)), flush=True)
    if len(sys.argv) > 1:   # optional: a file for the result tree
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    ctx.close()
print("done")
