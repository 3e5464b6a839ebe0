"""Kernel times of rgpu_rescore_phrase_batch for 1024 rows x window 100 of two-term phrases (exact, slop 2) on the benchmark's
positions corpus, beside rgpu_search_phrase_batch for the same 1024 phrases: median of five regions, from rgpu_kernel_stats
(DESIGN.md section 4). First pass: the TERM top-100 of each phrase's first term. `python scripts/measure_phrase_rescore.py [out.json]`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import _lib as gpu, indexgen  # noqa: E402

SEED_QUERIES = 0x527563656E65 ^ 0x51
DOCS, VOCAB, NQ, K = 10_000_000, 1_000_000, 1024, 100
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB, positions=True)
print("built in %.1f s" % (time.time() - t0), flush=True)
ctx = rucene_amd.Context(profile_kernels=True)
leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
ranks = indexgen.log_uniform_ranks(2 * NQ, 1, 1000, SEED_QUERIES ^ 0xF2).reshape(-1, 2) - 1
same = ranks[:, 0] == ranks[:, 1]   # a pair that names one term twice: refused at slop > 0; its second term becomes the next rank
print("pairs naming one term twice:", int(same.sum()), flush=True)
ranks = ranks.copy()
ranks[same, 1] += 1
T = rucene_amd.TermQuery
first, _ = g.search_batch([T(int(a)) for a, _ in ranks], K)   # the cheap first pass: TERM top-100 of each phrase's first term
print("first pass rows:", int((first["doc"] >= 0).sum()), "hits", flush=True)
try:
    out = {"docs": DOCS, "rows": NQ, "k": K, "window": K, "date": time.strftime("%Y-%m-%d")}
    for slop in (0, 2):
        queries = [rucene_amd.PhraseQuery([int(a), int(b)], slop=slop) for a, b in ranks]
        qs, ts = g.pack_phrases(queries, leaf)
        req = np.zeros(NQ, dtype=gpu.RESCORE_REQUEST_DTYPE)
        req["query_weight"], req["rescore_weight"], req["mode"], req["window_size"] = 1.0, 1.0, 3, K
        legs = {"rescore": lambda: leaf.segment.rescore_phrase_batch(qs, ts, req, first),
                "search": lambda: leaf.segment.search_phrase_batch(qs, ts, K)}
        for name, call in legs.items():
            for _ in range(2):
                res = call()
            regions, walls = [], []
            for _ in range(5):
                ctx.kernel_stats_reset()
                t = time.perf_counter()
                res = call()
                walls.append(1e3 * (time.perf_counter() - t))
                st = ctx.kernel_stats()
                regions.append({n: v["total_ms"] for n, v in st.items() if v["launches"]})
            names = sorted({n for r in regions for n in r})
            med = {n: float(np.median([r.get(n, 0.0) for r in regions])) for n in names}
            tot = float(np.median([sum(r.values()) for r in regions]))
            out["%s_slop%d" % (name, slop)] = {"kernels_ms_median": med, "kernels_ms_total_median": tot, "wall_ms_median": float(np.median(walls))}
            print(name, "slop", slop, "kernels %.3f ms, wall %.3f ms" % (tot, float(np.median(walls))), med, flush=True)
            if name == "rescore":
                changed = int((res["score"] != first["score"]).sum())
                out["rescore_slop%d" % slop]["hits_matched"] = changed
                print("  hits whose score changed (matches):", changed, flush=True)
    if len(sys.argv) > 1:   # optional: a file for the result tree
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    ctx.close()
print("done")
