"""Hit counts without scoring on the benchmark's 10 M-doc shard (DESIGN.md "Hit counts without scoring"): rgpu_count_batch beside the
call it replaces, rgpu_search_batch with k = 1, in the same process, alternating, the median of five timed regions each (wall time
of the synchronised call, and the kernels' share from rgpu_kernel_stats), with the min-max spread of either side.
  legs     1024 single-term rows, 1024 3-term AND rows, 1024 10-term OR rows (log-uniform term ranks 1..1000, as the benchmark's batches)
  segments without deletions (single-term rows are answered from doc_freq on the host) and with a tenth of the docs deleted
Counts are checked against the search's totals before anything is timed. `python scripts/measure_count.py [out.json]`."""
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
DOCS, VOCAB, NQ = 10_000_000, 1_000_000, 1024
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB)
print("built in %.1f s" % (time.time() - t0), flush=True)
ctx = rucene_amd.Context(profile_kernels=True)
T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery


def words_of(mask):
    b = np.packbits(mask, bitorder="little")
    return np.concatenate([b, np.zeros((-b.size) % 8, np.uint8)]).view(np.uint64)


def region(call):
    ctx.kernel_stats_reset()
    t = time.perf_counter()
    call()
    wall = 1e3 * (time.perf_counter() - t)
    kernels = {n: v["total_ms"] for n, v in ctx.kernel_stats().items() if v["launches"] and v["total_ms"] > 0}
    return wall, kernels


def summary(regions):
    walls = [w for w, _ in regions]
    names = sorted({n for _, k in regions for n in k})
    return {"wall_ms_median": float(np.median(walls)), "wall_ms_min_max": [float(min(walls)), float(max(walls))],
            "kernels_ms_total_median": float(np.median([sum(k.values()) for _, k in regions])),
            "kernels_ms_median": {n: float(np.median([k.get(n, 0.0) for _, k in regions])) for n in names}}


try:
    out = {"docs": DOCS, "rows": NQ, "date": time.strftime("%Y-%m-%d"), "legs": {}}
    leaf = rucene_amd.LeafReader.from_synthetic(seg)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    r3 = indexgen.log_uniform_ranks(3 * NQ, 1, 1000, SEED_QUERIES ^ 0xF3).reshape(-1, 3) - 1
    r10 = indexgen.log_uniform_ranks(10 * NQ, 1, 1000, SEED_QUERIES ^ 0xF4).reshape(-1, 10) - 1
    batches = {"term": [T(int(a)) for a, _, _ in r3], "and3": [B.build([T(int(t)) for t in row], []) for row in r3],
               "or10": [B.build([], [T(int(t)) for t in row]) for row in r10]}
    alive = np.random.default_rng(17).random(DOCS) < 0.9
    segments = {"no deletions": leaf.segment, "a tenth deleted": rucene_amd.Segment(ctx, seg.doc_bytes, seg.norms, seg.max_doc, live_docs=words_of(alive))}
    for seg_name, s in segments.items():
        for name, queries in batches.items():
            qs, ts = g.pack(queries, leaf)
            count, search = (lambda: s.count_batch(qs, ts)), (lambda: s.search_batch(qs, ts, 1))
            for _ in range(2):   # warm: terms prepared, bitmaps built, code objects loaded
                counts, (_, totals) = count(), search()
            assert (counts == totals).all(), "counts differ from the search's totals"
            rc, rs = [], []
            for _ in range(5):   # alternating: the two sides see the same machine
                rc.append(region(count))
                rs.append(region(search))
            m = {"count": summary(rc), "search_k1": summary(rs), "hits": int(counts.sum())}
            lo, hi = m["search_k1"]["wall_ms_min_max"]
            m["faster_beyond_the_baselines_spread"] = bool(m["count"]["wall_ms_median"] < lo)
            out["legs"]["%s, %s" % (name, seg_name)] = m
            print("%-6s %-16s count %.3f ms [%.3f .. %.3f] (kernels %.3f) | search k=1 %.3f ms [%.3f .. %.3f] (kernels %.3f) %s" % (
                name, seg_name, m["count"]["wall_ms_median"], *m["count"]["wall_ms_min_max"], m["count"]["kernels_ms_total_median"],
                m["search_k1"]["wall_ms_median"], lo, hi, m["search_k1"]["kernels_ms_total_median"], json.dumps(m["count"]["kernels_ms_median"])), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    ctx.close()
print("done")
