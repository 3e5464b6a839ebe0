"""Step and kernel times of rgpu_search_span_near_batch for 1024 two-clause ordered SpanNearQuerys at slop 2 (k = 10) on the benchmark's
positions corpus, beside rgpu_search_phrase_batch for the sloppy PhraseQuery of the same pairs at slop 2 in the same process (that
path is the yardstick: its code is untouched): two warm-up steps, then the median of five timed regions, kernel times from
rgpu_kernel_stats. The share of candidates the 64-candidate kernel hands on is read from the library's
RGPU_HOST_TIMING line in a forked child, so that the timed process runs without it. `python scripts/measure_span_near.py [out.json]`."""
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import indexgen  # noqa: E402

SEED_QUERIES = 0x527563656E65 ^ 0x51
DOCS, VOCAB, NQ, K, SLOP = int(os.environ.get("DOCS", 10_000_000)), 1_000_000, 1024, 10, 2
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB, positions=True)
print("built in %.1f s" % (time.time() - t0), flush=True)
ranks = indexgen.log_uniform_ranks(2 * NQ, 1, 1000, SEED_QUERIES ^ 0xF2).reshape(-1, 2) - 1   # bench.py's pairs
S, N = rucene_amd.SpanTermQuery, rucene_amd.SpanNearQuery


def opened():
    ctx = rucene_amd.Context(profile_kernels=True)
    leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    spans = g.pack_phrases([N([S(int(a)), S(int(b))], slop=SLOP) for a, b in ranks], leaf)
    phrases = g.pack_phrases([rucene_amd.PhraseQuery([int(a), int(b)], slop=SLOP) for a, b in ranks], leaf)
    return ctx, leaf, spans, phrases


def left_over():
    """(slots handed on, candidate slots of the batch) as the library prints them under RGPU_HOST_TIMING, from a child forked before
    this process touches the GPU"""
    with tempfile.NamedTemporaryFile(mode="r", suffix=".log") as log:
        pid = os.fork()
        if pid == 0:
            code = 1
            try:
                os.environ["RGPU_HOST_TIMING"] = "1"
                os.dup2(os.open(log.name, os.O_WRONLY | os.O_TRUNC), 2)
                ctx, leaf, spans, _ = opened()
                leaf.segment.search_span_near_batch(*spans, K)
                leaf.segment.search_span_near_batch(*spans, K)
                ctx.close()
                code = 0
            finally:
                os._exit(code)
        _, status = os.waitpid(pid, 0)
        if status != 0:
            raise SystemExit("the child that counts the left-over candidates ended with status %d" % status)
        found = re.findall(r"\[phrase\] (\d+) of (\d+) candidate slots left", log.read())
    return (int(found[-1][0]), int(found[-1][1])) if found else (0, 0)


listed, slots = left_over()
print("left over to k_span_near: %d of %d candidate slots" % (listed, slots), flush=True)
ctx, leaf, spans, phrases = opened()
try:
    out = {"docs": DOCS, "queries": NQ, "k": K, "slop": SLOP, "date": time.strftime("%Y-%m-%d"), "left_over_slots": listed, "candidate_slots": slots}
    legs = {"span_near": lambda: leaf.segment.search_span_near_batch(*spans, K), "sloppy_phrase": lambda: leaf.segment.search_phrase_batch(*phrases, K)}
    for name, call in legs.items():
        for _ in range(2):
            hits, totals = call()
        regions, walls = [], []
        for _ in range(5):
            ctx.kernel_stats_reset()
            t = time.perf_counter()
            hits, totals = call()
            walls.append(1e3 * (time.perf_counter() - t))
            regions.append({n: v["total_ms"] for n, v in ctx.kernel_stats().items() if v["launches"]})
        names = sorted({n for r in regions for n in r})
        med = {n: float(np.median([r.get(n, 0.0) for r in regions])) for n in names}
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
