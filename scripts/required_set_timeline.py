#!/usr/bin/env python3
"""What a doc set as the only required clause costs (DESIGN.md "Doc sets as the only required clause"): 1024 rows "b c #F" on the
benchmark's 10 M-doc shard through rgpu_search_batch_device_required_set, beside rgpu_search_batch_device_masked on the same rows
and mask (the scored part alone: the baseline), for a filter that holds about half the docs and one that holds 0.1 % of them, at
k = 10 and 100.
  step times   bench.py's procedure: the calls alternate between two streams, a region is 20 steps behind 5 warm-up steps, bracketed
               by device synchronisation; min / median / max of five regions, on a context WITHOUT per-kernel events
  kernel times rgpu_kernel_stats of one call on a context with them: k_required_set_fill, and the head's three launches
  head build   the first call on a fresh set against the second (wall), median of five sets
usage: required_set_timeline.py [out.json]"""
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import indexgen  # noqa: E402

import torch  # noqa: E402

SEED_QUERIES = 0x527563656E65 ^ 0x51
DOCS, VOCAB, NQ = 10_000_000, 1_000_000, 1024
STEPS, WARM, REGIONS = 20, 5, 5
HEAD_KERNELS = ("k_docset_chunk_counts", "k_docset_head_scan", "k_docset_select_head")


def words_of(mask):
    b = np.packbits(mask, bitorder="little")
    return np.concatenate([b, np.zeros((-b.size) % 8, np.uint8)]).view(np.uint64)


def regions(step):
    """-> [min, median, max] ms per step over REGIONS regions of STEPS steps on two streams"""
    per = []
    for _ in range(REGIONS):
        gc.collect()
        gc.disable()
        for i in range(WARM):
            step(i & 1)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(STEPS):
            step(i & 1)
        torch.cuda.synchronize()
        per.append(1e3 * (time.perf_counter() - t) / STEPS)
        gc.enable()
    per.sort()
    return [per[0], per[len(per) // 2], per[-1]]


t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB)
print("built in %.1f s" % (time.time() - t0), flush=True)
T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
ranks = indexgen.log_uniform_ranks(2 * NQ, 1, 1000, SEED_QUERIES ^ 0xF7).reshape(-1, 2) - 1
queries = [B.build([], [T(int(a)), T(int(b))]) for a, b in ranks]
rng = np.random.default_rng(23)
filters = {"half": rng.random(DOCS) < 0.5, "0.1 %": rng.random(DOCS) < 0.001}
out = {"docs": DOCS, "rows": NQ, "steps_per_region": STEPS, "regions": REGIONS, "date": time.strftime("%Y-%m-%d"), "filters": {}}

quiet = rucene_amd.Context()
timed = rucene_amd.Context(profile_kernels=True)
try:
    legs = []
    for c in (quiet, timed):
        leaf = rucene_amd.LeafReader.from_synthetic(seg)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
        legs.append((c, leaf, g, g.pack(queries, leaf)))
    (_, leaf_q, _, (qs, ts)), (_, leaf_t, _, (qs_t, ts_t)) = legs
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for name, mask in filters.items():
        res = {"cardinality": int(mask.sum())}
        w = words_of(mask)
        fset, tset = leaf_q.segment.docset_from_words(w), leaf_t.segment.docset_from_words(w)
        for k in (10, 100):
            rows = [(torch.empty((NQ, k), dtype=torch.int64, device="cuda"), torch.empty((NQ,), dtype=torch.int64, device="cuda")) for _ in range(2)]
            s = leaf_q.segment

            def required(lane, s=s, k=k, rows=rows):
                s.search_batch_device_required_set(fset, qs, ts, k, rows[lane][0].data_ptr(), rows[lane][1].data_ptr(), streams[lane].cuda_stream)

            def masked(lane, s=s, k=k, rows=rows):
                s.search_batch_device_masked(fset, qs, ts, k, rows[lane][0].data_ptr(), rows[lane][1].data_ptr(), streams[lane].cuda_stream)
            leg = {"masked_ms_per_step": regions(masked), "required_set_ms_per_step": regions(required)}
            # one call with per-kernel events: the fill's own time, and what else the call launches
            st = leaf_t.segment
            st.search_batch_required_set(tset, qs_t, ts_t, k)
            per = []
            for _ in range(REGIONS):
                timed.kernel_stats_reset()
                hits, totals = st.search_batch_required_set(tset, qs_t, ts_t, k)
                ks = timed.kernel_stats()
                per.append({n: v["total_ms"] for n, v in ks.items() if v["launches"]})
            leg["k_required_set_fill_ms"] = float(np.median([p.get("k_required_set_fill", 0.0) for p in per]))
            leg["kernels_ms"] = {n: float(np.median([p.get(n, 0.0) for p in per])) for n in sorted({n for p in per for n in p})}
            leg["rows_filled_from_the_head"] = int(((hits["score"] == 0) & (hits["doc"] >= 0)).any(axis=1).sum())
            leg["total_hits_per_row"] = int(totals[0])
            res["k=%d" % k] = leg
            print(name, "k", k, json.dumps(leg), flush=True)
        # the head, built by the first call on a fresh set
        builds = []
        for _ in range(REGIONS):
            d = leaf_t.segment.docset_from_words(w)
            timed.kernel_stats_reset()
            t = time.perf_counter()
            leaf_t.segment.docset_head(d, 100)
            first = 1e3 * (time.perf_counter() - t)
            ks = timed.kernel_stats()
            t = time.perf_counter()
            leaf_t.segment.docset_head(d, 100)
            builds.append((first, 1e3 * (time.perf_counter() - t), {n: ks.get(n, {"total_ms": 0.0})["total_ms"] for n in HEAD_KERNELS}, d.nbytes))
            d.close()
        res["head_build"] = {"first_call_ms": float(np.median([b[0] for b in builds])), "next_call_ms": float(np.median([b[1] for b in builds])),
                             "kernels_ms": {n: float(np.median([b[2][n] for b in builds])) for n in HEAD_KERNELS}, "set_bytes_with_head": int(builds[0][3]),
                             "words_bytes": int((DOCS + 63) // 64 * 8)}
        print(name, "head", json.dumps(res["head_build"]), flush=True)
        out["filters"][name] = res
        fset.close()
        tset.close()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    timed.close()
    quiet.close()
print("done")
