#!/usr/bin/env python3
"""Timeline of one k_search_term_query launch (the fused single-term step) from a -DRGPU_TERM_TRACE build
(RUCENE_GPU_LIB=build_variants/term_trace.so): one record per workgroup = per query.
usage: term_query_timeline.py [docs]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import rucene_amd  # noqa: E402
from rucene_amd import indexgen, _lib  # noqa: E402

docs = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
seg = indexgen.build_zipf(docs, 1_000_000)
ctx = rucene_amd.Context(profile_kernels=True)
leaf = rucene_amd.LeafReader.from_synthetic(seg)
s = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
tids = bench.build_queries(1024, "term", bench.SEED_QUERIES)
import torch  # noqa: E402
h = torch.empty((1024, 10), dtype=torch.int64, device="cuda")
t = torch.empty((1024,), dtype=torch.int64, device="cuda")
for _ in range(8):
    s.search_uniform_device(_lib.OP_TERM, tids, leaf, 10, h.data_ptr(), t.data_ptr())
    ctx.synchronize()
L = C.CDLL(_lib.lib_path())
# kernels/search_term_query.hpp TermQueryTraceRec: three slots of g_term_trace per workgroup
REC = np.dtype([("t0", "<u8"), ("t1", "<u8"), ("q", "<i4"), ("nblocks", "<i4"), ("rounds", "<i4"), ("entries", "<i4"), ("unpacked", "<i4"),
                ("offers", "<i4"), ("entered", "<i4"), ("d", "<u4", (7,)), ("waves", "<u4"), ("wave0_cycles", "<u4"), ("cyc", "<u4", (8, 3)),
                ("pad", "<u4", (16,))])
assert REC.itemsize == 240
buf = np.zeros(4096, dtype=REC)
n = L.rgpu_debug_trace(C.c_void_p(buf.ctypes.data), C.c_int32(3 * buf.size))
assert n == 3 * buf.size, n
st = ctx.kernel_stats()
ctx.close()
# (one record per workgroup = per query; slots behind them may still hold items of the k_search_term launch that prepared the terms)
rec = buf[:tids.shape[0]]
rec = rec[(rec["t1"] > 0) & (rec["waves"] > 0) & (rec["waves"] <= 8)]
name = [k for k in st if k.startswith("k_search_term_query")]
if name:
    print("%s median %.1f us (HIP events)" % (name[0], 1e3 * st[name[0]]["median_ms"]))
t0 = rec["t0"].min()
start = (rec["t0"] - t0) / 100.0
end = (rec["t1"] - t0) / 100.0
dur = end - start
W = int(rec["waves"][0])
print("%d workgroups of %d waves traced; launch span %.1f us" % (rec.size, W, end.max()))
one = rec["pad"][:, 0] == 1  # (the kernel marks a workgroup that took the one-chunk path)
print("%d workgroups took the one-chunk path (lists of at most RGPU_TERM_SHORT_BLOCKS blocks): mean %.1f us, max %.1f us" % (
    one.sum(), dur[one].mean() if one.any() else 0.0, dur[one].max() if one.any() else 0.0))
print("workgroup duration us: mean %.1f  p50 %.1f  p90 %.1f  p99 %.1f  max %.1f" % (dur.mean(), *np.percentile(dur, [50, 90, 99]), dur.max()))
print("workgroup start us: p50 %.1f  p90 %.1f  max %.1f;  sum of durations %.0f us = %.1f x the span" % (
    *np.percentile(start, [50, 90]), start.max(), dur.sum(), dur.sum() / end.max()))
for frac in (0.25, 0.5, 0.75, 0.9, 1.0):
    tcut = frac * end.max()
    print("  at %3.0f %% of the span (%.1f us): %5d workgroups running, %5d not started" % (100 * frac, tcut, ((start <= tcut) & (end > tcut)).sum(), (start > tcut).sum()))
print("by list length (FullBlocks): workgroups, mean / max duration us, blocks unpacked, offers, keys entered per offer")
for lo, hi in ((0, 0), (1, 15), (16, 63), (64, 4095), (4096, 1 << 30)):
    m = (rec["nblocks"] >= lo) & (rec["nblocks"] <= hi)
    if m.any():
        print("  %5d..%-10d %5d  %5.1f / %5.1f  unpacked %5.1f  offers %5.1f  entered per offer %4.1f  rounds %.2f  queue entries %.1f" % (
            lo, hi, m.sum(), dur[m].mean(), dur[m].max(), rec["unpacked"][m].mean(), rec["offers"][m].mean(),
            rec["entered"][m].sum() / max(1, rec["offers"][m].sum()), rec["rounds"][m].mean(), rec["entries"][m].mean()))
print("the last workgroups to finish:")
for i in np.argsort(-end)[:14]:
    r = rec[i]
    print("   end %.1f  dur %.1f  start %.1f  q %d  blocks %d  rounds %d  queue entries %d  unpacked %d  offers %d  keys entered %d" % (
        end[i], dur[i], start[i], r["q"], r["nblocks"], r["rounds"], r["entries"], r["unpacked"], r["offers"], r["entered"]))

PHASES = ["term descriptor in registers", "score table built", "sketch folded", "first gather", "first sort", "drain (all rounds)", "tail + row"]


def shares(sel, what):
    """each phase's share of the workgroups' wall time, and the lock's / step()'s share of their wave-cycles up to the end of the drain"""
    d = rec["d"][sel].astype(np.float64) / 100.0
    d = np.maximum.accumulate(np.where(d > 0, d, 0), axis=1)  # (a phase a workgroup never reached ends where the one before it did)
    seg_us = np.diff(np.concatenate([np.zeros((d.shape[0], 1)), d], axis=1), axis=1)
    total = dur[sel].sum()
    print("%s (%d workgroups, %.1f us each):" % (what, d.shape[0], dur[sel].mean()))
    for i, p in enumerate(PHASES):
        print("   %-30s %5.1f %% of the time, %6.2f us per workgroup" % (p, 100.0 * seg_us[:, i].sum() / total, seg_us[:, i].mean()))
    cyc = rec["cyc"][sel][:, :W, :].astype(np.float64)
    wave_cycles = W * rec["wave0_cycles"][sel].astype(np.float64)  # what the W waves had between the start and the end of the drain
    wait, hold, rest = (cyc[:, :, j].sum() for j in range(3))
    print("   of %d waves x shader cycles up to the end of the drain: lock wait %.1f %%, lock hold %.1f %% (together %.1f %%), the rest of step() %.1f %%" % (
        W, 100 * wait / wave_cycles.sum(), 100 * hold / wave_cycles.sum(), 100 * (wait + hold) / wave_cycles.sum(), 100 * rest / wave_cycles.sum()))
    offers = max(1, int(rec["offers"][sel].sum()))
    print("   per offer: %.0f cycles waiting, %.0f holding, %.1f keys entered; %.2f offers per unpacked block; ~%.0f shader cycles per us" % (
        wait / offers, hold / offers, rec["entered"][sel].sum() / offers, offers / max(1, int(rec["unpacked"][sel].sum())),
        (rec["wave0_cycles"][sel] / np.maximum(1e-9, rec["d"][sel][:, 5] / 100.0)).mean()))


shares(np.arange(rec.size), "all workgroups")
shares(np.argsort(-dur)[:50], "the 50 longest workgroups")
