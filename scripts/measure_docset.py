"""Doc sets on the benchmark's 10 M-doc shard (DESIGN.md "Doc sets"): per leg the median of five regions, per launch name, from
rgpu_kernel_stats, and the wall time of the call.
  collect      rgpu_docset_collect_batch of one dense term, of one 3-term AND and of one 10-term OR: kernel times, the bytes the list
               kernel touches (encoded bytes of the lists + the words it hits) and its GB/s, its atomics per posting (the distinct
               32-bit words of the lists over their postings, computed on the host from the decoded lists)
  masked AND   1024 3-term AND queries masked by a half-dense set, beside the same batch on a twin segment uploaded with the equal
               live docs (the same kernels: the difference is the call overhead) and the unmasked batch; the once-per-set mask
               formation is timed on its own (a segment with deletions)
  masked TERM  1024 single-term queries masked, beside the unmasked batch: the cost of the exhaustive path
`python scripts/measure_docset.py [out.json]`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rucene_amd  # noqa: E402
from rucene_amd import _lib as gpu  # noqa: E402
from rucene_amd import indexgen  # noqa: E402

SEED_QUERIES = 0x527563656E65 ^ 0x51
DOCS, VOCAB, NQ, K = 10_000_000, 1_000_000, 1024, 10
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB)
print("built in %.1f s" % (time.time() - t0), flush=True)
ctx = rucene_amd.Context(profile_kernels=True)
T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery


def words_of(mask):
    b = np.packbits(mask, bitorder="little")
    return np.concatenate([b, np.zeros((-b.size) % 8, np.uint8)]).view(np.uint64)


def measure(call, regions=5, warm=2):
    for _ in range(warm):
        res = call()
    per, walls = [], []
    for _ in range(regions):
        ctx.kernel_stats_reset()
        t = time.perf_counter()
        res = call()
        walls.append(1e3 * (time.perf_counter() - t))
        per.append({n: v["total_ms"] for n, v in ctx.kernel_stats().items() if v["launches"] and v["total_ms"] > 0})
    names = sorted({n for r in per for n in r})
    return res, {"kernels_ms_median": {n: float(np.median([r.get(n, 0.0) for r in per])) for n in names},
                 "kernels_ms_total_median": float(np.median([sum(r.values()) for r in per])), "wall_ms_median": float(np.median(walls)),
                 "wall_ms_min_max": [float(min(walls)), float(max(walls))]}


try:
    out = {"docs": DOCS, "rows": NQ, "k": K, "date": time.strftime("%Y-%m-%d")}
    leaf = rucene_amd.LeafReader.from_synthetic(seg)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    s = leaf.segment
    # ---- collect
    legs = {"dense term": T(0), "3-term AND": B.build([T(3), T(40), T(200)], []), "10-term OR": B.build([], [T(int(t)) for t in range(20, 220, 20)])}
    out["collect"] = {}
    for name, q in legs.items():
        qs, ts = g.pack([q], leaf)

        def fill(qs=qs, ts=ts):
            sets = s.docset_collect_batch(qs, ts)
            n = sets[0].cardinality
            sets[0].close()
            return n
        n, m = measure(fill)
        terms = [int(t["state"]["doc_freq"]) for t in ts]
        m.update(cardinality=int(n), postings=int(sum(terms)))
        if name != "3-term AND":   # the list kernel: bytes and atomics from the lists themselves
            st = np.array([t["state"] for t in ts], dtype=gpu.TERM_STATE_DTYPE)
            docs, _ = s.decode_terms(st)
            at, distinct = 0, 0
            for df in terms:   # one atomic per distinct 32-bit word per 128-posting block
                d = docs[at:at + df]
                blk = np.arange(df) // 128
                distinct += np.unique((blk.astype(np.int64) << 32) | (d >> 5)).size
                at += df
            enc = int(sum(int(t["state"]["skip_offset"]) if t["state"]["doc_freq"] > 128 and t["state"]["skip_offset"] > 0 else 2 * int(t["state"]["doc_freq"]) for t in ts))
            ms = m["kernels_ms_median"].get("k_docset_lists", 0.0)
            m.update(atomics=int(distinct), atomics_per_posting=distinct / max(1, sum(terms)), list_bytes=enc, word_bytes=4 * int(distinct),
                     lists_gb_per_s=(enc + 8 * distinct) / 1e6 / ms if ms else None)   # an atomic reads and writes its word
        out["collect"][name] = m
        print("collect", name, json.dumps(m), flush=True)
    # ---- masked batches
    ranks = indexgen.log_uniform_ranks(3 * NQ, 1, 1000, SEED_QUERIES ^ 0xF3).reshape(-1, 3) - 1
    rng = np.random.default_rng(17)
    half = rng.random(DOCS) < 0.5
    batches = {"and3": [B.build([T(int(a)), T(int(b)), T(int(c))], []) for a, b, c in ranks], "term": [T(int(a)) for a, _, _ in ranks]}
    hset = s.docset_from_words(words_of(half))
    twin = rucene_amd.Segment(ctx, seg.doc_bytes, seg.norms, seg.max_doc, live_docs=words_of(half))
    for name, queries in batches.items():
        qs, ts = g.pack(queries, leaf)
        res_m, masked = measure(lambda: s.search_batch_masked(hset, qs, ts, K))
        res_t, on_twin = measure(lambda: twin.search_batch(qs, ts, K))
        res_u, unmasked = measure(lambda: s.search_batch(qs, ts, K))
        assert res_m[0].tobytes() == res_t[0].tobytes() and (res_m[1] == res_t[1]).all(), "masked rows differ from the twin's"
        out[name] = {"masked": masked, "twin": on_twin, "unmasked": unmasked, "hits_masked": int(res_m[1].sum()), "hits_unmasked": int(res_u[1].sum())}
        print(name, "masked %.3f | twin %.3f | unmasked %.3f ms wall; kernels %.3f | %.3f | %.3f ms" % (
            masked["wall_ms_median"], on_twin["wall_ms_median"], unmasked["wall_ms_median"], masked["kernels_ms_total_median"],
            on_twin["kernels_ms_total_median"], unmasked["kernels_ms_total_median"]), flush=True)
    # ---- mask formation: once per set, on a segment that has deletions
    alive = rng.random(DOCS) < 0.9
    dseg = rucene_amd.Segment(ctx, seg.doc_bytes, seg.norms, seg.max_doc, live_docs=words_of(alive))
    qs, ts = g.pack(batches["and3"][:1], leaf)
    forms = []
    for _ in range(5):
        d = dseg.docset_from_words(words_of(half))
        ctx.kernel_stats_reset()
        t = time.perf_counter()
        dseg.search_batch_masked(d, qs, ts, K)
        first = 1e3 * (time.perf_counter() - t)
        combine = ctx.kernel_stats().get("k_docset_combine", {"total_ms": 0.0})["total_ms"]
        t = time.perf_counter()
        dseg.search_batch_masked(d, qs, ts, K)
        forms.append((first, 1e3 * (time.perf_counter() - t), combine))
        d.close()
    out["mask_formation"] = {"first_call_ms_median": float(np.median([f[0] for f in forms])), "next_call_ms_median": float(np.median([f[1] for f in forms])),
                             "k_docset_combine_ms_median": float(np.median([f[2] for f in forms])), "words_bytes": int((DOCS + 63) // 64 * 8)}
    print("mask formation", json.dumps(out["mask_formation"]), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    ctx.close()
print("done")
