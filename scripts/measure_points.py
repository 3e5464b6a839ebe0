"""Point ranges on the benchmark's 10 M-doc shard (DESIGN.md "Point ranges"): the forced value-ordered scatter (path 1) against the
forced doc-ordered scan (path 2) at selectivities 0.001 %, 0.1 %, 1 %, 10 %, 50 % and 100 %, on a dense 4-byte field (one point per
doc) and a sparse 8-byte field (every third doc holds a point) - where the medians meet is the crossover path 0 uses - and the same
ranges through the id route that was the only one before: host-side ids, rgpu_docset_from_docs.
  resident   rgpu_docset_from_point_ranges(path): per launch name the time between HIP events around the launch (rgpu_kernel_stats),
             summed over the call's launches; the wall time of the call, which ends synchronised; 2 warm-up calls, median of 7
  ids        np.flatnonzero over the host's copy of the column - a STAND-IN for the BKD walk of PointRangeQuery::create_scorer, which
             this script cannot run - then rgpu_docset_from_docs of the ids: wall time with and without the stand-in, kernel times
  batch      16 ranges of 1 % in one call under the forced scan (one pass) and under the forced scatter
`python scripts/measure_points.py [--route resident|ids|both] [--package-root DIR] [out.json]`; --package-root measures another build
of the package (the parent commit's, for the id route: it needs nothing this feature adds)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
route, package_root = "both", ROOT
if "--route" in args:
    i = args.index("--route")
    route = args[i + 1]
    del args[i:i + 2]
if "--package-root" in args:
    i = args.index("--package-root")
    package_root = os.path.abspath(args[i + 1])
    del args[i:i + 2]
sys.path.insert(0, package_root)
import rucene_amd  # noqa: E402
from rucene_amd import indexgen  # noqa: E402

DOCS, VOCAB = 10_000_000, 1_000_000
SELECTIVITIES = (0.00001, 0.001, 0.01, 0.1, 0.5, 1.0)
WARM, REPEATS = 2, 7
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB)
print("built in %.1f s" % (time.time() - t0), flush=True)
ctx = rucene_amd.Context(profile_kernels=True)


def be_rows(keys, width):
    """unsigned keys -> their big-endian bytes, [n, width] u8"""
    return np.ascontiguousarray(keys.astype(">u%d" % width)).view(np.uint8).reshape(-1, width)


def measure(call):
    for _ in range(WARM):
        call()
    per, walls = [], []
    for _ in range(REPEATS):
        ctx.kernel_stats_reset()
        t = time.perf_counter()
        call()
        walls.append(1e3 * (time.perf_counter() - t))
        per.append({n: v["total_ms"] for n, v in ctx.kernel_stats().items() if v["launches"] and v["total_ms"] > 0})
    names = sorted({n for r in per for n in r})
    return {"kernels_ms_median": {n: float(np.median([r.get(n, 0.0) for r in per])) for n in names},
            "kernels_ms_total_median": float(np.median([sum(r.values()) for r in per])), "wall_ms_median": float(np.median(walls)),
            "wall_ms_min_max": [float(min(walls)), float(max(walls))]}


try:
    out = {"docs": DOCS, "date": time.strftime("%Y-%m-%d"), "route": route, "warm": WARM, "repeats": REPEATS, "fields": {}}
    s = rucene_amd.Segment(ctx, seg.doc_bytes, seg.norms, seg.max_doc)
    rng = np.random.default_rng(23)
    fields = {"dense 4-byte": (4, np.arange(DOCS, dtype=np.int32), rng.integers(0, 2**32, DOCS, dtype=np.uint64).astype(np.uint32)),
              "sparse 8-byte": (8, np.arange(0, DOCS, 3, dtype=np.int32), rng.integers(0, 2**63, (DOCS + 2) // 3, dtype=np.uint64) * np.uint64(2))}
    for name, (width, docs, keys) in fields.items():
        order = np.sort(keys)
        n = keys.size
        pts = s.attach_points(width, docs, be_rows(keys, width)) if route != "ids" else None
        legs = {}
        for sel in SELECTIVITIES:
            m = max(1, int(round(sel * n)))
            start = 0 if m == n else n // 3
            lo, hi = order[start], order[start + m - 1]
            lo_b, hi_b = be_rows(np.array([lo]), width)[0].tobytes(), be_rows(np.array([hi]), width)[0].tobytes()
            leg = {"matching_points": int(m)}
            if route != "ids":
                for path, label in ((1, "scatter"), (2, "scan")):
                    def build(path=path):
                        (d,) = pts.range_docsets([(lo_b, hi_b)], path)
                        c = d.cardinality
                        d.close()
                        return c
                    leg[label] = measure(build)
                    leg[label]["cardinality"] = build()
                assert leg["scatter"]["cardinality"] == leg["scan"]["cardinality"]
            if route != "resident":
                def by_ids(with_walk=True, cache={}):
                    ids = docs[np.flatnonzero((keys >= lo) & (keys <= hi))] if with_walk or "ids" not in cache else cache["ids"]
                    cache["ids"] = ids
                    d = s.docset_from_docs(ids)
                    c = d.cardinality
                    d.close()
                    return c
                leg["ids with the stand-in walk"] = measure(by_ids)
                leg["ids alone"] = measure(lambda: by_ids(False))
                leg["ids alone"]["cardinality"] = by_ids(False)
            legs["%g %%" % (100 * sel)] = leg
            print(name, "%g %%" % (100 * sel), json.dumps(leg), flush=True)
        if route != "ids":
            m = n // 100
            sixteen = []
            for i in range(16):
                a = (i * (n - m)) // 16
                sixteen.append((be_rows(np.array([order[a]]), width)[0].tobytes(), be_rows(np.array([order[a + m - 1]]), width)[0].tobytes()))
            for path, label in ((1, "scatter"), (2, "scan")):
                def batch(path=path):
                    for d in pts.range_docsets(sixteen, path):
                        d.close()
                legs["16 ranges of 1 %% (%s)" % label] = measure(batch)
                print(name, "16 ranges of 1 %%, %s" % label, json.dumps(legs["16 ranges of 1 %% (%s)" % label]), flush=True)
            info = pts.info()
            legs["column"] = {"n_points": info["n_points"], "hbm_bytes": info["hbm_bytes"], "dense": info["dense"],
                              "scan_bytes": info["n_points"] * (width + (0 if info["dense"] else 4)), "set_bytes": (DOCS + 63) // 64 * 8}
            pts.close()
        out["fields"][name] = legs
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    ctx.close()
print("done")
