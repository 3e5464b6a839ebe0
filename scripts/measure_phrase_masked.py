"""Kernel times and wall time of rgpu_search_phrase_batch_masked for 1024 exact two-term phrases (k = 10) on the benchmark's positions
corpus under doc sets of about 100 %, 10 % and 1 % density (rgpu_docset_from_docs over seeded ids): with the compacting candidate
conjunction (the default), with RGPU_PHRASE_MASK_COMPACT=0 (the marking one), and the unmasked rgpu_search_phrase_batch as the baseline.
Median of five regions after two warm-ups, from rgpu_kernel_stats; the whole round runs twice, the legs alternating, to show the spread
(DESIGN.md section 3.zzzzzzz). The switch is read when a context is created: one context per setting, both over the same corpus.
`python scripts/measure_phrase_masked.py [out.json]`."""
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
SEED_SETS = 0x527563656E65 ^ 0x6D61736B
SWITCH = "RGPU_PHRASE_MASK_COMPACT"
DOCS, VOCAB, NQ, K = 10_000_000, 1_000_000, 1024, 10
DENSITIES = (1.0, 0.1, 0.01)
t0 = time.time()
seg = indexgen.build_zipf(DOCS, VOCAB, positions=True)
print("built in %.1f s" % (time.time() - t0), flush=True)
ranks = indexgen.log_uniform_ranks(3 * NQ, 1, 1000, SEED_QUERIES ^ 0xF3).reshape(-1, 3) - 1
phrases = [rucene_amd.PhraseQuery([int(a), int(b)]) for a, b, _ in ranks]
rng = np.random.default_rng(SEED_SETS)
ids = {d: (np.arange(DOCS, dtype=np.int32) if d == 1.0 else np.sort(rng.choice(DOCS, size=int(DOCS * d), replace=False)).astype(np.int32)) for d in DENSITIES}


class Side:
    """one context (one setting of the switch) with the corpus, the packed batch and the doc sets"""

    def __init__(self, compact):
        os.environ[SWITCH] = "1" if compact else "0"
        self.ctx = rucene_amd.Context(profile_kernels=True)
        self.leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
        self.g = rucene_amd.GpuIndexSearcher([self.leaf], ctx=self.ctx)
        self.qs, self.ts = self.g.pack_phrases(phrases, self.leaf)
        self.sets = {d: self.leaf.segment.docset_from_docs(ids[d]) for d in DENSITIES}

    def measure(self, call):
        for _ in range(2):
            res = call()
        regions, walls = [], []
        for _ in range(5):
            self.ctx.kernel_stats_reset()
            t = time.perf_counter()
            res = call()
            walls.append(1e3 * (time.perf_counter() - t))
            regions.append({n: v["total_ms"] for n, v in self.ctx.kernel_stats().items() if v["launches"]})
        names = sorted({n for r in regions for n in r})
        return res, {"kernels_ms_median": {n: float(np.median([r.get(n, 0.0) for r in regions])) for n in names},
                     "kernels_ms_total_median": float(np.median([sum(r.values()) for r in regions])), "wall_ms_median": float(np.median(walls)),
                     "hits": int(res[1].sum())}

    def masked(self, d):
        return self.measure(lambda: self.leaf.segment.search_phrase_batch_masked(self.sets[d], self.qs, self.ts, K))

    def unmasked(self):
        return self.measure(lambda: self.leaf.segment.search_phrase_batch(self.qs, self.ts, K))

    def close(self):
        for s in self.sets.values():
            s.close()
        self.leaf.segment.close()
        self.ctx.close()


compact, marked = Side(True), Side(False)
try:
    out = {"docs": DOCS, "rows": NQ, "k": K, "date": time.strftime("%Y-%m-%d"), "cardinality": {str(d): int(ids[d].size) for d in DENSITIES}, "rounds": []}
    for rnd in range(2):
        legs = {}
        base_rows, legs["unmasked"] = compact.unmasked()
        print(rnd, "unmasked", "kernels %.3f ms, wall %.3f ms" % (legs["unmasked"]["kernels_ms_total_median"], legs["unmasked"]["wall_ms_median"]), flush=True)
        for d in DENSITIES:
            sides = (("compact", compact), ("marked", marked)) if rnd == 0 else (("marked", marked), ("compact", compact))
            rows = {}
            for name, side in sides:
                rows[name], legs["%s %g" % (name, d)] = side.masked(d)
                m = legs["%s %g" % (name, d)]
                print(rnd, name, d, "kernels %.3f ms, wall %.3f ms, %d hits" % (m["kernels_ms_total_median"], m["wall_ms_median"], m["hits"]), m["kernels_ms_median"], flush=True)
            assert rows["compact"][0].tobytes() == rows["marked"][0].tobytes() and (rows["compact"][1] == rows["marked"][1]).all(), "the switch changes no byte"
            if d == 1.0:
                assert rows["compact"][0].tobytes() == base_rows[0].tobytes() and (rows["compact"][1] == base_rows[1]).all(), "a full mask is the unmasked call"
        out["rounds"].append(legs)
    if len(sys.argv) > 1:   # optional: a file for the result tree
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
finally:
    compact.close()
    marked.close()
print("done")
