"""The fused single-term call with its term descriptors resident on the device (`-m gpu`; csrc/api/fused.hpp term_batch_resident,
host/term_arena.hpp): a steady state launches no stage kernel; memo entries that evict each other, first touches on the other stream,
a released prepared store and an arena that turns over every few calls — all with launches in flight on two streams — return the
oracle's rows, bit for bit; RGPU_TERM_PLAN=staged and RGPU_TERM_KERNEL=items return the same rows and counters.

The fixture: 22 explicit lists of 1 .. 600 FullBlocks (and a df = 1 term, tail-only terms, an empty list) whose scores tie heavily
(three field lengths, freqs 1..3), in a term table that repeats them 2200 times — ids i and i + 22 * j name the same list, so there
are tens of thousands of distinct ids (memo entries, arena records) over a segment of 200 000 docs."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_DOC = 200_000
BLOCKS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 600]
REPEAT = 2200   # 48 400 ids: ids 46 368 apart share a slot of the planner's memo (Fibonacci hashing: nearer ids never do)
KS = (10, 100)


class Fixture:
    def __init__(self, oracle, version=1):
        from rucene_amd import indexgen
        rng = np.random.default_rng(808)
        lists = []
        for i, nb in enumerate(BLOCKS):
            df = 128 * nb + (0 if i % 3 == 0 else int(rng.integers(1, 128)))
            docs = np.sort(rng.permutation(MAX_DOC)[:df]).astype(np.int32)
            freqs = rng.integers(1, 4, size=df).astype(np.int32)
            freqs[rng.integers(0, df, size=3)] = 9
            lists.append((docs, freqs))
        for df in (1, 77, 0):  # a singleton, a tail-only list, a term the leaf does not hold
            docs = np.sort(rng.permutation(MAX_DOC)[:df]).astype(np.int32)
            lists.append((docs, rng.integers(1, 4, size=df).astype(np.int32)))
        self.norms = rng.choice(np.array([100, 110, 124], dtype=np.uint8), size=MAX_DOC)
        self.seg = indexgen.build_explicit(MAX_DOC, lists, norms=self.norms, version=version)
        self.n = len(lists)
        self.terms = np.tile(self.seg.terms, REPEAT)
        self.n_ids = self.terms.size
        self.sttf = 30 * MAX_DOC
        self.dfs = np.array([l[0].size for l in lists])
        self._oracle = oracle
        self._want = {}

    def want(self, k, live=None, norms=True):
        """The oracle's (docs, score, total) of every list, computed once per (k, variant)."""
        key = (k, live is not None, norms)
        if key not in self._want:
            o = self._oracle
            oseg = o.Segment(self.seg.doc_bytes, self.norms if norms else None, MAX_DOC, self.seg.terms, live_docs=live, sum_total_term_freq=self.sttf)
            osr = o.Searcher([oseg])
            self._want[key] = [osr.search(o.OP_TERM, [t], k, tie_mode=o.TIE_CANONICAL) for t in range(self.n)]
        return self._want[key]

    def assert_rows(self, rows, totals, ids, k, what, **variant):
        want = self.want(k, **variant)
        for j, t in enumerate(np.asarray(ids).reshape(-1)):
            if t < 0 or t >= self.n_ids:
                d, sc, total = np.zeros(0, np.int32), np.zeros(0, np.float32), 0
            else:
                d, sc, total = want[int(t) % self.n]
            assert totals[j] == total, (what, k, j, int(t), int(totals[j]), total)
            assert (rows[j]["doc"][:d.size] == d).all() and (rows[j]["doc"][d.size:] == -1).all(), (what, k, j, int(t))
            assert (rows[j]["score"][:d.size].view(np.int32) == sc.view(np.int32)).all(), (what, k, j, int(t))


@pytest.fixture(scope="module")
def fx(oracle):
    return Fixture(oracle)


def _context(env=None, **cfg):
    import rucene_amd
    env = env or {}
    saved = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        return rucene_amd.Context(profile_kernels=True, **cfg)
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


class Leaf:
    """The fixture's segment under one context, every list prepared (through the two-call path, which also builds the sketches)."""

    def __init__(self, fx, ctx, live=None, norms=True):
        import rucene_amd
        self.fx, self.ctx = fx, ctx
        self.leaf = rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms if norms else None, MAX_DOC, fx.terms, live_docs=live, sum_total_term_freq=fx.sttf)
        self.g = rucene_amd.GpuIndexSearcher([self.leaf], ctx=ctx)
        self.prepare()

    def prepare(self):
        import torch
        from rucene_amd import _lib as gpu
        sel = np.arange(self.fx.n, dtype=np.int64).reshape(-1, 1)
        qs, ts = self.g.pack_uniform(gpu.OP_TERM, sel, self.leaf)
        hits = torch.empty((sel.shape[0], 10), dtype=torch.int64, device="cuda")
        totals = torch.empty((sel.shape[0],), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.leaf.segment.search_batch_device(qs, ts, 10, hits.data_ptr(), totals.data_ptr())
        self.ctx.synchronize()

    def out(self, nq, k):
        import torch
        return torch.full((nq, k), -3, dtype=torch.int64, device="cuda"), torch.full((nq,), -3, dtype=torch.int64, device="cuda")

    def enqueue(self, ids, k, out, stream=0):
        from rucene_amd import _lib as gpu
        sel = np.asarray(ids, dtype=np.int64).reshape(-1, 1)
        self.g.search_uniform_device(gpu.OP_TERM, sel, self.leaf, k, out[0].data_ptr(), out[1].data_ptr(), stream=stream)

    def read(self, out):
        from rucene_amd import _lib as gpu
        nq, k = out[0].shape
        return out[0].cpu().numpy().view(gpu.HIT_DTYPE).reshape(nq, k), out[1].cpu().numpy()

    def call(self, ids, k, what, **variant):
        import torch
        out = self.out(len(ids), k)
        torch.cuda.synchronize()
        self.enqueue(ids, k, out)
        self.ctx.synchronize()
        rows, totals = self.read(out)
        self.fx.assert_rows(rows, totals, ids, k, what, **variant)
        return rows, totals


def _launches(ctx, name):
    st = ctx.kernel_stats()
    return st[name]["launches"] if name in st else 0


def _memo_slot(i):
    return ((int(i) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> 48


def _colliding_pairs(n_ids, n_pairs, held):
    """(a, b): ids that share a slot of the planner's direct-mapped memo (host/batch_planner.hpp), both naming terms the leaf holds"""
    first, pairs = {}, []
    for i in range(n_ids):
        if not held(i):
            continue
        s = _memo_slot(i)
        if s in first:
            pairs.append((first.pop(s), i))
            if len(pairs) == n_pairs:
                break
        else:
            first[s] = i
    assert len(pairs) == n_pairs
    return pairs


def test_steady_state_launches_no_stage_kernel(fx):
    ctx = _context()
    try:
        lf = Leaf(fx, ctx)
        rng = np.random.default_rng(3)
        ids = np.concatenate([np.arange(fx.n), rng.integers(0, fx.n_ids, size=150), [-1, fx.n_ids + 7]])
        for k in KS:
            ids_k = ids  # (the same ids under both k: k does not enter a descriptor, so the second k uploads nothing)
            s0, q0 = _launches(ctx, "k_stage_term_plan"), _launches(ctx, "term_query_launches")
            lf.call(ids_k, k, "first touch")
            first = _launches(ctx, "k_stage_term_plan") - s0
            assert first == (1 if k == KS[0] else 0), first   # the records go up once, with the call that made them
            assert _launches(ctx, "term_query_launches") - q0 == 1
            s1 = _launches(ctx, "k_stage_term_plan")
            for i, batch in enumerate((ids_k, ids_k[::-1].copy(), rng.permutation(ids_k))):
                q1 = _launches(ctx, "term_query_launches")
                lf.call(batch, k, ("steady", i))
                assert _launches(ctx, "term_query_launches") - q1 == 1
            assert _launches(ctx, "k_stage_term_plan") - s1 == 0
        # a batch with a few new ids among the known ones uploads those, once
        more = np.concatenate([ids[:50], fx.n_ids - 1 - np.arange(5)])
        s2 = _launches(ctx, "k_stage_term_plan")
        lf.call(more, 10, "a few new ids")
        lf.call(more, 10, "a few new ids again")
        assert _launches(ctx, "k_stage_term_plan") - s2 == 1
    finally:
        ctx.close()


def test_memo_collisions_with_launches_in_flight(fx):
    """Two batches whose ids share memo slots pairwise alternate on two streams, 200 calls without a synchronize: every call evicts
    the other batch's entries and appends new records, while up to four launches still read the records they named."""
    import torch
    ctx = _context()
    try:
        lf = Leaf(fx, ctx)
        pairs = _colliding_pairs(fx.n_ids, 24, lambda i: fx.dfs[i % fx.n] > 0)
        batches = [np.array([p[0] for p in pairs] + [5, 18]), np.array([p[1] for p in pairs] + [18, 5])]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        k = 10
        spare = [lf.out(len(batches[0]), k) for _ in range(2)]
        checked = []
        torch.cuda.synchronize()
        for i in range(200):
            b, s = i % 2, (i // 2 + i) % 2 if i % 7 == 0 else i % 2   # mostly batch b on stream b; now and then on the other one
            if i % 20 == 19 or i >= 198:
                out = lf.out(len(batches[b]), k)
                streams[s].wait_stream(torch.cuda.current_stream())   # (the fill of `out` runs on torch's stream)
                lf.enqueue(batches[b], k, out, stream=streams[s].cuda_stream)
                if i % 20 == 19:
                    streams[s].synchronize()
                    fx.assert_rows(*lf.read(out), batches[b], k, ("in flight", i))
                else:
                    checked.append((i, b, out))
            else:
                lf.enqueue(batches[b], k, spare[s], stream=streams[s].cuda_stream)
        for s in streams:
            s.synchronize()
        for i, b, out in checked:
            fx.assert_rows(*lf.read(out), batches[b], k, ("last two", i))
        assert _launches(ctx, "term_query_launches") == 200
    finally:
        ctx.close()


def test_first_touch_on_one_stream_use_on_the_other(fx):
    import torch
    ctx = _context()
    try:
        lf = Leaf(fx, ctx)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for r, k in enumerate(KS):
            ids = fx.n * (10 + r) + np.arange(fx.n)   # never named before
            outs = [lf.out(len(ids), k), lf.out(len(ids), k)]
            torch.cuda.synchronize()
            s0 = _launches(ctx, "k_stage_term_plan")
            lf.enqueue(ids, k, outs[0], stream=streams[0].cuda_stream)
            lf.enqueue(ids, k, outs[1], stream=streams[1].cuda_stream)
            streams[1].synchronize()
            fx.assert_rows(*lf.read(outs[1]), ids, k, "the other stream")
            streams[0].synchronize()
            fx.assert_rows(*lf.read(outs[0]), ids, k, "the uploading stream")
            assert _launches(ctx, "k_stage_term_plan") - s0 == 1
    finally:
        ctx.close()


def test_prepared_store_released_between_calls(fx):
    """rgpu_segment_release_prepared_terms with fused launches still enqueued: the store's epoch moves, the next call prepares its
    terms again through the full path, the ones after it upload fresh records — the same rows throughout."""
    import torch
    ctx = _context()
    try:
        lf = Leaf(fx, ctx)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        ids = np.concatenate([np.arange(fx.n), fx.n * 3 + np.arange(fx.n)])
        k = 10
        for rnd in range(3):
            outs = [lf.out(len(ids), k) for _ in range(4)]
            torch.cuda.synchronize()
            for j, out in enumerate(outs):
                lf.enqueue(ids, k, out, stream=streams[j % 2].cuda_stream)
            lf.leaf.segment.release_prepared_terms()   # (waits for what is in flight, then empties the store)
            for j, out in enumerate(outs):
                fx.assert_rows(*lf.read(out), ids, k, ("before the release", rnd, j))
            q0 = _launches(ctx, "term_query_launches")
            lf.call(ids, k, ("right after the release: the full path", rnd))
            assert _launches(ctx, "term_query_launches") == q0
            lf.call(ids, k, ("a new generation", rnd))
            lf.call(ids[::-1].copy(), k, ("its steady state", rnd))
            assert _launches(ctx, "term_query_launches") == q0 + 2
    finally:
        ctx.close()


def test_arena_turnover_with_launches_in_flight(fx):
    """An arena of 32 records and batches that together name about 100 distinct ids, 50 calls on two streams: a generation fills up
    every other call, and a batch of more distinct ids than the arena holds takes the staged plan."""
    import torch
    ctx = _context({"RGPU_TERM_ARENA_RECORDS": "32"})
    try:
        lf = Leaf(fx, ctx)
        held = [i for i in range(fx.n_ids) if fx.dfs[i % fx.n] > 0]
        batches = [np.array(held[0:20] + [21]), np.array(held[20:45]), np.array(held[40:60] * 2), np.array(held[60:100] + [-1]), np.array(held[95:110])]
        assert len({int(i) for b in batches for i in b}) >= 100 and len(set(batches[3].tolist())) > 32
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        k = 10
        outs = []
        torch.cuda.synchronize()
        for i in range(50):
            b = (i * 3) % len(batches)
            out = lf.out(len(batches[b]), k)
            streams[i % 2].wait_stream(torch.cuda.current_stream())
            lf.enqueue(batches[b], k, out, stream=streams[i % 2].cuda_stream)
            outs.append((i, b, out))
        for s in streams:
            s.synchronize()
        for i, b, out in outs:
            fx.assert_rows(*lf.read(out), batches[b], k, ("turnover", i, b))
        st = ctx.kernel_stats()
        assert st["fused_term_batches"]["launches"] == 50 and st["k_stage_term_plan"]["launches"] >= 20
    finally:
        ctx.close()   # (retired generations still tagged by a slot go here)


def test_staged_plan_items_kernel_and_default_agree(fx):
    got = {}
    rng = np.random.default_rng(9)
    ids = np.concatenate([np.arange(fx.n), rng.integers(0, fx.n_ids, size=100), [-5]])
    for name, env in (("resident", {}), ("staged", {"RGPU_TERM_PLAN": "staged"}), ("items", {"RGPU_TERM_KERNEL": "items"})):
        ctx = _context(env)
        try:
            lf = Leaf(fx, ctx)
            for k in KS:
                lf.call(ids, k, (name, "first"))
                rows, totals = lf.call(ids, k, name)
                got[name, k] = (rows.copy(), totals.copy(), ctx.last_search_counters()["postings_covered"])
            st = ctx.kernel_stats()
            assert (st.get("term_query_launches", {"launches": 0})["launches"] > 0) == (name != "items")
            # the staged plan runs the stage kernel every step, the resident one at first touch only
            assert st["k_stage_term_plan"]["launches"] == (1 if name == "resident" else 4), (name, st["k_stage_term_plan"]["launches"])
        finally:
            ctx.close()
    for k in KS:
        for name in ("staged", "items"):
            a, b = got["resident", k], got[name, k]
            assert (a[0]["doc"] == b[0]["doc"]).all() and (a[0]["score"].view(np.int32) == b[0]["score"].view(np.int32)).all(), (name, k)
            assert (a[1] == b[1]).all() and a[2] == b[2] and a[2] == int(fx.dfs[ids[:-1] % fx.n].sum()), (name, k)


@pytest.mark.parametrize("shape", ["waves 2", "waves 4", "waves 8", "legacy", "deleted docs", "no norms"])
def test_every_kernel_shape_reads_its_record_the_same_way(fx, oracle, shape):
    env, live, norms, f = {}, None, True, fx
    if shape.startswith("waves"):
        env = {"RGPU_TERM_QUERY_WAVES": shape.split()[1]}
    elif shape == "legacy":
        f = Fixture(oracle, version=0)
    elif shape == "deleted docs":
        alive = np.ones(MAX_DOC, bool)
        alive[::7] = False
        live = np.packbits(alive, bitorder="little")
        live = np.concatenate([live, np.zeros((-live.size) % 8, np.uint8)]).view(np.uint64)
    else:
        norms = False
    ctx = _context(env)
    try:
        lf = Leaf(f, ctx, live=live, norms=norms)
        ids = np.concatenate([np.arange(f.n)[::-1], f.n * 7 + np.arange(f.n), [f.n_ids]])
        variant = {"live": live, "norms": norms}
        for k in KS:
            q0 = _launches(ctx, "term_query_launches")
            lf.call(ids, k, (shape, "first"), **variant)
            lf.call(ids, k, (shape, "steady"), **variant)
            assert _launches(ctx, "term_query_launches") - q0 == 2
        assert _launches(ctx, "k_stage_term_plan") == 1
    finally:
        ctx.close()
