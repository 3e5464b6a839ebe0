"""The fused single-term step reading the planner's hot entries instead of its memo (`-m gpu`; host/batch_planner.hpp
for_each_flat_memo_hot, csrc/api/fused.hpp term_batch_resident), and the slot's event bound to the search kernel: every row equals the
oracle's and the rows of a context opened with RGPU_TERM_HOT=0, bit for bit, and `postings_covered` is the sum of the dfs — for
duplicate / absent / outside ids, ids that share a hot slot alternating on two streams, an arena that turns over every other call,
a released prepared store, and 200 enqueue-only calls on two streams under either slot event.

The leaf is tests/test_gpu_term_arena.py's (22 explicit lists, built through its Fixture / Leaf helpers); its term table is repeated
3300 times here instead of 2200, so that ids 65536 apart — one slot of the hot table — both exist."""
import numpy as np
import pytest

from test_gpu_term_arena import KS, Fixture, Leaf, _context, _launches

pytestmark = pytest.mark.gpu

HOT_SLOTS = 1 << 16   # BatchPlanner::HOT_SLOTS: ids this far apart share a hot entry
REPEAT = 3300


class WideFixture(Fixture):
    def __init__(self, oracle):
        super().__init__(oracle)
        self.terms = np.tile(self.seg.terms, REPEAT)
        self.n_ids = self.terms.size
        assert self.n_ids > HOT_SLOTS + 5000

    def df_sum(self, ids):
        ids = np.asarray(ids).reshape(-1)
        inside = ids[(ids >= 0) & (ids < self.n_ids)]
        return int(self.dfs[inside % self.n].sum())


@pytest.fixture(scope="module")
def fx(oracle):
    return WideFixture(oracle)


@pytest.fixture(scope="module")
def memo_rows(fx):
    """(ids, k) -> (rows, totals, postings_covered) of a context that reads the memo's records (RGPU_TERM_HOT=0), each batch asked once"""
    ctx = _context({"RGPU_TERM_HOT": "0"})
    lf = Leaf(fx, ctx)
    seen = {}

    def get(ids, k):
        key = (np.asarray(ids, dtype=np.int64).tobytes(), k)
        if key not in seen:
            lf.call(ids, k, "memo: first")
            rows, totals = lf.call(ids, k, "memo")
            seen[key] = (rows.copy(), totals.copy(), ctx.last_search_counters()["postings_covered"])
        return seen[key]
    yield get
    ctx.close()


def _same(got, want, what):
    rows, totals = got
    assert (rows["doc"] == want[0]["doc"]).all() and (rows["score"].view(np.int32) == want[0]["score"].view(np.int32)).all(), what
    assert (totals == want[1]).all(), what


def _hot_pairs(fx, n_pairs, start=0):
    """(a, b): ids that share a slot of the planner's hot table, both naming terms the leaf holds"""
    pairs = []
    for a in range(start, fx.n_ids - HOT_SLOTS):
        b = a + HOT_SLOTS
        if fx.dfs[a % fx.n] > 0 and fx.dfs[b % fx.n] > 0:
            pairs.append((a, b))
            if len(pairs) == n_pairs:
                return pairs
    raise AssertionError("not enough ids")


def test_duplicates_absent_and_outside_ids(fx, memo_rows):
    ctx = _context()
    try:
        lf = Leaf(fx, ctx)
        rng = np.random.default_rng(41)
        some = rng.integers(0, fx.n_ids, size=120)
        absent = fx.n - 1 + fx.n * np.array([0, 7, 2999])   # the list with df = 0, under three ids
        assert (fx.dfs[absent % fx.n] == 0).all()
        ids = np.concatenate([np.arange(fx.n), some, some[:40], some[:40], absent, [-1, -2**40, fx.n_ids, fx.n_ids + 7, 2**40], absent, [5, 5, 5]])
        for k in KS:
            want = memo_rows(ids, k)
            for rnd in range(3):
                q0 = _launches(ctx, "term_query_launches")
                got = lf.call(ids, k, ("hot", rnd))
                assert _launches(ctx, "term_query_launches") - q0 == 1
                _same(got, want, ("hot against memo", k, rnd))
                covered = ctx.last_search_counters()["postings_covered"]
                assert covered == fx.df_sum(ids) and covered == want[2], (k, rnd, covered)
        assert _launches(ctx, "k_stage_term_plan") == 1   # the records went up once; hits upload nothing
    finally:
        ctx.close()


def test_hot_collisions_alternating_on_two_streams(fx, memo_rows):
    """Two batches whose ids share hot slots pairwise, 50 enqueue-only calls on two streams: every call takes the other batch's hot
    entries; the memo keeps both, so nothing is uploaded after the first two calls."""
    import torch
    ctx = _context()
    try:
        lf = Leaf(fx, ctx)
        pairs = _hot_pairs(fx, 40)
        batches = [np.array([p[0] for p in pairs] + [5, 18, -1]), np.array([p[1] for p in pairs] + [18, fx.n_ids, 5])]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        k = 10
        outs = []
        torch.cuda.synchronize()
        for i in range(50):
            b = i % 2
            out = lf.out(len(batches[b]), k)
            streams[b].wait_stream(torch.cuda.current_stream())   # (the fill of `out` runs on torch's stream)
            lf.enqueue(batches[b], k, out, stream=streams[b].cuda_stream)
            outs.append((i, b, out))
        for s in streams:
            s.synchronize()
        for i, b, out in outs:
            got = lf.read(out)
            fx.assert_rows(*got, batches[b], k, ("hot collisions", i))
            _same(got, memo_rows(batches[b], k), ("hot collisions against memo", i))
        ctx.synchronize()
        assert ctx.last_search_counters()["postings_covered"] == fx.df_sum(batches[1])
        assert _launches(ctx, "term_query_launches") == 50 and _launches(ctx, "k_stage_term_plan") == 2
    finally:
        ctx.close()


def test_arena_turnover_every_other_call(fx, memo_rows):
    """An arena of 32 records and batches of about 20 distinct ids each: a generation fills up every other call, every hot entry goes
    with it (the stamp follows the arena's generation), and launches of the old generation are still in flight."""
    import torch
    ctx = _context({"RGPU_TERM_ARENA_RECORDS": "32"})
    try:
        lf = Leaf(fx, ctx)
        held = [i for i in range(200) if fx.dfs[i % fx.n] > 0]
        batches = [np.array(held[0:20] + [21]), np.array(held[20:40] + held[20:25]), np.array(held[40:60] + [-1]), np.array(held[60:80]),
                   np.array(held[10:30])]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        k = 10
        outs = []
        torch.cuda.synchronize()
        for i in range(30):
            b = (i * 3) % len(batches)
            out = lf.out(len(batches[b]), k)
            streams[i % 2].wait_stream(torch.cuda.current_stream())
            lf.enqueue(batches[b], k, out, stream=streams[i % 2].cuda_stream)
            outs.append((i, b, out))
        for s in streams:
            s.synchronize()
        for i, b, out in outs:
            got = lf.read(out)
            fx.assert_rows(*got, batches[b], k, ("turnover", i, b))
            _same(got, memo_rows(batches[b], k), ("turnover against memo", i))
        ctx.synchronize()
        assert ctx.last_search_counters()["postings_covered"] == fx.df_sum(batches[(29 * 3) % len(batches)])
        st = ctx.kernel_stats()
        assert st["fused_term_batches"]["launches"] == 30 and st["k_stage_term_plan"]["launches"] >= 12
    finally:
        ctx.close()


def test_prepared_store_released_between_calls(fx, memo_rows):
    """rgpu_segment_release_prepared_terms between fused calls: the epoch in the key moves, the hot entries of the old key are
    misses, the call after the release takes the full path and the ones after it upload fresh records."""
    import torch
    ctx = _context()
    try:
        lf = Leaf(fx, ctx)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        ids = np.concatenate([np.arange(fx.n), fx.n * 3 + np.arange(fx.n), [HOT_SLOTS + 4, 4]])
        k = 10
        want = memo_rows(ids, k)
        for rnd in range(2):
            outs = [lf.out(len(ids), k) for _ in range(4)]
            torch.cuda.synchronize()
            for j, out in enumerate(outs):
                lf.enqueue(ids, k, out, stream=streams[j % 2].cuda_stream)
            lf.leaf.segment.release_prepared_terms()
            for j, out in enumerate(outs):
                _same(lf.read(out), want, ("before the release", rnd, j))
            q0 = _launches(ctx, "term_query_launches")
            _same(lf.call(ids, k, ("right after the release: the full path", rnd)), want, ("full path", rnd))
            assert _launches(ctx, "term_query_launches") == q0
            _same(lf.call(ids, k, ("a new generation", rnd)), want, ("new generation", rnd))
            _same(lf.call(ids[::-1].copy(), k, ("its steady state", rnd)), (want[0][::-1], want[1][::-1]), ("steady", rnd))
            assert ctx.last_search_counters()["postings_covered"] == fx.df_sum(ids)
            assert _launches(ctx, "term_query_launches") == q0 + 2
    finally:
        ctx.close()


@pytest.mark.parametrize("slot_event", ["bound", "record"])
def test_200_enqueue_only_calls_on_two_streams(fx, memo_rows, slot_event):
    """No synchronize between 200 calls: each one waits, through its scratch slot's event alone, for the call four steps back —
    under the event bound to the search kernel (the default) and under RGPU_SLOT_EVENT=record (hipEventRecord behind the launch)."""
    import torch
    ctx = _context({"RGPU_SLOT_EVENT": "record"} if slot_event == "record" else {})
    try:
        lf = Leaf(fx, ctx)
        rng = np.random.default_rng(77)
        batches = [np.concatenate([np.arange(fx.n), rng.integers(0, fx.n_ids, size=100), [-1]]), np.concatenate([rng.integers(0, fx.n_ids, size=90), [fx.n_ids + 1], np.arange(fx.n)])]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        k = 10
        spare = [lf.out(len(batches[b]), k) for b in range(2)]
        last = []
        torch.cuda.synchronize()
        for i in range(200):
            b = i % 2
            if i >= 198:
                out = lf.out(len(batches[b]), k)
                streams[b].wait_stream(torch.cuda.current_stream())
                last.append((i, b, out))
            else:
                out = spare[b]
            lf.enqueue(batches[b], k, out, stream=streams[b].cuda_stream)
        ctx.synchronize()   # (must return: every slot's event completes)
        for s in streams:
            s.synchronize()
        for i, b, out in last:
            got = lf.read(out)
            fx.assert_rows(*got, batches[b], k, (slot_event, i))
            _same(got, memo_rows(batches[b], k), (slot_event, "against memo", i))
        assert ctx.last_search_counters()["postings_covered"] == fx.df_sum(batches[1])
        assert _launches(ctx, "term_query_launches") == 200 and _launches(ctx, "fused_term_batches") == 200
    finally:
        ctx.close()
