"""Parity at every edge of the bitmap disjunction kernel k_or_lazy (`-m gpu`): it answers every OR of 10 to 16 SHOULD clauses on a
rank-norm leaf without deletions at k <= 128. The fixtures of tests/lazy_spectrum.py put a posting on either side of each threshold
that code branches on: doc_freq 2304 | 2305 (walked | lazy) and 1152 | 1153 (without | with the four-bits-per-doc array), 0, 1, 4, 5,
6, 7 and 8 dense lists in one query, planted freqs of 14 | 15 | 16 and 254 | 255 | 256 | 5000 on docs that walked clauses touch and on
docs that only lazy lists hold, docs held by exactly m of six lazy lists around a threshold inside every bracket of their bounds,
63 .. 129 run entries of one clause in a window at run lanes 7 | 8 | 13 | 15 (a clause's position among the walked ones), 512 | 513
(and 1024 | 1025) touched docs in one 2048-doc step, cell groups that split, every step and window edge through a walked and a lazy list, ties across a window edge,
absent and repeated clauses, and the fixed-point floor.

Everything goes through GpuIndexSearcher.search_batch and the C ABI. Rows are judged under oracle/parity.py's heap-order rule at
rtol 1e-5 against the oracle's rows, hit counts and membership against the numpy set algebra. Where the reference separates the
k-th from the (k + 1)-th score by more than 1e-4 relative the doc-id set must be the oracle's, and every position whose neighbours
are that far away holds the oracle's doc (tests/test_lazy_spectrum_cpu.py proves the fixtures and both references on the CPU).
A query's row is the same bytes alone, three times in a batch, among its family, inside an 8192-row batch (two windows per
wavefront), through the device call, the fused call and with or_deferred, and - on a leaf of 253 windows - through the pilot
launch and the item pre-merge; kernel_stats() says which kernel answered.

Contexts: one module-scoped Context(profile_kernels=True, **knobs) per knob set, created on first use."""
import numpy as np
import pytest

import lazy_spectrum as lz
from lazy_spectrum import Query
from test_gpu_norm_spectrum import _assert_row

pytestmark = pytest.mark.gpu

KNOBS = {"default": {}, "cells1024": dict(or_lazy_cells=1024), "bm256": dict(or_bitmaps=256), "wide": dict(or_bitmaps=-1),
         "wide2048": dict(or_bitmaps=-1, or_wide_window_docs=2048), "deferred": dict(or_deferred=True)}
COMBOS = [(name, version) for version in lz.VERSIONS for name in ("default", "cells1024", "bm256", "wide", "wide2048")]
FIXED_POINT = ("k_or_lazy", "k_or_wide")


@pytest.fixture(scope="module")
def ctxs():
    import rucene_amd
    made = {}

    def get(name):
        if name not in made:
            made[name] = rucene_amd.Context(profile_kernels=True, **KNOBS[name])
        return made[name]
    yield get
    for c in made.values():
        c.close()
    _refs.clear()    # (the oracle's searchers go before the interpreter does)
    _rows.clear()


_refs, _rows = {}, {}


def _ref(oracle, fx):
    if fx.key not in _refs:
        _refs[fx.key] = lz.LazyRef(oracle, fx)
    return _refs[fx.key]


def _want(oracle, fx, queries, k):
    """The oracle's rows, computed once per (leaf, query, k) and shared by every test."""
    missing = [q for q in dict.fromkeys(queries) if (fx.key, q, k) not in _rows]
    if missing:
        for q, row in zip(missing, lz.oracle_rows(oracle, _ref(oracle, fx).osr, missing, k)):
            for a in row[:2]:
                a.setflags(write=False)
            _rows[(fx.key, q, k)] = row
    return [_rows[(fx.key, q, k)] for q in queries]


def _gpu_leaf(fx):
    import rucene_amd
    return rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, doc_base=0, live_docs=fx.live_docs, sum_total_term_freq=fx.sttf)


def _gpu_query(q):
    import rucene_amd
    T = rucene_amd.TermQuery
    if len(q.must) == 1 and not (q.should or q.must_not):
        return T(q.must[0])
    return rucene_amd.BooleanQuery.build([T(t) for t in q.must], [T(t) for t in q.should], must_nots=[T(t) for t in q.must_not], min_should_match=q.msm)


def _search(g, queries, k):
    hits, totals = g.search_batch([_gpu_query(q) for q in queries], k)
    assert hits.shape == (len(queries), k) and len(totals) == len(queries)
    return hits, totals


def _check(oracle, fx, queries, hits, totals, k, what, sharp=True):
    """Each row under the heap-order rule against the oracle's; total_hits and membership against the set algebra; where the
    reference's scores are further than 1e-4 apart, the oracle's docs themselves."""
    from oracle import parity
    ref = _ref(oracle, fx)
    for i, (q, (d, s, total)) in enumerate(zip(queries, _want(oracle, fx, queries, k))):
        docs = lz.ref_docs(fx, q)
        differing = parity.check_heap_order_row(ref.osr, oracle.OP_OR, list(q.should), hits[i]["doc"], hits[i]["score"], totals[i], d, s, d.size, total,
                                                rtol=1e-5, min_should_match=q.msm, what="%s k %d %s" % (what, k, q.should))
        assert totals[i] == docs.size and np.isin(hits[i]["doc"][:d.size], docs).all(), (what, k, i, q, "against the set algebra")
        # the rule lets a row name other members of the k-th band, and nothing below it: the last returned score is the k-th best
        # total under another rounding (each within 1e-5 of the exact sum, so within 2e-5 of each other)
        if d.size:
            assert float(hits[i]["score"][d.size - 1]) >= float(s[-1]) * (1.0 - 2e-5), (what, k, i, q, "a returned doc from below the k-th band")
        if not sharp:
            continue
        if ref.is_sharp(q, k):
            assert differing == 0, (what, k, i, q, "the doc-id set where the k-th score stands clear of the next")
        at = ref.separated(q, k)
        assert (hits[i]["doc"][at] == d[at]).all(), (what, k, i, q, "positions whose neighbours are further than 1e-4 away", at[hits[i]["doc"][at] != d[at]])


def _same_rows(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.asarray(a[1]).tolist() == np.asarray(b[1]).tolist()


def _stat(c, *names):
    st = c.kernel_stats()
    return [st[n]["launches"] if n in st else 0 for n in names]


class _Searcher:
    """A GPU leaf over a fixture leaf and its searcher, closed on the way out."""

    def __init__(self, fx, ctx):
        import rucene_amd
        self.leaf = _gpu_leaf(fx)
        self.g = rucene_amd.GpuIndexSearcher([self.leaf], ctx=ctx)

    def __enter__(self):
        return self.g

    def __exit__(self, *exc):
        self.leaf.segment.close()


# ---- parity, knob set by knob set ---------------------------------------------------------------------------------------------------
PARTS = list(lz.FAMILIES) + ["ladder brackets", "ties", "bail pairs and floor"]


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("knobs,version", COMBOS, ids=["%s-v%d" % c for c in COMBOS])
def test_families(ctxs, oracle, knobs, version, part):
    """Every family in a batch of its own at k in 1, 10, 64, 65, 100, 128; the ladder at the k of each bracket; the ties; the bail
    pairs and the floor query as plain rows."""
    fx = lz.Leaf(version=version)
    with _Searcher(fx, ctxs(knobs)) as g:
        if part in lz.FAMILIES:
            for k in lz.KS:
                _check(oracle, fx, lz.FAMILIES[part], *_search(g, lz.FAMILIES[part], k), k, (knobs, version, part))
        elif part == "ladder brackets":
            for k in sorted(lz.ladder_ks(_ref(oracle, fx)).values()):
                _check(oracle, fx, lz.FAMILIES["ladder"], *_search(g, lz.FAMILIES["ladder"], k), k, (knobs, version, part))
        elif part == "ties":
            for k in lz.TIE_KS:
                hits, _ = _search(g, lz.FAMILIES["tie"], k)
                for row in hits:   # equal fixed-point totals: exactly the smallest doc ids, ascending
                    assert row["doc"].tolist() == list(range(lz.CONST_LO, lz.CONST_LO + k)) and np.unique(row["score"].view(np.int32)).size == 1, (knobs, k)
        else:
            extra = [lz.FLOOR_Q] + [q for pair in lz.BAIL_Q.values() for q in pair]
            for k in (10, 128) + tuple(lz.FLOOR_K.values()):
                _check(oracle, fx, extra, *_search(g, extra, k), k, (knobs, version, part))


@pytest.mark.parametrize("where", ["touched", "lazy"])
@pytest.mark.parametrize("knobs", ["default", "bm256", "wide"])
def test_planted_freqs_come_back(ctxs, oracle, knobs, where):
    """Every planted freq - 14 | 15 | 16 around the nibble's 15, 254 | 255 | 256 | 5000 around the clamped byte - on a doc that a
    walked clause touches / that only lazy lists hold: the doc is in the row, at the reference's score."""
    fx = lz.Leaf()
    ref = _ref(oracle, fx)
    with _Searcher(fx, ctxs(knobs)) as g:
        hits, _ = _search(g, list(lz.FREQS_Q.values()), 64)
        for row, (name, q) in zip(hits, lz.FREQS_Q.items()):
            docs, sc = ref.scores(q)
            for f in lz.PLANTED_FREQS:
                doc = fx.built.freq_docs[(f, where)]
                at = np.flatnonzero(row["doc"] == doc)
                assert at.size == 1, (knobs, name, f, where, "missing")
                want = sc[np.searchsorted(docs, doc)]
                assert abs(float(row["score"][at[0]]) - want) <= 1e-5 * want, (knobs, name, f, where, float(row["score"][at[0]]), want)


@pytest.mark.parametrize("max_doc", lz.SMALL)
@pytest.mark.parametrize("knobs", ["default", "wide"])
def test_small_leaves(ctxs, oracle, knobs, max_doc):
    """One step, one whole window, one window and a doc: the lists that fit."""
    fx = lz.Leaf(max_doc)
    queries = lz.small_queries(fx)
    c = ctxs(knobs)
    with _Searcher(fx, c) as g:
        c.kernel_stats_reset()
        for k in (1, 10, 128):
            _check(oracle, fx, queries, *_search(g, queries, k), k, (knobs, max_doc))
        lazy, wide = _stat(c, *FIXED_POINT)
        assert (lazy > 0) if knobs == "default" else (lazy == 0 and wide > 0)


# ---- which kernel answered ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", ["default", "cells1024", "bm256", "wide", "wide2048"])
def test_each_family_runs_the_kernel_its_context_names(ctxs, oracle, knobs):
    c = ctxs(knobs)
    fx = lz.Leaf()
    with _Searcher(fx, c) as g:
        for name, fam in lz.FAMILIES.items():
            c.kernel_stats_reset()
            _search(g, fam, 10)
            lazy, wide, windows, bailed = _stat(c, "k_or_lazy", "k_or_wide", "k_or_windows", "or_lazy_bail_queries")
            if knobs.startswith("wide"):
                assert lazy == 0 and wide > 0 and windows == 0, (name, lazy, wide, windows)
            else:
                assert lazy > 0 and windows == 0 and (wide > 0) == (bailed > 0), (name, lazy, wide, windows, bailed)
                if knobs != "bm256":    # nothing of these families is too dense for its cells (under or_bitmaps = 256 fewer lists are walked still)
                    assert bailed == 0, (name, bailed)


@pytest.mark.parametrize("what", ["deleted doc", "raw norms", "k 129", "must_not", "min_should_match 2"])
def test_what_the_fixed_point_kernels_do_not_take(ctxs, oracle, what):
    """A leaf with a deleted doc or raw norms, k = 129, a MUST_NOT clause, min_should_match 2: neither k_or_lazy nor k_or_wide."""
    c = ctxs("default")
    fx = lz.Leaf(live="one") if what == "deleted doc" else lz.Leaf(raw=True) if what == "raw norms" else lz.Leaf()
    queries = lz.FAMILIES["dense"][:7]
    if what == "must_not":
        queries = [Query(should=q.should, must_not=(lz.EDGE_W,)) for q in queries]
    if what == "min_should_match 2":
        queries = [Query(should=q.should, msm=2) for q in queries]
    k = 129 if what == "k 129" else 10
    with _Searcher(fx, c) as g:
        c.kernel_stats_reset()
        hits, totals = _search(g, queries, k)
        lazy, wide, windows = _stat(c, "k_or_lazy", "k_or_wide", "k_or_windows")
        assert lazy == 0 and wide == 0 and windows > 0, (what, lazy, wide, windows)
        for i, q in enumerate(queries):
            assert totals[i] == lz.ref_docs(fx, q).size, (what, q)
        if what in ("deleted doc", "raw norms", "k 129"):
            _check(oracle, fx, queries, hits, totals, k, what, sharp=what != "raw norms")
        if what == "min_should_match 2":    # the reference sums these in clause order: bit for bit
            for i, want in enumerate(_want(oracle, fx, queries, k)):
                _assert_row(hits[i], totals[i], want, (what, queries[i]))


@pytest.mark.parametrize("knobs,or_bitmaps", [("default", 0), ("bm256", 256)])
def test_bitmaps_are_built_for_the_lists_above_the_bound(ctxs, knobs, or_bitmaps):
    fx = lz.Leaf()
    import rucene_amd
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(knobs))
    try:
        seen = []
        for name in ("bounds", "dense", "freqs", "edge"):
            seen += lz.FAMILIES[name]
            _search(g, lz.FAMILIES[name], 10)
            assert leaf.segment.footprint()["doc_bitmap_terms"] == len(fx.bitmap_terms(seen, or_bitmaps)), (knobs, name)
        assert len(fx.bitmap_terms(lz.FAMILIES["bounds"], or_bitmaps)) == (1 if or_bitmaps == 0 else 4)
    finally:
        leaf.segment.close()


def test_bail_outs_are_counted_one_by_one(ctxs, oracle):
    """512 | 513 touched docs in one 2048-doc step under 512 cells, 1024 | 1025 under 1024: the first stays in k_or_lazy, the second
    is answered by k_or_wide, and or_lazy_bail_queries rises by exactly one."""
    fx = lz.Leaf()
    for knobs, cells in (("default", 512), ("cells1024", 1024)):
        c = ctxs(knobs)
        with _Searcher(fx, c) as g:
            pairs = [lz.BAIL_Q[cells]] + ([lz.BAIL_Q[512]] if cells == 1024 else [])
            for n, (fits, bails) in enumerate(pairs):
                for k in (10, 128):
                    c.kernel_stats_reset()
                    got = _search(g, [fits], k)
                    lazy, wide, bailed = _stat(c, "k_or_lazy", "k_or_wide", "or_lazy_bail_queries")
                    assert lazy > 0 and wide == 0 and bailed == 0, (knobs, k, lazy, wide, bailed)
                    _check(oracle, fx, [fits], *got, k, (knobs, "fits"))
                    c.kernel_stats_reset()
                    got = _search(g, [bails], k)
                    lazy, wide, bailed = _stat(c, "k_or_lazy", "k_or_wide", "or_lazy_bail_queries")
                    if n == 0:
                        assert lazy > 0 and wide > 0 and bailed == 1, (knobs, k, lazy, wide, bailed)
                    else:            # 513 docs fit 1024 cells
                        assert lazy > 0 and wide == 0 and bailed == 0, (knobs, k, lazy, wide, bailed)
                    _check(oracle, fx, [bails], *got, k, (knobs, "bails"))
            # next to queries that stay: one more bail, the others' rows unchanged
            batch = [lz.LADDER_Q, pairs[0][1], lz.FAMILIES["dense"][4], pairs[0][0]]
            alone = [_search(g, [q], 10) for q in batch]
            c.kernel_stats_reset()
            hits, totals = _search(g, batch, 10)
            assert _stat(c, "or_lazy_bail_queries") == [1]
            for i in range(len(batch)):
                assert _same_rows((hits[i:i + 1], totals[i:i + 1]), alone[i]), (knobs, i)


@pytest.mark.parametrize("knobs", ["default", "wide"])
def test_the_fixed_point_floor(ctxs, oracle, knobs):
    """Twelve rare docs far above n * 2^17 fixed-point steps: the row stands. One more row reaches a doc that holds the every-doc
    list alone, far below them: the query is summed again in f32 and or_wide_redo_queries rises by one."""
    c = ctxs(knobs)
    fx = lz.Leaf()
    with _Searcher(fx, c) as g:
        for side, redo in (("hi", 0), ("lo", 1)):
            k = lz.FLOOR_K[side]
            c.kernel_stats_reset()
            got = _search(g, [lz.FLOOR_Q], k)
            assert _stat(c, "or_wide_redo_queries") == [redo] and sum(_stat(c, *FIXED_POINT)) > 0, (knobs, side)
            assert (_stat(c, "k_or_windows")[0] > 0) == bool(redo)
            _check(oracle, fx, [lz.FLOOR_Q], *got, k, (knobs, "floor", side))


def test_docs_that_lazy_lists_alone_hold_are_evaluated(ctxs, oracle):
    c = ctxs("default")
    fx = lz.Leaf()
    with _Searcher(fx, c) as g:
        for q in lz.FAMILIES["ladder"] + [lz.FREQS_Q["nibble"], lz.EDGE_Q["lazy"]]:
            c.kernel_stats_reset()
            _search(g, [q], 64)
            assert _stat(c, "or_lazy_only_docs")[0] > 0 and _stat(c, "or_lazy_evaluated_docs")[0] > 0, q


# ---- independence of the plan -------------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_batch(ctxs, oracle):
    """Alone, three copies in one batch, among its family: the same bytes (integer totals are order-free, nothing is approximated)."""
    fx = lz.Leaf()
    with _Searcher(fx, ctxs("default")) as g:
        for k in (10, 128):
            for name, fam in lz.FAMILIES.items():
                hits, totals = _search(g, fam, k)
                for i, q in enumerate(fam):
                    alone = _search(g, [q], k)
                    assert _same_rows(alone, (hits[i:i + 1], totals[i:i + 1])), (k, name, i, "alone against its family")
                    h3, t3 = _search(g, [q, q, q], k)
                    for j in range(3):
                        assert _same_rows(alone, (h3[j:j + 1], t3[j:j + 1])), (k, name, i, j, "three copies")


def test_two_windows_per_wavefront(ctxs, oracle):
    """8192 rows (eight distinct queries, over and over) in one call: 65536 / 8192 = 8 items per query, so two windows share a
    wavefront. The rows are those of the queries run alone."""
    fx = lz.Leaf()
    assert -(-65536 // 8192) == 8 < -(-fx.max_doc // lz.WINDOW) == 10
    k = 10
    with _Searcher(fx, ctxs("default")) as g:
        alone = [_search(g, [q], k) for q in lz.EIGHT]
        _check(oracle, fx, lz.EIGHT, np.concatenate([a[0] for a in alone]), np.concatenate([a[1] for a in alone]), k, "the eight, alone")
        hits, totals = _search(g, lz.EIGHT * 1024, k)
        for i in range(8):
            rows, tots = hits[i::8], totals[i::8]
            assert (tots == alone[i][1][0]).all() and rows.tobytes() == alone[i][0].tobytes() * 1024, (i, "inside the 8192-row batch")


def test_device_call_and_deferred_settling(ctxs, oracle):
    """The two-call device path (rgpu_search_batch_device into device memory), blocking and with or_deferred followed by
    synchronize - batches with a bail-out and with the floor's redo among them: the rows of search_batch."""
    import torch
    from rucene_amd import _lib as gpu
    fx = lz.Leaf()
    k = 10
    batches = [lz.FAMILIES["dense"], lz.FAMILIES["ladder"] + lz.FAMILIES["freqs"], [lz.BAIL_Q[512][1], lz.LADDER_Q, lz.FLOOR_Q, lz.EDGE_Q["both"]]]
    with _Searcher(fx, ctxs("default")) as g:
        want = [_search(g, b, k) for b in batches]
    for knobs in ("default", "deferred"):
        c = ctxs(knobs)
        s = _Searcher(fx, c)
        with s as g:
            outs = [(torch.full((len(b), k), -1, dtype=torch.int64, device="cuda"), torch.full((len(b),), -7, dtype=torch.int64, device="cuda")) for b in batches]
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            for b, (hits, totals) in zip(batches, outs):
                qs, ts = g.pack([_gpu_query(q) for q in b], s.leaf)
                s.leaf.segment.search_batch_device(qs, ts, k, hits.data_ptr(), totals.data_ptr(), stream.cuda_stream)
            c.synchronize()
            torch.cuda.synchronize()
            for b, (hits, totals), w in zip(batches, outs, want):
                got = (hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(len(b), k), totals.cpu().numpy())
                assert _same_rows(got, w), (knobs, b[0])


def test_pilot_launch_and_pre_merge_against_a_plain_plan(ctxs, oracle):
    """The 253-window leaf: alone a query runs as a pilot launch and a second one over 256 one-window items, folded by
    k_premerge_items; among 300 rows as one launch over 128 two-window items. The same bytes, and the oracle's rows."""
    fx = lz.LongLeaf()
    c = ctxs("default")
    names = ("k_or_lazy", "k_premerge_items", "k_or_wide", "k_or_windows")
    with _Searcher(fx, c) as g:
        for k in (10, 128):
            _search(g, lz.LONG_QUERIES, k)    # (the bitmaps are built)
            alone = []
            for q in lz.LONG_QUERIES:
                c.kernel_stats_reset()
                alone.append(_search(g, [q], k))
                assert _stat(c, *names) == [2, 1, 0, 0], (k, q, _stat(c, *names))
            hits, totals = np.concatenate([a[0] for a in alone]), np.concatenate([a[1] for a in alone])
            _check(oracle, fx, lz.LONG_QUERIES, hits, totals, k, "long leaf, alone")
            c.kernel_stats_reset()
            many = _search(g, lz.LONG_QUERIES * (lz.LONG_BATCH // len(lz.LONG_QUERIES)), k)
            assert _stat(c, *names) == [1, 0, 0, 0], (k, _stat(c, *names))
            n = len(lz.LONG_QUERIES)
            for lo in range(0, lz.LONG_BATCH, n):
                assert _same_rows((many[0][lo:lo + n], many[1][lo:lo + n]), (hits, totals)), (k, lo)


def _fused(g, leaf, queries, k):
    """A uniform OR batch through the one-call path (rgpu_planner_search_uniform_ids_device) into device memory."""
    import torch
    from rucene_amd import _lib as gpu
    ids = np.asarray([q.should for q in queries], dtype=np.int64)
    hits = torch.full(ids.shape[:1] + (k,), -3, dtype=torch.int64, device="cuda")
    totals = torch.full(ids.shape[:1], -3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.search_uniform_device(gpu.OP_OR, ids, leaf, k, hits.data_ptr(), totals.data_ptr())
    g.ctx.synchronize()
    return hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(ids.shape[0], k), totals.cpu().numpy()


@pytest.mark.parametrize("knobs", ["default", "deferred", "wide"])
def test_the_fused_call(ctxs, oracle, knobs):
    """Planning and search behind one C-ABI call: every ten-clause query of the families, a bail-out and the floor's redo among
    them, in one uniform batch and one by one - the rows of search_batch, byte for byte."""
    fx = lz.Leaf()
    queries = lz.UNIFORM_TEN
    assert len(queries) >= 40 and lz.BAIL_Q[512][1] in queries and lz.LADDER_Q in queries and set(lz.FREQS_Q.values()) <= set(queries)
    with _Searcher(fx, ctxs("default" if knobs == "deferred" else knobs)) as g:
        want = {k: _search(g, queries, k) for k in (10, 128)}
    c = ctxs(knobs)
    s = _Searcher(fx, c)
    with s as g:
        for k in (10, 128):
            c.kernel_stats_reset()
            assert _same_rows(_fused(g, s.leaf, queries, k), want[k]), (knobs, k, "one uniform batch")
            lazy, wide, bailed = _stat(c, "k_or_lazy", "k_or_wide", "or_lazy_bail_queries")
            assert (lazy > 0 and wide > 0 and bailed == 1) if knobs != "wide" else (lazy == 0 and wide > 0), (knobs, k, lazy, wide, bailed)
        for i, q in enumerate(queries):
            assert _same_rows(_fused(g, s.leaf, [q], 10), (want[10][0][i:i + 1], want[10][1][i:i + 1])), (knobs, i, q)


def test_the_fused_call_on_the_long_leaf(ctxs, oracle):
    """... and a query alone on the 253-window leaf: pilot launch and pre-merge behind the fused call, the row of search_batch."""
    fx = lz.LongLeaf()
    c = ctxs("default")
    queries = [q for q in lz.LONG_QUERIES if len(q.should) == 10]
    assert len(queries) == 3
    s = _Searcher(fx, c)
    with s as g:
        for k in (10, 128):
            want = _search(g, queries, k)
            _check(oracle, fx, queries, *want, k, "long leaf, search_batch")
            for i, q in enumerate(queries):
                c.kernel_stats_reset()
                got = _fused(g, s.leaf, [q], k)
                assert _stat(c, "k_or_lazy", "k_premerge_items") == [2, 1], (k, q)
                assert _same_rows(got, (want[0][i:i + 1], want[1][i:i + 1])), (k, q)
            assert _same_rows(_fused(g, s.leaf, queries * 100, k), (np.concatenate([want[0]] * 100), np.concatenate([want[1]] * 100))), k


# ---- next to other operators --------------------------------------------------------------------------------------------------------
def test_mixed_batches(ctxs, oracle):
    """Ten-clause rows next to TERM, AND and three-clause OR rows in one batch: every row as in a batch of its kind."""
    fx = lz.Leaf()
    others = [Query(must=(lz.D3,)), Query(must=(lz.D0, lz.D5)), Query(should=(lz.D6, lz.EDGE_W, lz.FREQS)), Query(must=(lz.LAST_DOC,)),
              Query(must=(lz.FREQS, lz.EDGE_LZ, lz.TIE_LZ)), Query(should=(lz.STRETCH_513, lz.CONST, lz.ABSENT))]
    ten = lz.FAMILIES["dense"][:6] + [lz.LADDER_Q, lz.FREQS_Q["nibble"], lz.EDGE_Q["both"], lz.BAIL_Q[512][1], lz.TIE_Q["both"], lz.FAMILIES["split"][2]]
    batch, rows = [], {"ten": [], "others": []}
    for i, q in enumerate(ten):
        rows["ten"].append(len(batch))
        batch.append(q)
        rows["others"].append(len(batch))
        batch.append(others[i % len(others)])
    for knobs in ("default", "wide"):
        with _Searcher(fx, ctxs(knobs)) as g:
            for k in (10, 100):
                apart = _search(g, ten, k)
                hits, totals = _search(g, batch, k)
                assert _same_rows((hits[rows["ten"]], totals[rows["ten"]]), apart), (knobs, k)
                _check(oracle, fx, ten, hits[rows["ten"]], totals[rows["ten"]], k, (knobs, "mixed"))
                for at in rows["others"]:
                    _assert_row(hits[at], totals[at], _want(oracle, fx, [batch[at]], k)[0], (knobs, k, batch[at]))
