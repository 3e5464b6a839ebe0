"""Unordered SpanNearQuery over SpanTermQuery clauses on the device (`-m gpu`): the fixtures of tests/span_unordered.py (proven on the
CPU by tests/test_span_unordered_cpu.py) through rgpu_search_span_unordered_batch against the model composed there - doc ids, hit
counts and score bits equal, nowhere a tolerance.

Every case runs in a batch of its own and the kernel statistics of that batch say which rung answered: k_span_unordered_lanes alone |
left over to k_span_unordered | its wide pool | (legacy) one candidate per wavefront | refused with the documented status, an
ordinary batch answering right behind it. No ordered-span, exact or sloppy launch appears. Then every non-refused case of a segment
in one mixed batch, with the redo list capped too; deleted docs; k on both sides of the hit count and of 128; 8193 candidates with
the first match at index 0 and at 8192; next_limit at SLOP 0; rank, raw and no norms; `.doc` versions 1 and 0; boost 0; the
refusals; the ordered call beside it (still refusing in_order = false, still the ordered model's rows); four leaves through the
Python mirror, the flag off reaching a cpu_fallback stub; the C++ mirror's demo. The launches of every batch are printed (`-s`)."""
import os
import subprocess

import numpy as np
import pytest

import phrase_spectrum as ps
import span_near as sn
import span_unordered as su
from test_gpu_norm_spectrum import _assert_row

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEGMENTS = [("walk", 1), ("ties", 1), ("pool", 1), ("terms", 1), ("place", 1), ("walk", 0), ("ties", 0), ("pool", 0), ("place", 0)]
IDS = ["%s-%s" % (n, "bp128" if v else "legacy") for n, v in SEGMENTS]
FOREIGN = sn.NAMES + ps.EXACT_NAMES + ps.SLOPPY_NAMES   # launches of the ordered span, exact and sloppy phrase rungs


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


def _open(oracle, fx, version=1, live_docs=None, norms=True):
    ix = fx.index(oracle, version)
    return ix, ps.leaf_of(ix, len(fx.postings), fx.norms if norms else None, fx.max_doc, fx.doc_count, fx.sum_ttf, live_docs=live_docs)


def _abi_limit(next_limit):
    return -1 if next_limit is None else (su.NEXT_LIMIT_ZERO if next_limit == 0 else int(next_limit))


def _pack(g, leaf, queries, next_limit=None, boost=1.0):
    import rucene_amd
    S, N = rucene_amd.SpanTermQuery, rucene_amd.SpanNearQuery
    qs, ts = g.pack_phrases([N([S(t) for t in q.terms], slop=q.slop, in_order=False, boost=boost) for q in queries], leaf)
    qs["next_limit"] = _abi_limit(next_limit)
    return qs, ts


def _search(ctx, g, leaf, queries, k, next_limit=None, boost=1.0):
    """One rgpu_search_span_unordered_batch -> (hits, totals, {launch name: launches} of this call)."""
    qs, ts = _pack(g, leaf, queries, next_limit, boost)
    ctx.kernel_stats_reset()
    hits, totals = leaf.segment.search_span_unordered_batch(qs, ts, k)
    return hits, totals, {n: v["launches"] for n, v in ctx.kernel_stats().items() if v["launches"]}


def _same(a, b):
    return (a[1] == b[1]).all() and (a[0]["doc"] == b[0]["doc"]).all() and (a[0]["score"].view(np.int32) == b[0]["score"].view(np.int32)).all()


@pytest.mark.parametrize("name,version", SEGMENTS, ids=IDS)
def test_every_case_alone(ctx, oracle, name, version):
    """Each query of each case in a batch of its own: the model's row, the designed doc a hit iff its hand-written width list is not
    empty, and the launches its rung promises. A refused query raises RgpuError with the documented status and leaves the context
    able to answer."""
    import rucene_amd
    fx = su.segment(name)
    ix, leaf = _open(oracle, fx, version)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        good = next(q for c in fx.cases for q in c.queries if q.error is None and c.designed is not None)
        for c in fx.cases:
            for q in c.queries:
                what = (name, version, c.name, "slop", q.slop)
                want = su.search_case(fx, q, 10)
                if q.error is not None:
                    with pytest.raises(rucene_amd.RgpuError) as e:
                        _search(ctx, g, leaf, [q], 10)
                    assert e.value.status == q.error, (what, e.value.status)
                    print(c.name, "slop", q.slop, "refused with status", e.value.status)
                    hits, totals, st = _search(ctx, g, leaf, [good], 10)   # an ordinary error return: the context goes on answering
                    _assert_row(hits[0], totals[0], su.search_case(fx, good, 10), (what, "the batch behind the refusal"))
                    continue
                hits, totals, st = _search(ctx, g, leaf, [q], 10)
                print(c.name, "slop", q.slop, q.level, st)
                _assert_row(hits[0], totals[0], want, what)
                if c.designed is None:   # a term the leaf lacks: nothing matches, nothing is launched for the row
                    assert totals[0] == 0 and not any(n in st for n in su.NAMES + (su.CANDIDATES,)), (what, st)
                    continue
                everything = su.search_case(fx, q, 1000)[0].tolist()
                assert want[2] >= 1 and (c.ordinary in everything or c.rung == "singleton"), what
                if q.widths is not None:   # the designed doc is a hit iff the hand-written list holds a span
                    assert (c.designed in everything) == bool(q.widths), what
                for launch, wanted in su.launches(q, legacy=version == 0).items():
                    assert (launch in st) == wanted, (what, q.level, launch, "launched" if launch in st else "not launched", st)
                assert not any(n in st for n in FOREIGN), (what, st)
    finally:
        leaf.segment.close()
        ix.close()


@pytest.mark.parametrize("name,version", SEGMENTS, ids=IDS)
def test_every_case_in_one_batch_and_the_redo_list_cap(ctx, oracle, name, version):
    """Every non-refused query of the segment in one mixed batch, k = 10 and 129; then the list of handed-on candidates capped at 0
    and at 1 entry: the same rows bit for bit."""
    import rucene_amd
    fx = su.segment(name)
    ix, leaf = _open(oracle, fx, version)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        mixed = [q for c in fx.cases for q in c.queries if q.error is None]
        assert len(mixed) >= len(fx.cases) - 2
        for k in (10, 129):
            hits, totals, st = _search(ctx, g, leaf, mixed, k)
            print(name, version, "mixed batch, k", k, st)
            for i, q in enumerate(mixed):
                _assert_row(hits[i], totals[i], su.search_case(fx, q, k), (name, version, "mixed", k, q.terms, q.slop))
            assert not any(n in st for n in FOREIGN), st
        free = _search(ctx, g, leaf, mixed, 10)
        for cap in ("0", "1"):
            os.environ["RGPU_PHRASE_REDO_CAP"] = cap
            try:
                capped = _search(ctx, g, leaf, mixed, 10)
            finally:
                del os.environ["RGPU_PHRASE_REDO_CAP"]
            print(name, version, "redo list capped at", cap, capped[2])
            assert _same(free, capped), (name, version, cap)
    finally:
        leaf.segment.close()
        ix.close()


@pytest.mark.parametrize("version", [1, 0], ids=["bp128", "legacy"])
def test_deleted_docs(ctx, oracle, version):
    """Every other case's designed doc deleted, a query's only matching doc among them (the singleton's): deleted candidates are
    approximations that are never checked."""
    import rucene_amd
    emptied = 0
    for name in ("walk", "ties", "place"):
        fx = su.segment(name)
        alive = np.ones(fx.max_doc, dtype=bool)
        gone = [c.designed for c in fx.cases[::2] if c.designed is not None] + [c.designed for c in fx.cases if c.rung == "singleton"]
        alive[gone] = False
        live = sn.live_words(alive)
        ix, leaf = _open(oracle, fx, version, live_docs=live)
        try:
            g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
            queries = [q for c in fx.cases for q in c.queries if q.error is None]
            hits, totals, st = _search(ctx, g, leaf, queries, 10)
            print(name, version, "deleted", gone, st)
            for i, q in enumerate(queries):
                want = su.search_case(fx, q, 10, live=live)
                _assert_row(hits[i], totals[i], want, (name, version, "deleted docs", q.terms, q.slop))
                assert not set(hits[i]["doc"].tolist()) & set(gone)
                emptied += want[2] == 0 and su.search_case(fx, q, 10)[2] > 0
        finally:
            leaf.segment.close()
            ix.close()
    assert emptied >= 1   # the singleton's query lost its only matching doc


# ---- the collector: 8193 candidates --------------------------------------------------------------------------------------------------------
N_CHUNK = ps.CHUNK + 1


@pytest.fixture(scope="module")
def chunk_leaf(oracle):
    fx = ps.chunks(N_CHUNK)
    ix, leaf = _open(oracle, fx)
    yield fx, ix, leaf
    if leaf.segment is not None:
        leaf.segment.close()
    ix.close()


def _pairs(fx):
    """(q, p) - the clauses transposed: a matching doc reads "p q p" """
    return [su.usq([2 * j + 1, 2 * j], 0) for j in range(len(fx.first))]


def test_collector_at_every_k(ctx, chunk_leaf):
    """8193 candidates per query, the first match at candidate 0, 8191 and 8192; k = 1, hits - 1, hits, hits + 1 and 129."""
    import rucene_amd
    fx, ix, leaf = chunk_leaf
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    queries = _pairs(fx)
    n_hits = int(fx.matches[0].sum())
    assert fx.first == [0, ps.CHUNK - 1, ps.CHUNK] and n_hits > 129 and int(fx.matches[2].sum()) == 1
    for k in (1, n_hits - 1, n_hits, n_hits + 1, 129):
        hits, totals, st = _search(ctx, g, leaf, queries, k)
        print("k", k, st)
        for i, q in enumerate(queries):
            _assert_row(hits[i], totals[i], su.search_case(fx, q, k), ("collector", "k", k, q.terms))
        assert totals.tolist() == [int(m.sum()) for m in fx.matches]
        assert (hits["doc"] >= 0).sum(axis=1).tolist() == [min(k, t) for t in totals.tolist()]
        assert ps.COLLECT in st and (ps.MERGE in st) == (k <= ps.PASS_K), (k, st)
        assert hits[2]["doc"][0] == ps.CHUNK


def test_next_limit_applies_at_slop_0(ctx, chunk_leaf):
    """Two-phase at slop 0 too: with n non-matching candidates in front of the first hit, next_limit n - 1 abandons the leaf (no
    hits, total 0) and n serves it; RGPU_NEXT_LIMIT_ZERO serves only a first candidate that matches; -1 and the default serve
    everything."""
    import rucene_amd
    fx, ix, leaf = chunk_leaf
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    queries = _pairs(fx)
    abandoned = served = 0
    for limit in sorted({x for n in fx.first for x in (n - 1, n) if x >= 0}) + [None]:
        hits, totals, st = _search(ctx, g, leaf, queries, 10, next_limit=limit)
        print("next_limit", limit, st, totals.tolist())
        for i, q in enumerate(queries):
            want = su.search_case(fx, q, 10, next_limit=limit)
            _assert_row(hits[i], totals[i], want, ("next_limit", limit, q.terms))
            yields = limit is None or fx.first[i] <= limit
            assert totals[i] == (int(fx.matches[i].sum()) if yields else 0), (limit, fx.first[i])
            if not yields:
                assert (hits[i]["doc"] == -1).all()
            abandoned += not yields
            served += bool(yields and limit is not None and fx.first[i] == limit)
    assert abandoned >= 3 and served == 3
    qs, ts = _pack(g, leaf, queries)
    for raw in (0, -1):   # the searcher's default of 500 000 | no limit
        qs["next_limit"] = raw
        hits, totals = leaf.segment.search_span_unordered_batch(qs, ts, 10)
        for i, q in enumerate(queries):
            _assert_row(hits[i], totals[i], su.search_case(fx, q, 10), ("next_limit field", raw, q.terms))
    qs["next_limit"] = -3
    with pytest.raises(rucene_amd.RgpuError) as e:
        leaf.segment.search_span_unordered_batch(qs, ts, 10)
    assert e.value.status == ps.ILLEGAL_ARGUMENT


def test_deleted_candidates_in_front_of_the_first_hit_count(ctx, oracle):
    """The first 100 docs deleted: the first live match of pair 0 is candidate 111; next_limit 110 abandons, 111 serves. Everything
    deleted: no hits, no error."""
    import rucene_amd
    fx = ps.chunks(N_CHUNK)
    ix = fx.index(oracle)
    try:
        for alive in (np.arange(fx.n) >= 100, np.zeros(fx.n, dtype=bool)):
            live = fx.live_words(alive)
            leaf = ps.leaf_of(ix, len(fx.postings), fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf, live_docs=live)
            try:
                g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
                queries = _pairs(fx)
                for limit in (110, 111, None):
                    hits, totals, st = _search(ctx, g, leaf, queries, 10, next_limit=limit)
                    for i, q in enumerate(queries):
                        _assert_row(hits[i], totals[i], su.search_case(fx, q, 10, live=live, next_limit=limit), ("deleted in front", int(alive.sum()), limit, q.terms))
                    if alive.any():
                        assert (totals[0] > 0) == (limit != 110), (limit, totals.tolist())
                    else:
                        assert not totals.any() and (hits["doc"] == -1).all()
            finally:
                leaf.segment.close()
    finally:
        ix.close()


def test_boost_0_hits_score_0(ctx, chunk_leaf):
    """A doc with a span is a hit whatever its score: boost 0 gives every hit the score 0.0, doc 0 among them, ranked by doc id."""
    import rucene_amd
    fx, ix, leaf = chunk_leaf
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
    queries = _pairs(fx)
    hits, totals, st = _search(ctx, g, leaf, queries, 10, boost=0.0)
    for i, q in enumerate(queries):
        _assert_row(hits[i], totals[i], su.search_case(fx, q, 10, boost=0.0), ("boost 0", q.terms))
    assert totals.tolist() == [int(m.sum()) for m in fx.matches]
    assert hits[0]["doc"][0] == 0 and (hits[0]["score"].view(np.int32) == 0).all() and (np.diff(hits[0]["doc"]) > 0).all()


# ---- norms --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["raw-norms", "no-norms"])
@pytest.mark.parametrize("version", [1, 0], ids=["bp128", "legacy"])
def test_raw_and_no_norms(ctx, oracle, kind, version):
    """The default context ranks the norm bytes (every other test here); raw_norms=True reads the bytes, a field without norms
    scores with k1: the walk, the ties and the 16-bit / block-edge cases, lanes and left-over kernels alike."""
    import rucene_amd
    own = rucene_amd.Context(profile_kernels=True, raw_norms=True) if kind == "raw-norms" else None
    use = own or ctx
    try:
        for name in ("walk", "ties", "place"):
            fx = su.segment(name)
            ix, leaf = _open(oracle, fx, version, norms=kind != "no-norms")
            try:
                g = rucene_amd.GpuIndexSearcher([leaf], ctx=use)
                queries = [q for c in fx.cases for q in c.queries if q.error is None]
                hits, totals, st = _search(use, g, leaf, queries, 10)
                print(kind, name, version, st)
                for i, q in enumerate(queries):
                    want = su.search(fx.postings, fx.norms if kind != "no-norms" else None, fx.max_doc, fx.doc_count, fx.sum_ttf, q, 10)
                    _assert_row(hits[i], totals[i], want, (kind, name, version, q.terms, q.slop))
                assert (su.ONE if version == 0 else su.LANES) in st and (version == 0 or name == "walk" or su.LEFT in st)
            finally:
                leaf.segment.close()
                ix.close()
    finally:
        if own is not None:
            own.close()


# ---- refusals on the host, and the ordered call beside the new one --------------------------------------------------------------------------
def test_refused_inputs_are_refused_before_any_launch(ctx, oracle):
    import rucene_amd
    fx = su.segment("walk")
    ix, leaf = _open(oracle, fx)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        q = fx.cases[0].queries[0]
        seg = leaf.segment

        def refused(status, k=10, call=None, **fields):
            qs, ts = _pack(g, leaf, [q, q])
            for key, value in fields.items():
                (qs if key in qs.dtype.names else ts)[key][-1] = value
            ctx.kernel_stats_reset()
            with pytest.raises(rucene_amd.RgpuError) as e:
                (call or seg.search_span_unordered_batch)(qs, ts, k)
            assert e.value.status == status, (fields, k, e.value.status)
            assert not any(v["launches"] for n, v in ctx.kernel_stats().items() if n in su.NAMES + sn.NAMES + (su.CANDIDATES,)), (fields, ctx.kernel_stats())
            hits, totals, st = _search(ctx, g, leaf, [q], 10)   # an ordinary batch answers right behind it
            _assert_row(hits[0], totals[0], su.search_case(fx, q, 10), ("the batch behind the refusal", fields, k))

        refused(ps.ILLEGAL_ARGUMENT, n_terms=1)
        refused(ps.ILLEGAL_ARGUMENT, n_terms=ps.MAX_TERMS + 1)
        refused(ps.ILLEGAL_ARGUMENT, position=0)     # the second clause's position must be 1
        refused(ps.ILLEGAL_ARGUMENT, reserved=1)
        refused(ps.ILLEGAL_ARGUMENT, slop=-1)
        refused(ps.ILLEGAL_ARGUMENT, sim_table=1 << 20)
        refused(ps.ILLEGAL_ARGUMENT, k=0)
        refused(ps.UNSUPPORTED, k=rucene_amd._lib.MAX_K + 1)
        # the ordered call goes on refusing in_order = false
        refused(ps.UNSUPPORTED, call=lambda qs, ts, k: seg.search_span_near_batch(qs, ts, k, in_order=False))
        assert rucene_amd._lib.lib().rgpu_abi_version() == 6
    finally:
        leaf.segment.close()
        ix.close()


def test_a_segment_without_positions_is_refused(ctx, oracle):
    """rgpu_search_span_unordered_batch on a segment whose .pos file is not attached: IllegalState (-1), as the ordered call
    answers; the same rows on the leaf that has it attached answer right behind it."""
    import rucene_amd
    fx = su.segment("walk")
    ix, leaf = _open(oracle, fx)
    bare = ps.leaf_of(ix, len(fx.postings), fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        rucene_amd.GpuIndexSearcher([bare], ctx=ctx)   # (makes bare.segment; nothing attaches its positions)
        q = fx.cases[0].queries[0]
        qs, ts = _pack(g, leaf, [q])
        for call in (bare.segment.search_span_unordered_batch, bare.segment.search_span_near_batch):
            with pytest.raises(rucene_amd.RgpuError) as e:
                call(qs, ts, 10)
            assert e.value.status == -1, e.value.status   # RGPU_ERR_ILLEGAL_STATE
        hits, totals, st = _search(ctx, g, leaf, [q], 10)
        _assert_row(hits[0], totals[0], su.search_case(fx, q, 10), "behind the refusal")
    finally:
        leaf.segment.close()
        if bare.segment is not None:
            bare.segment.close()
        ix.close()


def test_the_ordered_call_still_gives_the_ordered_models_rows(ctx, oracle):
    """The same clause lists through rgpu_search_span_near_batch: the ordered model's rows and the ordered kernels' launches, none of
    the unordered ones - and the other way round. The two calls share one stage."""
    import rucene_amd
    S, N = rucene_amd.SpanTermQuery, rucene_amd.SpanNearQuery
    differ = 0
    for name in ("walk", "ties"):
        fx = su.segment(name)
        ix, leaf = _open(oracle, fx)
        try:
            g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
            queries = [q for c in fx.cases for q in c.queries if q.error is None]
            qs, ts = g.pack_phrases([N([S(t) for t in q.terms], slop=q.slop) for q in queries], leaf)
            qs["next_limit"] = -1
            ctx.kernel_stats_reset()
            hits, totals = leaf.segment.search_span_near_batch(qs, ts, 10)
            st = {n for n, v in ctx.kernel_stats().items() if v["launches"]}
            assert sn.LANES in st and not any(n in st for n in su.NAMES), st
            ctx.kernel_stats_reset()
            uhits, utotals = leaf.segment.search_span_unordered_batch(qs, ts, 10)
            st = {n for n, v in ctx.kernel_stats().items() if v["launches"]}
            assert su.LANES in st and not any(n in st for n in sn.NAMES), st
            for i, q in enumerate(queries):
                _assert_row(hits[i], totals[i], sn.search_case(fx, q, 10), (name, "ordered", q.terms, q.slop))
                _assert_row(uhits[i], utotals[i], su.search_case(fx, q, 10), (name, "unordered", q.terms, q.slop))
                differ += int(totals[i] != utotals[i])
        finally:
            leaf.segment.close()
            ix.close()
    assert differ >= 1


# ---- the Python mirror: four leaves with doc bases -----------------------------------------------------------------------------------------
def test_python_mirror_over_four_leaves(ctx, oracle):
    """GpuIndexSearcher(unordered_spans=True).search_batch / search over four leaves (one lacks a case's terms): the statistics
    leaf's weight, every leaf's rows merged, ordered rows beside them. With the flag off the same query is UnsupportedOperation and
    reaches cpu_fallback; nested clauses and span queries inside other queries are refused either way."""
    import rucene_amd
    S, N, T, B = rucene_amd.SpanTermQuery, rucene_amd.SpanNearQuery, rucene_amd.TermQuery, rucene_amd.BooleanQuery
    fxs = su.four_leaves()
    ixs = [fx.index(oracle) for fx in fxs]
    leaves, base = [], 0
    for fx, ix in zip(fxs, ixs):
        leaf = ps.leaf_of(ix, len(fx.postings), fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf)
        leaf.doc_base = base
        base += fx.max_doc
        leaves.append(leaf)
    fell_back = []
    try:
        g = rucene_amd.GpuIndexSearcher(leaves, ctx=ctx, cpu_fallback=lambda q, c: fell_back.append(q), unordered_spans=True)
        queries = [q for c in fxs[0].cases for q in c.queries]
        gq = [N([S(t) for t in q.terms], slop=q.slop, in_order=False) for q in queries]
        ordered = N([S(t) for t in queries[0].terms], slop=queries[0].slop)
        mixed = gq + [T(0), ordered]   # beside a term row and an ordered span row
        for k in (10, 40):
            ctx.kernel_stats_reset()
            hits, totals = g.search_batch(mixed, k)
            for i, q in enumerate(queries):
                _assert_row(hits[i], totals[i], su.search_leaves(fxs, q, k), ("four leaves", k, q.terms, q.slop))
            _assert_row(hits[-1], totals[-1], sn.search_leaves(fxs, queries[0], k), ("four leaves", k, "the ordered row"))
            assert su.LANES in ctx.kernel_stats() and sn.LANES in ctx.kernel_stats()
        assert (hits[:len(queries)]["doc"].max(axis=1) >= fxs[0].max_doc).any()   # hits beyond the first leaf carry their doc base
        boosted = N([S(t) for t in queries[0].terms], slop=queries[0].slop, in_order=False, boost=2.5)
        hits, totals = g.search_batch([boosted], 10)
        _assert_row(hits[0], totals[0], su.search_leaves(fxs, queries[0], 10, boost=2.5), "boost 2.5")
        limited = rucene_amd.GpuIndexSearcher(leaves, ctx=ctx, next_limit=0, unordered_spans=True)
        hits, totals = limited.search_batch(gq, 10)
        for i, q in enumerate(queries):
            _assert_row(hits[i], totals[i], su.search_leaves(fxs, q, 10, next_limit=0), ("four leaves, next_limit 0", q.terms, q.slop))
        collector = rucene_amd.TopDocsCollector(10)
        g.search(gq[0], collector)
        want = su.search_leaves(fxs, queries[0], 10)
        top = collector.top_docs()
        assert top.total_hits() == want[2] and [d for d, _ in top.score_docs()] == want[0].tolist() and not fell_back
        near = gq[0]
        unserved = [N([S(0), N([S(1), S(2)], in_order=False)], in_order=False), B.build([near, T(3)], []), B.build([], [near, T(3)]),
                    rucene_amd.DisjunctionMaxQuery([T(1), near]), rucene_amd.BoostingQuery.build(near, T(1), 0.5)]
        for q in unserved:
            g.search(q, rucene_amd.TopDocsCollector(10))
            assert fell_back and fell_back[-1] is q, q
        assert len(fell_back) == len(unserved)
        # the flag off: the CPU searcher's, as before
        stub = []
        off = rucene_amd.GpuIndexSearcher(leaves, ctx=ctx, cpu_fallback=lambda q, c: stub.append(q))
        off.search(near, rucene_amd.TopDocsCollector(10))
        assert stub == [near]
        strict = rucene_amd.GpuIndexSearcher(leaves, ctx=ctx)
        first = strict.search_batch([T(0)], 10)[0]
        for call in (lambda: strict.search_batch([near], 10), lambda: g.rescore_batch(first, [near])):
            with pytest.raises(rucene_amd.RgpuError) as e:
                call()
            assert e.value.status == ps.UNSUPPORTED
    finally:
        for leaf in leaves:
            if leaf.segment is not None:
                leaf.segment.close()
        for ix in ixs:
            ix.close()


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror_gives_the_models_rows(oracle, tmp_path):
    """GpuIndexSearcher::search_many / search with unordered_spans = true (tests/cpp/span_unordered_demo.cpp, compiled
    warnings-as-errors) over the ties segment with deletions: the model's rows; with the flag off, and for the unserved shapes,
    UnsupportedOperation."""
    fx = su.segment("ties")
    exe = str(tmp_path / "span_unordered_demo")
    libdir = os.path.join(ROOT, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "span_unordered_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    alive = np.ones(fx.max_doc, dtype=bool)
    alive[fx.cases[3].designed] = False
    live = sn.live_words(alive)
    ix, leaf = _open(oracle, fx, live_docs=live)
    try:
        doc_bytes, pos_bytes = ix.files()
        for name, blob in (("doc", doc_bytes), ("pos", pos_bytes), ("norms", fx.norms.tobytes()), ("terms", leaf.terms.tobytes()),
                           ("tpos", leaf.term_positions.tobytes()), ("live", live.tobytes())):
            (tmp_path / (name + ".bin")).write_bytes(bytes(blob))
        queries = [q for c in fx.cases for q in c.queries]
        boosts = [1.0 if i % 3 else 2.0 for i in range(len(queries))]
        (tmp_path / "queries.txt").write_text("".join("%d %s %s\n" % (q.slop, b, ",".join(map(str, q.terms))) for q, b in zip(queries, boosts)))
        k = 16
        out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.doc_count), str(fx.sum_ttf), str(k)], text=True, timeout=120).strip().splitlines()
        assert len(out) == len(queries) + 3 and out[-2:] == ["refused 1 1 1 1 1", "built 1"], out[-3:]

        def row_of(line, head):
            parts = line.split()
            assert parts[:len(head)] == head, line
            return int(parts[len(head)]), [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[len(head) + 1:]]
        for i, (q, b) in enumerate(zip(queries, boosts)):
            d, sc, total = su.search_case(fx, q, k, live=live, boost=b)
            assert row_of(out[i], ["row", str(i)]) == (total, list(zip(d.tolist(), sc.view(np.uint32).tolist()))), (i, out[i])
        d, sc, total = su.search_case(fx, queries[0], k, live=live, boost=boosts[0])
        assert row_of(out[len(queries)], ["single"]) == (total, list(zip(d.tolist(), sc.view(np.uint32).tolist())))
    finally:
        if leaf.segment is not None:
            leaf.segment.close()
        ix.close()
