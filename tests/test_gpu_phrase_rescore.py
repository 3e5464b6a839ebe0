"""QueryRescorer with PhraseQuery rows on the device (`-m gpu`): rgpu_rescore_phrase_batch through GpuIndexSearcher.rescore_batch
against tests/phrase_rescore.py's rescore_ref (proven against the oracle's QueryRescorer by tests/test_phrase_rescore_cpu.py) over
the oracle's phrase scores - docs and score bits equal, nowhere a tolerance. The kernel statistics of a batch say which launches
answered it (`-s` shows them)."""
import os
import subprocess

import numpy as np
import pytest

import phrase_rescore as pr
import phrase_spectrum as ps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


class Opened:
    """A fixture as a one-leaf searcher beside its oracle index."""

    def __init__(self, oracle, ctx, fx, version=1, woven=False, live_docs=None):
        import rucene_amd
        self.fx = fx
        self.ix = fx.index(oracle, version=version, woven=woven)
        self.leaf = pr.leaf_of(self.ix, fx, live_docs=live_docs, woven=woven)
        self.g = rucene_amd.GpuIndexSearcher([self.leaf], ctx=ctx)

    def second(self, q):
        return self.fx.second(self.ix, q.terms, q.slop, q.positions, q.boost)

    def close(self):
        self.leaf.segment.close()
        self.ix.close()


@pytest.fixture(scope="module")
def membership(oracle, ctx):
    o = Opened(oracle, ctx, pr.membership())
    yield o
    o.close()


@pytest.fixture(scope="module")
def wide(oracle, ctx):
    o = Opened(oracle, ctx, pr.wide())
    yield o
    o.close()


def PQ(terms, slop=0, boost=1.0):
    import rucene_amd
    return rucene_amd.PhraseQuery(terms, boost=boost, slop=slop)


def _rescore(ctx, g, rows, queries, k, **kw):
    """One batch -> (rescored hit rows, {launch name: launches} of this batch)."""
    ctx.kernel_stats_reset()
    got = g.rescore_batch(pr.as_hits(rows, k), queries, **kw)
    st = {n: v["launches"] for n, v in ctx.kernel_stats().items() if v["launches"]}
    assert pr.CANDIDATES in st and pr.COMBINE in st and pr.SORT in st, st
    assert not [n for n in pr.NEVER if n in st], st
    return got, st


def _per_row(v, n):
    return np.broadcast_to(np.asarray(v), (n,)).tolist()


def _check(o, got, rows, queries, what, query_weight=1.0, rescore_weight=1.0, mode=pr.TOTAL, window_size=None, k=None):
    """Every row against rescore_ref; returns how many hits the second queries matched inside their windows."""
    n = len(rows)
    qw, rw, md = _per_row(query_weight, n), _per_row(rescore_weight, n), _per_row(mode, n)
    win = _per_row(k if window_size is None else window_size, n)
    matched = 0
    for i, (row, q) in enumerate(zip(rows, queries)):
        second = o.second(q)
        window = min(win[i], pr.WINDOW_CAP)
        pr.assert_rows(got[i], pr.rescore_ref(row, second, window, qw[i], rw[i], md[i]), (what, i, q.terms, q.slop, md[i], win[i]))
        matched += sum(d in second for d, _ in row[:window])
    return matched


def _raw(leaf, g, queries, rows, k, finish=1, **req_fields):
    """rgpu_rescore_phrase_batch itself on a buffer of the caller's -> (status, the buffer afterwards, the buffer before)."""
    from rucene_amd import _lib as gpu
    qs, ts = g.pack_phrases(queries, leaf)
    req = np.zeros(len(queries), dtype=gpu.RESCORE_REQUEST_DTYPE)
    req["query_weight"], req["rescore_weight"], req["mode"], req["window_size"] = 1.0, 1.0, pr.TOTAL, k
    for name, v in req_fields.items():
        req[name] = v
    hits = pr.as_hits(rows, k)
    before = hits.copy()
    rc = gpu.lib().rgpu_rescore_phrase_batch(leaf.segment._h, qs.ctypes.data, qs.size, ts.ctypes.data, ts.size, req.ctypes.data, k, hits.ctypes.data, finish)
    return rc, hits, before


# ---- 1. membership ------------------------------------------------------------------------------------------------------------------
def test_membership_of_a_hit_in_every_term(ctx, membership):
    """One window with a phrase match at posting 127 and at posting 128 of the df-129 term, a doc with all terms and no phrase, a doc
    that lacks the rarest term, one that lacks only the most frequent, docs below a first and above a last posting; a three-term
    phrase with the singleton term; a row where no hit matches; a row whose phrase has an absent term; the sloppy twin."""
    o, D = membership, pr.DESIGN
    side = pr.side_by_side_row()
    rows = [side, pr.make_row([D["match"], D["match-block-last"], D["lacks-rarest"]], 2), pr.make_row([30, 40, 21, 5, 12, 270, 280], 3),
            pr.make_row([D["match"], D["match-block-last"]], 4), pr.side_by_side_row(5)]
    queries = [PQ([pr.T, pr.B]), PQ([pr.S, pr.T, pr.B]), PQ([pr.T, pr.B]), PQ([pr.T, pr.ABSENT]), PQ([pr.B, pr.T], slop=2)]
    got, st = _rescore(ctx, o.g, rows, queries, 16, query_weight=0.7, rescore_weight=2.5)
    print("membership", st)
    assert _check(o, got, rows, queries, "membership", query_weight=0.7, rescore_weight=2.5, k=16) == 3 + 1 + 0 + 0 + 3
    for i, row in enumerate(rows):   # alone, a row gets what it gets in the batch
        alone, _ = _rescore(ctx, o.g, [row], [queries[i]], 16, query_weight=0.7, rescore_weight=2.5)
        assert (alone[0] == got[i]).all(), i
    no_match = pr.rescore_ref(rows[2], {}, 16, 0.7, 2.5, pr.TOTAL)
    pr.assert_rows(got[2], no_match, "no hit matches")
    pr.assert_rows(got[3], pr.rescore_ref(rows[3], {}, 16, 0.7, 2.5, pr.TOTAL), "absent term")


# ---- 2. scoring ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", pr.MODES)
def test_every_mode_and_weights(ctx, membership, mode):
    o = membership
    rows = [pr.side_by_side_row(10 + mode), pr.side_by_side_row(20 + mode)]
    queries = [PQ([pr.T, pr.B]), PQ([pr.B, pr.T], slop=1)]
    for qw, rw in ((1.0, 1.0), (0.7, 2.5), (1.75, 0.125)):
        got, _ = _rescore(ctx, o.g, rows, queries, 10, query_weight=qw, rescore_weight=rw, mode=mode)
        assert _check(o, got, rows, queries, "modes", query_weight=qw, rescore_weight=rw, mode=mode, k=10) >= 3


@pytest.mark.parametrize("mode", [pr.AVG, pr.MULTIPLY, pr.MIN])
def test_a_match_that_scores_zero_is_still_a_match(ctx, membership, mode):
    """A phrase with boost 0 scores +0.0 on every doc it matches: AVG halves such a hit, MULTIPLY and MIN zero it; a hit the phrase
    does not match keeps first * query_weight."""
    o = membership
    rows = [pr.side_by_side_row(31)]
    q = PQ([pr.T, pr.B], boost=0.0)
    got, _ = _rescore(ctx, o.g, rows, [q], 10, query_weight=0.7, rescore_weight=2.5, mode=mode)
    assert _check(o, got, rows, [q], "boost 0", query_weight=0.7, rescore_weight=2.5, mode=mode, k=10) == 3
    as_no_match = pr.rescore_ref(rows[0], {}, 10, 0.7, 2.5, mode)
    assert [s for _, s in as_no_match] != got[0]["score"][:len(rows[0])].tolist()


def test_a_tie_after_combining_is_broken_by_doc(ctx, membership):
    """MAX, weights 1: a hit the phrase does not match carries, as its first score, exactly the phrase score of a matching hit of a
    smaller doc id that sits behind it in the first pass: equal scores afterwards, the smaller doc first."""
    o = membership
    q = PQ([pr.T, pr.B])
    second = o.second(q)
    m, x = pr.DESIGN["match"], pr.DESIGN["above-most-frequent-last"]
    sm = second[m]
    assert m < x and x not in second and sm > 0 and np.float32(sm / 8) > 0
    rows = [[(x, sm), (m, np.float32(sm / 4)), (40, np.float32(sm / 8))]]
    got, _ = _rescore(ctx, o.g, rows, [q], 4, mode=pr.MAX)
    _check(o, got, rows, [q], "tie", mode=pr.MAX, k=4)
    assert got[0]["doc"][:2].tolist() == [m, x] and got[0]["score"][0] == got[0]["score"][1]


# ---- 3. windows and k ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64, 65, 128])
def test_windows_at_every_k(ctx, wide, k):
    """Windows 0, 1, k - 1, k and above k, full rows and rows with fewer hits than the window."""
    o = wide
    windows = sorted({0, 1, max(k - 1, 0), k, k + 7})
    rows, queries, win = [], [], []
    for j, w in enumerate(windows):
        rows += [pr.wide_rows(1, k, 40 + j)[0], pr.wide_rows(1, max(1, k // 2), 60 + j)[0]]
        queries += [PQ(*pr.WIDE_PHRASES[j % 3]), PQ(*pr.WIDE_PHRASES[3 + j % 3])]
        win += [w, w]
    win = np.array(win, dtype=np.int32)
    got, st = _rescore(ctx, o.g, rows, queries, k, query_weight=0.7, rescore_weight=1.5, mode=pr.TOTAL, window_size=win)
    print("k", k, st)
    matched = _check(o, got, rows, queries, ("windows", k), query_weight=0.7, rescore_weight=1.5, window_size=win, k=k)
    assert matched > 0 or k == 1


def test_k_200_is_clipped_at_128_and_a_batch_of_70_rows(ctx, wide):
    o = wide
    rows = pr.wide_rows(2, 200, 90)
    queries = [PQ([0, 1]), PQ([0, 1, 2], slop=1)]
    got, _ = _rescore(ctx, o.g, rows, queries, 200, query_weight=0.7, rescore_weight=1.5, window_size=200)
    assert _check(o, got, rows, queries, "k 200", query_weight=0.7, rescore_weight=1.5, window_size=200, k=200) > 10
    assert got[0]["doc"][128:200].tolist() == [d for d, _ in rows[0][128:]]   # the tail keeps its order
    rows = pr.wide_rows(70, 9, 91)
    queries = [PQ(*pr.WIDE_PHRASES[i % len(pr.WIDE_PHRASES)]) for i in range(70)]
    modes = np.arange(70) % 5
    got, _ = _rescore(ctx, o.g, rows, queries, 10, query_weight=1.25, rescore_weight=0.5, mode=modes, window_size=7)
    assert _check(o, got, rows, queries, "70 rows", query_weight=1.25, rescore_weight=0.5, mode=modes, window_size=7, k=10) > 20


# ---- 4. slop ------------------------------------------------------------------------------------------------------------------------
def test_sloppy_phrases_and_repeated_terms(ctx, wide):
    """Slop 1 and 2 over two and three distinct terms (the 64-candidate kernel), seven distinct terms (past it: the one-candidate
    kernel); a sloppy phrase that names a term twice is refused and leaves the rows alone; the exact "a b a" is served."""
    import rucene_amd
    o = wide
    sloppy = [q for q in pr.WIDE_PHRASES if q.slop > 0 and len(q.terms) <= 3]
    rows = pr.wide_rows(len(sloppy), 40, 95)
    queries = [PQ(*q) for q in sloppy]
    got, st = _rescore(ctx, o.g, rows, queries, 40)
    print("slop", st)
    assert _check(o, got, rows, queries, "slop", k=40) > 10
    assert ps.S_LANES in st and ps.S_WIDE not in st and ps.LANES not in st, st
    every_fifth = [d for d in range(0, pr.WIDE_DOCS, 5)][:30] + [1, 2, 3]
    rows = [pr.make_row(every_fifth, 96)]
    got, st = _rescore(ctx, o.g, rows, [PQ(pr.SEVEN, slop=2)], 40)
    print("seven terms", st)
    assert _check(o, got, rows, [PQ(pr.SEVEN, slop=2)], "seven", k=40) > 5
    assert ps.S_LANES in st and ps.S_LEFT in st and ps.S_WIDE not in st, st
    rows = pr.wide_rows(1, 40, 97)
    rc, hits, before = _raw(o.leaf, o.g, [PQ([0, 1, 0], slop=1)], rows, 40)
    assert rc == pr.UNSUPPORTED and (hits == before).all()
    with pytest.raises(rucene_amd.RgpuError) as e:
        o.g.rescore_batch(pr.as_hits(rows, 40), [PQ([0, 1, 0], slop=1)])
    assert e.value.status == pr.UNSUPPORTED
    got, st = _rescore(ctx, o.g, rows, [PQ([0, 1, 0])], 40)
    assert _check(o, got, rows, [PQ([0, 1, 0])], "a b a", k=40) > 0 and ps.LANES in st


def test_refusals_leave_the_rows_alone(ctx, oracle, membership):
    """The argument statuses of rgpu_rescore_phrase_batch on a live segment, the buffer untouched every time."""
    import rucene_amd
    from rucene_amd import _lib as gpu
    o = membership
    rows = [pr.side_by_side_row(7)]
    q = [PQ([pr.T, pr.B])]
    for fields in (dict(mode=5), dict(mode=-1), dict(window_size=-1)):
        rc, hits, before = _raw(o.leaf, o.g, q, rows, 10, **fields)
        assert rc == pr.ILLEGAL_ARGUMENT and (hits == before).all(), fields
    qs, ts = o.g.pack_phrases(q, o.leaf)
    req = np.zeros(1, dtype=gpu.RESCORE_REQUEST_DTYPE)
    req["query_weight"], req["rescore_weight"], req["mode"], req["window_size"] = 1.0, 1.0, pr.TOTAL, 10

    def call(qs_, ts_, k=10, seg=o.leaf.segment):
        hits = pr.as_hits(rows, max(k, 10))
        before = hits.copy()
        rc = gpu.lib().rgpu_rescore_phrase_batch(seg._h, qs_.ctypes.data, qs_.size, ts_.ctypes.data, ts_.size, req.ctypes.data, k, hits.ctypes.data, 1)
        assert (hits == before).all()
        return rc
    for field, bad in (("n_terms", 1), ("n_terms", 17), ("slop", -1), ("first_term", 1), ("first_term", -1), ("sim_table", 10_000), ("sim_table", -1)):
        bq = qs.copy()
        bq[field][0] = bad
        assert call(bq, ts) == pr.ILLEGAL_ARGUMENT, (field, bad)
    bt = ts.copy()
    bt["positions"]["pos_start_fp"][0] = 1 << 40
    assert call(qs, bt) == pr.ILLEGAL_ARGUMENT
    assert call(qs, ts, k=0) == pr.ILLEGAL_ARGUMENT and call(qs, ts, k=1025) == pr.UNSUPPORTED
    bare = rucene_amd.Segment(ctx, o.leaf.doc_bytes, o.fx.norms, o.fx.max_doc, index_options=3)   # no .pos file attached
    try:
        assert call(qs, ts, seg=bare) == pr.ILLEGAL_STATE
    finally:
        bare.close()
    got, _ = _rescore(ctx, o.g, rows, q, 10)   # ordinary error returns: the context goes on answering
    assert _check(o, got, rows, q, "behind the refusals", k=10) == 3


# ---- 5. the ladder ------------------------------------------------------------------------------------------------------------------
LADDER = ("freq-10", "freq-11", "freq-128", "freq-129", "freq-1025", "pool-256", "pool-257")


def test_every_rung_of_the_position_list_ladder(ctx, oracle):
    """A hit that holds a term 10 | 11, 128 | 129 and 1025 times, sloppy pools of 256 | 257: the rows, and from the kernel
    statistics which launches answered - the 64-candidate kernel alone, "left by the 64-candidate kernel", the wide lists / pool,
    or the refusal (status -5, rows untouched)."""
    import rucene_amd
    fx = ps.segment("freq")
    ix = fx.index(oracle)
    leaf = ps.leaf_of(ix, len(fx.postings), fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        cases = {c.name: c for c in fx.cases}
        for name in LADDER:
            c = cases[name]
            row = pr.make_row([c.ordinary, c.designed, c.designed + 1, 0], 300 + len(name))
            for q in c.queries:
                what = (name, "slop", q.slop, q.level)
                gq = rucene_amd.PhraseQuery(q.terms, q.positions, slop=q.slop)
                if q.error is not None:
                    rc, hits, before = _raw(leaf, g, [gq], [row], 8)
                    assert rc == q.error == pr.UNSUPPORTED and (hits == before).all(), what
                    print(name, "slop", q.slop, "refused with status", rc)
                    continue
                docs, scores, total = fx.search(ix, q, fx.max_doc)
                second = {int(d): s for d, s in zip(docs, scores)}
                assert c.designed in second and c.designed + 1 not in second, what
                got, st = _rescore(ctx, g, [row], [gq], 8, query_weight=0.7, rescore_weight=2.5)
                print(name, "slop", q.slop, q.level, st)
                pr.assert_rows(got[0], pr.rescore_ref(row, second, 8, 0.7, 2.5, pr.TOTAL), what)
                lanes, left, wide_ = (ps.LANES, ps.LEFT, ps.WIDE) if q.slop == 0 else (ps.S_LANES, ps.S_LEFT, ps.S_WIDE)
                assert lanes in st and (left in st) == (q.level != "lanes") and (wide_ in st) == (q.level == "wide"), (what, st)
                assert ps.ONE not in st and ps.S_ONE not in st, (what, st)
    finally:
        leaf.segment.close()
        ix.close()


# ---- 6. other encodings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["legacy", "payloads+offsets", "no-norms", "raw-norms"])
def test_other_encodings(ctx, oracle, kind):
    import rucene_amd
    own = rucene_amd.Context(profile_kernels=True, raw_norms=True) if kind == "raw-norms" else None
    c = own or ctx
    o = Opened(oracle, c, pr.membership(norms=kind != "no-norms"), version=0 if kind == "legacy" else 1, woven=kind == "payloads+offsets")
    try:
        rows = [pr.side_by_side_row(50), pr.side_by_side_row(51), pr.make_row([100, 264, 40], 52)]
        queries = [PQ([pr.T, pr.B]), PQ([pr.B, pr.T], slop=2), PQ([pr.S, pr.T, pr.B])]
        got, st = _rescore(c, o.g, rows, queries, 12, query_weight=0.7, rescore_weight=2.5, mode=pr.AVG)
        print(kind, st)
        assert _check(o, got, rows, queries, kind, query_weight=0.7, rescore_weight=2.5, mode=pr.AVG, k=12) == 7
        if kind == "legacy":   # the one-candidate kernels answer
            assert ps.ONE in st and ps.S_ONE in st and ps.LANES not in st and ps.S_LANES not in st, st
        else:
            assert ps.LANES in st and ps.S_LANES in st, st
    finally:
        o.close()
        if own is not None:
            own.close()


# ---- 7. leaves ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deleted", [False, True], ids=["all-live", "a-match-between-two-hits-deleted"])
def test_three_leaves(ctx, oracle, deleted):
    """Hits in all three leaves, the third lacking a phrase term; one call per leaf, the last one finishing: every score takes
    query_weight once. A deleted doc that matches the phrase and lies between two hits changes nothing (the rescorer consults no
    live docs, and the doc is no hit)."""
    import rucene_amd
    fxs = pr.leaves()
    ixs = [fx.index(oracle) for fx in fxs]
    live = None
    if deleted:
        alive = np.ones(fxs[1].max_doc, dtype=bool)
        alive[266] = False   # a match of leaf 1, between the hits 30 and 270 of that leaf
        live = np.packbits(np.concatenate([alive, np.zeros(-alive.size % 64, dtype=bool)]), bitorder="little").view(np.uint64).copy()
    leaves = [pr.leaf_of(ix, fx, doc_base=base, live_docs=live if i == 1 else None) for i, (ix, fx, base) in enumerate(zip(ixs, fxs, pr.LEAF_BASES))]
    try:
        g = rucene_amd.GpuIndexSearcher(leaves, ctx=ctx)
        assert g._stats_leaf == 0
        stats = (g.max_doc(), fxs[0].doc_count, fxs[0].sum_ttf)
        docs = [100, 264, 30, 40, 300 + 20, 300 + 30, 300 + 270, 300 + 100, 600 + 10, 600 + 3, 5, 300 + 21]
        rows = [pr.make_row(docs, 70), pr.make_row(docs[::-1], 71)]
        queries = [PQ([pr.T, pr.B]), PQ([pr.B, pr.T], slop=2)]
        for window in (12, 9):
            got, st = _rescore(ctx, g, rows, queries, 16, query_weight=0.7, rescore_weight=2.5, mode=pr.TOTAL, window_size=window)
            assert st[pr.CANDIDATES] == st[pr.COMBINE] == 3 and st[pr.SORT] == 1, st
            for i, q in enumerate(queries):
                second = {}
                for ix, fx, base in zip(ixs[:2], fxs[:2], pr.LEAF_BASES):   # (the third leaf lacks T: no scorer there)
                    second.update(fx.second(ix, q.terms, q.slop, stats=stats, doc_base=base))
                assert sum(d in second for d, _ in rows[i][:window]) >= 2
                pr.assert_rows(got[i], pr.rescore_ref(rows[i], second, window, 0.7, 2.5, pr.TOTAL), ("leaves", deleted, window, i))
    finally:
        for leaf in leaves:
            if leaf.segment is not None:
                leaf.segment.close()
        for ix in ixs:
            ix.close()


def test_a_sloppy_phrase_whose_terms_are_both_absent_from_a_leaf(ctx, oracle):
    """A slop-2 phrase of two different terms over three leaves, the third holding neither term: absent terms all look alike (no
    postings), which is no "term named twice" - the leaf is served (PhraseWeight::create_scorer -> None: its hits take
    first * query_weight), status 0, rows equal to rescore_ref."""
    import rucene_amd
    fxs = pr.leaves()
    assert fxs[2].docs_of(pr.T) == [] and fxs[2].docs_of(pr.S) == []
    ixs = [fx.index(oracle) for fx in fxs]
    leaves = [pr.leaf_of(ix, fx, doc_base=base) for ix, fx, base in zip(ixs, fxs, pr.LEAF_BASES)]
    try:
        g = rucene_amd.GpuIndexSearcher(leaves, ctx=ctx)
        stats = (g.max_doc(), fxs[0].doc_count, fxs[0].sum_ttf)
        q = PQ([pr.T, pr.S], slop=2)
        rows = [pr.make_row([264, 100, 300 + 100, 300 + 30, 600 + 10, 600 + 3, 40], 75)]
        got, st = _rescore(ctx, g, rows, [q], 8, query_weight=0.7, rescore_weight=2.5, mode=pr.AVG, window_size=6)
        second = {}
        for ix, fx, base in zip(ixs[:2], fxs[:2], pr.LEAF_BASES):
            second.update(fx.second(ix, q.terms, q.slop, stats=stats, doc_base=base))
        assert sorted(second) == [100, 400]
        pr.assert_rows(got[0], pr.rescore_ref(rows[0], second, 6, 0.7, 2.5, pr.AVG), "both terms absent from the third leaf")
        alone = [pr.make_row([610, 603, 620], 76)]   # the call for that leaf by itself
        rc, hits, _ = _raw(leaves[2], g, [q], alone, 4, query_weight=0.7)
        assert rc == 0
        pr.assert_rows(hits[0], pr.rescore_ref(alone[0], {}, 4, 0.7, 1.0, pr.TOTAL), "the leaf that holds neither term")
    finally:
        for leaf in leaves:
            if leaf.segment is not None:
                leaf.segment.close()
        for ix in ixs:
            ix.close()


# ---- 8. mirrors ---------------------------------------------------------------------------------------------------------------------
def test_a_batch_mixing_term_boolean_and_phrase_rows(ctx, membership):
    """Each row of a mixed batch through GpuIndexSearcher.rescore_batch gets what it gets alone."""
    import rucene_amd
    o = membership
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    queries = [T(pr.B), PQ([pr.T, pr.B]), B.build([T(pr.T), T(pr.B)], []), PQ([pr.B, pr.T], slop=2), B.build([], [T(pr.S), T(pr.T)]), PQ([pr.T, pr.ABSENT])]
    rows = [pr.side_by_side_row(80 + i) for i in range(len(queries))]
    modes = np.array([0, 1, 2, 3, 4, 0])
    hits = pr.as_hits(rows, 12)
    ctx.kernel_stats_reset()
    got = o.g.rescore_batch(hits, queries, query_weight=0.7, rescore_weight=2.5, mode=modes, window_size=8)
    st = {n for n, v in ctx.kernel_stats().items() if v["launches"]}
    assert "k_rescore" in st and pr.CANDIDATES in st and pr.COMBINE in st, st
    for i, q in enumerate(queries):
        alone = o.g.rescore_batch(hits[i:i + 1], [q], query_weight=0.7, rescore_weight=2.5, mode=int(modes[i]), window_size=8)
        assert (alone[0] == got[i]).all(), i
    for i in (1, 3, 5):
        pr.assert_rows(got[i], pr.rescore_ref(rows[i], o.second(queries[i]), 8, 0.7, 2.5, int(modes[i])), ("mixed", i))


def test_cpp_host_mirror_gives_the_python_mirrors_rows(ctx, membership, tmp_path):
    """GpuIndexSearcher::rescore (csrc/host/gpu_index_searcher.hpp) with phrase, term and boolean rows in one batch:
    tests/cpp/phrase_window_rescore_demo.cpp over the same files prints the rows the Python mirror returns."""
    import rucene_amd
    o, fx = membership, membership.fx
    exe = str(tmp_path / "phrase_window_rescore_demo")
    libdir = os.path.join(ROOT, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "phrase_window_rescore_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    doc_bytes, pos_bytes = o.ix.files()
    for name, blob in (("doc", doc_bytes), ("pos", pos_bytes), ("norms", fx.norms.tobytes()), ("terms", o.leaf.terms.tobytes()),
                       ("tpos", o.leaf.term_positions.tobytes())):
        (tmp_path / (name + ".bin")).write_bytes(bytes(blob))
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    specs = [("p", 0, [pr.T, pr.B], pr.TOTAL, 0.7, 2.5, 10), ("t", 0, [pr.B], pr.MAX, 1.0, 1.0, 10), ("p", 2, [pr.B, pr.T], pr.AVG, 1.5, 0.5, 6),
             ("a", 0, [pr.T, pr.B], pr.MULTIPLY, 0.5, 1.0, 10), ("p", 0, [pr.S, pr.T, pr.B], pr.MIN, 1.0, 3.0, 4), ("p", 0, [pr.T, pr.ABSENT], pr.TOTAL, 0.7, 1.0, 10)]
    rows = [pr.side_by_side_row(120 + i) for i in range(len(specs))]
    lines = []
    for (kind, slop, terms, mode, qw, rw, window), row in zip(specs, rows):
        cells = ["%d:%08x" % (d, int(np.float32(s).view(np.uint32))) for d, s in row]
        lines.append(" ".join([kind, str(slop), str(len(terms))] + [str(t) for t in terms] + [str(mode), repr(float(qw)), repr(float(rw)), str(window), str(len(row))] + cells))
    (tmp_path / "rows.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.doc_count), str(fx.sum_ttf)], text=True).strip().splitlines()
    assert len(out) == len(specs)
    k = len(rows[0])
    for i, (kind, slop, terms, mode, qw, rw, window) in enumerate(specs):
        q = PQ(terms, slop=slop) if kind == "p" else (T(terms[0]) if kind == "t" else B.build([T(t) for t in terms], []))
        want = o.g.rescore_batch(pr.as_hits([rows[i]], k), [q], query_weight=qw, rescore_weight=rw, mode=mode, window_size=window)[0]
        parts = out[i].split()
        assert parts[0] == "rescore" and int(parts[1]) == i
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[2:]]
        assert [g_[0] for g_ in got] == want["doc"].tolist() and [g_[1] for g_ in got] == want["score"].view(np.uint32).tolist(), (i, kind)


# ---- 9. cross-check against search --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slop", [0, 2])
def test_rescored_zero_rows_are_the_searchs_scores(ctx, membership, slop):
    """rgpu_search_phrase_batch with k = max_doc names the matching docs and their scores; rows of exactly those docs with first
    score 0, rescored with TOTAL, weights 1 and a window that covers them, carry the search's scores bit for bit."""
    o = membership
    q = PQ([pr.T, pr.B] if slop == 0 else [pr.B, pr.T], slop=slop)
    hits, totals = o.g.search_phrase_batch([q], o.fx.max_doc)
    n = int(totals[0])
    assert n == len(pr.MATCHES) and sorted(hits[0]["doc"][:n].tolist()) == sorted(pr.MATCHES)
    rows = [[(int(d), np.float32(0.0)) for d in sorted(hits[0]["doc"][:n].tolist())]]
    got, _ = _rescore(ctx, o.g, rows, [q], 8, query_weight=1.0, rescore_weight=1.0, mode=pr.TOTAL, window_size=8)
    assert got[0]["doc"][:n].tolist() == hits[0]["doc"][:n].tolist()
    assert got[0]["score"][:n].view(np.uint32).tolist() == hits[0]["score"][:n].view(np.uint32).tolist()
    assert (got[0]["doc"][n:] == -1).all()
