"""Cross-field queries on the GPU (`-m gpu`): rgpu_segment_attach_field / _prepare_field_terms / _get_field_info and
rgpu_search_fields_batch through the C ABI's Python binding, against tests/cross_field.py (which tests/test_cross_field_cpu.py ties to
the oracle's own searches). Everything is compared bit for bit: doc ids, score bits, -1 padding, hit counts.

The leaf: three fields in ONE .doc file over 549 docs = one 512-doc window and a last window of 37.
  field 0 `title`  30 distinct norm bytes (RANK mode), short; lists of df 400, 127, 128, 129, 256, 0, and a singleton LAST
  field 1 `body`   70 distinct norm bytes (RAW mode), long;   a singleton FIRST (same file pointer as title's last), df 400, 129, 256,
                   0, 37, and a singleton last (the file pointer of tags' first list, a block list)
  field 2 `tags`   no norms; df 256 at freq 3 and every doc at freq 2 (without norms a score depends on the freq alone: bands of equal
                   scores across the window edge and across two work items, resolved by doc ascending), df 5, df 1
Docs 511 and 512 (W - 1 and W) are in the long lists of every field. Work items hold one window by default and two under
RGPU_FIELDS_WINDOWS_PER_ITEM=2 (read when a context is made)."""
import numpy as np
import pytest

import cross_field as cf
from cross_field import dismax, must, should, term

pytestmark = pytest.mark.gpu

MAX_DOC = cf.W + 37
EDGE = (cf.W - 1, cf.W)
T400, T127, T128, T129, T256, T0, T1 = range(7)            # title
B1, B400, B129, B256, B0, B37, B1L = range(7)              # body
G256, GALL, G5, G1 = range(4)                              # tags
LIVE = ("none", "seeded", "all")


def _fields(rng):
    def lists(dfs, hold):
        return [(cf.spread(rng, MAX_DOC, df, EDGE if df in hold else ()), cf.freqs_of(rng, df)) for df in dfs]
    title = cf.Field(lists((400, 127, 128, 129, 256, 0, 1), (400, 256)), rng.integers(95, 125, size=MAX_DOC), 6 * MAX_DOC)
    body = cf.Field(lists((1, 400, 129, 256, 0, 37, 1), (400, 129)), 60 + rng.permutation(MAX_DOC) % 70, 90 * MAX_DOC)
    tags = cf.Field([(cf.spread(rng, MAX_DOC, 256, EDGE), np.full(256, 3, np.int32)), (np.arange(MAX_DOC, dtype=np.int32), np.full(MAX_DOC, 2, np.int32)),
                     (cf.spread(rng, MAX_DOC, 5), cf.freqs_of(rng, 5)), (cf.spread(rng, MAX_DOC, 1), cf.freqs_of(rng, 1))], None, 3 * MAX_DOC)
    # one doc of both 400-lists whose norm byte differs between the fields: a wrong-field norm changes score bits
    both = np.intersect1d(title.lists[T400][0], body.lists[B400][0])
    assert (title.norms[both] != body.norms[both]).any()
    return [title, body, tags]


_leaves = {}


def _leaf(live="none", version=1):
    if (live, version) not in _leaves:
        rng = np.random.default_rng(77)
        fields = _fields(rng)
        alive = {"none": None, "seeded": np.random.default_rng(3).random(MAX_DOC) < 0.6, "all": np.zeros(MAX_DOC, bool)}[live]
        _leaves[(live, version)] = cf.CrossLeaf(MAX_DOC, fields, alive=alive, version=version)
    return _leaves[(live, version)]


class Gpu:
    """One leaf on the GPU with its fields attached, the per-field sim tables, and a CrossRef"""

    def __init__(self, ctx, oracle, leaf, attach=True):
        import rucene_amd
        self.ctx, self.leaf, self.ref = ctx, leaf, cf.CrossRef(oracle, leaf)
        f0 = leaf.fields[0]
        self.seg = rucene_amd.Segment(ctx, leaf.doc_bytes, f0.norms, leaf.max_doc, live_docs=leaf.live_docs, index_options=2 if f0.has_freqs else 1)
        self.slots = [0]
        if attach:
            for fld in leaf.fields[1:]:
                self.slots.append(self.seg.attach_field(fld.norms, 2 if fld.has_freqs else 1))
        self.tables = []
        for f, fld in enumerate(leaf.fields):
            present = [t for t, (d, _) in enumerate(fld.lists) if d.size]
            self.tables.append(ctx.sim_table(self.ref.weight((f, present[0]))[1], cf.K1))

    def search(self, queries, k, **kw):
        q, g, c = cf.pack(self.ref, queries, self.tables, field_of=lambda f: self.slots[f])
        return self.seg.search_fields_batch(q, g, c, k, **kw)

    def check(self, queries, k, what):
        hits, totals = self.search(queries, k)
        assert hits.shape == (len(queries), k)
        for i, q in enumerate(queries):
            cf.check_row(hits[i], totals[i], self.ref, q, (what, k, i, q))

    def close(self):
        self.seg.close()


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


NINE_GROUPS = [term(0, T400), term(1, B400), term(2, G256), term(0, T129), term(1, B129), term(0, T0), term(1, B37), term(2, G5), term(0, T1)]
NINE_DISJUNCTS = [(0, T400), (1, B1), (1, B400), (2, G256), (0, T127), (1, B0), (2, GALL), (1, B1L), (0, T256)]
QUERIES = [
    # groups: 1, 2, 9; disjuncts: 1, 2, 9; ties 0, 0.1, 1
    should([term(1, B400)]),                                                       # a lone TermQuery of another field
    should([dismax(0.1, [(0, T400), (1, B400)])]),                                 # title:gpu | body:gpu
    should([dismax(0.0, [(0, T400), (1, B400)]), dismax(1.0, [(0, T256), (1, B256)])]),   # the multi-field query
    should([dismax(0.1, [(1, B400)])]),                                            # one disjunct
    should([dismax(0.1, NINE_DISJUNCTS)]),
    should([dismax(1.0, NINE_DISJUNCTS), term(0, T129)]),
    should(NINE_GROUPS),
    should([dismax(0.1, [(0, T0), (1, B129)])]),                                   # one disjunct present in the leaf: that TermScorer
    should([dismax(0.1, [(0, T0), (1, B0)]), term(2, G5)]),                        # a group absent from the leaf drops ...
    should([dismax(0.1, [(0, T0), (1, B0)])]),                                     # ... and a query of absent groups matches nothing
    should([term(0, T1), term(1, B1)]),                                            # two singletons at one file pointer
    should([dismax(0.5, [(1, B1L), (2, G256)])]),                                  # a singleton at the file pointer of a block list
    should([term(0, T127), term(0, T128), term(1, B129), term(2, G256), term(0, T1)]),   # tails of 127, 0, 1 and 0 postings, a singleton
    should([term(2, GALL)]),                                                       # every doc, every score equal
    should([term(2, G256), term(2, GALL)]),                                        # two bands of equal scores
    # min_should_match: 2, n, n + 1; a doc held by two disjuncts of one group counts once
    should([dismax(0.0, [(0, T400), (1, B400)]), term(2, G256), term(0, T129)], msm=2),
    should([dismax(0.0, [(0, T400), (1, B400)]), term(2, G256), term(0, T129)], msm=3),
    should([dismax(0.0, [(0, T400), (1, B400)]), term(2, G256), term(0, T129)], msm=4),
    should([dismax(0.0, [(0, T400), (1, B400)]), term(0, T0), term(0, T129)], msm=3),      # an absent group drops, msm stays: unreachable
    # summation order
    should([term(0, T400), term(1, B400), term(1, B256)]),                         # clause order
    should([term(1, B256), term(1, B400), term(0, T400)]),
    must([term(0, T400), term(1, B400), term(1, B256)]),                           # cost order 256, 400, 400: (c + a) + b
    must([term(1, B400), term(0, T400), term(1, B256)]),                           # equal costs: the stable sort keeps b before a
    must([dismax(0.1, [(0, T129), (1, B129)]), term(0, T256), term(2, GALL)]),     # a dismax group's cost is the sum 258: behind 256
    must([dismax(0.1, [(0, T127), (1, B129)]), term(0, T256), term(2, GALL)]),     # ... 256: equal, clause order keeps it first
    must([term(2, GALL)]),                                                         # one group: that scorer
    must([dismax(0.1, [(0, T400), (1, B400)])], msm=5),                            # min_should_match has no effect
    must([term(1, B400), term(0, T0)]),                                            # a group absent from the leaf: dead
    must([term(1, B400), dismax(0.1, [(0, T0), (1, B0)])]),
    must(NINE_GROUPS[:5] + [term(1, B256)]),
    # exclusion: in the other field, holding the window edge, excluding everything
    should([term(1, B400)], must_not=[(0, T400)]),
    should([dismax(0.1, [(0, T256), (1, B256)])], must_not=[(2, G256), (1, B0), (0, T1)]),
    should([term(0, T400), term(1, B400)], must_not=[(2, GALL)]),
    must([term(0, T400), term(1, B400)], msm=2, must_not=[(2, G256), (1, B37)]),
    must([term(2, GALL), term(0, T256)], must_not=[(0, T0)]),                      # an absent MUST_NOT clause drops
]


@pytest.mark.parametrize("live", LIVE)
@pytest.mark.parametrize("version", [1, 0], ids=["bp128", "legacy"])
def test_every_query(ctx, oracle, live, version):
    """The whole query set in one batch, k = 10 and 128 (the wide lists), both .doc formats, without deletions, with seeded ones and
    with every doc deleted"""
    g = Gpu(ctx, oracle, _leaf(live, version))
    try:
        info = [g.seg.field_info(s) for s in g.slots]
        assert [i["norm_mode"] for i in info] == [1, 2, 0] and info[0]["n_norm_ranks"] == np.unique(g.leaf.fields[0].norms).size
        assert [i["norms_bytes"] for i in info] == [MAX_DOC, MAX_DOC, 0] and info[1]["n_norm_ranks"] == 0
        assert all(i["index_options"] == 2 and i["skip_values"] == 2 for i in info)
        for k in (10, 128):
            g.check(QUERIES, k, (live, version))
    finally:
        g.close()


def test_a_batch_of_dead_queries(ctx, oracle):
    """Every query is dead in the leaf: no clause is walked, no run is scored (no k_score_terms launch), the rows are padding"""
    g = Gpu(ctx, oracle, _leaf("seeded"))
    try:
        dead = [should([dismax(0.1, [(0, T0), (1, B0)])]), must([term(1, B400), term(0, T0)]), should([term(0, T0), term(1, B0)], must_not=[(2, GALL)]),
                should([dismax(0.0, [(0, T400), (1, B400)]), term(0, T0)], msm=2)]
        assert [g.ref.rows(q)[2] for q in dead] == [0, 0, 0, 0]
        for k in (1, 10, 128):
            ctx.kernel_stats_reset()
            hits, totals = g.search(dead, k)
            assert (totals == 0).all() and (hits["doc"] == -1).all() and (hits["score"] == 0).all()
            stats = ctx.kernel_stats()
            assert not [n for n in stats if n.startswith("k_score_terms") and stats[n]["launches"]] and stats["k_fields_windows"]["launches"] == 1
        g.check(dead[:2] + QUERIES[:2], 10, "dead rows beside live ones")
    finally:
        g.close()


def test_the_fixture_is_what_the_names_say(oracle):
    leaf = _leaf()
    t, b, gs = leaf.fields
    assert t.terms[T1]["doc_start_fp"] == b.terms[B1]["doc_start_fp"] and t.terms[T1]["doc_freq"] == b.terms[B1]["doc_freq"] == 1
    assert b.terms[B1L]["doc_start_fp"] == gs.terms[G256]["doc_start_fp"] and gs.terms[G256]["doc_freq"] == 256
    assert np.unique(t.norms).size <= 64 < np.unique(b.norms).size
    for fld, tid in ((t, T400), (t, T256), (b, B400), (b, B129), (gs, G256), (gs, GALL)):
        assert set(EDGE) <= set(fld.lists[tid][0].tolist())
    ref = cf.CrossRef(oracle, leaf)
    assert ref.weight((0, T400))[1].tobytes() != ref.weight((1, B400))[1].tobytes()          # different average lengths
    d, s, n = ref.rows(should([term(2, G256), term(2, GALL)]))
    assert n == MAX_DOC and np.unique(s).size == 2 and (np.diff(d[:256]) > 0).all() and d[255] > cf.W > d[0]   # a band across the edge
    # the orders the queries name differ from one another in score bits
    a = ref.scores(should([term(0, T400), term(1, B400), term(1, B256)]))[1]
    c = ref.scores(should([term(1, B256), term(1, B400), term(0, T400)]))[1]
    assert (a.view(np.int32) != c.view(np.int32)).any()
    q = must([term(0, T400), term(1, B400), term(1, B256)])
    assert [x[2] for x in ref.order(q)] == [256, 400, 400]
    assert (ref.scores(q)[1].view(np.int32) != ref.scores(q, order=[ref.group(x) for x in q["groups"]])[1].view(np.int32)).any()
    assert [x[2] for x in ref.order(must([dismax(0.1, [(0, T129), (1, B129)]), term(0, T256), term(2, GALL)]))] == [256, 258, MAX_DOC]
    # the maximum of a dismax pair sits in the first disjunct on some docs and in the last on others
    da, sa = ref.clause((0, T400))
    db, sb = ref.clause((1, B400))
    both, ia, ib = np.intersect1d(da, db, return_indices=True)
    assert (sa[ia] > sb[ib]).any() and (sa[ia] < sb[ib]).any()


@pytest.mark.parametrize("live", ("none", "seeded"))
def test_k_around_the_hit_count(ctx, oracle, live):
    """k = 1, hits - 1, hits, hits + 1, 128 (fewer docs than k) on rows of a few hits; bands of equal scores cut at every k"""
    g = Gpu(ctx, oracle, _leaf(live))
    try:
        small = [should([term(2, G5), term(0, T1)]), must([term(1, B37), term(0, T400)]), should([term(2, G256)], must_not=[(0, T400)])]
        for q in small:
            hits = g.ref.rows(q)[2]
            for k in sorted({1, max(1, hits - 1), max(1, hits), hits + 1, 128}):
                if k <= 128:
                    g.check([q], k, ("small", live))
        ties = [should([term(2, GALL)]), should([term(2, G256), term(2, GALL)]), must([term(2, GALL), term(2, G256)])]
        for k in (1, 2, 63, 64, 65, 127, 128):
            g.check(ties, k, ("ties", live))
    finally:
        g.close()


def test_two_windows_per_item(oracle, monkeypatch):
    """RGPU_FIELDS_WINDOWS_PER_ITEM=2: both windows in one work item (the cursors carry over); the default is one window per item"""
    import rucene_amd
    monkeypatch.setenv("RGPU_FIELDS_WINDOWS_PER_ITEM", "2")
    c = rucene_amd.Context(profile_kernels=True)
    try:
        for live in ("none", "seeded"):
            g = Gpu(c, oracle, _leaf(live))
            try:
                g.check(QUERIES, 10, ("two-per-item", live))
                g.check(QUERIES[12:16], 128, ("two-per-item", live))
            finally:
                g.close()
    finally:
        c.close()


def test_three_leaves_whose_cost_orders_differ(ctx, oracle):
    """The same MUST query over three leaves in which the three lists swap their lengths: the library sorts per leaf"""
    q = must([term(0, 0), term(1, 0), dismax(0.3, [(0, 1), (1, 1)])])
    orders = set()
    for n, dfs in enumerate(((300, 200, 40, 50), (100, 250, 200, 100), (200, 90, 30, 59))):
        rng = np.random.default_rng(n)
        max_doc = 300 + 130 * n
        a = cf.Field([(cf.spread(rng, max_doc, dfs[0]), cf.freqs_of(rng, dfs[0])), (cf.spread(rng, max_doc, dfs[2]), cf.freqs_of(rng, dfs[2]))],
                     rng.integers(100, 124, size=max_doc), 7 * max_doc)
        b = cf.Field([(cf.spread(rng, max_doc, dfs[1]), cf.freqs_of(rng, dfs[1])), (cf.spread(rng, max_doc, dfs[3]), cf.freqs_of(rng, dfs[3]))],
                     rng.integers(60, 140, size=max_doc), 70 * max_doc)
        g = Gpu(ctx, oracle, cf.CrossLeaf(max_doc, [a, b]))
        try:
            orders.add(tuple(x[2] for x in g.ref.order(q)))
            assert g.ref.rows(q)[2] > 0
            g.check([q, should(q["groups"], msm=2)], 10, ("leaf", n))
        finally:
            g.close()
    assert orders == {(90, 200, 300), (100, 250, 300), (89, 90, 200)}


def test_a_docs_only_field_without_norms(ctx, oracle):
    """field 1 is indexed with IndexOptions::Docs and omits norms (like the golden directory's `id`): every freq reads 1"""
    rng = np.random.default_rng(12)
    max_doc = 640
    body = cf.Field([(cf.spread(rng, max_doc, df), cf.freqs_of(rng, df)) for df in (300, 1, 129)], rng.integers(100, 124, size=max_doc), 40 * max_doc)
    ident = cf.Field([(cf.spread(rng, max_doc, df), np.ones(df, np.int32)) for df in (129, 1, 7, 256)], None, -1)
    for version in (1, 0):
        leaf = cf.docs_only_leaf(oracle, max_doc, body, ident, alive=rng.random(max_doc) < 0.7, version=version)
        g = Gpu(ctx, oracle, leaf)
        try:
            assert g.seg.field_info(1) == dict(norms_bytes=0, norm_mode=0, n_norm_ranks=0, index_options=1, skip_values=2)
            g.check([should([dismax(0.1, [(0, 0), (1, 3)]), term(1, 2)]), must([term(1, 0), term(0, 0)], must_not=[(1, 1)]),
                     should([term(1, 1), term(0, 1), term(1, 3)], msm=2), should([term(1, 0)])], 10, ("docs-only", version))
        finally:
            g.close()


def _untouched(g, q, gr, c, k, status):
    from rucene_amd import _lib
    hits = np.full((max(len(q), 1), max(k, 1)), 7, dtype=np.int64).view(_lib.HIT_DTYPE)
    totals = np.full(max(len(q), 1), -99, dtype=np.int64)
    before = hits.tobytes()
    with pytest.raises(_lib.RgpuError) as e:
        g.seg.search_fields_batch(q, gr, c, k, hits=hits, totals=totals)
    assert e.value.status == status, (e.value, status)
    assert hits.tobytes() == before and (totals == -99).all()


def test_refusals_leave_the_outputs_untouched(ctx, oracle):
    from rucene_amd import _lib
    g = Gpu(ctx, oracle, _leaf())
    UNSUPPORTED, ILLEGAL = -5, -2
    try:
        def packed(queries):
            return cf.pack(g.ref, queries, g.tables, field_of=lambda f: g.slots[f])
        ten = [term(0, T400)] * 10
        _untouched(g, *packed([should(ten)]), 10, UNSUPPORTED)
        _untouched(g, *packed([should([dismax(0.1, [(0, T400)] * 10)])]), 10, UNSUPPORTED)
        _untouched(g, *packed([should([term(0, T400)])]), 129, UNSUPPORTED)
        _untouched(g, *packed([should([term(0, T400)])]), 0, ILLEGAL)
        _untouched(g, *packed([should([term(0, T400), term(1, B400)], msm=2, must_not=[(2, G5)])]), 10, UNSUPPORTED)
        q, gr, c = packed([should([term(0, T400), term(1, B400)])])
        for occur, status in ((_lib.OCCUR_MUST | _lib.OCCUR_SHOULD, UNSUPPORTED), (_lib.OCCUR_FILTER, UNSUPPORTED), (_lib.OCCUR_MUST | _lib.OCCUR_FILTER, UNSUPPORTED),
                              (0, ILLEGAL)):
            q2 = q.copy()
            q2["occur"] = occur
            _untouched(g, q2, gr, c, 10, status)
        q2 = q.copy()
        q2["n_groups"] = 0
        _untouched(g, q2, gr, c, 10, ILLEGAL)                                   # zero groups
        c2 = c.copy()
        c2["field"][1] = 3
        _untouched(g, q, gr, c2, 10, ILLEGAL)                                   # a field slot that is not attached
        c2["field"][1] = -1
        _untouched(g, q, gr, c2, 10, ILLEGAL)
        q3, g3, c3 = packed([should([dismax(0.1, [(0, T400), (1, B400)])])])
        for bad in (np.inf, -np.inf, np.nan):
            g4 = g3.copy()
            g4["tie_bits"] = np.float32(bad).view(np.uint32)
            _untouched(g, q3, g4, c3, 10, ILLEGAL)                               # a non-finite tie
        # a term prepared under one field and named under another
        c5 = c.copy()
        c5["field"][1] = 0
        g.search([should([term(1, B400)])], 10)
        _untouched(g, q, gr, c5, 10, ILLEGAL)
        g.check(QUERIES[:3], 10, "after the refusals")
        # one doc_start_fp under two fields in ONE batch, on an empty store: refused before anything is prepared - nothing is filed
        # under the wrong slot, and the same term under its true field is served right afterwards
        g.seg.release_prepared_terms()
        q6, g6, c6 = packed([should([term(0, T256), term(1, B256), term(1, B256)])])
        c6["field"][2] = 0
        _untouched(g, q6, g6, c6, 10, ILLEGAL)
        c6["field"][1], c6["field"][2] = 0, 1
        _untouched(g, q6, g6, c6, 10, ILLEGAL)
        assert g.seg.footprint()["prepared_terms"] == 0
        g.check([should([term(0, T256), term(1, B256)])] + QUERIES[:3], 10, "after a batch that named a term under two fields")
        # a ninth field is one too many
        extra = [g.seg.attach_field(None, 1) for _ in range(_lib.MAX_FIELDS - 1 - 2)]
        assert extra == [3, 4, 5, 6, 7]
        with pytest.raises(_lib.RgpuError) as e:
            g.seg.attach_field(None, 1)
        assert e.value.status == UNSUPPORTED
    finally:
        g.close()


def _single_field_batch(g):
    """TERM, AND, OR (msm, MUST_NOT) and dismax rows over field 0 for rgpu_search_batch / rgpu_count_batch"""
    from rucene_amd import _lib
    t0 = g.leaf.fields[0]
    rows = [(0, [T400], 0), (1, [T400, T256, T129], 0), (2, [T400, T127, T1, T0], 0), (2 | (2 << 8), [T400, T256, T128], 0),
            (2, [T400, T129], 1), (_lib.OP_DISMAX, [T400, T256], int(np.float32(0.1).view(np.int32)))]
    q = np.zeros(len(rows), _lib.QUERY_DTYPE)
    terms = []
    for i, (op, tids, extra) in enumerate(rows):
        q[i] = (op, len(tids) - (extra if op != _lib.OP_DISMAX else 0), len(terms), extra)
        for t in tids:
            row = np.zeros(1, _lib.QUERY_TERM_DTYPE)[0]
            row["state"], row["weight"], row["sim_table"] = t0.terms[t], g.ref.weight((0, t))[0], g.tables[0]
            terms.append(row)
    return q, np.array(terms, _lib.QUERY_TERM_DTYPE)


def test_existing_entry_points_do_not_see_attached_fields(ctx, oracle):
    """rgpu_search_batch and rgpu_count_batch on field 0: the same bytes on a leaf without fields, with fields attached, and after a
    cross-field search has prepared other fields' terms; the new call launches k_fields_windows and no k_or_windows"""
    plain = Gpu(ctx, oracle, _leaf("seeded"), attach=False)
    g = Gpu(ctx, oracle, _leaf("seeded"))
    try:
        q, t = _single_field_batch(g)
        want = [plain.seg.search_batch(q, t, k) for k in (10, 129)] + [plain.seg.count_batch(q, t)]
        assert want[0][1].sum() > 0
        for stage in ("attached", "after a cross-field search"):
            got = [g.seg.search_batch(q, t, k) for k in (10, 129)] + [g.seg.count_batch(q, t)]
            for (wh, wt), (gh, gt) in zip(want[:2], got[:2]):
                assert wh.tobytes() == gh.tobytes() and (wt == gt).all(), stage
            assert (want[2] == got[2]).all(), stage
            ctx.kernel_stats_reset()
            g.check(QUERIES[:6], 10, stage)
            stats = ctx.kernel_stats()
            assert stats["k_fields_windows"]["launches"] == 1 and stats["k_merge_items"]["launches"] == 1
            assert {n for n in stats if n.startswith("k_score_terms")} == {"k_score_terms(field 0)", "k_score_terms(field 1)", "k_score_terms(field 2)"}
            assert not [n for n in stats if n.startswith("k_or_")]
        assert plain.seg.footprint()["norms_bytes"] == g.seg.footprint()["norms_bytes"] == MAX_DOC
    finally:
        plain.close()
        g.close()


def test_the_prepared_store_can_be_dropped(ctx, oracle):
    """rgpu_segment_release_prepared_terms, then the same batch: the same rows; explicit preparation per field beforehand changes nothing"""
    g = Gpu(ctx, oracle, _leaf("seeded"))
    try:
        for f, fld in enumerate(g.leaf.fields):
            g.seg.prepare_field_terms(g.slots[f], fld.terms)
        n_prepared = g.seg.footprint()["prepared_terms"]
        assert n_prepared == sum(int((fld.terms["doc_freq"] >= 2).sum()) for fld in g.leaf.fields)
        first = g.search(QUERIES, 10)
        g.seg.release_prepared_terms()
        assert g.seg.footprint()["prepared_terms"] == 0
        again = g.search(QUERIES, 10)
        assert first[0].tobytes() == again[0].tobytes() and (first[1] == again[1]).all()
        g.check(QUERIES, 10, "after the release")
        from rucene_amd import _lib
        with pytest.raises(_lib.RgpuError) as e:   # a term belongs to one field
            g.seg.prepare_field_terms(0, g.leaf.fields[1].terms[B400:B400 + 1])
        assert e.value.status == -2
    finally:
        g.close()


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------------
def _mirror_query(q):
    """A cross_field query dict as the Python mirror's query objects: field 0 is the primary field `title`"""
    import rucene_amd
    names = (None, "body", "tags")
    T, B, D = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery

    def clause(g):
        return T(g[1][1], field=names[g[1][0]]) if g[0] == "term" else D([T(t, field=names[f]) for f, t in g[2]], g[1])
    groups = [clause(g) for g in q["groups"]]
    nots = [T(t, field=names[f]) for f, t in q["must_not"]]
    if len(groups) == 1 and not nots and q["msm"] <= 1:
        return groups[0]
    return B(groups, [], 0, nots) if q["occur"] == "must" else B([], groups, max(1, q["msm"]), nots)


def test_python_mirror_over_four_leaves(ctx, oracle):
    """GpuIndexSearcher: TermQuery(field=...) routes to rgpu_search_fields_batch; idf and the norm cache are per field, from the
    statistics leaf (the largest); presence and the MUST cost order are per leaf; rows merge under the canonical tie rule. Rows that
    name the primary field alone ride in the same batch and go where they went."""
    import rucene_amd
    sizes = (300, 1100, 130, MAX_DOC)
    leaves = []
    for n, max_doc in enumerate(sizes):
        rng = np.random.default_rng([n, 9])
        def lists(fracs):
            return [(cf.spread(rng, max_doc, max(0, int(max_doc * fr))), cf.freqs_of(rng, max(0, int(max_doc * fr)))) for fr in fracs]
        absent_here = 0.0 if n == 2 else 0.3   # body term 3 has no postings in leaf 2
        title = cf.Field(lists((0.7, 0.25, 0.5, 0.01)), rng.integers(100, 124, size=max_doc), (5 + n) * max_doc)
        body = cf.Field(lists((0.5, 0.6 if n % 2 else 0.1, 0.24, absent_here)), 60 + rng.permutation(max_doc) % 70, (60 + 9 * n) * max_doc)
        tags = cf.Field(lists((0.4, 0.05)), None, 2 * max_doc)
        alive = None if n == 0 else rng.random(max_doc) < 0.8
        leaves.append(cf.CrossLeaf(max_doc, [title, body, tags], alive=alive))
    refs = cf.index_refs(oracle, leaves)
    queries = [should([dismax(0.1, [(0, 0), (1, 0)]), dismax(0.1, [(0, 1), (1, 1)])]), should([term(1, 2)]), must([term(0, 0), term(1, 1), term(2, 0)]),
               must([dismax(0.5, [(0, 1), (1, 3)]), term(1, 0)]), should([term(0, 2), term(1, 2), term(2, 1)], msm=2),
               should([dismax(0.0, [(0, 3), (1, 3)])], must_not=[(2, 0)]), must([term(1, 3), term(0, 0)])]
    assert len({tuple(np.argsort([r.df((0, 0)), r.df((1, 1)), r.df((2, 0))], kind="stable")) for r in refs}) > 1   # the cost orders differ
    gl = []
    for leaf in leaves:
        t, b, g = leaf.fields
        lr = rucene_amd.LeafReader(leaf.doc_bytes, t.norms, leaf.max_doc, t.terms, doc_base=leaf.doc_base, live_docs=leaf.live_docs,
                                   sum_total_term_freq=t.sttf, field="title")
        lr.add_field("body", b.norms, b.terms, sum_total_term_freq=b.sttf)
        lr.add_field("tags", g.norms, g.terms, sum_total_term_freq=g.sttf)
        gl.append(lr)
    s = rucene_amd.GpuIndexSearcher(gl, ctx=ctx)
    try:
        assert [leaf.segment.field_info(leaf.extra_fields["body"].slot)["norm_mode"] for leaf in gl] == [2, 2, 2, 2]
        T = rucene_amd.TermQuery
        plain = [T(0), rucene_amd.BooleanQuery.build([], [T(0), T(2)])]
        for k in (10, 128):
            hits, totals = s.search_batch([_mirror_query(q) for q in queries] + plain, k)
            alone = s.search_batch(plain, k)
            assert hits[len(queries):].tobytes() == alone[0].tobytes() and (totals[len(queries):] == alone[1]).all()
            for i, q in enumerate(queries):
                d, sc, tot = cf.index_rows(refs, q, k)
                assert totals[i] == tot and (hits[i]["doc"][:d.size] == d).all() and (hits[i]["doc"][d.size:] == -1).all(), (k, i)
                assert (hits[i]["score"][:d.size].view(np.int32) == sc.view(np.int32)).all(), (k, i)
        # what the call cannot express is the CPU path's
        B, D = rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery
        for q in (B([T(0, field="body")], [T(1)], 0), B([T(0, field="body")], [], 0, [], [T(1)]), B([], [T(i % 3, field="body") for i in range(10)], 1),
                  D([T(i % 3, field="body") for i in range(10)], 0.1), B([], [T(0, field="body"), T(1)], 2, [T(2)]),
                  rucene_amd.BoostingQuery.build(T(0, field="body"), T(1), 0.5)):
            with pytest.raises(rucene_amd.RgpuError) as e:
                s.search_batch([q], 10)
            assert e.value.status == -5, str(q)
        with pytest.raises(rucene_amd.RgpuError) as e:
            s.search_batch([T(0, field="nope")], 10)
        assert e.value.status == -2
        with pytest.raises(rucene_amd.RgpuError) as e:
            s.search_batch([T(0, field="body")], 129)
        assert e.value.status == -5
        seen = []
        s.cpu_fallback = lambda query, collector: seen.append(query)
        q = B([T(0, field="body")], [T(1)], 0)
        s.search(q, rucene_amd.TopDocsCollector(10))
        assert seen == [q]
    finally:
        for leaf in gl:
            leaf.segment.close()


def test_the_golden_directory_with_its_id_field(ctx):
    """open_directory(tests/golden/dir, extra_fields=["id"]): `id` is indexed with IndexOptions::Docs, omits norms and holds no postings
    in this segment - a disjunct in it drops out, a MUST clause in it leaves nothing"""
    import os
    import rucene_amd
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dir")
    leaves = rucene_amd.open_directory(root, field="body", extra_fields=["id"])
    plain_leaves = rucene_amd.open_directory(root, field="body")
    s = rucene_amd.GpuIndexSearcher(leaves, ctx=ctx)
    p = rucene_amd.GpuIndexSearcher(plain_leaves, ctx=ctx)
    try:
        xf = leaves[0].extra_fields["id"]
        assert xf.slot == 1 and xf.norms is None and xf.index_options == 1
        assert leaves[0].segment.field_info(1) == dict(norms_bytes=0, norm_mode=0, n_norm_ranks=0, index_options=1, skip_values=2)
        T, B, D = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery
        both = D([T(b"w001"), T(b"w001", field="id")], 0.1)
        hits, totals = s.search_batch([both, B([T(b"w003"), T(b"w003", field="id")], [], 0), B([], [both, D([T(b"w002", field="id"), T(b"w002")], 0.0)], 1)], 10)
        want = p.search_batch([T(b"w001"), B.build([], [T(b"w001"), T(b"w002")])], 10)
        assert totals[0] == want[1][0] > 0 and hits[0].tobytes() == want[0][0].tobytes()     # one disjunct left: that TermScorer
        assert totals[1] == 0 and (hits[1]["doc"] == -1).all()
        assert totals[2] == want[1][1] and hits[2].tobytes() == want[0][1].tobytes()         # 0.0f + a + b, as the OR sums
    finally:
        for leaf in leaves + plain_leaves:
            leaf.segment.close()


def test_a_positions_field_attached_beside_a_phrase_on_field_0(ctx):
    """A DocsAndFreqsAndPositions segment (skip entries of four values, a position cell per directory slot): some of its terms are
    declared as a further field `alt` with the same index options, norms and statistics. A phrase call on field 0 returns the same
    bytes with the field attached, and after a cross-field search has prepared `alt`'s terms; the cross-field rows over `alt` equal
    rgpu_search_batch's over the same lists on a plain upload (same norms and weights: the same f32 sums)."""
    import rucene_amd
    from rucene_amd import indexgen
    rng = np.random.default_rng(31)
    max_doc = 900
    postings = []
    for df in (300, 280, 129, 400, 257, 1):
        docs = cf.spread(rng, max_doc, df, (5, 6) if df >= 280 else ())
        postings.append([(int(d), np.sort(rng.choice(40, size=int(rng.integers(1, 6)), replace=False)).tolist()) for d in docs])
    norms = rng.integers(100, 124, size=max_doc).astype(np.uint8)
    seg = indexgen.build_explicit_positions(max_doc, postings, norms=norms)
    T, B, D, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery, rucene_amd.PhraseQuery
    plain = rucene_amd.LeafReader.from_synthetic_positions(seg)
    fielded = rucene_amd.LeafReader.from_synthetic_positions(seg)
    fielded.add_field("alt", norms, seg.terms, doc_count=plain.doc_count, sum_total_term_freq=plain.sum_total_term_freq, index_options=3)
    p = rucene_amd.GpuIndexSearcher([plain], ctx=ctx)
    s = rucene_amd.GpuIndexSearcher([fielded], ctx=ctx)
    try:
        assert fielded.segment.field_info(1) == dict(norms_bytes=max_doc, norm_mode=1, n_norm_ranks=np.unique(norms).size, index_options=3, skip_values=4)
        phrases = [P([0, 1]), P([1, 0], slop=2), P([2, 0])]
        want = p.search_batch(phrases, 10)
        assert want[1].sum() > 0
        got = s.search_batch(phrases, 10)
        assert got[0].tobytes() == want[0].tobytes() and (got[1] == want[1]).all()
        cross = s.search_batch([B.build([], [T(3, field="alt"), T(4, field="alt"), T(5, field="alt")]), B.build([T(4, field="alt"), T(3, field="alt")], []),
                                T(3, field="alt")], 10)
        flat = p.search_batch([B.build([], [T(3), T(4), T(5)]), B.build([T(4), T(3)], []), T(3)], 10)
        assert cross[1].tolist() == flat[1].tolist() and cross[1].min() > 0
        assert cross[0].tobytes() == flat[0].tobytes()
        got = s.search_batch(phrases, 10)   # field 0's position cells were not disturbed by the other field's preparation
        assert got[0].tobytes() == want[0].tobytes() and (got[1] == want[1]).all()
    finally:
        plain.segment.close()
        fielded.segment.close()


def test_the_same_term_bytes_in_two_fields(ctx, oracle):
    """One block-tree dictionary holds the words w000 .. under TWO field numbers: the same bytes resolve to two different lists, scored
    with two different norms arrays and statistics. (One norms file holds one field here: `title` is declared without norms in the
    field infos and handed its norm bytes directly.)"""
    import rucene_amd
    rng = np.random.default_rng(41)
    max_doc = 700
    dfs = (300, 129, 1, 256, 40)
    def field(norms):
        lists = [(cf.spread(rng, max_doc, df), cf.freqs_of(rng, df)) for df in dfs]
        return cf.Field(lists, norms, sum(int(f.sum()) for _, f in lists))
    body = field(60 + rng.permutation(max_doc) % 70)
    title = field(rng.integers(110, 124, size=max_doc))
    alive = rng.random(max_doc) < 0.8
    leaf = cf.CrossLeaf(max_doc, [body, title], alive=alive)
    ref = cf.CrossRef(oracle, leaf)
    words = [b"w%03d" % t for t in range(len(dfs))]

    def states(fld):
        st = np.zeros(len(dfs), dtype=oracle.FULL_TERM_STATE_DTYPE)
        st["base"] = fld.terms
        st["last_pos_block_offset"] = -1
        return st
    tim, tip = oracle.blocktree_write([dict(number=0, doc_count=max_doc, terms=words, states=states(body)),
                                       dict(number=3, doc_count=max_doc, terms=words, states=states(title))])
    nvm, nvd = oracle.norms_write(body.norms.astype(np.int64), field_number=0)
    fnm = oracle.field_infos_write([dict(name="body", number=0, index_options=2), dict(name="title", number=3, index_options=2, omit_norms=True)])
    lr = rucene_amd.LeafReader.from_index_files(leaf.doc_bytes, tim, tip, nvm, nvd, max_doc, field="body", fnm=fnm, extra_fields=["title"],
                                                liv=oracle.live_docs_write(leaf.live_docs, max_doc, int(max_doc - alive.sum()), gen=1),
                                                del_count=int(max_doc - alive.sum()))
    xf = lr.extra_fields["title"]
    assert xf.field_number == 3 and xf.sum_total_term_freq == title.sttf and lr.sum_total_term_freq == body.sttf
    xf.norms = title.norms
    a, b = lr.term_state(words[0]), xf.term_state(words[0])
    assert a["doc_start_fp"] != b["doc_start_fp"] and a["doc_freq"] == b["doc_freq"] == 300
    s = rucene_amd.GpuIndexSearcher([lr], ctx=ctx)
    try:
        T, B, D = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery
        both = lambda t, tie: D([T(words[t]), T(words[t], field="title")], tie)
        queries = [(both(0, 0.1), should([dismax(0.1, [(0, 0), (1, 0)])])),
                   (B([], [both(0, 0.0), both(3, 1.0)], 1), should([dismax(0.0, [(0, 0), (1, 0)]), dismax(1.0, [(0, 3), (1, 3)])])),
                   (T(words[1], field="title"), should([term(1, 1)])),
                   (B([T(words[0], field="title"), T(words[0]), T(words[3], field="title")], [], 0), must([term(1, 0), term(0, 0), term(1, 3)])),
                   (B([], [both(2, 0.5), T(words[4], field="title")], 1, [T(words[4])]), should([dismax(0.5, [(0, 2), (1, 2)]), term(1, 4)], must_not=[(0, 4)]))]
        hits, totals = s.search_batch([q for q, _ in queries], 10)
        for i, (_, spec) in enumerate(queries):
            cf.check_row(hits[i], totals[i], ref, spec, ("same bytes", i))
        assert totals[0] > 300 and totals[3] > 0
    finally:
        lr.segment.close()


def test_cpp_demo_rows(oracle, tmp_path):
    """tests/cpp/cross_field_demo.cpp: the C++ mirror's routing (TermQuery::field, LeafReader::extra_fields, MultiFieldQuery) on the
    three-field leaf - the lines it prints are tests/cross_field.py's rows, and what the call cannot express reaches the CPU hooks"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cross_field_demo")
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "cpp", "cross_field_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    leaf = _leaf()
    ref = cf.CrossRef(oracle, leaf)
    (tmp_path / "doc.bin").write_bytes(np.asarray(leaf.doc_bytes).tobytes())
    for f, fld in enumerate(leaf.fields):
        (tmp_path / ("norms%d.bin" % f)).write_bytes(b"" if fld.norms is None else fld.norms.tobytes())
        (tmp_path / ("terms%d.bin" % f)).write_bytes(np.ascontiguousarray(fld.terms).tobytes())
    out = subprocess.check_output([exe, str(tmp_path), str(leaf.max_doc)] + [str(fld.sttf) for fld in leaf.fields], text=True).strip().splitlines()
    specs = [should([dismax(0.1, [(0, T400), (1, B400)])]), should([dismax(0.0, [(0, T400), (1, B400)]), dismax(1.0, [(0, T256), (1, B256)])]),
             should([term(0, T400)]), should([term(1, B400)]), must([term(0, T400), term(1, B400), term(1, B256)]),
             should([term(0, T400), term(1, B400)], must_not=[(2, G256)]),
             must([dismax(0.1, [(0, T129), (1, B129)]), term(0, T256), term(2, GALL)]),
             should([dismax(0.0, [(0, T400), (1, B400)]), term(2, G256), term(0, T129)], msm=2), should([dismax(0.1, [(0, T0), (1, B0)])])]
    assert len(out) == len(specs) + 2, out
    for i, line in enumerate(out[:-1]):
        spec = specs[i] if i < len(specs) else specs[1]   # the last row line: the multi-field query through search() and a collector
        parts = line.split()
        d, sc, total = ref.rows(spec, 10)
        assert parts[0] == "cross" and int(parts[1]) == i and int(parts[2]) == total, line
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        assert [x[0] for x in got] == d.tolist() and [x[1] for x in got] == sc.view(np.uint32).tolist(), line
    # two cross-field trees the call cannot express + a phrase-boolean, a phrase disjunction, a phrase and a span query with a term of `body`
    assert out[-1] == "fallback 6 count -7 cache_filter 1 unknown 1 rescore 1", out[-1]
