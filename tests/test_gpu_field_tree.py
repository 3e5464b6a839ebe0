"""Cross-field query-string trees on the GPU (`-m gpu`): rgpu_search_fields_tree_batch through the C ABI's Python binding and through
GpuIndexSearcher(field_trees=True), against tests/field_tree.py (which tests/test_field_tree_cpu.py ties to the oracle's own
searches and to its mutants). Everything is compared bit for bit: doc ids, score bits, -1 padding, hit counts.

The leaf is field_tree.TreeLeaf: 4099 docs (eight 512-doc windows and a last one of 3), title in rank mode, body in raw mode, tags
without norms; both .doc formats; without and with deletions. Work items hold one window by default, three or all nine under
RGPU_FIELDS_WINDOWS_PER_ITEM (read when a context is made)."""
import numpy as np
import pytest

import cross_field as cf
import field_tree as ft
from field_tree import T, dismax, sum_, term, tree

pytestmark = pytest.mark.gpu

UNSUPPORTED, ILLEGAL = -5, -2


class Gpu:
    """One leaf on the GPU with its fields attached, the per-field sim tables, and a TreeRef"""

    def __init__(self, ctx, oracle, leaf):
        import rucene_amd
        self.ctx, self.leaf, self.ref = ctx, leaf, ft.TreeRef(oracle, leaf)
        f0 = leaf.fields[0]
        self.seg = rucene_amd.Segment(ctx, leaf.doc_bytes, f0.norms, leaf.max_doc, live_docs=leaf.live_docs, index_options=2 if f0.has_freqs else 1)
        self.slots = [0] + [self.seg.attach_field(fld.norms, 2 if fld.has_freqs else 1) for fld in leaf.fields[1:]]
        self.tables = []
        for f, fld in enumerate(leaf.fields):
            present = [t for t, (d, _) in enumerate(fld.lists) if d.size]
            self.tables.append(ctx.sim_table(self.ref.weight((f, present[0]))[1], cf.K1))

    def packed(self, queries):
        return ft.pack(self.ref, queries, self.tables, field_of=lambda f: self.slots[f])

    def search(self, queries, k, **kw):
        return self.seg.search_fields_tree_batch(*self.packed(queries), k, **kw)

    def check(self, queries, k, what, rule=True):
        hits, totals = self.search(queries, k)
        assert hits.shape == (len(queries), k)
        for i, q in enumerate(queries):
            ft.check_row(hits[i], totals[i], self.ref, q, (what, k, i), rule=rule)

    def close(self):
        self.seg.close()


@pytest.fixture(scope="module", params=[0, -1], ids=["rule", "add"])
def ctx(request):
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True, req_opt_rule=request.param)
    c.rule = request.param == 0
    yield c
    c.close()


@pytest.fixture(scope="module")
def rule_ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


def _all_queries():
    return list(ft.rule_queries().items()) + list(ft.sum_queries().items()) + list(ft.emission_queries().items())


@pytest.mark.parametrize("live", ("none", "seeded"))
@pytest.mark.parametrize("version", [1, 0], ids=["bp128", "legacy"])
def test_every_query(ctx, oracle, live, version):
    """The rule sequences, the sum-group queries and the emission queries in one batch, in both rule modes: k = 10 and the wide lists"""
    g = Gpu(ctx, oracle, ft.TreeLeaf(live, version))
    try:
        assert [g.seg.field_info(s)["norm_mode"] for s in g.slots] == [1, 2, 0]
        queries = [q for _, q in _all_queries()]
        for k in (10, 128):
            g.check(queries, k, (live, version), rule=ctx.rule)
    finally:
        g.close()


def test_every_query_alone_and_the_answering_kernels(rule_ctx, oracle):
    """One query per call: the kernels that answer a required/optional query under the rule are k_fields_tree_windows and
    k_req_opt_scan (no k_merge_items), every other one k_fields_tree_windows and k_merge_items; never k_fields_windows"""
    g = Gpu(rule_ctx, oracle, ft.TreeLeaf("seeded"))
    try:
        for name, q in _all_queries():
            rule_ctx.kernel_stats_reset()
            g.check([q], 10, name)
            stats = {n: s["launches"] for n, s in rule_ctx.kernel_stats().items() if s["launches"]}
            both = bool(q["must"]) and any(g.ref.group(x) is not None for x in q["should"]) and all(g.ref.group(x) is not None for x in q["must"])
            assert stats.get("k_fields_tree_windows") == 1 and "k_fields_windows" not in stats, (name, stats)
            assert ("k_req_opt_scan" in stats, "k_merge_items" in stats) == ((True, False) if both else (False, True)), (name, stats)
    finally:
        g.close()


def test_add_mode_is_one_pass(oracle):
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True, req_opt_rule=-1)
    g = Gpu(c, oracle, ft.TreeLeaf("none"))
    try:
        q = ft.rule_queries()["KEEPS_STATE"]
        c.kernel_stats_reset()
        g.check([q], 10, "add", rule=False)
        stats = {n for n, s in c.kernel_stats().items() if s["launches"]}
        assert "k_req_opt_scan" not in stats and {"k_fields_tree_windows", "k_merge_items"} <= stats
        assert g.ref.rows(q, 128)[1].tobytes() != g.ref.rows(q, 128, rule=False)[1].tobytes()     # (the rule would have changed the row)
        g.check([q], 128, "add", rule=False)
    finally:
        g.close()
        c.close()


@pytest.mark.parametrize("per_item", [1, 3, 9])
def test_windows_per_item(oracle, monkeypatch, per_item):
    """1, 3 and all 9 windows in a work item: the cursors carry over, an item's records start where the lead group's lower bounds say"""
    import rucene_amd
    monkeypatch.setenv("RGPU_FIELDS_WINDOWS_PER_ITEM", str(per_item))
    c = rucene_amd.Context(profile_kernels=True)
    try:
        g = Gpu(c, oracle, ft.TreeLeaf("seeded"))
        try:
            queries = [q for _, q in _all_queries()]
            g.check(queries, 10, ("per item", per_item))
            g.check(queries[:8], 128, ("per item", per_item))
        finally:
            g.close()
    finally:
        c.close()


def test_a_batch_served_in_passes(oracle, monkeypatch):
    """RGPU_FIELDS_TREE_RECORDS_PER_PASS=150 (read per call): the batch is served in runs of consecutive queries whose lead groups
    hold at most 150 postings together, a query above that on its own; the rows are the one-pass rows"""
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    g = Gpu(c, oracle, ft.TreeLeaf("seeded"))
    try:
        queries = [q for _, q in _all_queries()]
        one_pass = g.search(queries, 10)
        monkeypatch.setenv("RGPU_FIELDS_TREE_RECORDS_PER_PASS", "150")
        c.kernel_stats_reset()
        passes = g.search(queries, 10)
        assert c.kernel_stats()["k_fields_tree_windows"]["launches"] > 8
        assert one_pass[0].tobytes() == passes[0].tobytes() and (one_pass[1] == passes[1]).all()
        g.check(queries, 10, "passes")
        # one doc_start_fp under two fields, in the LAST query of the batch only: refused before the first pass prepares or launches
        # anything (a fresh segment: nothing is prepared yet)
        g.close()
        g = Gpu(c, oracle, ft.TreeLeaf("seeded"))
        a, b = (0, T["THIRD"]), (1, ft.B_400)
        q, gr, cl = g.packed(queries + [tree([sum_([a, b])], [term(*b)])])
        assert (cl["state"][-1] == cl["state"][-2]) and cl["field"][-1] == g.slots[1]
        cl["field"][-1] = g.slots[0]
        c.kernel_stats_reset()
        _untouched(g, q, gr, cl, 10, ILLEGAL)
        assert not [n for n, s in c.kernel_stats().items() if s["launches"]] and g.seg.footprint()["prepared_terms"] == 0
    finally:
        g.close()
        c.close()


def test_k_edges(ctx, oracle):
    """k = 1, 64 | 65, 128 and more than the hits, on rule, sum and emission queries"""
    g = Gpu(ctx, oracle, ft.TreeLeaf("seeded"))
    try:
        rq, sq, eq = ft.rule_queries(), ft.sum_queries(), ft.emission_queries()
        queries = [rq["S100"], rq["KEEPS two-field"], rq["DEAD_ALL"], sq["two clauses"], sq["sum, dismax and term under MUST"], eq["64 hits in a step"],
                   eq["both ends"], eq["a singleton lead"], sq["every group absent"]]
        assert min(g.ref.rows(q)[2] for q in queries[:-1]) < 64 < 128 < max(g.ref.rows(q)[2] for q in queries)
        for k in (1, 2, 63, 64, 65, 127, 128):
            g.check(queries, k, "k", rule=ctx.rule)
    finally:
        g.close()


def test_single_occur_rows_are_the_old_calls_bytes(ctx, oracle):
    """TERM / DISMAX queries of one side: byte-identical to rgpu_search_fields_batch; so is a MUST side whose SHOULD groups are all
    absent from the leaf"""
    g = Gpu(ctx, oracle, ft.TreeLeaf("seeded"))
    try:
        a, b, c = (0, T["THIRD"]), (1, ft.B_400), (1, ft.B_2000)
        pairs = [(cf.should([term(*a), dismax(0.3, [b, c]), term(2, ft.G_256)], must_not=[(2, ft.G_5)]), {}),
                 (cf.must([term(2, ft.G_ALL), dismax(0.3, [(0, T["HOLD"]), c]), term(*b)]), {}),
                 (cf.should([term(*a), term(*b), term(*c)], msm=2), {}),
                 (cf.must([dismax(0.0, [a, b]), term(*c)]), dict(should=[sum_([(1, ft.B_0)]), term(1, ft.B_0)]))]
        old = [p[0] for p in pairs]
        new = [tree(q["groups"] if q["occur"] == "must" else [], extra.get("should", []) if q["occur"] == "must" else q["groups"], q["msm"], q["must_not"])
               for q, extra in pairs]
        for k in (10, 128):
            want = g.seg.search_fields_batch(*cf.pack(g.ref, old, g.tables, field_of=lambda f: g.slots[f]), k)
            got = g.search(new, k)
            assert want[0].tobytes() == got[0].tobytes() and (want[1] == got[1]).all() and want[1].min() > 0
    finally:
        g.close()


def test_field_0_trees_equal_rgpu_search_batch(ctx, oracle):
    """+a b c over field 0 alone: bit-equal to rgpu_search_batch with RGPU_OP_WITH_SHOULD, in both rule modes"""
    from rucene_amd import _lib
    leaf = ft.TreeLeaf("seeded")
    g = Gpu(ctx, oracle, leaf)
    try:
        w = lambda t: g.ref.weight((0, t))[0]   # noqa: E731
        cases = [([T["S100"]], [T["ALL"], T["THIRD"]]), ([T["KEEPS_STATE"]], [T["ALL"]]), ([T["DEAD_ALL"], T["HOLD"]], [T["THIRD"], T["ALL"]])]
        terms, queries, trees = [], [], []
        for m, s in cases:
            first = len(terms)
            for t in m + s:
                row = np.zeros(1, _lib.QUERY_TERM_DTYPE)[0]
                row["state"], row["weight"], row["sim_table"] = leaf.fields[0].terms[t], w(t), g.tables[0]
                terms.append(row)
            queries.append(((_lib.OP_TERM if len(m) == 1 else _lib.OP_AND) | (len(s) << 16), len(m), first, 0))
            trees.append(tree([term(0, t) for t in m], [term(0, t) for t in s]))
        want = g.seg.search_batch(np.array(queries, _lib.QUERY_DTYPE), np.array(terms, _lib.QUERY_TERM_DTYPE), 10)
        got = g.search(trees, 10)
        assert want[0].tobytes() == got[0].tobytes() and (np.asarray(want[1]) == got[1]).all()
    finally:
        g.close()


def test_a_docs_only_field(ctx, oracle):
    """field 1 is indexed with IndexOptions::Docs and omits norms: every freq reads 1; both .doc formats"""
    rng = np.random.default_rng(12)
    max_doc = 1100
    body = cf.Field([(cf.spread(rng, max_doc, df), cf.freqs_of(rng, df)) for df in (700, 1, 129)], rng.integers(100, 124, size=max_doc), 40 * max_doc)
    ident = cf.Field([(cf.spread(rng, max_doc, df), np.ones(df, np.int32)) for df in (129, 1, 7, 600)], None, -1)
    for version in (1, 0):
        leaf = cf.docs_only_leaf(oracle, max_doc, body, ident, alive=rng.random(max_doc) < 0.7, version=version)
        g = Gpu(ctx, oracle, leaf)
        try:
            g.check([tree([sum_([(0, 0), (1, 3)])], [sum_([(0, 2), (1, 0)]), term(1, 2)]), tree(should=[sum_([(1, 0), (0, 2)]), sum_([(1, 3)])]),
                     tree([sum_([(1, 3), (1, 1)]), term(0, 0)], [term(1, 0)], must_not=[(1, 2)])], 10, ("docs-only", version), rule=ctx.rule)
        finally:
            g.close()


def _untouched(g, q, gr, c, k, status):
    from rucene_amd import _lib
    hits = np.full((max(len(q), 1), max(k, 1)), 7, dtype=np.int64).view(_lib.HIT_DTYPE)
    totals = np.full(max(len(q), 1), -99, dtype=np.int64)
    before = hits.tobytes()
    with pytest.raises(_lib.RgpuError) as e:
        g.seg.search_fields_tree_batch(q, gr, c, k, hits=hits, totals=totals)
    assert e.value.status == status, (e.value, status)
    assert hits.tobytes() == before and (totals == -99).all()


def test_refusals_leave_the_outputs_untouched(rule_ctx, oracle):
    g = Gpu(rule_ctx, oracle, ft.TreeLeaf("none"))
    try:
        a, b = (0, T["THIRD"]), (1, ft.B_400)
        ten = [term(*a)] * 10
        rule_ctx.kernel_stats_reset()
        _untouched(g, *g.packed([tree(ten, [term(*b)])]), 10, UNSUPPORTED)                    # ten groups on a side
        _untouched(g, *g.packed([tree([term(*b)], ten)]), 10, UNSUPPORTED)
        _untouched(g, *g.packed([tree(should=[sum_([a] * 10)])]), 10, UNSUPPORTED)            # ten disjuncts
        _untouched(g, *g.packed([tree([sum_([a, b], 2)], [term(*b)])]), 10, UNSUPPORTED)      # a nested min_should_match of 2
        _untouched(g, *g.packed([tree(should=[sum_([a, b], 2)])]), 10, UNSUPPORTED)
        _untouched(g, *g.packed([tree([term(*a)], [sum_([b])])]), 129, UNSUPPORTED)
        _untouched(g, *g.packed([tree([term(*a)], [sum_([b])])]), 0, ILLEGAL)
        _untouched(g, *g.packed([tree(should=[term(*a), sum_([b])], msm=2, must_not=[(2, ft.G_5)])]), 10, UNSUPPORTED)
        q, gr, c = g.packed([tree([sum_([a, b])], [term(*b)])])
        for field, value in (("n_must", 0), ("n_must", -1), ("n_should", -1), ("n_must", 2), ("first_group", 1), ("first_group", -1), ("min_should_match", -1)):
            q2 = q.copy()
            q2[field] = value
            if (field, value) == ("n_must", 0):
                q2["n_should"] = 0                                                            # a query with no group
            _untouched(g, q2, gr, c, 10, ILLEGAL)
        for field, value in (("kind", 3), ("kind", -1), ("n_terms", 0), ("n_terms", -1), ("first_term", 2), ("min_should_match", -1)):
            g2 = gr.copy()
            g2[field][0] = value
            _untouched(g, q, g2, c, 10, ILLEGAL)
        g2 = gr.copy()
        g2["reserved"][0] = 1                                                                 # what the header says is 0 is 0
        _untouched(g, q, g2, c, 10, ILLEGAL)
        g2 = gr.copy()
        g2["min_should_match"][1] = 1                                                         # ... a TERM group's min_should_match too
        _untouched(g, q, g2, c, 10, ILLEGAL)
        g2 = gr.copy()
        g2["kind"][0] = 0                                                                     # a TERM group of two clauses
        _untouched(g, q, g2, c, 10, ILLEGAL)
        c2 = c.copy()
        c2["field"][1] = 3                                                                    # a field slot that is not attached
        _untouched(g, q, gr, c2, 10, ILLEGAL)
        c2 = c.copy()
        c2["sim_table"][0] = 99
        _untouched(g, q, gr, c2, 10, ILLEGAL)
        c2 = c.copy()
        c2["field"][0], c2["field"][2] = g.slots[1], g.slots[0]                                # one doc_start_fp under two fields: c[1] and c[2] are B_400
        c2["state"][0] = c2["state"][1]
        _untouched(g, q, gr, c2, 10, ILLEGAL)
        assert not [n for n, s in rule_ctx.kernel_stats().items() if s["launches"]]          # nothing was launched
        g.check([tree([sum_([a, b])], [term(*b)])], 10, "served after the refusals")
    finally:
        g.close()


# ---- the mirror -----------------------------------------------------------------------------------------------------------------------
NAMES = ("title", "body", "tags")


def _mirror_query(q):
    import rucene_amd
    Tq, B, D = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery

    def clause(g):
        if g[0] == "term":
            return Tq(g[1][1], field=NAMES[g[1][0]])
        if g[0] == "dismax":
            return D([Tq(t, field=NAMES[f]) for f, t in g[2]], g[1])
        return B([], [Tq(t, field=NAMES[f]) for f, t in g[2]], max(1, g[1]))
    return B([clause(g) for g in q["must"]], [clause(g) for g in q["should"]], q["msm"] if q["must"] else max(1, q["msm"]),
             [Tq(t, field=NAMES[f]) for f, t in q["must_not"]])


def _searcher(ctx, leaves, **kw):
    import rucene_amd
    gl = []
    for leaf in leaves:
        t, b, g = leaf.fields
        lr = rucene_amd.LeafReader(leaf.doc_bytes, t.norms, leaf.max_doc, t.terms, doc_base=leaf.doc_base, live_docs=leaf.live_docs,
                                   sum_total_term_freq=t.sttf, field="title")
        lr.add_field("body", b.norms, b.terms, sum_total_term_freq=b.sttf)
        lr.add_field("tags", g.norms, g.terms, sum_total_term_freq=g.sttf)
        gl.append(lr)
    return rucene_amd.GpuIndexSearcher(gl, ctx=ctx, **kw), gl


def _small_leaf(n, max_doc):
    rng = np.random.default_rng([n, 19])
    def lists(fracs):
        return [(cf.spread(rng, max_doc, int(max_doc * fr)), cf.freqs_of(rng, int(max_doc * fr))) for fr in fracs]
    n_title, n_body, n_tags = len(ft.TreeLeaf().fields[0].lists), len(ft.TreeLeaf().fields[1].lists), 3
    title = cf.Field(lists([0.6, 0.3, 0.5, 0.02] + [0.1] * (n_title - 4)), rng.integers(100, 124, size=max_doc), (50 + n) * max_doc)
    body = cf.Field(lists([0.5, 0.3, 0.0 if n == 1 else 0.2, 0.1, 0.45, 0.0] + [0.05] * (n_body - 6)), 60 + rng.permutation(max_doc) % 70, (60 + 9 * n) * max_doc)
    tags = cf.Field(lists([0.4, 0.05, 0.01][:n_tags]), None, 2 * max_doc)
    return cf.CrossLeaf(max_doc, [title, body, tags], alive=rng.random(max_doc) < 0.8)


def test_python_mirror_over_four_leaves(ctx, oracle):
    """GpuIndexSearcher(field_trees=True): nested should-only groups and MUST beside SHOULD route to rgpu_search_fields_tree_batch;
    every leaf sums in its own orders and starts the rule afresh (TWO: leaf B's first 101 scored docs take the optional sum); rows
    the old call can express keep going there; without the flag the trees are UnsupportedOperation, as they have been"""
    import rucene_amd
    leaves = [ft.TreeLeaf("seeded", which="A"), _small_leaf(1, 700), ft.TreeLeaf("seeded", which="B"), _small_leaf(3, 1300)]
    refs = ft.index_refs(oracle, leaves)
    rq, sq, eq = ft.rule_queries(), ft.sum_queries(), ft.emission_queries()
    queries = [rq["TWO"], rq["S101"], rq["KEEPS two-field"], rq["two-clause lead"], sq["nested against flat"], sq["sum, dismax and term under MUST"],
               sq["sum cost above a term"], sq["a group absent under SHOULD"], eq["every doc twice"], eq["thin conjunction"], eq["msm beside MUST"]]
    s, gl = _searcher(ctx, leaves, field_trees=True)
    try:
        Tq, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
        old = [cf.should([dismax(0.1, [(0, T["THIRD"]), (1, ft.B_400)]), term(2, ft.G_256)]), cf.must([term(0, T["HOLD"]), term(1, ft.B_2000)])]
        old_q = [B([], [rucene_amd.DisjunctionMaxQuery([Tq(T["THIRD"]), Tq(ft.B_400, field="body")], 0.1), Tq(ft.G_256, field="tags")], 1),
                 B([Tq(T["HOLD"]), Tq(ft.B_2000, field="body")], [], 0)]
        for k in (10, 128):
            ctx.kernel_stats_reset()
            hits, totals = s.search_batch([_mirror_query(q) for q in queries] + old_q, k)
            stats = {n: st["launches"] for n, st in ctx.kernel_stats().items() if st["launches"]}
            assert stats["k_fields_tree_windows"] == stats["k_fields_windows"] == len(leaves), stats
            for i, q in enumerate(queries):
                d, sc, tot = ft.index_rows(refs, q, k, rule=ctx.rule)
                assert totals[i] == tot and (hits[i]["doc"][:d.size] == d).all() and (hits[i]["doc"][d.size:] == -1).all(), (k, i)
                assert (hits[i]["score"][:d.size].view(np.int32) == sc.view(np.int32)).all(), (k, i)
            for j, q in enumerate(old):
                d, sc, tot = cf.index_rows(refs, q, k)
                i = len(queries) + j
                assert totals[i] == tot and (hits[i]["doc"][:d.size] == d).all() and (hits[i]["score"][:d.size].view(np.int32) == sc.view(np.int32)).all()
        # still the CPU path's with the flag on
        for q in (B([B([Tq(0)], [Tq(1, field="body")], 0)], [Tq(1)], 0), B([], [B([], [Tq(0, field="body"), Tq(1)], 2), Tq(2)], 1),
                  B([Tq(0, field="body")], [Tq(1)], 0, [], [Tq(2)]), B([Tq(0, field="body")], [Tq(i % 3) for i in range(10)], 0)):
            with pytest.raises(rucene_amd.RgpuError) as e:
                s.search_batch([q], 10)
            assert e.value.status == -5, str(q)
        with pytest.raises(rucene_amd.RgpuError) as e:
            s.search_batch([_mirror_query(queries[0])], 129)
        assert e.value.status == -5
        plain = rucene_amd.GpuIndexSearcher(gl, ctx=ctx)
        for q in (queries[0], queries[4]):
            with pytest.raises(rucene_amd.RgpuError) as e:
                plain.search_batch([_mirror_query(q)], 10)
            assert e.value.status == -5
    finally:
        for leaf in gl:
            leaf.segment.close()


def test_query_string_round_trip(ctx, oracle):
    """QueryStringQueryBuilder("gpu +search", [title, body]) on a field_trees searcher: the reference's rows; on a default searcher
    UnsupportedOperation; phrase syntax and min_should_match >= 2 over several fields are the CPU path's"""
    import rucene_amd
    leaves = [ft.TreeLeaf("seeded", which="A"), ft.TreeLeaf("none", which="B")]
    refs = ft.index_refs(oracle, leaves)
    vocab = {"title": {"gpu": T["ALL"], "search": T["KEEPS_STATE"], "wave": T["THIRD"]}, "body": {"gpu": ft.B_ALL, "search": ft.B_0, "wave": ft.B_2000}}
    fields = [("title", 1.0), ("body", 1.0)]
    def build(text, msm=0):
        return rucene_amd.QueryStringQueryBuilder(text, fields, msm, 1.0, term=lambda f, w: vocab[f][w]).build()
    def word(w):
        return sum_([(0, vocab["title"][w]), (1, vocab["body"][w])], 1)
    s, gl = _searcher(ctx, leaves, field_trees=True)
    try:
        cases = [("gpu +search", tree([word("search")], [word("gpu")])), ("gpu wave", tree(should=[word("gpu"), word("wave")])),
                 ("+wave +search gpu", tree([word("wave"), word("search")], [word("gpu")])), ("wave", tree(should=[word("wave")]))]
        hits, totals = s.search_batch([build(text) for text, _ in cases], 10)
        for i, (text, q) in enumerate(cases):
            d, sc, tot = ft.index_rows(refs, q, 10, rule=ctx.rule)
            assert tot > 0 and totals[i] == tot and (hits[i]["doc"][:d.size] == d).all(), text
            assert (hits[i]["score"][:d.size].view(np.int32) == sc.view(np.int32)).all(), text
        if ctx.rule:     # the rule decides some row of "gpu +search"
            assert ft.index_rows(refs, cases[0][1], 10000)[1].tobytes() != ft.index_rows(refs, cases[0][1], 10000, rule=False)[1].tobytes()
        for q in (build('"gpu wave"~1 search'), build("gpu wave search", 2)):
            with pytest.raises(rucene_amd.RgpuError) as e:
                s.search_batch([q], 10)
            assert e.value.status == -5
        seen = []
        plain = rucene_amd.GpuIndexSearcher(gl, ctx=ctx, cpu_fallback=lambda query, collector: seen.append(query))
        q = build("gpu +search")
        with pytest.raises(rucene_amd.RgpuError) as e:
            plain.search_batch([q], 10)
        assert e.value.status == -5
        plain.search(q, rucene_amd.TopDocsCollector(10))
        assert seen == [q]
    finally:
        for leaf in gl:
            leaf.segment.close()


def test_cpp_demo_rows(oracle, tmp_path):
    """tests/cpp/field_tree_demo.cpp: the C++ mirror's routing (MultiFieldQuery's sum groups and must_should form behind
    GpuIndexSearcher::field_trees) - the lines it prints are tests/field_tree.py's rows; without the flag the trees reach the CPU hook"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "field_tree_demo")
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "cpp", "field_tree_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    leaf = ft.TreeLeaf("none")
    ref = ft.TreeRef(oracle, leaf)
    (tmp_path / "doc.bin").write_bytes(np.asarray(leaf.doc_bytes).tobytes())
    for f, fld in enumerate(leaf.fields):
        (tmp_path / ("norms%d.bin" % f)).write_bytes(b"" if fld.norms is None else fld.norms.tobytes())
        (tmp_path / ("terms%d.bin" % f)).write_bytes(np.ascontiguousarray(fld.terms).tobytes())
    ids = [T["KEEPS_STATE"], T["ALL"], T["THIRD"], ft.B_0, ft.B_ALL, ft.B_2000, ft.G_256]
    out = subprocess.check_output([exe, str(tmp_path), str(leaf.max_doc)] + [str(fld.sttf) for fld in leaf.fields] + [str(i) for i in ids],
                                  text=True).strip().splitlines()
    word = lambda w: sum_([(0, ids[w]), (1, ids[3 + w])], 1)   # noqa: E731
    specs = [tree([word(0)], [word(1)]), tree(should=[word(1), word(2)], msm=1),
             tree([word(0), term(2, ft.G_256)], [word(1), word(2)], must_not=[(1, ft.B_2000)]), tree([word(1), word(2)]),
             cf.should([dismax(0.3, [(0, T["ALL"]), (1, ft.B_ALL)]), term(2, ft.G_256)])]
    assert len(out) == len(specs) + 1, out
    for i, line in enumerate(out[:-1]):
        parts = line.split()
        d, sc, total = ref.rows(specs[i], 10)
        assert parts[0] == "tree" and int(parts[1]) == i and int(parts[2]) == total > 0, line
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        assert [x[0] for x in got] == d.tolist() and [x[1] for x in got] == sc.view(np.uint32).tolist(), line
    assert out[-1] == "fallback 1 refused 2", out[-1]
