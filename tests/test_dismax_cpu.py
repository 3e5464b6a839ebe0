"""DisjunctionMaxQuery on the CPU side (`-m "not gpu"`): the composed reference of tests/dismax_ref.py held against the oracle's own
TERM and OR searches, and what the mirrors pack for RGPU_OP_DISMAX (include/rucene_gpu.h: op 3, the f32 tie_breaker_multiplier's
bit pattern in rgpu_query.n_must_not). The fixtures are the 257-doc rank-mode leaf with seeded deletions and the twins() index of
tests/segment_spectrum.py, whose present-clause count differs from leaf to leaf."""
import numpy as np
import pytest

import segment_spectrum as ss
from dismax_ref import DismaxRef

TIES = (0.0, 0.1, 1.0)
CLAUSES = [(ss.FIFTH,), (ss.EVEN, ss.FIFTH), (ss.FIFTH, ss.FIFTH), (ss.EVERY, ss.FIRST, ss.LAST, ss.EVEN, ss.FIFTH, ss.ABSENT, ss.SOMETIMES, ss.CONST, ss.EVEN),
           (ss.EVERY, ss.FIRST, ss.LAST, ss.EVEN, ss.FIFTH, ss.CONST, ss.EVERY, ss.EVEN, ss.FIFTH, ss.CONST), (ss.ABSENT, ss.SOMETIMES), (ss.ABSENT, ss.ABSENT)]
INDEXES = {"leaf-257-rank-seeded": lambda: [ss.Leaf(257, "rank", "seeded")], "twins": ss.twins}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module", params=sorted(INDEXES))
def world(request, oracle):
    leaves = INDEXES[request.param]()
    ref = DismaxRef(oracle, leaves)
    return oracle, leaves, ref


def test_one_clause_is_the_term_query(world):
    """One disjunct: s + (s - s) * tie = s at any finite tie - the oracle's OP_TERM row, bit for bit."""
    oracle, leaves, ref = world
    for t in ss.QUERIED:
        want = ref.osr.search(oracle.OP_TERM, [t], ref.max_doc, tie_mode=oracle.TIE_CANONICAL)
        for tie in TIES + (7.5, -0.25):
            d, s, total = ref.rows((t,), tie)
            assert total == want[2] and (d == want[0]).all(), (t, tie)
            assert (s.view(np.int32) == want[1].view(np.int32)).all(), (t, tie)


def test_tie_zero_is_the_maximum_of_the_term_scores(world):
    oracle, leaves, ref = world
    for clauses in CLAUSES:
        best = np.full(ref.max_doc, -np.inf, np.float32)
        for t in clauses:
            d, s, _ = ref.osr.search(oracle.OP_TERM, [t], ref.max_doc, tie_mode=oracle.TIE_CANONICAL)
            np.maximum.at(best, d, s)
        want_docs = np.flatnonzero(best > -np.inf)
        d, s, total = ref.rows(clauses, 0.0)
        assert total == want_docs.size and (np.sort(d) == want_docs).all(), clauses
        assert (s.view(np.int32) == best[d].view(np.int32)).all(), clauses
        assert ((np.diff(s) < 0) | ((np.diff(s) == 0) & (np.diff(d) > 0))).all(), clauses


def test_hit_counts_are_the_union(world):
    oracle, leaves, ref = world
    for clauses in CLAUSES:
        _, _, or_total = ref.osr.search(oracle.OP_OR, list(clauses), 10, tie_mode=oracle.TIE_CANONICAL)
        want = ss.ref_docs(leaves, ss.Query(should=clauses))
        for tie in TIES:
            d, _, total = ref.rows(clauses, tie)
            assert total == or_total == want.size and (np.sort(d) == want).all(), (clauses, tie)
            assert ref.rows(clauses, tie, 10)[0].size == min(10, total)


def test_the_same_term_twice(world):
    """[t, t]: sum = 2s, max = s, score = s + s * tie (2s and 2s - s are exact in f32)."""
    oracle, leaves, ref = world
    for t in (ss.FIFTH, ss.EVERY, ss.LAST):
        d, s, total = ref.osr.search(oracle.OP_TERM, [t], ref.max_doc, tie_mode=oracle.TIE_CANONICAL)
        by_doc = np.zeros(ref.max_doc, np.float32)
        by_doc[d] = s
        for tie in TIES:
            gd, gs, gt = ref.rows((t, t), tie)
            want = (by_doc[gd] + (by_doc[gd] * np.float32(tie)).astype(np.float32)).astype(np.float32)
            assert gt == total and (gs.view(np.int32) == want.view(np.int32)).all(), (t, tie)


def test_present_counts_differ_per_leaf():
    leaves = ss.twins()
    c9 = CLAUSES[3]
    per_leaf = [sum(1 for t in c9 if leaf.lists[t][0].size > 0) for leaf in leaves]
    assert len(set(per_leaf)) > 1 and max(per_leaf) < 10, per_leaf


# ---- packing ------------------------------------------------------------------------------------------------------------------------
class _FakeCtx:
    def sim_table(self, cache, k1):
        return 7


@pytest.fixture(scope="module")
def packer():
    import rucene_amd
    fx = ss.Leaf(257, "rank", "seeded")
    leaf = rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, live_docs=fx.live_docs, sum_total_term_freq=fx.sttf)
    s = object.__new__(rucene_amd.GpuIndexSearcher)     # no Context: pack() is host-only (as in tests/test_pack.py)
    s.leaves, s.ctx, s.similarity, s._stats_leaf, s._weights = [leaf], _FakeCtx(), rucene_amd.BM25Similarity(), 0, {}
    s._planners, s._stats_terms, s.flatten_nested, s.cpu_fallback = {}, None, False, None
    s.collection_statistics = rucene_amd.CollectionStatistics("body", 0, fx.max_doc, fx.max_doc, fx.sttf)
    return rucene_amd, leaf, s


def _bits(x):
    return int(np.float32(x).view(np.int32))


def test_pack_writes_op_3_and_the_tie_bits(packer):
    ra, leaf, s = packer
    T, B, D = ra.TermQuery, ra.BooleanQuery, ra.DisjunctionMaxQuery
    assert ra.OP_DISMAX == 3
    queries = [D([T(ss.FIFTH)], 0.5), T(ss.EVEN), D([T(ss.EVEN), T(ss.ABSENT), T(ss.FIFTH, 2.0)], 0.1), B.build([], [T(ss.EVEN), T(ss.FIFTH)], must_nots=[T(ss.FIRST)]),
               D([T(t) for t in CLAUSES[4]], 0.0), D([T(ss.LAST), T(ss.LAST)], -1.0)]
    for q, t in (s.pack(queries, leaf), s._pack_clause_by_clause(queries, leaf)):
        assert q["op"].tolist() == [3, 0, 3, 2, 3, 3]
        assert q["n_terms"].tolist() == [1, 1, 3, 2, 10, 2]
        assert q["first_term"].tolist() == [0, 1, 2, 5, 8, 18]
        assert q["n_must_not"].tolist() == [_bits(0.5), 0, _bits(0.1), 1, 0, _bits(-1.0)]
        assert t.size == 20 and t["state"]["doc_freq"][3] == 0 and (t["sim_table"] == 7).all()
        assert t["weight"][4] == np.float32(2.0) * t["weight"][0]          # the boost rides in the clause weight, as for OR
    a, b = s.pack(queries, leaf), s._pack_clause_by_clause(queries, leaf)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # the same clauses as an OR query: the clause records are the same, only op and n_must_not differ
    q_or, t_or = s.pack([B.build([], [T(ss.EVEN), T(ss.ABSENT), T(ss.FIFTH, 2.0)])], leaf)
    assert t_or.tobytes() == a[1][2:5].tobytes() and q_or["op"][0] == 2


def test_query_object(packer):
    ra, leaf, s = packer
    T, D = ra.TermQuery, ra.DisjunctionMaxQuery
    with pytest.raises(ra.RgpuError) as e:
        D([], 0.1)                                     # DisjunctionMaxQuery::build: "sub query should not be empty!"
    assert e.value.status == -2
    with pytest.raises(ra.RgpuError):
        D.build([], 0.1)
    lone = T(3)
    assert D.build([lone], 0.1) is lone and isinstance(D.build([T(3), T(4)], 0.1), D)
    q = D([T(3), T(4, 2.0)], 0.1)
    assert [t.term for t in q.extract_terms()] == [3, 4]
    assert str(q) == "DisjunctionMaxQuery(disjunctions: %s, %s, tie_breaker_multiplier: 0.1)" % (T(3), T(4, 2.0))   # an f32's Display
    assert str(D([T(3)], 1.0)).endswith("tie_breaker_multiplier: 1)") and str(D([T(3)])).endswith("tie_breaker_multiplier: 0)")
    assert str(D([T(3)], 0.25)).endswith(": 0.25)") and str(D([T(3)], 1e-3)).endswith(": 0.001)")
    assert q.tie_bits() == _bits(0.1) and D([T(1)]).tie_bits() == 0


def test_other_disjuncts_are_declined(packer):
    ra, leaf, s = packer
    T, B, D = ra.TermQuery, ra.BooleanQuery, ra.DisjunctionMaxQuery
    for inner in (ra.PhraseQuery([1, 2]), B.build([T(1), T(2)], []), D([T(1), T(2)], 0.0)):
        q = D([T(ss.EVEN), inner], 0.1)
        with pytest.raises(ra.RgpuError) as e:
            s.pack([T(1), q], leaf)
        assert e.value.status == -5                    # UnsupportedOperation: the caller's CPU path
        seen = []
        s.cpu_fallback = lambda query, collector: seen.append(query)
        try:
            s.search(q, ra.TopDocsCollector(10))
        finally:
            s.cpu_fallback = None
        assert seen == [q]


def test_the_planner_refuses_op_3(packer):
    """rgpu_plan_batch_ids / rgpu_plan_uniform_ids: UnsupportedOperation (n_must_not is no clause count there)."""
    ra, leaf, s = packer
    p = s._planner(leaf)
    for call in (lambda: p.plan_batch([3], [2], [ss.EVEN, ss.FIFTH], [_bits(0.1)]), lambda: p.plan_batch([0, 3], [1, 1], [ss.EVEN, ss.FIFTH]),
                 lambda: p.plan_uniform(3, np.array([[ss.EVEN, ss.FIFTH]]))):
        with pytest.raises(ra.RgpuError) as e:
            call()
        assert e.value.status == -5
