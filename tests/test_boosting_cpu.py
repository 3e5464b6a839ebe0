"""BoostingQuery on the CPU side (`-m "not gpu"`): the composed reference of tests/boosting_ref.py held against the oracle's own
searches, and what the Python mirror packs for a BoostingQuery (include/rucene_gpu.h RGPU_NOT_WITH_DEMOTE: the demoting clauses
behind the MUST_NOT ones, their count in the second byte of rgpu_query.n_must_not, negative_boost in each one's weight). The fixtures
are the 257-doc rank-mode leaf with seeded deletions and the twins() index of tests/segment_spectrum.py, in which SOMETIMES has no
posting in the leaves whose max_doc is a multiple of 3."""
import numpy as np
import pytest

import segment_spectrum as ss
from boosting_ref import BoostingRef, Positive, hollow_leaves_with_positive_docs

E, F, L, V, Q5, A, S, C = ss.EVERY, ss.FIRST, ss.LAST, ss.EVEN, ss.FIFTH, ss.ABSENT, ss.SOMETIMES, ss.CONST
BOOSTS = (0.5, 0.1, float(np.nextafter(np.float32(1), np.float32(0))))
POSITIVES = [Positive("term", (Q5,)), Positive("term", (E,)), Positive("and", (V, Q5)), Positive("and", (E, V, C)), Positive("or", (F, L, Q5)),
             Positive("or", (V, Q5, S), msm=2), Positive("or", (E, L, V, Q5, A, S, C, V, Q5), must_not=(F,))]
INDEXES = {"leaf-257-rank-seeded": lambda: [ss.Leaf(257, "rank", "seeded")], "twins": ss.twins}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module", params=sorted(INDEXES))
def world(request, oracle):
    leaves = INDEXES[request.param]()
    return oracle, leaves, BoostingRef(oracle, leaves)


# ---- (1) the composition against the oracle ------------------------------------------------------------------------------------------
def test_a_negative_without_postings_matches_nothing(world):
    oracle, leaves, ref = world
    for p in POSITIVES:
        for neg in ((A,), (A, A)):
            d, s, total = ref.rows(p, neg, 0.5)
            assert d.size == 0 and s.size == 0 and total == 0, (p, neg)
        assert ref.positive(p)[2] > 0, p


def test_a_negative_that_holds_no_positive_doc_reproduces_the_oracle_row(world):
    """One leaf: odd docs never meet EVEN's list, so a negative of EVEN leaves every score alone. (On twins() the negative has a scorer
    in every leaf, so nothing is dropped either.)"""
    oracle, leaves, ref = world
    odd = {leaf.doc_base + d for leaf in leaves for d in range(1, leaf.max_doc, 2)}
    for p in POSITIVES:
        if p.must_not == () and p.op != "or":
            q = Positive(p.op, p.terms, must_not=(V,))            # the positive's docs are all odd: none is in EVEN
            want_d, want_s, want_t = ref.positive(q)
            assert set(want_d.tolist()) <= odd
            for b in BOOSTS:
                d, s, total = ref.rows(q, (V,), b)
                assert total == want_t and (d == want_d).all() and (s.view(np.int32) == want_s.view(np.int32)).all(), (q, b)


def test_a_negative_of_every_doc_multiplies_every_score(world):
    oracle, leaves, ref = world
    for p in POSITIVES:
        want_d, want_s, want_t = ref.positive(p)
        for b in BOOSTS:
            d, s, total = ref.rows(p, (E,), b)
            scaled = (want_s * np.float32(b)).astype(np.float32)
            # (rounding can make neighbours equal, never swap them: the row is the oracle's order up to ties, which go by doc id)
            order = np.lexsort((want_d, -scaled.astype(np.float64)))
            assert total == want_t and (d == want_d[order]).all(), (p, b)
            assert (s.view(np.int32) == scaled[order].view(np.int32)).all(), (p, b)
            assert (np.diff(scaled) <= 0).all(), (p, b)                   # ... "keeps the order"


def test_the_union_multiplies_once(world):
    oracle, leaves, ref = world
    p = Positive("term", (E,))
    want_d, want_s, _ = ref.positive(p)
    by_doc = np.zeros(ref.max_doc, np.float32)
    by_doc[want_d] = want_s
    held, scorer = ref.negative_mask((V, Q5))
    both = np.zeros(ref.max_doc, bool)
    for leaf in leaves:
        both[leaf.doc_base:leaf.doc_base + leaf.max_doc] = leaf.has[V] & leaf.has[Q5]
    d, s, _ = ref.rows(p, (V, Q5), 0.5)
    assert both[d].any() and scorer.all()
    want = np.where(held[d], (by_doc[d] * np.float32(0.5)).astype(np.float32), by_doc[d])
    assert (s.view(np.int32) == want.view(np.int32)).all()


def test_hollow_leaves_contribute_nothing():
    """twins(): SOMETIMES has no posting in the 129- and 33-doc leaves (multiples of 3): their docs leave the row and the count."""
    leaves = ss.twins()
    p = Positive("term", (E,))
    hollow = hollow_leaves_with_positive_docs(leaves, p, (S,))
    assert hollow == [0, 2]


def test_hollow_leaves_against_the_oracle(oracle):
    leaves = ss.twins()
    ref = BoostingRef(oracle, leaves)
    p = Positive("term", (E,))
    d, s, total = ref.rows(p, (S,), 0.5)
    gone = sum(int(leaves[i].alive.sum()) for i in (0, 2))
    assert gone > 0 and total == ref.positive(p)[2] - gone
    assert not set(ss.leaf_of(leaves, d).tolist()) & {0, 2}


# ---- (2) packing ---------------------------------------------------------------------------------------------------------------------
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


def test_pack_op_clause_order_count_and_boost_bits(packer):
    ra, leaf, s = packer
    T, B, Bo = ra.TermQuery, ra.BooleanQuery, ra.BoostingQuery
    queries = [Bo(T(Q5), T(F), 0.5),                                                             # TERM + one demoting term
               T(V),
               Bo(B.build([T(V), T(Q5)], []), B.build([], [T(A), T(Q5)]), 0.1),                  # AND + a union of two
               Bo(B.build([], [T(V), T(Q5), T(S)], min_should_match=2), T(E), BOOSTS[2]),        # OR msm 2
               Bo(B.build([], [T(F), T(L)], must_nots=[T(C)]), B.build([], [T(V), T(S), T(L)]), 0.5),   # OR + MUST_NOT + three demoting
               Bo(B.build([T(E)], [], must_nots=[T(F), T(L)]), T(V), 0.25),                      # one MUST + two MUST_NOT: AND of one clause
               B.build([T(E)], [], must_nots=[T(F)])]
    for q, t in (s.pack(queries, leaf), s._pack_clause_by_clause(queries, leaf)):
        assert q["op"].tolist() == [0, 0, 1, 2 | (2 << 8), 2, 1, 1]
        assert q["n_terms"].tolist() == [1, 1, 2, 3, 2, 1, 1]
        assert q["first_term"].tolist() == [0, 2, 3, 7, 11, 17, 21]
        assert q["n_must_not"].tolist() == [ra.not_with_demote(0, 1), 0, ra.not_with_demote(0, 2), ra.not_with_demote(0, 1), ra.not_with_demote(1, 3),
                                            ra.not_with_demote(2, 1), 1]
        assert ra.not_with_demote(1, 3) == 1 | (3 << 8) and ra.not_with_demote(2, 0) == 2
        assert t.size == 23
        # clause order: scored, MUST_NOT, demoting - by the doc_freq each term has in the leaf
        df = [int(leaf.terms[x]["doc_freq"]) for x in range(ss.N_TERMS)]
        order = [Q5, F, V, V, Q5, A, Q5, V, Q5, S, E, F, L, C, V, S, L, E, F, L, V, E, F]
        assert t["state"]["doc_freq"].tolist() == [df[x] for x in order]
        # negative_boost's bits in every demoting clause's weight
        demoting = {1: 0.5, 5: 0.1, 6: 0.1, 10: BOOSTS[2], 14: 0.5, 15: 0.5, 16: 0.5, 20: 0.25}
        for at, b in demoting.items():
            assert _bits(t["weight"][at]) == _bits(b), (at, b)
        # the scored clauses are the positive query's own records
        alone_q, alone_t = s.pack([B.build([T(V), T(Q5)], [])], leaf)
        assert alone_t.tobytes() == t[3:5].tobytes() and alone_q["op"][0] == 1
    a, b = s.pack(queries, leaf), s._pack_clause_by_clause(queries, leaf)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1]["state"].tobytes() == b[1]["state"].tobytes()
    sc = [i for i in range(23) if i not in (1, 5, 6, 10, 13, 14, 15, 16, 18, 19, 20, 22)]      # scored clauses: weight and table agree
    assert a[1]["weight"][sc].tobytes() == b[1]["weight"][sc].tobytes() and (a[1]["sim_table"][sc] == 7).all()


def test_query_object(packer):
    ra, leaf, s = packer
    T, B, Bo = ra.TermQuery, ra.BooleanQuery, ra.BoostingQuery
    q = Bo.build(B.build([T(3), T(4, 2.0)], []), T(5), 0.5)
    assert isinstance(q, Bo) and [t.term for t in q.extract_terms()] == [3, 4]      # boosting_query.rs:62-64: the positive's terms
    assert str(Bo(T(3), T(5), 0.5)) == "BoostingQuery(positive: %s, negative: %s, negative_boost: 0.5)" % (T(3), T(5))
    assert q.boost_bits() == _bits(0.5)
    assert [t.term for t in Bo(T(1), B.build([], [T(2), T(3)]), 0.5).demoting_terms()] == [2, 3]
    assert Bo(T(1), B.build([T(2), T(3)], []), 0.5).demoting_terms() is None
    assert Bo(T(1), B.build([], [T(2), T(3), T(4)], min_should_match=2), 0.5).demoting_terms() is None


def test_fall_back_cases(packer):
    ra, leaf, s = packer
    T, B, Bo, D = ra.TermQuery, ra.BooleanQuery, ra.BoostingQuery, ra.DisjunctionMaxQuery
    declined = [Bo(T(V), T(Q5), 0.0), Bo(T(V), T(Q5), 1.0), Bo(T(V), T(Q5), -0.5), Bo(T(V), T(Q5), float("nan")), Bo(T(V), T(Q5), float("inf")),
                Bo(T(V), T(Q5), 1.5),
                Bo(B.build([T(V)], [T(Q5)]), T(F), 0.5),                                   # MUST + SHOULD positive
                Bo(B.build([T(V), B.build([], [T(Q5), T(S)])], []), T(F), 0.5),            # nested positive
                Bo(D([T(V), T(Q5)], 0.1), T(F), 0.5), Bo(ra.PhraseQuery([1, 2]), T(F), 0.5),
                Bo(Bo(T(V), T(F), 0.5), T(L), 0.5),
                Bo(T(V), B.build([T(Q5), T(S)], []), 0.5),                                 # a conjunction as the negative
                Bo(T(V), B.build([], [T(Q5), T(S), T(F)], min_should_match=2), 0.5),
                Bo(T(V), B.build([], [T(Q5)], must_nots=[T(F)]), 0.5),
                Bo(T(V), D([T(Q5), T(S)], 0.0), 0.5), Bo(T(V), Bo(T(F), T(L), 0.5), 0.5)]
    for q in declined:
        with pytest.raises(ra.RgpuError) as e:
            s.pack([T(1), q], leaf)
        assert e.value.status == -5, str(q)                   # UnsupportedOperation: the caller's CPU path
        seen = []
        s.cpu_fallback = lambda query, collector: seen.append(query)
        try:
            s.search(q, ra.TopDocsCollector(10))
        finally:
            s.cpu_fallback = None
        assert seen == [q]
        with pytest.raises(ra.RgpuError) as e:                # no hook: the error reaches the caller
            s.search(q, ra.TopDocsCollector(10))
        assert e.value.status == -5
    with pytest.raises(ra.RgpuError) as e:                    # over RGPU_MAX_QUERY_TERMS with the demoting clauses counted
        s.pack([Bo(B.build([], [T(V)] * 60), B.build([], [T(Q5)] * 5), 0.5)], leaf)
    assert e.value.status == -5


def test_the_planner_refuses_a_demote_byte(packer):
    """rgpu_plan_batch_ids: UnsupportedOperation for a non-zero second byte of n_must_not."""
    ra, leaf, s = packer
    p = s._planner(leaf)
    with pytest.raises(ra.RgpuError) as e:
        p.plan_batch([0], [1], [V, Q5], [ra.not_with_demote(0, 1)])
    assert e.value.status == -5
    qs, ts = p.plan_batch([0], [1], [V, Q5], [1])            # the same clause as a MUST_NOT clause is planned
    assert qs["n_must_not"][0] == 1 and ts.size == 2


def test_the_cpp_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/boosting_demo.cpp + rucene::BoostingQuery of csrc/host/gpu_index_searcher.hpp link against the C ABI on a CPU-only box
    (running it needs a GPU: tests/test_gpu_boosting.py)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(tmp_path / "boosting_demo"),
                           os.path.join(root, "tests", "cpp", "boosting_demo.cpp"), "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
