"""The fixtures and the composed reference of tests/phrase_or.py, proven without a GPU against the oracle itself, no doc exempted:
queries whose clauses are all terms equal oracle.search / search_not with OR bit for bit (min_should_match and MUST_NOT included), a
lone phrase clause equals phrase_search, the doc sets under min_should_match equal mock_disjunction's; the sum-order cases really
are order-sensitive; the fixtures hold the edges they are there for. Then the mirror's routing and refusals, the pinned shapes that
still refuse, the new struct's layout against a C compile of the header, and the host plan (csrc/host/phrase_or_plan.hpp) under the
sanitizers as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import phrase_bool as pb
import phrase_or as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def indexes(oracle):
    out = {"main": pb.Index(oracle, [po.main()]), "pb": pb.Index(oracle, [pb.main()]), "leaves": pb.Index(oracle, pb.leaves()),
           "deleted": pb.Index(oracle, [po.main()], deleted=[{0, 1023, 1100, 3099}])}
    yield out
    for ix in out.values():
        ix.close()


def _bits(scores):
    return np.asarray(scores, dtype=np.float32).view(np.uint32).tolist()


TERM_QUERIES = [("main", po.Q([po.DENSE, po.T300, po.T5])), ("main", po.Q([po.T5, po.DENSE, po.T300], msm=2)), ("main", po.Q([po.T300, po.DENSE, po.T5], msm=3)),
                ("main", po.Q([po.T300, po.T5], msm=3)), ("main", po.Q([po.DENSE, po.ABSENT, po.T300], msm=2)),
                ("pb", po.Q([pb.D600, pb.T129, pb.R20, pb.S])), ("pb", po.Q([pb.T129, pb.D600, pb.T40], msm=2)),
                ("leaves", po.Q([pb.T129, pb.R20, pb.D600], msm=2)), ("leaves", po.Q([pb.R20, pb.S]))]


@pytest.mark.parametrize("which,q", TERM_QUERIES, ids=[w + ": " + repr(q.shoulds) + " msm %d" % q.msm for w, q in TERM_QUERIES])
def test_term_only_queries_equal_the_oracles_disjunction(indexes, oracle, which, q):
    ix = indexes[which]
    d, s = po.rows(ix, q)
    od, os_, total = ix.osr.search(oracle.OP_OR, q.shoulds, ix.max_doc, tie_mode=oracle.TIE_CANONICAL, min_should_match=q.msm)
    assert total == od.size == d.size and d.tolist() == od.tolist() and _bits(s) == _bits(os_), q
    assert d.size > 0 or q.msm >= len(q.shoulds)


@pytest.mark.parametrize("which,shoulds,nots", [("main", [po.DENSE, po.T300], [po.T5]), ("main", [po.DENSE, po.T300, po.NOT1], [po.T5, po.ABSENT]),
                                                ("pb", [pb.T129, pb.D600, pb.R20], [pb.N1, pb.N3]), ("leaves", [pb.D600, pb.T40], [pb.N1, pb.N2])])
def test_term_only_queries_with_must_not_equal_the_oracles(indexes, oracle, which, shoulds, nots):
    """(MUST_NOT terms of at most 128 docs: ReqNotScorer advance()s them, and the oracle's plain Segment does not parse the skip data
    of a positions field's longer lists.)"""
    ix = indexes[which]
    q = po.Q(shoulds, nots)
    d, s = po.rows(ix, q)
    od, os_, total = ix.osr.search_not(oracle.OP_OR, shoulds, nots, ix.max_doc, tie_mode=oracle.TIE_CANONICAL)
    assert total == od.size == d.size > 0 and d.tolist() == od.tolist() and _bits(s) == _bits(os_)
    without = po.rows(ix, po.Q(shoulds))[0]
    assert d.size < without.size


LONE = [("main", c) for c in (po.WIDE, po.C0, po.C1, po.C63, po.C64, po.C65, po.FULL, po.ONE, po.TWO)] + \
       [("deleted", c) for c in (po.WIDE, po.C65, po.FULL)] + [("pb", c) for c in (pb.AB, pb.BC, pb.ABC, pb.GAP, pb.ABA)]


@pytest.mark.parametrize("which,c", LONE, ids=["%s: %r" % (w, c.terms) for w, c in LONE])
def test_a_lone_phrase_clause_equals_phrase_search(indexes, which, c):
    """0.0f + score == score for every score the phrase scorer yields: the one-child disjunction is the phrase search (live docs too)."""
    ix = indexes[which]
    fx = ix.fxs[0]
    d, s = po.rows(ix, po.Q([c]))
    od, os_, total = ix.ixs[0].phrase_search(list(c.terms), fx.max_doc, fx.norms, *ix.stats, offsets=pb.phrase_positions(c), live_docs=ix.live(0))
    assert total == od.size == d.size and d.tolist() == od.tolist() and _bits(s) == _bits(os_)


MSM_SETS = [("main", q) for q in po.MSM_QUERIES + po.WINDOW_QUERIES + po.BUCKET_QUERIES] + [("pb", q) for q in po.PB_QUERIES] + \
           [("pb", po.Q(q.shoulds, msm=m)) for q in po.PB_QUERIES[:6] for m in (2, 3)]


@pytest.mark.parametrize("which,q", MSM_SETS, ids=["%s: %s msm %d" % (w, q.name, q.msm) for w, q in MSM_SETS])
def test_doc_sets_under_min_should_match_equal_mock_disjunction(indexes, oracle, which, q):
    """DisjunctionSumScorer over mock children that hold the clauses' doc lists (a mock child scores its doc id: a doc on n children
    sums to n * doc): the same docs, and the same number of children on each."""
    ix = indexes[which]
    fx = ix.fxs[0]
    lists = [sorted(ix.clause_scores(0, c)) for c in po.present(fx, q)]
    got = po.leaf_rows(ix, 0, po.Q(q.shoulds, msm=q.msm))
    if not lists:
        assert got == {}
        return
    docs, scores = oracle.mock_disjunction(lists, max(q.msm, 1))
    assert docs == sorted(got)
    held = {d: sum(d in set(lst) for lst in lists) for d in docs}
    assert all(s == float(held[d] * d) for d, s in zip(docs, scores))


def test_the_sum_order_cases_are_order_sensitive(indexes):
    """The same three clauses as P T T, T P T and T T P: some doc's f32 sum differs in bits between two of the orders, so a kernel
    that added the phrase's score first (or last) everywhere cannot pass by luck. The doc sets are the same."""
    ix = indexes["pb"]
    got = [po.rows(ix, q) for q in po.SUM_ORDER]
    as_map = [dict(zip(d.tolist(), _bits(s))) for d, s in got]
    assert as_map[0].keys() == as_map[1].keys() == as_map[2].keys() and len(as_map[0]) > 100
    three = [d for d in as_map[0] if d in ix.clause_scores(0, pb.AB) and d in ix.clause_scores(0, pb.T129) and d in ix.clause_scores(0, pb.D600)]
    assert len(three) >= 10
    assert any(as_map[0][d] != as_map[1][d] for d in three) or any(as_map[0][d] != as_map[2][d] for d in three)
    assert any(as_map[1][d] != as_map[2][d] for d in three) or any(as_map[0][d] != as_map[2][d] for d in three)
    # and leaf_rows's `order` says the same: query order against the phrase moved to the end
    right, wrong = po.leaf_rows(ix, 0, po.SUM_ORDER[0]), po.leaf_rows(ix, 0, po.SUM_ORDER[0], order=[1, 2, 0])
    assert right.keys() == wrong.keys() and any(f32(right[d]).view(np.uint32) != f32(wrong[d]).view(np.uint32) for d in right)


def test_the_fixtures_hold_the_edges_they_are_there_for(indexes):
    main, pbm, leaves, deleted = indexes["main"], indexes["pb"], indexes["leaves"], indexes["deleted"]
    fx = main.fxs[0]
    B = po.BUCKET
    assert fx.max_doc == po.MAIN_DOCS and (fx.max_doc + B - 1) // B == 4
    wide = sorted(main.clause_scores(0, po.WIDE))
    assert wide == po.WIDE_MATCHES and set(po.WIDE_EDGES) <= set(wide) and wide[0] == 0 and wide[-1] == fx.max_doc - 1
    assert {B - 1, B, 2 * B - 1, 255, 256} <= set(wide) and len(fx.postings[po.W1]) // 128 == 3 and 0 < len(wide) < len(fx.postings[po.W1])
    for n, c in po.COUNTS.items():
        got = sorted(main.clause_scores(0, c))
        assert got == po.count_matches(n) and sum(B <= d < 2 * B for d in got) == n and pb.clause_cost(fx, c) > len(got)
    full = sorted(main.clause_scores(0, po.FULL))
    assert full == list(range(0, B)) + list(range(2 * B, 3 * B)) and pb.clause_cost(fx, po.FULL) == 2 * B + 10
    assert pb.clause_cost(fx, po.ONE) == 1 and sorted(main.clause_scores(0, po.ONE)) == [1500]
    assert pb.clause_cost(fx, po.TWO) == 2 and sorted(main.clause_scores(0, po.TWO)) == [10, 3000]
    by = {q.name: q for q in po.MAIN_QUERIES + po.PB_QUERIES + po.LEAF_QUERIES}
    hits = lambda ix, name: po.rows(ix, by[name])[0].tolist()   # noqa: E731
    # phrase-only docs: hits of [WIDE, T5], gone under MUST_NOT / deletion
    assert set(po.PHRASE_ONLY) <= set(hits(main, "window edges")) and {1023, 3099} <= set(po.PHRASE_ONLY)
    assert not {1023, 3099} & set(hits(main, "MUST_NOT removes phrase-only docs")) and {1023, 3099} <= set(hits(main, "candidates appended by four wavefronts"))
    assert hits(main, "MUST_NOT twice and absent") == [d for d in hits(main, "window edges") if d not in po.NOT1_DOCS]
    assert not {0, 1023, 1100, 3099} & set(po.rows(deleted, by["window edges"])[0].tolist())
    # min_should_match: 2 of 3 keeps fewer docs than 1, n keeps some, n + 1 none; a dropped clause does not lower it
    n1, n2, n3 = len(hits(main, "dense, phrase, sparse")), len(hits(main, "msm 2 of 3")), len(hits(main, "msm n"))
    assert n1 > n2 > n3 > 0 and hits(main, "msm n + 1") == [] and hits(main, "msm 3, a phrase dropped: nothing can reach it") == []
    assert 0 < len(hits(main, "msm 2, a clause absent")) < len(hits(main, "a dense term beside the phrase"))
    assert hits(main, "every clause absent") == [] and hits(main, "absent terms around the phrase") == hits(main, "the lone wide phrase")
    assert hits(main, "candidates, no match, alone") == [] and len(hits(main, "0 matches in bucket 1")) == 5
    assert len(hits(main, "a dense term beside the phrase")) > 129
    # boost 0: the docs of the boost-1 query; the phrase-only ones score +0.0 and are hits
    zero = po.rows(pbm, by["boost 0: the phrase-only docs count"])
    assert sorted(zero[0].tolist()) == sorted(po.rows(pbm, po.Q([pb.AB, pb.R20]))[0].tolist())
    only = set(pbm.clause_scores(0, pb.AB)) - set(pbm.clause_scores(0, pb.R20))
    assert only and all(_bits([s])[0] == 0 for d, s in zip(*zero) if d in only)
    ab, r20, t40 = (set(pbm.clause_scores(0, c)) for c in (pb.AB, pb.R20, pb.T40))
    two = hits(pbm, "boost 0 counts towards msm")
    assert any(d in ab and (d in r20) != (d in t40) for d in two) and all((d in ab) + (d in r20) + (d in t40) >= 2 for d in two)
    # the same phrase twice: every score is s + s
    twice, once = po.rows(pbm, by["the same phrase twice"]), pbm.clause_scores(0, pb.AB)
    assert all(f32(s) == f32(f32(once[d]) + f32(once[d])) for d, s in zip(*twice)) and twice[0].size == len(once)
    assert pb.ELEVEN_DOC in hits(pbm, "eleven positions in a doc")
    # the leaves
    q = by["a leaf without the term, a leaf without the phrase"]
    assert [len(po.present(fx_, q)) for fx_ in leaves.fxs] == [2, 1, 1] and all(po.leaf_rows(leaves, li, q) for li in range(3))
    q = by["a leaf without every clause"]
    assert [len(po.present(fx_, q)) for fx_ in leaves.fxs] == [2, 2, 0] and po.leaf_rows(leaves, 0, q) and not po.leaf_rows(leaves, 2, q)


def test_routing_and_refusals_of_the_mirror():
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    G = rucene_amd.GpuIndexSearcher
    q = B.build([], [P([1, 2]), T(3), P([4, 5], [0, 3])], must_nots=[T(6)], min_should_match=2)
    assert isinstance(q, B) and q.has_phrases() and not q.must_queries and not q.filter_queries
    shoulds, nots, msm = G.phrase_or_parts(q)
    assert [type(c) for c in shoulds] == [P, T, P] and [t.term for t in nots] == [6] and msm == 2
    assert G.phrase_or_parts(B.build([], [P([1, 2]), T(3)]))[2] == 1              # BooleanQuery::build makes 0 a 1
    assert isinstance(B.build([], [P([1, 2])]), P)                                  # a lone SHOULD phrase is that PhraseQuery
    assert isinstance(B.build([], [P([1, 2])], must_nots=[T(3)]), B)
    nine = [P([1, 2])] + [T(10 + i) for i in range(8)]
    assert len(G.phrase_or_parts(B.build([], nine))[0]) == 9
    for bad in (B.build([], [P([1, 2], slop=1), T(3)]), B.build([], nine + [T(99)]), B.build([], [T(3), T(4)], must_nots=[P([1, 2])]),
                B.build([], [P([1, 2]), T(3)], must_nots=[P([4, 5])]), B.build([], [P([1, 2]), B.build([T(3), T(4)], [])]),
                B.build([], [P([1, 2]), P([2, 3]), P([3, 4]), P([4, 5]), P([5, 6])]), B.build([P([1, 2])], [T(3)])):
        with pytest.raises(rucene_amd.RgpuError) as e:
            G.phrase_or_parts(bad)
        assert e.value.status == -5


def test_the_pinned_shapes_still_refuse_through_phrase_bool_parts():
    """Every shape with a MUST or FILTER clause keeps going to phrase_bool_parts, which answers as before."""
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    G = rucene_amd.GpuIndexSearcher
    for bad in (B.build([P([1, 2], slop=1), T(3)], []), B.build([T(3)], [P([1, 2]), T(4)]), B.build([T(3), T(5)], [], must_nots=[P([1, 2])]),
                B.build([P([1, 2])], [T(3)]), B.build([P([1, 2])] * 5, []), B.build([], [P([1, 2])], filters=[T(3)])):
        assert bad.must_queries or bad.filter_queries
        with pytest.raises(rucene_amd.RgpuError) as e:
            G.phrase_bool_parts(bad)
        assert e.value.status == -5
    # phrase_bool_parts itself is what it was for a disjunction too (search_batch no longer asks it about one)
    with pytest.raises(rucene_amd.RgpuError) as e:
        G.phrase_bool_parts(B.build([], [P([1, 2]), T(3)]))
    assert e.value.status == -5
    ok = G.phrase_bool_parts(B.build([P([1, 2]), T(3)], [], must_nots=[T(4)]))
    assert len(ok[0]) == 2 and ok[1] == 2


def test_header_export_and_layout_of_the_new_struct(tmp_path):
    """include/rucene_gpu.h declares rgpu_search_phrase_or_batch, the library exports it, _lib binds it, and what the C compiler lays
    out for rgpu_phrase_or_query is what PHRASE_OR_QUERY_DTYPE assumes."""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from rucene_amd import _lib
    assert "rgpu_search_phrase_or_batch" in _lib.EXPORTS and hasattr(C.CDLL(_lib.lib_path()), "rgpu_search_phrase_or_batch")
    assert _lib.lib().rgpu_abi_version() == 6
    dt = _lib.PHRASE_OR_QUERY_DTYPE
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "rucene_gpu.h"), "int main(void) {",
             '  printf("%zu %d", sizeof(rgpu_phrase_or_query), RGPU_MAX_BOOL_PHRASES);']
    lines += ['  printf(" %s=%%zu", offsetof(rgpu_phrase_or_query, %s));' % (f, f) for f in dt.names]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-o", exe, str(src)])
    parts = subprocess.check_output([exe], text=True).split()
    assert int(parts[0]) == dt.itemsize == 48 and dt.itemsize % 8 == 0
    assert int(parts[1]) == _lib.MAX_BOOL_PHRASES == dt.fields["phrase_slot"][0].shape[0]
    assert parts[2:] == ["%s=%d" % (f, dt.fields[f][1]) for f in dt.names]


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/phrase_or_plan_test.cpp: the clause order, dropped clauses, dead queries, capacities, MUST_NOT terms and the limits
    of csrc/host/phrase_or_plan.hpp, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "phrase_or_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "phrase_or_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("phrase_or_plan_test OK"), out.stdout
