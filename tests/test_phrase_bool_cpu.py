"""The fixtures and the composed reference of tests/phrase_bool.py, proven without a GPU: a brute-force derivation written from the
holdings (phrase frequency by position arithmetic, BM25 in np.float32 from Searcher.term_weight) agrees with the composed reference
bit for bit on every fixture query; the order cases really are order-sensitive; degenerate queries equal the oracle alone;
BooleanQuery.build's rules for phrase clauses; the new struct's layout against a C compile of the header; the host plan
(csrc/host/phrase_bool_plan.hpp) under the sanitizers as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import phrase_bool as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
K1 = f32(1.2)


@pytest.fixture(scope="module")
def indexes(oracle):
    out = {"main": pb.Index(oracle, [pb.main()]), "groups": pb.Index(oracle, [pb.groups()]), "leaves": pb.Index(oracle, pb.leaves()),
           "deleted": pb.Index(oracle, [pb.main()], deleted=[{0, 254}])}
    yield out
    for ix in out.values():
        ix.close()


ALL = [("main", q) for q in pb.MAIN_QUERIES] + [("groups", q) for q in pb.GROUP_QUERIES] + [("leaves", q) for q in pb.LEAF_QUERIES] + \
      [("deleted", q) for q in pb.MAIN_QUERIES[:4]]


# ---- the brute-force derivation -----------------------------------------------------------------------------------------------------
def _bm25(weight, freq, norm_value):
    """BM25SimScorer::compute_score in f32: weight * (k1 + 1) * freq / (freq + norm)"""
    wk = f32(f32(weight) * f32(K1 + f32(1.0)))
    return f32(f32(wk * f32(freq)) / f32(f32(freq) + f32(norm_value)))


def _phrase_freq(holding, c):
    offs = pb.phrase_positions(c)
    if any(t not in holding for t in c.terms):
        return 0
    starts = set(p - offs[0] for p in holding[c.terms[0]])
    for t, o in zip(c.terms[1:], offs[1:]):
        starts &= set(p - o for p in holding[t])
    return len(starts)


def _holdings(fx):
    h = {}
    for t, pl in enumerate(fx.postings):
        for d, ps in pl:
            h.setdefault(d, {})[t] = ps
    return h


def brute_force(ix, q):
    scored = {}
    for li, fx in enumerate(ix.fxs):
        req = q.required()
        if any(pb.clause_cost(fx, c) == 0 for c, _ in req):
            continue
        order = pb.cost_order(fx, q)
        for d, holding in _holdings(fx).items():
            if d in ix.deleted[li] or any(t in holding for t in q.must_nots):
                continue
            addends, ok = [], True
            for c, scoring in req:
                if isinstance(c, pb.Ph):
                    freq = _phrase_freq(holding, c)
                    # PhraseWeight: idf summed over the terms in f32 (each from the statistics leaf's doc_freq), times the boost
                    w = f32(0.0)
                    for t in c.terms:
                        w = f32(w + f32(ix.osr.term_weight(t, 1.0)[0]))
                    w = f32(w * f32(c.boost))
                    cache = ix.osr.term_weight(c.terms[0], 1.0)[1]
                else:
                    freq = len(holding.get(c, ()))
                    w, cache = ix.osr.term_weight(c, 1.0)
                if freq == 0:
                    ok = False
                    break
                addends.append(_bm25(w, freq, cache[fx.norms[d]]) if scoring else f32(0.0))
            if ok:
                scored[d + ix.bases[li]] = pb.sum_in_order([addends[i] for i in order])
    return pb.rank(scored)


@pytest.mark.parametrize("which,q", ALL, ids=[w + ": " + q.name for w, q in ALL])
def test_brute_force_agrees_with_the_composed_reference(indexes, which, q):
    ix = indexes[which]
    d, s = ix.rows(q)
    bd, bs = brute_force(ix, q)
    assert d.tolist() == bd.tolist(), (q, d[:10], bd[:10])
    assert s.view(np.uint32).tolist() == bs.view(np.uint32).tolist(), q


def test_the_fixtures_hold_the_edges_they_are_there_for(indexes):
    main, groups = indexes["main"], indexes["groups"]
    by_name = {q.name: q for q in pb.MAIN_QUERIES + pb.GROUP_QUERIES + pb.LEAF_QUERIES}
    hits = lambda ix, name: ix.rows(by_name[name])[0].tolist()   # noqa: E731
    assert hits(main, "singleton clause") == [pb.SINGLETON_DOC]
    assert {254, 256} <= set(hits(main, "block + one clause")) and {254, 256} <= set(hits(main, "tail-only clause"))
    assert pb.ELEVEN_DOC in hits(main, "eleven positions in plane 1") and len(main.fxs[0].postings[pb.PC][pb.PC_DOCS.index(pb.ELEVEN_DOC)][1]) == 11
    top = hits(main, "bitmap clause")[0]
    assert top in main.fxs[0].docs_of(pb.N1) and top not in hits(main, "MUST_NOT removes the top hit")
    assert len(hits(main, "three MUST_NOT")) < len(hits(main, "MUST_NOT removes the top hit")) < len(hits(main, "bitmap clause"))
    assert hits(main, "MUST_NOT absent from the leaf") == hits(main, "bitmap clause")
    assert hits(main, "a required term absent") == [] and hits(main, "a phrase term absent") == []
    assert len(hits(main, "four phrases")) >= 2 and len(hits(main, "a repeated term beside a term")) >= 3 and len(hits(main, "a gapped phrase")) >= 3
    # FILTER: the bits of the query without it, fewer docs
    with_f, without = main.rows(by_name["FILTER term"]), main.rows(by_name["bitmap clause"])
    scores = dict(zip(without[0].tolist(), without[1].view(np.uint32).tolist()))
    assert 0 < with_f[0].size < without[0].size
    assert all(scores[d] == s for d, s in zip(with_f[0].tolist(), with_f[1].view(np.uint32).tolist()))
    fp = main.rows(by_name["FILTER phrase"])
    plain = main.rows(pb.Q([pb.T129, pb.D600]))
    scores = dict(zip(plain[0].tolist(), plain[1].view(np.uint32).tolist()))
    assert 0 < fp[0].size < plain[0].size and all(scores[d] == s for d, s in zip(fp[0].tolist(), fp[1].view(np.uint32).tolist()))
    # boost 0: the docs of the boost-1 query, other scores
    assert sorted(hits(main, "boost 0")) == sorted(main.rows(pb.Q([pb.AB, pb.T129, pb.D600]))[0].tolist())
    # the groups
    assert [len(groups.leaf_rows(0, by_name[n])) for n in ("63 candidates", "64 candidates", "65 candidates", "no candidate", "236 hits")] == [32, 50, 65, 0, 236]
    odd = [d for d in hits(groups, "a group without survivors") if d < 128 and d % 2]
    assert odd == [] and len(hits(groups, "a group without survivors")) == 128
    # the leaves: hits in the first two, none in the third; the cost order differs
    leaves = indexes["leaves"]
    q = by_name["the cost order differs between the leaves"]
    assert pb.cost_order(leaves.fxs[0], q) == [1, 0, 2] and pb.cost_order(leaves.fxs[1], q) == [0, 1, 2]
    assert leaves.leaf_rows(0, q) and leaves.leaf_rows(1, q) and not leaves.leaf_rows(2, q)
    q = by_name["a leaf without the MUST term"]
    assert leaves.leaf_rows(0, q) and not leaves.leaf_rows(1, q)
    # deleted docs are gone
    assert not {0, 254} & set(indexes["deleted"].rows(pb.ORDER_CASES[0])[0].tolist()) and {0, 254} & set(main.rows(pb.ORDER_CASES[0])[0].tolist())


@pytest.mark.parametrize("q,wrong_order", list(zip(pb.ORDER_CASES, pb.WRONG_ORDERS)), ids=[q.name for q in pb.ORDER_CASES])
def test_the_order_cases_are_order_sensitive(indexes, q, wrong_order):
    """Some doc's f32 sum differs in bits between the stable cost order and the order a scorer would use that kept the query's
    order or broke a tie the other way: such a scorer cannot pass by luck."""
    ix = indexes["main"]
    assert pb.cost_order(ix.fxs[0], q) != wrong_order
    right = ix.leaf_rows(0, q)
    wrong = ix.leaf_rows(0, q, order=wrong_order)
    assert right.keys() == wrong.keys() and right
    differ = [d for d in right if f32(right[d]).view(np.uint32) != f32(wrong[d]).view(np.uint32)]
    assert differ, q


def test_degenerate_queries_equal_the_oracle_alone(indexes, oracle):
    """A phrase plus FILTER-only terms is phrase_search restricted to the FILTER docs; the docs of a conjunction are what the
    oracle's ConjunctionScorer over the same doc lists yields (a mock child scores its doc id: n children sum to n * doc)."""
    ix = indexes["main"]
    fx = ix.fxs[0]
    q = pb.Q([pb.AB], filters=[pb.T40, pb.D600])
    d, s = ix.rows(q)
    od, os_, total = ix.ixs[0].phrase_search([pb.PA, pb.PB], fx.max_doc, fx.norms, *ix.stats)
    keep = np.isin(od, list(set(fx.docs_of(pb.T40)) & set(fx.docs_of(pb.D600))))
    assert d.tolist() == od[keep].tolist() and s.view(np.uint32).tolist() == os_[keep].view(np.uint32).tolist() and 0 < d.size < total
    for q in pb.ORDER_CASES:
        lists = [sorted(ix.clause_scores(0, c)) for c, _ in q.required()]
        docs, scores = oracle.mock_conjunction(lists)
        assert docs == sorted(ix.leaf_rows(0, q)) and scores == [float(len(lists) * x) for x in docs]


def test_boolean_query_build_rules_for_phrase_clauses():
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    G = rucene_amd.GpuIndexSearcher
    q = B.build([P([1, 2]), T(3)], [], must_nots=[T(4)], filters=[T(5)])
    assert isinstance(q, B) and q.has_phrases() and not q.is_flat() and len(q.must_queries) == 2
    assert [t.term for t in q.extract_terms()] == [1, 2, 3, 5]
    required, n_must, nots = G.phrase_bool_parts(q)
    assert len(required) == 3 and n_must == 2 and [t.term for t in nots] == [4]
    lone = B.build([P([1, 2])], [])                       # a lone MUST phrase is that PhraseQuery (boolean_query.rs:66-75)
    assert isinstance(lone, P) and lone.boost == 1.0
    lone = B.build([], [], filters=[P([1, 2], slop=0)])   # a lone FILTER phrase: ConstantScoreQuery with boost 0
    assert isinstance(lone, P) and lone.boost == 0.0 and lone.terms == [1, 2]
    assert isinstance(B.build([P([1, 2])], [], must_nots=[T(3)]), B)   # MUST_NOT beside it: not collapsed
    assert not B.build([T(1), T(2)], []).has_phrases()
    for bad in (B.build([P([1, 2], slop=1), T(3)], []), B.build([T(3)], [P([1, 2]), T(4)]), B.build([T(3), T(5)], [], must_nots=[P([1, 2])]),
                B.build([P([1, 2])], [T(3)]), B.build([P([1, 2]), B.build([T(3), T(4)], [])], []),
                B.build([P([1, 2]), P([2, 3]), P([3, 4]), P([4, 5]), P([5, 6])], [])):
        with pytest.raises(rucene_amd.RgpuError) as e:
            G.phrase_bool_parts(bad)
        assert e.value.status == -5


def test_header_export_and_layout_of_the_new_struct(tmp_path):
    """include/rucene_gpu.h declares rgpu_search_phrase_bool_batch, the library exports it, _lib binds it, and what the C compiler lays
    out for rgpu_phrase_bool_query is what PHRASE_BOOL_QUERY_DTYPE assumes."""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from rucene_amd import _lib
    assert "rgpu_search_phrase_bool_batch" in _lib.EXPORTS and hasattr(C.CDLL(_lib.lib_path()), "rgpu_search_phrase_bool_batch")
    assert _lib.lib().rgpu_abi_version() == 6
    dt = _lib.PHRASE_BOOL_QUERY_DTYPE
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "rucene_gpu.h"), "int main(void) {",
             '  printf("%zu %d", sizeof(rgpu_phrase_bool_query), RGPU_MAX_BOOL_PHRASES);']
    lines += ['  printf(" %s=%%zu", offsetof(rgpu_phrase_bool_query, %s));' % (f, f) for f in dt.names]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-o", exe, str(src)])
    parts = subprocess.check_output([exe], text=True).split()
    assert int(parts[0]) == dt.itemsize == 48 and int(parts[1]) == _lib.MAX_BOOL_PHRASES == dt.fields["phrase_slot"][0].shape[0]
    assert parts[2:] == ["%s=%d" % (f, dt.fields[f][1]) for f in dt.names]


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/phrase_bool_plan_test.cpp: the reference order, the de-duplication, the plane layout, dead queries and the limits of
    csrc/host/phrase_bool_plan.hpp, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "phrase_bool_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "phrase_bool_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("phrase_bool_plan_test OK"), out.stdout
