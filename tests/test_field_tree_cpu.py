"""tests/field_tree.py proves itself (no GPU): TreeRef against the oracle's own searches where every clause sits in field 0, every
mutant caught by some fixture, the preconditions the GPU tests rely on, the host plan under the sanitizers, the struct layouts, and
QueryStringQueryBuilder against query_string.rs's rules."""
import os
import subprocess

import numpy as np
import pytest

import cross_field as cf
import field_tree as ft
from field_tree import T, sum_, term, tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def _same(a, b):
    return a[2] == b[2] and a[0].size == b[0].size and (a[0] == b[0]).all() and (_bits(a[1]) == _bits(b[1])).all()


@pytest.fixture(scope="module")
def leaf():
    return ft.TreeLeaf("seeded")


@pytest.fixture(scope="module")
def ref(oracle, leaf):
    return ft.TreeRef(oracle, leaf)


ONE_FIELD = [(["S100"], ["ALL"], []), (["S101"], ["THIRD", "ALL"], []), (["KEEPS_STATE"], ["ALL"], []), (["DEAD_ALL", "HOLD"], ["ALL", "THIRD"], ["BAN"]),
             (["EQUAL"], ["ALL"], []), (["DEAD_DEL"], ["THIRD"], []), (["DF_257", "HOLD", "ALL"], ["THIRD"], ["BAN"])]


@pytest.mark.parametrize("exact", [False, True], ids=["rule", "add"])
def test_one_field_trees_equal_the_oracles_req_opt_search(oracle, leaf, ref, exact):
    """+a [+b] c [d] -n over field 0 alone, as term groups and as sum groups of one clause: search_opt with the rule and with exact=True"""
    osr = leaf.searcher(oracle, 0)
    for musts, shoulds, nots in ONE_FIELD:
        m, s, n = [T[x] for x in musts], [T[x] for x in shoulds], [T[x] for x in nots]
        want = osr.search_opt(oracle.OP_TERM if len(m) == 1 else oracle.OP_AND, m, s, 5000, must_not_ids=n, exact=exact)
        assert want[2] > 100
        q = tree([term(0, t) for t in m], [term(0, t) for t in s], must_not=[(0, t) for t in n])
        assert _same(ref.rows(q, rule=not exact), want), (musts, shoulds, nots)
        q = tree([sum_([(0, t)]) for t in m], [sum_([(0, t)]) for t in s], must_not=[(0, t) for t in n])
        assert _same(ref.rows(q, rule=not exact), want), ("sum groups of one", musts, shoulds, nots)
        # the optional side as ONE sum group: 0.0f + (0.0f + c + d) has the bits of 0.0f + c + d
        q = tree([term(0, t) for t in m], [sum_([(0, t) for t in s])], must_not=[(0, t) for t in n])
        assert _same(ref.rows(q, rule=not exact), want), ("one optional sum group", musts, shoulds, nots)


def test_one_field_trees_equal_the_oracles_or_and_nested_searches(oracle, leaf, ref):
    osr = leaf.searcher(oracle, 0)
    a, b, c = T["THIRD"], T["S101"], T["KEEPS_STATE"]
    assert _same(ref.rows(tree(should=[sum_([(0, a)]), sum_([(0, b)]), term(0, c)])), osr.search(oracle.OP_OR, [a, b, c], 5000))
    assert _same(ref.rows(tree(should=[sum_([(0, a), (0, b), (0, c)])])), osr.search(oracle.OP_OR, [a, b, c], 5000))
    assert _same(ref.rows(tree([sum_([(0, a)]), term(0, T["HOLD"]), sum_([(0, T["ALL"])])])), osr.search(oracle.OP_AND, [a, T["HOLD"], T["ALL"]], 5000))
    # "+a +(b c)": ConjunctionScorer over [a, DisjunctionSumScorer(b, c)] from its parts, the cheaper child first
    held_a, sc_a, cost_a = ref.group(term(0, T["HOLD"]))
    held_n, sc_n, cost_n = ref.group(sum_([(0, b), (0, c)]))
    d, s = ref.scores(tree([term(0, T["HOLD"]), sum_([(0, b), (0, c)])]))
    assert cost_n < cost_a and (d == np.flatnonzero(held_a & held_n & leaf.alive)).all()
    assert (_bits(s) == _bits((sc_n[d] + sc_a[d]).astype(np.float32))).all()      # the cheaper child first


def test_every_mutant_is_caught_by_some_fixture(oracle):
    leaves = [ft.TreeLeaf("seeded", which="A"), ft.TreeLeaf("seeded", which="B")]
    refs = ft.index_refs(oracle, leaves)
    queries = list(ft.rule_queries().values()) + list(ft.sum_queries().values()) + list(ft.emission_queries().values())
    good = [ft.index_rows(refs, q, 10000) for q in queries]
    for name, mut in ft.MUTANTS.items():
        bad_refs = ft.index_refs(oracle, leaves, **mut)
        caught = [i for i, q in enumerate(queries) if not _same(ft.index_rows(bad_refs, q, 10000), good[i])]
        assert caught, name


def test_the_preconditions_of_the_gpu_tests(oracle, leaf, ref):
    rq = ft.rule_queries()
    differs = 0
    for name, q in rq.items():
        docs, final, skipped, _ = ref.walk(q)
        assert skipped.any(), name
        differs += not _same(ref.rows(q, 128), ref.rows(q, 128, rule=False))
    assert differs
    # the 100th | 101st | 102nd scored doc: two | one | none of the 20 LOW docs behind 99 | 100 | 101 HIGH ones take the optional sum
    for name, taken in (("S99", 2), ("S100", 1), ("S101", 0)):
        docs, final, skipped, _ = ref.walk(rq[name])
        assert docs.size == int(name[1:]) + 20 and int((~skipped).sum()) == int(name[1:]) + taken, name
    # EQUAL: 2 * req == sum / num exactly on the 102nd doc, which is not skipped
    docs, final, skipped, _ = ref.walk(rq["EQUAL"])
    req = ref.clause((0, T["EQUAL"]))[1]
    s = np.float32(0)
    for r in req[:101]:
        s = np.float32(s + r)
    assert np.float32(2.0) * req[101] == s / np.float32(101) and not skipped[101] and skipped[102:].all()
    # dead docs, MUST_NOT-held docs: lead postings that are no hits, between hits
    lead = leaf.fields[0].lists[T["DEAD_ALL"]][0]
    docs = ref.walk(rq["DEAD_ALL"])[0]
    gone = np.setdiff1d(lead, docs)
    assert gone.size >= 20 and (~leaf.alive[gone]).any() and np.isin(gone, leaf.fields[0].lists[T["BAN"]][0]).any() and gone.min() < docs.max()
    # optional postings on non-matching docs, and hits no optional group holds
    docs = ref.walk(rq["OPT_MISS"])[0]
    third = leaf.fields[0].lists[T["THIRD"]][0]
    assert 0 < np.isin(docs, third).sum() < docs.size and np.setdiff1d(third, docs).size
    # some doc's nested sum differs in bits from the flat clause-order sum; some doc's cost-order sum from its clause-order sum
    sq = ft.sum_queries()
    q = sq["nested against flat"]
    assert (_bits(ref.scores(q)[1]) != _bits(ref.scores(ft.flat(q))[1])).any()
    q = sq["sum cost below a term"]
    assert [g[2] for g in ref.order(dict(occur="must", groups=q["must"], msm=0, must_not=[]))] == [2400, 4099]
    q = sq["sum cost above a term"]
    req_q = dict(occur="must", groups=q["must"], msm=0, must_not=[])
    assert [g[2] for g in ref.order(req_q)] == [2000, 4099, 4499]
    assert (_bits(ref.scores(q)[1]) != _bits(cf.CrossRef.scores(ref, req_q, [ref.group(g) for g in q["must"]])[1])).any()
    for name in ("sum cost equal to a term's, sum second", "sum cost equal to a term's, sum first"):
        assert [g[2] for g in ref.order(dict(occur="must", groups=sq[name]["must"], msm=0, must_not=[]))] == [4099, 4099, 4099]
    a, b = ref.scores(sq["sum cost equal to a term's, sum second"])[1], ref.scores(sq["sum cost equal to a term's, sum first"])[1]
    assert (_bits(a) != _bits(b)).any()      # the stable order is the clause order
    # the emission fixtures: n hits inside one 256-doc scan step, the leaf's two ends, a lead group that counts docs twice
    eq = ft.emission_queries()
    for b_, n in ((ft.B_63, 63), (ft.B_64, 64), (ft.B_65, 65)):
        docs = ref.walk(eq["%d hits in a step" % n])[0]
        lst = leaf.fields[1].lists[b_][0]
        assert lst.size == n and (lst // 256 == ft.STEP_OF[b_] // 256).all() and 0 < docs.size <= n
    lst = leaf.fields[1].lists[ft.B_ENDS][0]
    assert lst.tolist() == [0, ft.MAX_DOC - 1]
    shared = np.intersect1d(leaf.fields[0].lists[T["S100"]][0], leaf.fields[1].lists[ft.B_HALF100][0])
    assert shared.size == 60
    assert ft.MAX_DOC == 8 * ft.W + 3
    assert np.unique(leaf.fields[0].norms).size <= 64 < np.unique(leaf.fields[1].norms).size and leaf.fields[2].norms is None
    # the nine-clause sum group has nine present clauses; the absent-group queries are what their names say
    assert all(ref.df(c) > 0 for c in ft.NINE) and len(ft.NINE) == 9
    assert ref.rows(sq["every group absent"])[2] == 0 and ref.rows(sq["a group absent under MUST"])[2] == 0 and ref.rows(sq["dead beside SHOULD"])[2] == 0
    must_alone = sq["MUST side alone"]
    assert _same(ref.rows(must_alone), ref.rows(tree(must_alone["must"])))


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/fields_tree_plan_test.cpp: csrc/host/fields_tree_plan.hpp as a stand-alone program built with
    -fsanitize=address,undefined"""
    exe = str(tmp_path / "fields_tree_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "fields_tree_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("fields_tree_plan_test OK"), out.stdout


def test_struct_layouts_match_the_header(tmp_path):
    from rucene_amd import _lib
    structs = {"rgpu_field_tree_group": _lib.FIELD_TREE_GROUP_DTYPE, "rgpu_fields_tree_query": _lib.FIELDS_TREE_QUERY_DTYPE,
               "rgpu_field_clause": _lib.FIELD_CLAUSE_DTYPE, "rgpu_field_group": _lib.FIELD_GROUP_DTYPE, "rgpu_fields_query": _lib.FIELDS_QUERY_DTYPE}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "rucene_gpu.h"), "int main(void) {"]
    for name, dt in structs.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (name, name))
        for field in dt.names:
            lines.append('  printf(" %s=%%zu", offsetof(%s, %s));' % (field, name, field))
        lines.append('  printf("\\n");')
    lines += ['  printf("%d\\n", RGPU_GROUP_SUM);', "  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-o", exe, str(src)])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    for line, (name, dt) in zip(out, structs.items()):
        parts = line.split()
        assert parts[0] == name and int(parts[1]) == dt.itemsize, line
        assert parts[2:] == ["%s=%d" % (f, dt.fields[f][1]) for f in dt.names], line
    assert int(out[-1]) == _lib.GROUP_SUM == ft.KIND["sum"]
    assert "rgpu_search_fields_tree_batch" in _lib.EXPORTS


# ---- QueryStringQueryBuilder ----------------------------------------------------------------------------------------------------------
def _shape(q):
    import rucene_amd as r
    if isinstance(q, r.TermQuery):
        return (q.field, q.term.decode("utf-8"), float(np.float32(q.boost)))
    if isinstance(q, r.PhraseQuery):
        return ("phrase", q.field, tuple(t.decode("utf-8") for t in q.terms), q.slop, float(np.float32(q.boost)))
    assert isinstance(q, r.BooleanQuery) and not q.must_not_queries and not q.filter_queries
    return dict(must=[_shape(c) for c in q.must_queries], should=[_shape(c) for c in q.should_queries], msm=q.min_should_match)


def test_query_string_builder():
    import rucene_amd as r
    one, two = [("title", 1.0)], [("title", 2.0), ("body", 0.5)]
    def build(s, fields, msm=0, boost=1.0):
        return _shape(r.QueryStringQueryBuilder(s, fields, msm, boost).build())
    def word(w, b=1.0):
        return dict(must=[], should=[("title", w, 2.0 * b), ("body", w, 0.5 * b)], msm=1)
    # one field: a word is a TermQuery, a level of one clause is that clause, `boost` is unused
    assert build("kernel", one, 0, 7.0) == ("title", "kernel", 1.0)
    assert build("+kernel", one) == ("title", "kernel", 1.0)
    assert build("(wave^0.25 | lane^4)", one) == dict(must=[], should=[("title", "wave", 0.25), ("title", "lane", 4.0)], msm=1)
    assert build('wave^0.25 "lane"^4', one) == dict(must=[], should=[("title", "wave", 0.25), ("title", "lane", 4.0)], msm=1)
    assert build("+wave lane +tile", one) == dict(must=[("title", "wave", 1.0), ("title", "tile", 1.0)], should=[("title", "lane", 1.0)], msm=0)
    assert build("+(wave lane) tile", one) == dict(must=[dict(must=[], should=[("title", "wave", 1.0), ("title", "lane", 1.0)], msm=1)],
                                                   should=[("title", "tile", 1.0)], msm=0)
    # several fields: every word a nested should-only BooleanQuery, the field's boost times the word's
    assert build("gpu", two) == word("gpu")
    assert build("gpu +search", two) == dict(must=[word("search")], should=[word("gpu")], msm=0)
    assert build("gpu|search^2", two) == word("gpu|search", 2.0)                                         # `|` inside a word is the word's
    assert build("gpu | search^2", two) == dict(must=[], should=[word("gpu"), word("search", 2.0)], msm=1)
    assert build("+gpu +(tile | lane)", two) == dict(must=[word("gpu"), dict(must=[], should=[word("tile"), word("lane")], msm=1)], should=[], msm=0)
    # min_should_match is handed to every nested build
    q = build("a b c", two, 2)
    assert q["msm"] == 2 and all(c["msm"] == 2 for c in q["should"])
    # phrases: one boosted PhraseQuery per field; the quote swallows the character behind it
    assert build('"wave front"~2', one) == ("phrase", "title", ("wave", "front"), 2, 1.0)
    assert build('"wave front"~1 +lane', two) == dict(
        must=[word("lane")], should=[dict(must=[], should=[("phrase", "title", ("wave", "front"), 1, 2.0), ("phrase", "body", ("wave", "front"), 1, 0.5)], msm=1)],
        msm=0)
    assert build('"lane"+tile', one) == dict(must=[], should=[("title", "lane", 1.0), ("title", "tile", 1.0)], msm=1)   # the `+` is gone
    # errors: IllegalArgument, as the reference bails
    for bad in ("", "   ", "lane)", '"one"~2', "lane^x", '"a b"~x'):
        with pytest.raises(r.RgpuError) as e:
            r.QueryStringQueryBuilder(bad, one, 0, 1.0).build()
        assert e.value.status == -2, bad
    assert build("(lane tile", one) == dict(must=[], should=[("title", "lane", 1.0), ("title", "tile", 1.0)], msm=1)     # an open parenthesis ends with the string
    assert build("() lane", one) == ("title", "lane", 1.0)                                                              # a nested parse that fails is dropped
    # terms by id for leaves without a dictionary
    ids = {"gpu": 3, "search": 9}
    q = r.QueryStringQueryBuilder("gpu +search", two, 0, 1.0, term=lambda f, w: ids[w]).build()
    assert [t.term for t in q.must_queries[0].should_queries] == [9, 9] and [t.field for t in q.should_queries[0].should_queries] == ["title", "body"]
