"""tests/phrase_opt.py proven on the CPU: the composed reference against the oracle's ReqOptScorer where the oracle has one (queries
without a phrase), the rule fixtures against what they claim (a skipped doc in walk_rule's trace, every mutant changes a named
fixture's row), the order dependence of the optional sum, the opt-in routing's refusals, and the host plan
(tests/cpp/phrase_opt_plan_test.cpp) under the sanitizers. No GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import opt_spectrum as osp
import phrase_bool as pb
import phrase_opt as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def main_ix(oracle):
    ix = pb.Index(oracle, [pb.main()])
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def leaves_ix(oracle):
    ix = pb.Index(oracle, pb.leaves())
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def rule_ix(oracle):
    fx, deleted = po.rule("A")
    ix = pb.Index(oracle, [fx], deleted=[deleted])
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def two_ix(oracle):
    (a, da), (b, db) = po.rule("A"), po.rule("B")
    ix = pb.Index(oracle, [a, b], deleted=[da, db])
    yield ix
    ix.close()


def _bits(s):
    return np.asarray(s, np.float32).view(np.uint32).tolist()


def _same(a, b):
    return a[0].tolist() == b[0].tolist() and _bits(a[1]) == _bits(b[1])


@pytest.mark.parametrize("exact", [False, True])
def test_phraseless_queries_equal_the_oracle(oracle, main_ix, leaves_ix, two_ix, exact):
    """search_opt is the oracle's own ReqOptScorer over term clauses: every fixture query without a phrase that it can walk
    (PHRASELESS_WALKED; the rule fixture's RULE_PHRASELESS, which trips the rule in both leaves) must compose to its rows, with the
    rule and without."""
    n = 0
    assert po.skipped_docs(two_ix, po.RULE_PHRASELESS)
    for ix, queries in ((main_ix, po.PHRASELESS_WALKED), (leaves_ix, po.PHRASELESS_WALKED), (two_ix, [po.RULE_PHRASELESS])):
        for q in queries:
            d, s = po.rows(ix, q, exact=exact)
            od, os_, total = ix.osr.search_opt(oracle.OP_TERM if len(q.musts) == 1 else oracle.OP_AND, list(q.musts), list(q.shoulds), ix.max_doc,
                                               must_not_ids=list(q.must_nots), exact=exact)
            assert total == d.size and od.tolist() == d.tolist() and _bits(os_) == _bits(s), (q, exact)
            n += d.size
    assert n > 200


def test_the_fixture_queries_have_hits_and_the_presence_cases_do_what_they_say(main_ix):
    for q in po.MAIN_QUERIES:
        d, s = po.rows(main_ix, q)
        dead = q.name in ("an absent required term", "a required phrase lacking a term")
        assert (d.size == 0) == dead, q
    by = {q.name: q for q in po.MAIN_QUERIES}
    # every optional clause absent: the required scorer's row
    q = by["every optional clause absent"]
    assert not po.present(main_ix.fxs[0], q) and _same(po.rows(main_ix, q), main_ix.rows(q.req()))
    # an optional clause changes scores, never the hit set
    q = by['+"a b" c']
    d, s = po.rows(main_ix, q)
    rd, rs = main_ix.rows(q.req())
    assert sorted(d.tolist()) == sorted(rd.tolist()) and _bits(s) != _bits(rs)
    # a weight-0 optional phrase hits and adds +0.0: the row is the one without it, bit for bit
    with0, without = by["optional phrase of weight 0"], po.Q([po.D600], [po.T40])
    assert _same(po.rows(main_ix, with0), po.rows(main_ix, without))
    assert any(h for _, _, _, _, h in po.leaf_records(main_ix, 0, po.Q([po.D600], [po.AB0])))
    # FILTER-only required side: req is 0.0, the score is the optional sum
    q = by['#"a b" c']
    assert all(r == 0.0 for _, _, r, _, _ in po.leaf_records(main_ix, 0, q))


def test_join_fixture_edges(oracle):
    fx = po.join()
    ix = pb.Index(oracle, [fx])
    try:
        assert fx.docs_of(po.ENDS) == [fx.docs_of(po.R63)[0], fx.docs_of(po.R63)[-1]]
        assert max(fx.docs_of(po.BEFORE)) < min(fx.docs_of(po.R65)) and min(fx.docs_of(po.BEHIND)) > max(fx.docs_of(po.R65))
        assert 301 in fx.docs_of(po.R63) and 300 in fx.docs_of(po.O63) and 302 in fx.docs_of(po.O63) and 301 not in fx.docs_of(po.O63)
        for q in po.JOIN_QUERIES:
            recs = po.leaf_records(ix, 0, q)
            assert recs, q
            hits = sum(h for _, _, _, _, h in recs)
            if q.name in ("optional run of 0", "wholly before", "wholly behind", "optional phrase wholly before"):
                assert hits == (0 if q.name != "optional phrase wholly before" else len(recs) // 2 + 1), q
            else:
                assert 0 < hits <= len(recs), q
    finally:
        ix.close()


def test_rule_fixtures_trip_the_rule(rule_ix, two_ix):
    """Every fixture meant to trip the rule has a skipped doc in walk_rule's trace; the edges are where the fixture says."""
    fx = rule_ix.fxs[0]
    for name, q in po.RULE_QUERIES.items():
        skipped = po.skipped_docs(rule_ix, q)
        assert skipped, name
        tr = po.traces(rule_ix, q)[0]
        assert tr and any(two < mean for _, _, mean, two in tr), name
        # a skipped doc the optional PHRASE holds scores req alone
        recs = {d: (r, o, h) for d, _, r, o, h in po.leaf_records(rule_ix, 0, q)}
        d, s = po.rows(rule_ix, q)
        got = dict(zip(d.tolist(), s))
        for doc in skipped:
            r, o, h = recs[doc]
            assert h and o > 0 and got[doc].view(np.uint32) == np.float32(r).view(np.uint32), (name, doc)
    # S99: the first two LOW docs are the 100th and 101st scored docs and take the optional sum; S100: one; S101: none
    for t, name, taken in ((po.S99, "S99", 2), (po.S100, "S100", 1), (po.S101, "S101", 0)):
        low = [po.RULE_FIRST[t] + i for i, p in enumerate(po._seq("A")[t]) if (p.freq, p.byte) == po.LOW]
        assert sorted(set(low) - set(po.skipped_docs(rule_ix, po.RULE_QUERIES[name]))) == low[:taken], name
    # DEAD: deleted and MUST_NOT docs among the first 100 do not count - the first LOW doc is the 101st scored one and takes the sum
    dead_low = [po.RULE_FIRST[po.DEAD] + i for i, p in enumerate(po._seq("A")[po.DEAD]) if (p.freq, p.byte) == po.LOW]
    assert sorted(po.skipped_docs(rule_ix, po.RULE_QUERIES["DEAD"])) == dead_low[1:]
    dead = [m for _, m, _, _, _ in po.leaf_records(rule_ix, 0, po.RULE_QUERIES["DEAD"])]
    assert dead.count(False) == 25 and dead[:125].count(False) == 25
    # KEEP: the MID docs are skipped because the LOWs never entered the mean; the last two HIGH docs are not
    keep = po.skipped_docs(rule_ix, po.RULE_QUERIES["KEEP"])
    assert len(keep) == 33 and max(keep) == po.RULE_FIRST[po.KEEP] + 133
    # the second leaf starts afresh: its first 5 LOW docs take the optional sum there
    q = po.RULE_QUERIES["S101"]
    second = [d - two_ix.bases[1] for d in po.skipped_docs(two_ix, q) if d >= two_ix.bases[1]]
    assert second and min(second) >= po.RULE_FIRST[po.S101] + 110
    assert fx.max_doc == po.RULE_DOCS


MUTANT_FIXTURE = [("threshold 99", dict(threshold=99), "S99"), ("threshold 101", dict(threshold=101), "S101"), ("ge", dict(ge=True), "S100"),
                  ("update_on_skip", dict(update_on_skip=True), "KEEP"), ("count_dead", dict(count_dead=True), "DEAD")]


@pytest.mark.parametrize("what,flags,name", MUTANT_FIXTURE)
def test_each_mutant_changes_a_named_fixture(rule_ix, what, flags, name):
    q = po.RULE_QUERIES[name]
    assert not _same(po.rows(rule_ix, q), po.rows(rule_ix, q, **flags)), (what, name)


def test_le_mutant_and_the_state_carried_across_leaves(oracle, two_ix):
    """`<=` for `<` changes EQUAL: the fixture's 102nd doc doubles to the f32 mean exactly (walk_rule's trace says so), so the strict
    rule lets it take the optional sum and the mutant skips it. The levels are those opt_spectrum.equal_search finds for the
    fixture's fixed statistics (run again here). The carried state is shown on the two-leaf index."""
    from rucene_amd import _lib
    fx = po.equal()
    w, _idf, cache = _lib.bm25_compute_weight(1.2, 0.75, fx.max_doc, fx.doc_count, fx.sum_ttf, [po.EQUAL_DF], 1.0)
    assert osp.equal_search(w, cache) == po.EQUAL_FOUND
    ix = pb.Index(oracle, [fx])
    try:
        tr = po.traces(ix, po.EQUAL_QUERY)[0]
        at = [t for t in tr if t[0] == po.EQUAL_DOC - 1]
        assert len(at) == 1 and at[0][1] == 101 and at[0][3] == at[0][2], at
        assert po.EQUAL_DOC not in po.skipped_docs(ix, po.EQUAL_QUERY)
        assert not _same(po.rows(ix, po.EQUAL_QUERY), po.rows(ix, po.EQUAL_QUERY, le=True))
    finally:
        ix.close()
    q = po.RULE_QUERIES["S101"]
    assert not _same(po.rows(two_ix, q), po.rows(two_ix, q, carry=True))


def test_reordering_the_optional_addends_changes_score_bits(leaves_ix):
    q = po.ARITH
    base = po.rows(leaves_ix, q, exact=True)
    changed = 0
    for perm in itertools.permutations(range(3)):
        if perm == (0, 1, 2):
            continue
        scored = {}
        for li in range(len(leaves_ix.fxs)):
            n_present = len(po.present(leaves_ix.fxs[li], q))
            order = [i for i in perm if i < n_present]
            scored.update(po.leaf_rows(leaves_ix, li, q, exact=True, opt_order=order)[0])
        changed += not _same(base, pb.rank(scored))
    assert changed >= 1
    # ... beside a required sum whose cost order differs between the first two leaves
    assert pb.cost_order(leaves_ix.fxs[0], q) != pb.cost_order(leaves_ix.fxs[1], q)


def test_routing_is_opt_in_and_parts_refuse_what_the_call_cannot_express():
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    parts = rucene_amd.GpuIndexSearcher.phrase_opt_parts
    req, n_must, shoulds, nots, msm = parts(B.build([T(1), P([2, 3])], [P([4, 5]), T(6)], filters=[T(7)], must_nots=[T(8)], min_should_match=2))
    assert [type(c) for c in req] == [T, P, T] and n_must == 2 and [type(c) for c in shoulds] == [P, T] and len(nots) == 1 and msm == 2
    refused = [
        B.build([T(1)], [P([2, 3], slop=1)]),                                   # a sloppy clause
        B.build([P([2, 3], slop=2)], [T(1)]),
        B.build([T(1)], [P([2, 3])], must_nots=[P([4, 5])]),                    # a phrase under MUST_NOT
        B.build([T(1)], [P([2, 3]), B.build([T(4), T(5)], [])]),                # nested clauses beside a phrase
        B.build([T(1)], [P([2, 3])] + [T(10 + i) for i in range(9)]),           # ten optional clauses
        B.build([T(1)], [P([2, 3 + i]) for i in range(5)]),                     # five phrases on one side
        B.build([T(1), T(2)], [], filters=[P([2, 3])]),                         # no optional clause
        B.build([], [P([2, 3]), T(1)]),                                         # no required clause
    ]
    for q in refused:
        with pytest.raises(rucene_amd.RgpuError) as e:
            parts(q)
        assert e.value.status == po.UNSUPPORTED, q
    # the sibling parts keep raising what they raise
    with pytest.raises(rucene_amd.RgpuError) as e:
        rucene_amd.GpuIndexSearcher.phrase_bool_parts(B.build([P([2, 3])], [T(1)]))
    assert e.value.status == po.UNSUPPORTED and "SHOULD clauses beside a required phrase" in str(e.value)
    with pytest.raises(rucene_amd.RgpuError) as e:
        rucene_amd.GpuIndexSearcher.phrase_or_parts(B.build([T(1)], [P([2, 3])]))
    assert e.value.status == po.UNSUPPORTED
    import inspect
    assert inspect.signature(rucene_amd.GpuIndexSearcher.__init__).parameters["optional_phrases"].default is False


def test_struct_layout_matches_the_header(tmp_path):
    from rucene_amd import _lib
    dt = _lib.PHRASE_OPT_QUERY_DTYPE
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "rucene_gpu.h"), "int main(void) {",
             '  printf("%zu", sizeof(rgpu_phrase_opt_query));']
    lines += ['  printf(" %s=%%zu", offsetof(rgpu_phrase_opt_query, %s));' % (f, f) for f in dt.names]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-o", exe, str(src)])
    parts = subprocess.check_output([exe], text=True).split()
    assert int(parts[0]) == dt.itemsize == 64
    assert [p.split("=") for p in parts[1:]] == [[f, str(dt.fields[f][1])] for f in dt.names]


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/phrase_opt_plan_test.cpp: validation and every refusal, presence per leaf, dead queries, the cost order and the run
    capacities of csrc/host/phrase_opt_plan.hpp, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "phrase_opt_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "phrase_opt_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("phrase_opt_plan_test OK"), out.stdout
