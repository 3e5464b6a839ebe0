"""tests/cross_field.py (the cross-field reference) against what is already trusted, the host plan under the sanitizers and the new
structs' layouts. No GPU.

With every clause in ONE field the composition must give the oracle's own OP_OR / OP_AND rows and tests/dismax_ref.py's rows, bit
for bit; a few two-field docs are computed by hand from the BM25 expression with each field's own weight and norm cache."""
import os
import subprocess

import numpy as np
import pytest

import cross_field as cf
from dismax_ref import DismaxRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _leaf(max_doc=700, seed=5, alive_frac=None):
    """Two fields of different average length: `title` (narrow norms, short) and `body` (70 distinct norm bytes, long)"""
    rng = np.random.default_rng([max_doc, seed])
    dfs = (1, 5, 127, 128, 129, 256, 0, 400)
    title = cf.Field([(cf.spread(rng, max_doc, df), cf.freqs_of(rng, df)) for df in dfs], rng.integers(118, 126, size=max_doc), 9 * max_doc)
    body = cf.Field([(cf.spread(rng, max_doc, df), cf.freqs_of(rng, df)) for df in dfs], 60 + rng.permutation(max_doc) % 70, 80 * max_doc)
    alive = None if alive_frac is None else rng.random(max_doc) < alive_frac
    return cf.CrossLeaf(max_doc, [title, body], alive=alive)


@pytest.mark.parametrize("alive_frac", [None, 0.6], ids=["no-deletions", "seeded"])
def test_one_field_is_the_oracles_own_search(oracle, alive_frac):
    leaf = _leaf(alive_frac=alive_frac)
    ref = cf.CrossRef(oracle, leaf)
    for f in (0, 1):
        osr = leaf.searcher(oracle, f)
        for tids, msm in (([2, 3, 4], 0), ([7, 1, 5, 6, 0], 0), ([7, 5, 4, 3], 2), ([7, 5, 4], 3), ([6, 2], 0), ([6], 0)):
            d, s, total = osr.search(oracle.OP_OR, tids, leaf.max_doc, tie_mode=oracle.TIE_CANONICAL, min_should_match=msm)
            gd, gs, gt = ref.rows(cf.should([cf.term(f, t) for t in tids], msm=msm))
            assert gt == total and (gd == d).all() and (gs.view(np.int32) == s.view(np.int32)).all(), ("OR", f, tids, msm)
        # conjunctions: the clause order differs from the cost order, two equal costs included ([5, 5])
        for tids in ([7, 5, 2], [5, 7, 3, 4], [3, 2, 4], [5, 5, 7], [7, 6], [4]):
            d, s, total = osr.search(oracle.OP_AND, tids, leaf.max_doc, tie_mode=oracle.TIE_CANONICAL)
            gd, gs, gt = ref.rows(cf.must([cf.term(f, t) for t in tids]))
            assert gt == total and (gd == d).all() and (gs.view(np.int32) == s.view(np.int32)).all(), ("AND", f, tids)
        dref = DismaxRef(oracle, [leaf.view(f)])
        for tids in ([2, 3], [7, 6, 5, 1], [6, 3], [6, 6]):
            for tie in (0.0, 0.1, 1.0):
                d, s, total = dref.rows(tids, tie)
                gd, gs, gt = ref.rows(cf.should([cf.dismax(tie, [(f, t) for t in tids])]))
                assert gt == total and (gd == d).all() and (gs.view(np.int32) == s.view(np.int32)).all(), ("dismax", f, tids, tie)


def _bm25(ref, c, doc):
    """TermScorer's score of `doc` by hand: weight * (k1 + 1) * freq / (freq + cache[norm byte of THE CLAUSE'S field])"""
    fld = ref.leaf.fields[c[0]]
    w, cache = ref.weight(c)
    d, fr = fld.lists[c[1]]
    freq = np.float32(fr[np.searchsorted(d, doc)])
    wk = np.float32(np.float32(w) * np.float32(cf.K1 + 1.0))
    return np.float32(np.float32(wk * freq) / np.float32(freq + cache[fld.norms[doc]]))


def test_two_field_docs_by_hand(oracle):
    """Term 7 (df 400) of both fields: a doc in both lists whose norm bytes differ between the fields"""
    leaf = _leaf()
    ref = cf.CrossRef(oracle, leaf)
    a, b = (0, 7), (1, 7)
    both = np.intersect1d(leaf.fields[0].lists[7][0], leaf.fields[1].lists[7][0])
    both = both[leaf.fields[0].norms[both] != leaf.fields[1].norms[both]][:5]
    assert both.size == 5
    assert ref.weight(a)[1].tobytes() != ref.weight(b)[1].tobytes()   # different average lengths: different norm caches
    tie = np.float32(0.1)
    dm_docs, dm_scores = ref.scores(cf.should([cf.dismax(0.1, [a, b])]))
    or_docs, or_scores = ref.scores(cf.should([cf.term(*a), cf.term(*b)]))
    and_docs, and_scores = ref.scores(cf.must([cf.term(*b), cf.term(*a)]))
    for doc in both:
        sa, sb = _bm25(ref, a, doc), _bm25(ref, b, doc)
        total = np.float32(np.float32(np.float32(0.0) + sa) + sb)
        best = max(sa, sb)
        want = np.float32(best + np.float32(np.float32(total - best) * tie))
        assert dm_scores[np.searchsorted(dm_docs, doc)].view(np.int32) == want.view(np.int32)
        assert or_scores[np.searchsorted(or_docs, doc)].view(np.int32) == total.view(np.int32)
        assert and_scores[np.searchsorted(and_docs, doc)].view(np.int32) == np.float32(sa + sb).view(np.int32)   # equal costs: clause order b, a; a + b == b + a
        # the other field's norm byte would have given another score
        fld = leaf.fields[0]
        w, cache = ref.weight(a)
        freq = np.float32(fld.lists[7][1][np.searchsorted(fld.lists[7][0], doc)])
        wrong = np.float32(np.float32(np.float32(w) * np.float32(2.2)) * freq) / np.float32(freq + cache[leaf.fields[1].norms[doc]])
        assert np.float32(wrong) != sa
    only_a = np.setdiff1d(leaf.fields[0].lists[7][0], leaf.fields[1].lists[7][0])[:3]
    for doc in only_a:   # one disjunct on the doc: max + (sum - max) * tie over that one score
        sa = _bm25(ref, a, doc)
        total = np.float32(np.float32(0.0) + sa)
        assert dm_scores[np.searchsorted(dm_docs, doc)].view(np.int32) == np.float32(sa + np.float32(np.float32(total - sa) * tie)).view(np.int32)
        assert doc not in and_docs


def test_summation_order_matters_in_the_fixture(oracle):
    """(a + b) + c != a + (b + c) on some doc: a wrong order would show"""
    leaf = _leaf()
    ref = cf.CrossRef(oracle, leaf)
    q = cf.should([cf.term(0, 7), cf.term(1, 7), cf.term(1, 5)])
    docs, sc = ref.scores(q)
    gs = ref.order(q)
    _, other = ref.scores(q, order=[gs[2], gs[1], gs[0]])
    assert (sc.view(np.int32) != other.view(np.int32)).any()
    qm = cf.must([cf.term(0, 7), cf.term(1, 7), cf.term(1, 5)])   # costs 400, 400, 256: the order is 1:5, 0:7, 1:7 - (c + a) + b, not (a + b) + c
    gm = ref.order(qm)
    assert [g[2] for g in gm] == [256, 400, 400]
    docs, sc = ref.scores(qm)
    _, other = ref.scores(qm, order=[ref.group(g) for g in qm["groups"]])
    assert docs.size > 20 and (sc.view(np.int32) != other.view(np.int32)).any()


def test_presence_rules(oracle):
    leaf = _leaf()
    ref = cf.CrossRef(oracle, leaf)
    absent = (0, 6)
    assert ref.rows(cf.must([cf.term(1, 7), cf.term(*absent)]))[2] == 0
    assert ref.rows(cf.must([cf.term(1, 7), cf.dismax(0.5, [absent, (1, 6)])]))[2] == 0
    a = ref.rows(cf.should([cf.term(1, 7), cf.term(*absent)], msm=2))
    assert a[2] == 0    # the absent group drops, min_should_match stays: two groups can no longer hold a doc
    one = ref.rows(cf.should([cf.dismax(0.5, [absent, (1, 5)])]))
    plain = ref.rows(cf.should([cf.term(1, 5)]))
    assert one[2] == plain[2] == 256 and (one[1].view(np.int32) == plain[1].view(np.int32)).all()
    # a doc held by two disjuncts of ONE group counts once
    q = cf.should([cf.dismax(0.0, [(0, 7), (1, 7)]), cf.term(1, 1)], msm=2)
    docs, _ = ref.scores(q)
    assert set(docs) == set(np.intersect1d(np.union1d(leaf.fields[0].lists[7][0], leaf.fields[1].lists[7][0]), leaf.fields[1].lists[1][0]))
    # MUST_NOT in the other field
    q = cf.should([cf.term(0, 7)], must_not=[(1, 7)])
    assert set(ref.scores(q)[0]) == set(np.setdiff1d(leaf.fields[0].lists[7][0], leaf.fields[1].lists[7][0]))


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/fields_plan_test.cpp: validation and refusals, presence, dead queries, the stable MUST cost order, run capacities and
    item counts of csrc/host/fields_plan.hpp, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "fields_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "fields_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("fields_plan_test OK"), out.stdout


def test_struct_layouts_match_the_header(tmp_path):
    from rucene_amd import _lib
    structs = {"rgpu_field_clause": _lib.FIELD_CLAUSE_DTYPE, "rgpu_field_group": _lib.FIELD_GROUP_DTYPE, "rgpu_fields_query": _lib.FIELDS_QUERY_DTYPE,
               "rgpu_segment_field_info": _lib.SEGMENT_FIELD_INFO_DTYPE}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "rucene_gpu.h"), "int main(void) {"]
    for name, dt in structs.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (name, name))
        for field in dt.names:
            lines.append('  printf(" %s=%%zu", offsetof(%s, %s));' % (field, name, field))
        lines.append('  printf("\\n");')
    lines += ['  printf("%d %d %d %d %d %d %d %d %d\\n", RGPU_MAX_FIELDS, RGPU_MAX_FIELD_GROUPS, RGPU_MAX_GROUP_DISJUNCTS, RGPU_MAX_FIELDS_QUERY_CLAUSES, '
              'RGPU_GROUP_TERM, RGPU_GROUP_DISMAX, RGPU_OCCUR_SHOULD, RGPU_OCCUR_MUST, RGPU_OCCUR_FILTER);', "  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-o", exe, str(src)])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    for line, (name, dt) in zip(out, structs.items()):
        parts = line.split()
        assert parts[0] == name and int(parts[1]) == dt.itemsize, line
        assert parts[2:] == ["%s=%d" % (f, dt.fields[f][1]) for f in dt.names], line
    assert [int(x) for x in out[-1].split()] == [_lib.MAX_FIELDS, _lib.MAX_FIELD_GROUPS, _lib.MAX_GROUP_DISJUNCTS, _lib.MAX_FIELDS_QUERY_CLAUSES,
                                                  _lib.GROUP_TERM, _lib.GROUP_DISMAX, _lib.OCCUR_SHOULD, _lib.OCCUR_MUST, _lib.OCCUR_FILTER]


def test_the_docs_only_splice_reads_back(oracle):
    """docs_only_leaf: both fields decode from the ONE spliced file at their (moved) file pointers"""
    rng = np.random.default_rng(8)
    max_doc = 300
    body = cf.Field([(cf.spread(rng, max_doc, df), cf.freqs_of(rng, df)) for df in (130, 1, 40)], rng.integers(100, 120, size=max_doc), 50 * max_doc)
    ident = cf.Field([(cf.spread(rng, max_doc, df), np.ones(df, np.int32)) for df in (129, 1, 7, 256)], None, -1)
    leaf = cf.docs_only_leaf(oracle, max_doc, body, ident)
    whole_b = oracle.Segment(leaf.doc_bytes, None, max_doc, ident.terms, sum_total_term_freq=-1, has_freqs=False)
    for t, (d, _) in enumerate(ident.lists):
        assert (whole_b.decode_term(ident.terms[t])[0] == d).all()
    whole_a = oracle.Segment(leaf.doc_bytes, body.norms, max_doc, body.terms, sum_total_term_freq=body.sttf)
    for t, (d, f) in enumerate(body.lists):
        got = whole_a.decode_term(body.terms[t])
        assert (got[0] == d).all() and (got[1] == f).all()


class _RecordingCtx:
    def __init__(self):
        self.caches = []

    def sim_table(self, cache, k1):
        key = np.asarray(cache, np.float32).tobytes()
        if key not in self.caches:
            self.caches.append(key)
        return self.caches.index(key)


def test_python_mirror_packs_cross_field_rows(oracle):
    """GpuIndexSearcher without a context (packing is host-only): which rows are routed, what the call's arrays hold, and that a
    clause's weight and norm cache are its FIELD's - bit-equal to the per-field oracle searcher's"""
    import rucene_amd
    from rucene_amd import _lib
    leaf = _leaf()
    ref = cf.CrossRef(oracle, leaf)
    title, body = leaf.fields
    lr = rucene_amd.LeafReader(leaf.doc_bytes, title.norms, leaf.max_doc, title.terms, sum_total_term_freq=title.sttf, field="title")
    lr.add_field("body", body.norms, body.terms, sum_total_term_freq=body.sttf).slot = 1
    s = object.__new__(rucene_amd.GpuIndexSearcher)
    s.leaves, s.ctx, s.similarity, s._stats_leaf, s._weights = [lr], _RecordingCtx(), rucene_amd.BM25Similarity(), 0, {}
    s._stats_terms, s._field_weights = None, {}
    s.collection_statistics = rucene_amd.CollectionStatistics("title", 0, leaf.max_doc, leaf.max_doc, title.sttf)
    T, B, D = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.DisjunctionMaxQuery
    assert not s._names_other_field(B.build([T(1), T(2, field="title")], [])) and not s._names_other_field(D([T(1), T(2)], 0.5))
    q = B.build([], [D([T(7), T(7, field="body")], 0.1), T(5, field="body"), T(6, field="body")], must_nots=[T(1, field="body")])
    assert s._names_other_field(q)
    Q, G, C = s.pack_fields([s._cross_spec(q), s._cross_spec(B.build([T(7, 2.0, field="body"), T(4)], [], min_should_match=3))], lr)
    assert Q.tolist() == [(_lib.OCCUR_SHOULD, 0, 3, 1, 4, 1), (_lib.OCCUR_MUST, 3, 2, 0, 7, 0)]
    assert G["n_terms"].tolist() == [2, 1, 1, 1, 1] and G["kind"].tolist() == [1, 0, 0, 0, 0] and G["first_term"].tolist() == [0, 2, 3, 5, 6]
    assert G["tie_bits"][0] == np.float32(0.1).view(np.uint32)
    assert C["field"].tolist() == [0, 1, 1, 1, 1, 1, 0] and C["state"]["doc_freq"].tolist() == [400, 400, 256, 0, 5, 400, 129]
    for row, c in ((0, (0, 7)), (1, (1, 7)), (2, (1, 5)), (6, (0, 4))):
        w, cache = ref.weight(c)
        assert C["weight"][row].view(np.int32) == np.float32(w).view(np.int32), c
        assert s.ctx.caches[C["sim_table"][row]] == cache.tobytes(), c
    assert C["weight"][5] == np.float32(2.0) * C["weight"][1] and C["weight"][4] == 0 and C["sim_table"][0] != C["sim_table"][1]
    for bad, status in ((B([T(0, field="body")], [T(1)], 0), -5), (B([T(0, field="body")], [], 0, [], [T(1)]), -5), (T(0, field="nope"), -2),
                        (D([T(i % 3, field="body") for i in range(10)], 0.1), -5), (B([], [T(0, field="body"), T(1)], 2, [T(2)]), -5),
                        (D([T(0, field="body"), rucene_amd.PhraseQuery([1, 2])], 0.1), -5)):
        with pytest.raises(rucene_amd.RgpuError) as e:
            s._cross_spec(bad)
        assert e.value.status == status, str(bad)


def _host_searcher(with_field=True):
    import rucene_amd
    leaf = _leaf()
    title, body = leaf.fields
    lr = rucene_amd.LeafReader(leaf.doc_bytes, title.norms, leaf.max_doc, title.terms, sum_total_term_freq=title.sttf, field="title")
    if with_field:
        lr.add_field("body", body.norms, body.terms, sum_total_term_freq=body.sttf).slot = 1
    s = object.__new__(rucene_amd.GpuIndexSearcher)
    s.leaves, s.ctx, s.similarity, s._stats_leaf, s._weights = [lr], _RecordingCtx(), rucene_amd.BM25Similarity(), 0, {}
    s._stats_terms, s._field_weights, s._planners, s.flatten_nested, s.cpu_fallback = None, {}, {}, False, None
    s.required_sets = s.filtered_phrases = s.unordered_spans = False
    s._masks, s._points, s._range_filters, s._every_doc, s._not_filters = {}, {}, {}, None, {}
    s.collection_statistics = rucene_amd.CollectionStatistics("title", 0, leaf.max_doc, leaf.max_doc, title.sttf)
    return rucene_amd, lr, s


def test_only_search_serves_a_further_field():
    """count, count_batch, rescore_batch, cache_filter and the packers read the primary field alone: a tree that names a further
    field is UnsupportedOperation there (the CPU hooks take it), never an answer for the wrong field"""
    ra, lr, s = _host_searcher()
    T, B, D = ra.TermQuery, ra.BooleanQuery, ra.DisjunctionMaxQuery
    other = [T(7, field="body"), B.build([T(7), T(5, field="body")], []), B.build([], [T(7), T(5)], must_nots=[T(1, field="body")]),
             D([T(7), T(7, field="body")], 0.1), ra.BoostingQuery.build(T(7), T(5, field="body"), 0.5)]
    hits = np.zeros((1, 10), ra.HIT_DTYPE)
    for q in other:
        for call in (lambda: s._flatten(q), lambda: s.pack([q], lr), lambda: s._peel(q, build=False), lambda: s.count_batch([q]),
                     lambda: s.cache_filter(q), lambda: s.rescore_batch(hits, [q])):
            with pytest.raises(ra.RgpuError) as e:
                call()
            assert e.value.status == -5, (str(q), e.value)
    seen = []
    s.cpu_count_fallback = lambda query: seen.append(query) or -7
    assert s.count(T(7, field="body")) == -7 and len(seen) == 1   # (no deletions: the doc_freq shortcut is the primary field's alone)
    assert s.pack([T(7, field="title"), T(7)], lr)[1]["state"]["doc_freq"].tolist() == [400, 400]   # the primary field by its name


def test_a_dismax_clause_in_one_field_reaches_the_cpu_path():
    """BooleanQuery.build lets a DisjunctionMaxQuery clause through for the cross-field route; in the primary field alone the tree is
    UnsupportedOperation when searched - an RgpuError, so search() hands it to cpu_fallback"""
    ra, lr, s = _host_searcher(with_field=False)
    T, B, D = ra.TermQuery, ra.BooleanQuery, ra.DisjunctionMaxQuery
    trees = [B.build([], [D([T(1), T(2)], 0.1), T(3)]), B.build([T(3), D([T(1), T(2)], 0.1)], []), B.build([T(3)], [D([T(1), T(2)], 0.1)]),
             B.build([], [T(3), T(4), D([T(1), T(2)], 0.1)], must_nots=[T(5)]), B([T(3), T(4)], [], 0, [D([T(1), T(2)], 0.1)])]
    for q in trees:
        assert q.flattened() is None and q.required_disjunction() is None and q.nested_disjunction_first() is None and q.nested_conjunction() is None
        for call in (lambda: s._flatten(q), lambda: s.pack([q], lr), lambda: s.search_batch([q], 10), lambda: s.count_batch([q])):
            with pytest.raises(ra.RgpuError) as e:
                call()
            assert e.value.status == -5, (str(q), e.value)
        seen = []
        s.cpu_fallback = lambda query, collector: seen.append(query)
        s.search(q, ra.TopDocsCollector(10))
        s.cpu_fallback = None
        assert seen == [q]
