"""The span-near fixtures and their reference model, proven without a GPU (tests/span_near.py; tests/test_gpu_span_near.py runs them
through rgpu_search_span_near_batch): the two restatements of NearSpansOrdered + SpanScorer agree, the designed docs give the freqs
written out by hand, the model's weight, norms and ranking are the oracle's (distinct terms at slop 0 = the exact phrase), its score
function is the oracle's on fractional freqs, the fixtures lie where the ladder's rungs say, and the entry point is declared in
every layer."""
import os
import subprocess

import numpy as np
import pytest

import phrase_spectrum as ps
import span_near as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _same_walk(a, b):
    return a[0] == b[0] and _bits(a[1]) == _bits(b[1]) and a[2] == b[2]


def test_the_two_restatements_agree():
    """On every candidate doc of every fixture query, and on 4000 seeded random small docs: 2..5 clauses, 0..12 positions each, clauses
    that repeat a term, slop 0..6."""
    n = 0
    for name, c in sn.all_cases():
        fx = sn.segment(name)
        for q in c.queries:
            for doc, lists in sn.doc_lists(fx.postings, q.terms).items():
                assert _same_walk(sn.walk_reference(lists, q.slop), sn.walk_lower_bound(lists, q.slop)), (name, c.name, q.slop, doc)
                n += 1
    assert n > 100
    hits = spans = empty = repeats = 0
    for lists, slop in sn.random_docs(4000):
        a, b = sn.walk_reference(lists, slop), sn.walk_lower_bound(lists, slop)
        assert _same_walk(a, b), (lists, slop, a, b)
        hits += a[0]
        spans += len(a[2]) > 1
        empty += any(not x for x in lists)
        repeats += len({id(x) for x in lists}) < len(lists)
    assert hits > 500 and spans > 200 and empty > 20 and repeats > 500, (hits, spans, empty, repeats)


def test_the_designed_docs_give_the_freqs_written_out_by_hand():
    stated = 0
    for name, c in sn.all_cases():
        fx = sn.segment(name)
        for q in c.queries:
            if q.want is None:
                continue
            lists = sn.doc_lists(fx.postings, q.terms)[c.designed]
            hit, freq, widths = sn.walk_reference(lists, q.slop)
            assert hit == (float(q.want) != 0.0) and _bits(freq) == _bits(q.want), (name, c.name, q.slop, freq, q.want, widths)
            stated += 1
    assert stated >= 40
    # the values themselves, as the issue states them
    by = {c.name: c for c in sn.segment("walk").cases}
    assert [float(q.want) for q in by["shared-later-position"].queries] == [0.25 + 0.5]
    assert [float(q.want) for q in by["three-widths-add"].queries] == [0.0, 0.25]
    assert [float(q.want) for q in by["width-2"].queries] == [0.0, float(np.float32(1.0) / np.float32(3.0))]
    assert [float(q.want) for q in by["x-x"].queries][0] == 1.0
    # a doc of nine spans of different widths: the f32 sum depends on the order it is formed in
    q = by["sum-order"].queries[0]
    widths = sn.walk_reference(sn.doc_lists(sn.segment("walk").postings, q.terms)[by["sum-order"].designed], q.slop)[2]
    assert widths == list(sn.ORDER_WIDTHS) and len(set(widths)) == len(widths) >= 8
    assert _bits(sn.f32sum(widths)) != _bits(sn.f32sum(widths[::-1]))


def test_the_fixtures_lie_where_the_rungs_say():
    """What makes a case's level: clauses, positions per clause and doc, 16-bit cells, packed position blocks around the doc."""
    for name, c in sn.all_cases():
        fx = sn.segment(name)
        for q in c.queries:
            if c.designed is None:
                continue
            cands = sn.doc_lists(fx.postings, q.terms)
            assert c.designed in cands and (c.ordinary in cands or c.rung == "singleton"), (name, c.name)
            top = max(len(ps_) for lists in cands.values() for ps_ in lists)
            big = max(p for lists in cands.values() for ps_ in lists for p in ps_)
            trailing = False
            for t in set(q.terms):
                if len(fx.postings[t]) == 1:
                    trailing = True   # a singleton's positions are a VInt block
                    continue
                for doc in cands:
                    pl = ps.place(fx.postings[t], doc)
                    trailing = trailing or any(kd != "packed" for kd in pl["between"])
            if q.error == ps.ILLEGAL_ARGUMENT:
                assert len(q.terms) > ps.MAX_TERMS
            elif q.error == ps.UNSUPPORTED:
                assert top > ps.LIST_CAP
            elif q.level == "lanes":
                assert len(q.terms) <= ps.LANE_TERMS and top <= ps.LANE_CAP and big <= 32767 and not trailing, (name, c.name, top, big, trailing)
            elif q.level == "left":
                assert top <= ps.SMALL_CAP and (len(q.terms) > ps.LANE_TERMS or top > ps.LANE_CAP or big > 32767 or trailing), (name, c.name)
            else:
                assert q.level == "wide" and ps.SMALL_CAP < top <= ps.LIST_CAP, (name, c.name, top)
    place = {c.name: c for c in sn.segment("place").cases}
    for end in (ps.BLOCK - 1, ps.BLOCK, ps.BLOCK + 1):
        c = place["end-%d-behind-packed" % end]
        pl = ps.place(sn.segment("place").postings[c.shape["placed"]], c.designed)
        assert pl["skip"] + pl["freq"] == end and pl["kind"] == "packed" and pl["block"] == 2, (end, pl)
    c = place["end-%d-behind-trailing" % (ps.BLOCK + 1)]
    assert ps.place(sn.segment("place").postings[c.shape["placed"]], c.designed)["behind"] == "trailing"
    assert [c.shape["value"] for c in (place["pos-32767"], place["pos-32768"])] == [32767, 32768]
    for fx in [sn.segment(n) for n in sn.BUILDERS] + sn.four_leaves():
        assert 100 < fx.max_doc < 1000, (fx.name, fx.max_doc)
    four = sn.four_leaves()
    assert len({fx.max_doc for fx in four}) == 4 and not four[1].postings[0] and four[0].postings[0]


def _oracle_row(fx, ix, q, k, slop=0, live=None, norms=True):
    return ix.phrase_search(q.terms, k, fx.norms if norms else None, fx.max_doc, fx.doc_count, fx.sum_ttf, slop=slop, live_docs=live)


def test_distinct_terms_at_slop_0_are_the_oracles_exact_phrase(oracle):
    """With distinct terms and slop 0 a doc's span freq is its exact phrase freq as an f32: the model's rows - candidates, weight,
    norms, ranking, total - equal PositionsIndex.phrase_search(slop=0) bit for bit, with and without deleted docs and norms."""
    rows = 0
    for name in sn.BUILDERS:
        fx = sn.segment(name)
        ix = fx.index(oracle)
        alive = np.ones(fx.max_doc, dtype=bool)
        alive[[c.designed for c in fx.cases[::2] if c.designed is not None]] = False
        live = sn.live_words(alive)
        try:
            for c in fx.cases:
                for q in c.queries:
                    if len(set(q.terms)) < len(q.terms) or c.designed is None:
                        continue
                    q0 = q._replace(slop=0)
                    for k in (1, 10, 1000):
                        for lv in (None, live):
                            want = _oracle_row(fx, ix, q0, k, live=lv)
                            got = sn.search_case(fx, q0, k, live=lv)
                            assert got[2] == want[2] and (got[0] == want[0]).all() and (_bits(got[1]) == _bits(want[1])).all(), (name, c.name, k, got, want)
                    want = _oracle_row(fx, ix, q0, 10, norms=False)
                    got = sn.search(fx.postings, None, fx.max_doc, fx.doc_count, fx.sum_ttf, q0, 10)
                    assert got[2] == want[2] and (got[0] == want[0]).all() and (_bits(got[1]) == _bits(want[1])).all(), (name, c.name, "no norms")
                    rows += 1
        finally:
            ix.close()
    assert rows >= 30


def test_the_score_function_is_the_oracles_on_fractional_freqs(oracle):
    """sloppy_freqs and phrase_search(slop > 0) of fixture phrases: score(freq, norm byte) restated here equals the oracle's score
    by score."""
    fx = sn.segment("walk")
    ix = fx.index(oracle)
    checked = fractional = 0
    try:
        for c in fx.cases:
            q = c.queries[0]
            if c.name not in ("width-2", "shared-later-position", "three-widths-add", "sum-order"):
                continue
            for slop in (3, 12, 40):
                docs, freqs = ix.sloppy_freqs(q.terms, slop)
                by_doc = dict(zip(docs.tolist(), freqs))
                weight, cache = sn.weight_of([len(fx.postings[t]) for t in q.terms], fx.max_doc, fx.doc_count, fx.sum_ttf)
                for norms in (True, False):
                    d, sc, total = _oracle_row(fx, ix, q, 1000, slop=slop, norms=norms)
                    assert total == d.size >= 1
                    for doc, s in zip(d.tolist(), sc):
                        f = by_doc[doc]
                        mine = sn.score(weight, cache, f, fx.norms[doc] if norms else None)
                        assert _bits(mine) == _bits(s), (c.name, slop, doc, float(f), float(mine), float(s))
                        checked += 1
                        fractional += float(f) != int(f)
    finally:
        ix.close()
    assert checked >= 20 and fractional >= 8, (checked, fractional)


def test_the_two_phase_rule_of_the_model_at_slop_0():
    """n non-matching candidates in front of the first hit: next_limit n - 1 abandons the leaf, n serves it - at slop 0 too; deleted
    candidates in front count; 0 serves only a first candidate that matches."""
    fx = ps.chunks(ps.CHUNK + 1)
    assert fx.first == [0, ps.CHUNK - 1, ps.CHUNK]
    for j, n in enumerate(fx.first):
        q = sn.sq([2 * j, 2 * j + 1], 0)
        full = sn.search_case(fx, q, 10)
        assert full[2] == int(fx.matches[j].sum()) and full[0].min() >= n
        if n:
            assert sn.search_case(fx, q, 10, next_limit=n - 1)[2] == 0
        served = sn.search_case(fx, q, 10, next_limit=n)
        assert served[2] == full[2] and (served[0] == full[0]).all()
        assert sn.search_case(fx, q, 10, next_limit=0)[2] == (full[2] if n == 0 else 0)
    alive = np.arange(fx.n) >= 100
    live = fx.live_words(alive)
    first = int(np.argmax(fx.matches[0] & alive))
    q = sn.sq([0, 1], 0)
    assert first == 111 and sn.search_case(fx, q, 10, live=live, next_limit=first - 1)[2] == 0
    assert sn.search_case(fx, q, 10, live=live, next_limit=first)[2] == int((fx.matches[0] & alive).sum())


def test_the_entry_point_is_declared_in_every_layer():
    """The header, the Python binding's export list, the Rust FFI and its documentation name rgpu_search_span_near_batch; the query
    classes exist and are built by the reference's rules; what the GPU path does not serve is UnsupportedOperation (-5)."""
    import rucene_amd
    from rucene_amd import _lib, searcher
    name = "rgpu_search_span_near_batch"
    for path in ("include/rucene_gpu.h", "rust/gpu/ffi.rs", "INTEGRATION.md"):
        with open(os.path.join(ROOT, path)) as fh:
            assert name in fh.read(), path
    assert name in _lib.EXPORTS and hasattr(_lib.Segment, "search_span_near_batch")
    S, N = rucene_amd.SpanTermQuery, rucene_amd.SpanNearQuery
    near = N([S(1), S(2)], slop=3)
    assert (near.slop, near.in_order, near.boost, near.terms, near.positions) == (3, True, 1.0, [1, 2], [0, 1])
    assert [t.term for t in N([S(4), S(4), S(b"x")]).extract_terms()] == [4, 4, b"x"]
    for clauses in ([], [S(1)]):
        with pytest.raises(rucene_amd.RgpuError) as e:
            N(clauses)
        assert e.value.status == -2
    searcher._refuse_unserved_spans(near)
    searcher._refuse_unserved_spans(rucene_amd.TermQuery(1))
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    unserved = [N([S(1), S(2)], in_order=False), N([S(1), N([S(2), S(3)])]), S(1), N([S(i) for i in range(17)]),
                B.build([near, T(3)], []), B.build([], [near, T(3)]), B.build([T(3)], [], must_nots=[near]), B.build([T(3)], [], filters=[near]),
                rucene_amd.DisjunctionMaxQuery([T(1), near]), rucene_amd.BoostingQuery.build(near, T(1), 0.5),
                rucene_amd.BoostingQuery.build(T(1), near, 0.5), B.build([B.build([near, T(1)], []), T(2)], [])]
    for q in unserved:
        with pytest.raises(rucene_amd.RgpuError) as e:
            searcher._refuse_unserved_spans(q)
        assert e.value.status == -5, q


def test_cpp_span_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/span_near_demo.cpp links against the C ABI on a CPU-only box (running it needs a GPU: tests/test_gpu_span_near.py)."""
    import __graft_entry__ as entry
    entry.build()
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "span_near_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "span_near_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
