"""Exact phrases under doc-set masks, without a GPU: the equivalence the masked phrase calls rest on, proven on the oracle for every
fixture query of tests/phrase_masked.py, and the mirrors' routing decisions with the filtered_phrases opt-in on and off."""
import os
import subprocess

import numpy as np
import pytest

import phrase_bool as pb
import phrase_masked as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plain(oracle):
    ix = pb.Index(oracle, [pb.main()])
    yield ix
    ix.close()


@pytest.mark.parametrize("deleted", [(), (24, 120, 254)], ids=["no deletions", "deletions"])
@pytest.mark.parametrize("case", range(len(pm.PROOFS)), ids=[repr(p[1]) for p in pm.PROOFS])
def test_filtered_rows_equal_the_rows_on_the_twin_leaf(oracle, plain, case, deleted):
    """rows("Q #F -X") on live docs L == rows(Q) on a twin leaf whose live docs are L AND F AND NOT X: docs, f32 score bits, total.
    F / X ride as zero-weight FILTER / MUST_NOT term clauses whose postings are the set."""
    kind, filtered, bare, fs, xs = pm.PROOFS[case]
    fx = pb.main()
    ix = plain if not deleted else pb.Index(oracle, [fx], deleted=[set(deleted)])
    twin = pb.Index(oracle, [fx], deleted=[pm.twin_deleted(fx, deleted, fs, xs)])
    try:
        d, s = pm.reference_rows(kind, ix, filtered)
        td, ts = pm.reference_rows(kind, twin, bare)
        assert d.size == td.size and d.tolist() == td.tolist()
        assert s.view(np.uint32).tolist() == ts.view(np.uint32).tolist()
        assert d.size > 0, "a proof over an empty row shows nothing"
        ud, _ = pm.reference_rows(kind, ix, bare)
        assert ud.size >= d.size and (ud.size > d.size or pb.T129 in fs), "the set clauses remove something (T129 holds every doc of PB's)"
    finally:
        twin.close()
        if ix is not plain:
            ix.close()


def test_the_grid_fixture_is_what_its_docstring_says():
    fx = pm.grid()
    a = fx.docs_of(pm.A130)
    assert len(a) == 130 and a[0] == 0 and a[1] == 63 and a[2] == 64 and a[-1] == pm.GRID_DOCS - 1
    assert all(pm.phrase_holds(d) for d in (0, 63, 64, pm.GRID_DOCS - 1))
    m = pm.masks()
    for n in (0, 1, 63, 64, 65):
        assert len(set(m["first %d" % n]) & set(a)) == n
    block = a[:128]
    assert not set(m["middle group empty"]) & set(block[1::2]) and len(set(m["middle group empty"]) & set(a)) == 66
    assert not set(m["disjoint"]) & set(a) and m["empty"] == [] and len(m["full"]) == pm.GRID_DOCS
    assert set(m["overlaps deletions"]) & pm.DELETED and set(m["overlaps deletions"]) & set(a) - pm.DELETED
    assert set(a) & pm.DELETED and 0 < len(set(m["handful"]) & set(fx.docs_of(pm.A16385))) < 10
    assert pm.words_of(130, [0, 64, 129]).tolist() == [1, 1, 2]


def _searcher(on):
    from rucene_amd.searcher import GpuIndexSearcher
    g = GpuIndexSearcher.__new__(GpuIndexSearcher)   # (the peeling reads nothing of the searcher but the opt-in)
    if on is not None:
        g.filtered_phrases = on
    return g


def test_routing_is_opt_in():
    """Without filtered_phrases (unset, as on a searcher made with __new__, or False) every filtered phrase is UnsupportedOperation, as
    it has been; with it the served shapes peel to (the phrase query, the sets) and the rest stays refused."""
    import rucene_amd
    from rucene_amd.searcher import CachedFilter, FilterQuery, PointRangeQuery
    T, Bq, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    on = _searcher(True)
    F, X = CachedFilter(on, []), CachedFilter(on, [])
    served = [
        (FilterQuery(P([1, 2]), [F]), P, [F], []),
        (FilterQuery(Bq.build([P([1, 2]), T(3)], [], must_nots=[T(4)]), [F]), Bq, [F], []),
        (FilterQuery(Bq.build([], [P([1, 2]), T(3)]), [F]), Bq, [F], []),                       # FilterQuery asks only for a scorer
        (Bq.build([P([1, 2])], [], filters=[F]), P, [F], []),                                   # +"a b" #F: what is left is the phrase
        (Bq.build([P([1, 2])], [], filters=[F], must_nots=[X]), P, [F], [X]),
        (Bq.build([P([1, 2]), T(3)], [], filters=[F, T(5)], must_nots=[X, T(4)]), Bq, [F], [X]),
        (Bq.build([], [P([1, 2]), T(3)], must_nots=[X]), Bq, [], [X]),                          # "a b" c -X
        (Bq.build([], [P([1, 2]), T(3)], must_nots=[X, T(4)], min_should_match=1), Bq, [], [X]),
        (Bq.build([], [P([1, 2])], must_nots=[X]), P, [], [X]),                                 # "a b" -X
    ]
    for q, kind, f, x in served:
        rest, (gf, gx) = on._peel(q)
        assert isinstance(rest, kind) and gf == f and gx == x, q
        if isinstance(rest, Bq):
            assert rest.has_phrases() and not any(isinstance(c, CachedFilter) for c in rest.filter_queries + rest.must_not_queries)
        for g in (_searcher(None), _searcher(False)):
            with pytest.raises(rucene_amd.RgpuError) as e:
                g._peel(q)
            assert e.value.status == pm.UNSUPPORTED, q
    rest, _ = on._peel(Bq.build([], [P([1, 2]), T(3)], must_nots=[X]))
    assert rest.min_should_match == 1 and len(rest.should_queries) == 2 and not rest.must_not_queries
    refused = [
        (FilterQuery(P([1, 2], slop=1), [F]), "a filtered phrase"),
        (Bq.build([P([1, 2], slop=2)], [], filters=[F]), "a filtered phrase"),
        (Bq.build([P([1, 2], slop=1), T(3)], [], filters=[F]), "a sloppy phrase inside a boolean query"),
        (Bq.build([], [P([1, 2], slop=1), T(3)], must_nots=[X]), "a sloppy phrase inside a boolean query"),
        (Bq.build([], [P([1, 2]), T(3)], filters=[F]), "a doc set as the only required clause"),                 # "a b" c #F
        (Bq.build([], [P([1, 2]), T(3)], filters=[F], must_nots=[X]), "a doc set as the only required clause"),
        (Bq.build([], [P([1, 2]), T(3)], must_nots=[X], min_should_match=2), "beside min_should_match >= 2"),
        (Bq.build([P([1, 2])], [T(3)], filters=[F]), "SHOULD clauses beside a required phrase"),
        (Bq.build([T(3)], [], filters=[F], must_nots=[P([1, 2])]), "under SHOULD or MUST_NOT"),
        (Bq.build([P([1, 2])] * 5, [], filters=[F]), "more than 4 phrases"),
        (Bq.build([], [T(1), T(2)], must_nots=[X]), "a doc set as the only required clause"),                    # b c -X stays refused
    ]
    for q, why in refused:
        with pytest.raises(rucene_amd.RgpuError) as e:
            on._peel(q)
        assert e.value.status == pm.UNSUPPORTED and why in str(e.value), (q, str(e.value))
    # a point range in those positions is checked and peeled like a cached filter (build=False: no set is built)
    from rucene_amd.searcher import IntPoint
    r = IntPoint.new_range_query("n", 1, 5)
    assert isinstance(r, PointRangeQuery)
    on._points = {"n": (4, [])}
    for q, kind in ((Bq.build([P([1, 2])], [], filters=[r]), P), (Bq.build([P([1, 2]), r], [], must_nots=[T(4)]), Bq),
                    (Bq.build([], [P([1, 2]), T(3)], must_nots=[r]), Bq)):
        rest, (gf, gx) = on._peel(q, build=False)
        assert isinstance(rest, kind) and (gf + gx) == [r], q
        off = _searcher(False)
        off._points = on._points
        with pytest.raises(rucene_amd.RgpuError) as e:
            off._peel(q, build=False)
        assert e.value.status == pm.UNSUPPORTED
    # rows without doc-set clauses go the way they went
    plain = Bq.build([P([1, 2]), T(3)], [])
    assert on._peel(plain) == (plain, ([], []))


def test_cpp_mirror_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/phrase_masked_demo.cpp (FilteredQuery over the phrase queries of csrc/host/gpu_index_searcher.hpp with
    filtered_phrases on) links against the C ABI on a CPU-only box, warnings as errors; running it needs a GPU."""
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "phrase_masked_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "phrase_masked_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_the_library_exports_the_masked_phrase_calls():
    """The three entry points exist in the built library and in the ctypes binding (they are what the GPU tests call)."""
    import ctypes

    import __graft_entry__ as g
    from rucene_amd import _lib
    g.build()
    lib = ctypes.CDLL(g.GPU_LIB)
    for name in ("rgpu_search_phrase_batch_masked", "rgpu_search_phrase_bool_batch_masked", "rgpu_search_phrase_or_batch_masked"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    for name in ("search_phrase_batch_masked", "search_phrase_bool_batch_masked", "search_phrase_or_batch_masked"):
        assert callable(getattr(_lib.Segment, name))
