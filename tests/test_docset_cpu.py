"""Doc sets without a GPU (`-m "not gpu"`): the semantic fact the masked search entry points rest on, proven on the oracle; the numpy
reference of rgpu_docset_collect_batch held against the oracle's own postings; the host plan (csrc/host/docset_plan.hpp) under the
sanitizers; the header, the exports and the mirror's routing rules.

The fact: for a query Q with a scorer of its own, a FILTER doc set F, a MUST_NOT doc set X and live docs L, "Q #F -X" collects the
docs, the hit count and the f32 scores Q alone collects on live docs L AND F AND NOT X. The oracle takes FILTER clauses as boost-0
required clauses (Searcher.search, boosts) and MUST_NOT clauses through search_not / search_opt, never both in one call, so the
two halves are proven separately and then chained - the FILTER half again on live docs that already lack X:
    Q #f  on L          ==  Q on L AND docs(f)
    Q -g  on L          ==  Q on L AND NOT docs(g)
    Q #f  on L AND NOT docs(g)  ==  Q on L AND NOT docs(g) AND docs(f)
MUST + SHOULD queries (ReqOptScorer, whose running mean sees collected docs only) have no boosts in the oracle's call: for them the
MUST_NOT half is proven, and the FILTER half through the live-docs side alone (a filter term with boost 1 is another query)."""
import os
import subprocess

import numpy as np
import pytest

import docset as ds
import segment_spectrum as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, what):
    assert a[2] == b[2], (what, "total_hits", a[2], b[2])
    assert a[0].tolist() == b[0].tolist(), (what, "docs")
    assert a[1].view(np.int32).tolist() == b[1].view(np.int32).tolist(), (what, "score bits")


def _search(oracle, osr, must, should, k, filt=(), must_not=()):
    if should:
        assert not filt
        return osr.search_opt(oracle.OP_TERM if len(must) == 1 else oracle.OP_AND, list(must), list(should), k, must_not_ids=list(must_not))
    if must_not:
        assert not filt
        return osr.search_not(oracle.OP_TERM if len(must) == 1 else oracle.OP_AND, list(must), list(must_not), k)
    req = list(must) + list(filt)
    return osr.search(oracle.OP_TERM if len(req) == 1 else oracle.OP_AND, req, k, boosts=[1.0] * len(must) + [0.0] * len(filt))


@pytest.mark.parametrize("live", ["none", "seeded"])
def test_filter_and_must_not_clauses_equal_a_search_on_fewer_live_docs(oracle, live):
    leaf = ds.equiv_leaf()
    L = np.ones(leaf.max_doc, bool) if live == "none" else ds.seeded_alive(leaf.max_doc)
    not_g = ~leaf.has[ds.G]
    searchers = {}

    def osr(alive):
        key = alive.tobytes()
        if key not in searchers:
            searchers[key] = oracle.Searcher([leaf.oracle_segment(oracle, None if alive.all() else alive)])
        return searchers[key]
    checked = skipping = 0
    for must, should in ds.EQ_QUERIES:
        for k in ds.EQ_KS:
            what = (live, must, should, k)
            # the MUST_NOT half
            with_g = _search(oracle, osr(L), must, should, k, must_not=(ds.G,))
            _same(with_g, _search(oracle, osr(L & not_g), must, should, k), what + ("-g",))
            assert 0 < with_g[2] < _search(oracle, osr(L), must, should, k)[2]   # (the clause removed something, and not everything)
            if should:
                skipping += with_g[2] > 100
                continue
            for f in ds.EQ_FILTERS:
                has_f = leaf.has[f]
                # the FILTER half, with the zero-score clause first, in the middle and last in the cost order
                with_f = _search(oracle, osr(L), must, (), k, filt=(f,))
                _same(with_f, _search(oracle, osr(L & has_f), must, (), k), what + ("#f", f))
                assert 0 < with_f[2] < _search(oracle, osr(L), must, (), k)[2]
                # ... and chained behind the MUST_NOT half: Q #f -g
                _same(_search(oracle, osr(L & not_g), must, (), k, filt=(f,)), _search(oracle, osr(L & not_g & has_f), must, (), k), what + ("#f -g", f))
                checked += 1
    assert checked == 5 * len(ds.EQ_KS) * 3 and skipping >= 2   # ReqOptScorer's rule had its 100 docs
    # the cost orders the docstring of tests/docset.py promises
    dfs = [d.size for d, _ in leaf.lists]
    assert dfs[ds.F_CHEAP] < min(dfs[ds.A], dfs[ds.B], dfs[ds.C]) and max(dfs[ds.A], dfs[ds.B], dfs[ds.C]) < dfs[ds.F_DEAR]
    assert dfs[ds.B] < dfs[ds.F_MID] < dfs[ds.A]


def test_the_filter_clause_adds_a_positive_zero():
    """x + 0.0 == x bit for bit for every f32 but -0.0: the one documented deviation (a BM25 score is never -0.0: weights of
    boost 0 give +0.0, and a negative boost gives a negative score, not a negative zero)."""
    x = np.array([0.0, 1.0, 1e-45, 3.4e38, -1.5, np.inf, 0.1], np.float32)
    assert ((x + np.float32(0.0)).view(np.int32) == x.view(np.int32)).all()
    assert (np.float32(-0.0) + np.float32(0.0)).view(np.int32) != np.float32(-0.0).view(np.int32)


@pytest.mark.parametrize("version", [1, 0])
def test_collect_reference_against_the_oracles_postings(oracle, version):
    """The numpy reference of rgpu_docset_collect_batch stands on the raw lists: they are what the oracle decodes from the .doc
    bytes; a term query's set is its list, live docs or not; conjunctions and disjunctions are the oracle's hit sets on a leaf
    without deletions; the words have no bit at or past max_doc."""
    leaf = ds.collect_leaf(version)
    oseg = leaf.oracle_segment(oracle)
    for t, (d, _) in enumerate(leaf.lists):
        if d.size:
            assert (oseg.decode_term(leaf.terms[t])[0] == d).all(), t
    assert [leaf.lists[t][0].size for t in ds.CO_TERM_LISTS] == [1, 127, 128, 129, 2176, 2304, 10001]
    assert leaf.lists[ds.DENSE][0].size >= max(1024, leaf.max_doc // 64)   # dense enough for a doc bitmap under either rule
    osr = oracle.Searcher([oseg])
    k = leaf.max_doc
    sizes = []
    for q in ds.COLLECT_QUERIES:
        m = ds.ref_set(leaf.has, q)
        sizes.append(int(m.sum()))
        words = ss.live_words(m)
        assert words.size == (leaf.max_doc + 63) // 64 and int(words[-1]) >> (leaf.max_doc % 64) == 0
        pos = list(q.must or q.should)
        if not pos or q is ds.COLLECT_QUERIES[0]:
            continue
        op = oracle.OP_OR if q.should else (oracle.OP_TERM if len(pos) == 1 else oracle.OP_AND)
        d, _, total = osr.search_not(op, pos, list(q.must_not), k) if q.must_not else osr.search(op, pos, k)
        assert total == m.sum() and sorted(d.tolist()) == np.flatnonzero(m).tolist(), q
    assert 0 in sizes and max(sizes) > 10000 and len({len(q.should) for q in ds.COLLECT_ORS}) >= 5
    assert {len(q.must_not) for q in ds.COLLECT_QUERIES} == {0, 1, 2}


def test_masks_of_the_sweep():
    for n in ds.SWEEP_SIZES:
        alive = ss.alive_mask(n, "seeded")
        got = {name: ds.mask_of(name, n, alive) for name in ds.MASKS}
        assert not got["empty"].any() and got["full"].all() and got["single"].sum() == 1 and got["single"][n - 1]
        assert not (got["not-live"] & alive).any() and (got["not-live"] | alive).all()
        assert got["half"].any() and (n < 64 or 0.3 * n < got["half"].sum() < 0.7 * n)
        for m in got.values():
            assert m.dtype == bool and m.size == n and ss.live_words(m).size == (n + 63) // 64


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/docset_plan_test.cpp: the last word of a caller's bit set, which clauses exist in the leaf, dead conjunctions, distinct
    terms and the cost order, the list kernel's jobs, the refusals and the mirror's grouping of csrc/host/docset_plan.hpp, as a
    stand-alone program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "docset_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "docset_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("docset_plan_test OK"), out.stdout


def test_header_exports_and_bindings():
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from rucene_amd import _lib
    names = ["rgpu_docset_from_words", "rgpu_docset_from_docs", "rgpu_docset_collect_batch", "rgpu_docset_combine", "rgpu_docset_cardinality",
             "rgpu_docset_words", "rgpu_docset_bytes", "rgpu_docset_free", "rgpu_search_batch_masked", "rgpu_search_batch_device_masked"]
    L = C.CDLL(_lib.lib_path())
    header = open(os.path.join(ROOT, "include", "rucene_gpu.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(L, n) and (n + "(") in header, n
    assert _lib.lib().rgpu_abi_version() == 6
    # argument errors are codes, never crashes, and need no GPU
    out = C.c_void_p()
    G = _lib.lib()
    assert G.rgpu_docset_from_words(None, None, C.byref(out)) == -2 and G.rgpu_docset_from_docs(None, None, 0, C.byref(out)) == -2
    assert G.rgpu_docset_collect_batch(None, None, 0, None, 0, None) == -2 and G.rgpu_docset_combine(None, None, 0, None, 0, C.byref(out)) == -2
    assert G.rgpu_docset_cardinality(None, None) == -2 and G.rgpu_docset_words(None, None) == -2 and G.rgpu_docset_bytes(None) == 0
    assert G.rgpu_search_batch_masked(None, None, None, 0, None, 0, 10, None, None) == -2
    assert G.rgpu_search_batch_device_masked(None, None, None, 0, None, 0, 10, None, None, None) == -2
    G.rgpu_docset_free(None)


def test_mirror_routing_rules():
    """BooleanQuery.build takes a CachedFilter under filters= / must_nots= only; GpuIndexSearcher._peel serves the two equivalent
    shapes and refuses the rest with UnsupportedOperation (what search() hands to cpu_fallback) - no GPU needed for the decision."""
    import rucene_amd
    from rucene_amd.searcher import CachedFilter, FilterQuery, GpuIndexSearcher
    T, Bq, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    g = GpuIndexSearcher.__new__(GpuIndexSearcher)   # (the peeling reads nothing of the searcher)
    F, X = CachedFilter(g, []), CachedFilter(g, [])
    q = Bq.build([T(1)], [], filters=[F])
    assert isinstance(q, Bq) and q.filter_queries == [F] and [t.term for t in q.extract_terms()] == [1]
    rest, (f, x) = g._peel(q)
    assert isinstance(rest, T) and rest.term == 1 and f == [F] and x == []
    rest, (f, x) = g._peel(Bq.build([T(1), T(2)], [T(3)], filters=[F, T(4)], must_nots=[X, T(5)]))
    assert [c.term for c in rest.must_queries] == [1, 2] and [c.term for c in rest.filter_queries] == [4] and [c.term for c in rest.must_not_queries] == [5]
    assert [c.term for c in rest.should_queries] == [3] and f == [F] and x == [X]
    rest, (f, x) = g._peel(Bq.build([], [], filters=[T(4), F]))       # a term FILTER is a clause of its own
    assert isinstance(rest, T) and rest.boost == 0.0 and f == [F]
    rest, (f, x) = g._peel(FilterQuery(Bq.build([], [T(1), T(2)]), [F]))   # FilterQuery asks only for a scorer
    assert len(rest.should_queries) == 2 and f == [F]
    rest, (f, x) = g._peel(FilterQuery(Bq.build([T(1)], [], must_nots=[X]), [F]))
    assert isinstance(rest, T) and rest.term == 1 and f == [F] and x == [X]   # (what is left is one clause: BooleanQuery::build's rewrite)
    plain = Bq.build([T(1)], [T(2)])
    assert g._peel(plain) == (plain, ([], [])) and g._peel(T(7))[1] == ([], [])
    refused = [Bq.build([], [T(1), T(2)], filters=[F]),                          # b c #F: the reference matches all of F
               Bq.build([], [], filters=[F]),                                    # a lone #F
               Bq.build([], [T(1), T(2)], must_nots=[X]),                        # no required clause of its own
               Bq.build([T(1)], [T(2), T(3)], must_nots=[X], min_should_match=2),   # -X beside min_should_match 2
               Bq.build([P([1, 2])], [], filters=[F]), FilterQuery(P([1, 2]), [F]), FilterQuery(P([1, 2], slop=1), [F]),   # filtered phrases
               Bq.build([T(1), P([1, 2])], [], must_nots=[X])]
    for q in refused:
        with pytest.raises(rucene_amd.RgpuError) as e:
            g._peel(q)
        assert e.value.status == -5, q
    for bad in (lambda: Bq.build([F], []), lambda: Bq.build([T(1)], [F]), lambda: FilterQuery(T(1), []), lambda: FilterQuery(T(1), [T(2)])):
        with pytest.raises(rucene_amd.RgpuError) as e:
            bad()
        assert e.value.status == -2


def test_cpp_mirror_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/docset_demo.cpp (CachedFilter / FilteredQuery of csrc/host/gpu_index_searcher.hpp) links against the C ABI on a CPU-only
    box, warnings as errors; running it needs a GPU (tests/test_gpu_docset_mirror.py)."""
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "docset_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "docset_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
