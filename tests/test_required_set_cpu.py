"""Doc sets as the only required clause, proved on the CPU: what tests/required_set.py composes from the oracle's parts IS what the
oracle's own ReqOptScorer search collects ("b c #F" matches all of F), min_should_match has no effect there, the skipping rule of
ReqOptScorer::score never fires under a required score of 0.0, every fixture sits on the edge it is named after, and
GpuIndexSearcher._peel routes exactly the shapes the option names - no GPU anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import docset as ds
import required_set as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _searcher(oracle, alive=None):
    fx = ds.equiv_leaf()
    return fx, oracle.Searcher([fx.oracle_segment(oracle, alive)])


@pytest.mark.parametrize("live", ["none", "seeded"])
@pytest.mark.parametrize("filt", [ds.F_CHEAP, ds.F_MID, ds.F_DEAR])
def test_composed_docs_and_totals_are_the_req_opt_search(oracle, filt, live):
    """A set equal to term f's docs: the composed rows hold the docs, and the total, of search_opt(TERM f, shoulds) - the reference
    collects ALL of F, the docs that hold neither SHOULD clause included - and where no SHOULD clause matches the composed score is
    +0.0. (The scores differ by design: the oracle's required TermScorer scores f, a doc set scores 0.0.)"""
    alive = None if live == "none" else ds.seeded_alive(ds.EQ_MAX_DOC)
    fx, osr = _searcher(oracle, alive)
    m = fx.has[filt] & (np.ones(fx.max_doc, bool) if alive is None else alive)
    for shoulds in ((ds.S1, ds.S2), (ds.S2,), (ds.S1, ds.S2, ds.A, ds.B)):
        k = int(m.sum()) + 10
        d, s, total = rs.composed(oracle, osr, [(0, m)], shoulds, k)
        od, _os, ototal = osr.search_opt(oracle.OP_TERM, [filt], list(shoulds), k, tie_mode=oracle.TIE_CANONICAL)
        assert total == ototal == int(m.sum())
        assert sorted(d.tolist()) == sorted(od.tolist()) == np.flatnonzero(m).tolist()
        any_should = np.zeros(fx.max_doc, bool)
        for t in shoulds:
            any_should |= fx.has[t]
        zero = s.view(np.int32) == 0
        assert (zero == ~any_should[d]).all() and zero.any() and not zero.all(), (filt, shoulds)
        # ranked: the scored docs first, then the unscored ones in doc order
        assert (np.diff(d[zero]) > 0).all() and not zero[:int((~zero).sum())].any()
        # a smaller k is a prefix of it
        d10, s10, _ = rs.composed(oracle, osr, [(0, m)], shoulds, 10)
        assert d10.tolist() == d[:10].tolist() and s10.view(np.int32).tolist() == s[:10].view(np.int32).tolist()


def test_min_should_match_has_no_effect_beside_a_required_clause(oracle):
    """ReqOptScorer only advance()s the optional scorer: search_opt with min_should_match = 2 is search_opt with 0, bit for bit"""
    fx, osr = _searcher(oracle)
    for filt in ds.EQ_FILTERS:
        for exact in (False, True):
            a = osr.search_opt(oracle.OP_TERM, [filt], [ds.S1, ds.S2, ds.C], 200, min_should_match=0, exact=exact)
            b = osr.search_opt(oracle.OP_TERM, [filt], [ds.S1, ds.S2, ds.C], 200, min_should_match=2, exact=exact)
            assert a[0].tolist() == b[0].tolist() and a[1].view(np.int32).tolist() == b[1].view(np.int32).tolist() and a[2] == b[2]


def test_the_skipping_rule_never_fires_under_a_required_score_of_zero():
    """req_opt_scorer.rs:42-65 in f32, literally: score = req.score() = 0.0; past OPT_SCORE_THRESHOLD docs the optional clause is
    skipped when 2.0 * score < scores_sum / scores_num - with scores_sum the sum of REQUIRED scores, 0.0 for ever: 0 < 0."""
    f32 = np.float32
    rng = np.random.default_rng(91)
    opt = np.where(rng.random(400) < 0.5, rng.random(400).astype(np.float32) * f32(9.0), f32(0.0)).astype(np.float32)
    scores_sum, scores_num, skipped, out = f32(0.0), 0, 0, []
    threshold = 100   # OPT_SCORE_THRESHOLD
    for i in range(400):
        score = f32(0.0)
        if scores_num > threshold and f32(2.0) * score < scores_sum / f32(scores_num):
            skipped += 1
            out.append(score)
            continue
        scores_sum = f32(scores_sum + score)
        scores_num += 1
        if opt[i] != 0:
            score = f32(score + opt[i])
        out.append(score)
    assert skipped == 0 and scores_num == 400 > 300 and scores_sum.view(np.int32) == 0
    assert np.array(out, np.float32).view(np.int32).tolist() == opt.view(np.int32).tolist()   # 0.0 + S(d) == S(d), +0.0 elsewhere


def test_should_clauses_beside_an_excluded_set_match_the_disjunction_alone(oracle):
    """"b c -X" gets no MatchAllDocsQuery (boolean_query.rs:76-79 adds one only when there is no MUST, SHOULD or FILTER clause):
    ReqNotScorer over the disjunction collects the docs of b | c outside X - not every doc outside X. The mirror searches it masked."""
    fx, osr = _searcher(oracle)
    d, _s, total = osr.search_not(oracle.OP_OR, [ds.S1, ds.S2], [ds.G], 10)
    inside = (fx.has[ds.S1] | fx.has[ds.S2]) & ~fx.has[ds.G]
    assert total == int(inside.sum()) < int((~fx.has[ds.G]).sum()) and inside[d].all()


def test_every_fixture_sits_on_its_edge():
    import __graft_entry__ as g
    g.build()
    from rucene_amd import _lib
    header = open(os.path.join(ROOT, "include", "rucene_gpu.h")).read()
    assert int(re.search(r"#define RGPU_DOCSET_HEAD_CHUNK_WORDS (\d+)", header).group(1)) == _lib.DOCSET_HEAD_CHUNK_WORDS == rs.HEAD_CHUNK_WORDS
    assert rs.BIG_MAX_DOC == 3 * rs.HEAD_CHUNK_WORDS * 64 + 65 and max(rs.KS) == _lib.MAX_K
    lists = rs.big_lists()
    assert [lists[rs.T[n]][0].size for n in rs.SIZES] == rs.SIZES and lists[rs.T[0]][0].size == 0
    assert {0, rs.CHUNK_DOCS - 1, rs.CHUNK_DOCS, rs.BIG_MAX_DOC - 1} <= set(lists[rs.R[0]][0].tolist())
    for i in range(rs.N_R):   # every R list reaches into every chunk
        assert set(np.unique(lists[rs.R[i]][0] // rs.CHUNK_DOCS).tolist()) >= {0, 1, 2}
    seq = rs.seq_mask()
    for k in rs.KS:
        for n in rs.sizes_of(k):
            assert n in rs.T
            o = np.zeros(rs.BIG_MAX_DOC, bool)
            o[lists[rs.T[n]][0]] = True
            for name in rs.PLACEMENTS:
                m = rs.placement_mask(name)
                head = np.flatnonzero(m)[:k]
                assert np.flatnonzero(m).size > k + 1   # M never runs out before the row is full
                if name == "inside":
                    assert int((o & m).sum()) == n and (n == 0 or o[head].sum() == min(n, (k + 1) // 2)) and o[head[0]] == (n > 0)
                elif name == "behind":
                    assert int((o & m).sum()) == n and not o[head].any()
                else:
                    assert not (o & m).any() and not (seq & m).any()
    assert set((rs.edge_docs() // rs.CHUNK_DOCS).tolist()) == {0, 1, 2, 3}
    for n in rs.HEAD_NS:
        sets = rs.head_sets(n)
        m = max(n, 2)
        both, one = np.flatnonzero(sets["chunk edge, both in"]), np.flatnonzero(sets["chunk edge, one in"])
        assert both[m - 2] == rs.CHUNK_DOCS - 1 and both[m - 1] == rs.CHUNK_DOCS and one[m - 1] == rs.CHUNK_DOCS - 1 and one[m] == rs.CHUNK_DOCS
        assert [int(sets[s].sum()) for s in ("n - 1 docs", "n docs", "n + 1 docs")] == [max(n - 1, 0), n, n + 1]
        assert np.flatnonzero(sets["last chunk only"]).min() == 3 * rs.CHUNK_DOCS and sets["last chunk only"][rs.BIG_MAX_DOC - 1]
        assert sets["bits 63 | 64"][[63, 64]].all() and not sets["empty"].any() and sets["every doc"].all()
        spread = sets["spread"]
        assert spread.sum() > 1024 and set(np.unique(np.flatnonzero(spread) // rs.CHUNK_DOCS).tolist()) == {0, 1, 2, 3}
        gone = rs.head_deletions(spread, max(n, 1))
        docs = np.flatnonzero(spread)
        assert not gone["first doc"][docs[0]] and not gone["rank n - 1"][docs[max(n, 1) - 1]] and not gone["first chunk"][:rs.CHUNK_DOCS].any()
        assert not (gone["the whole set"] & spread).any()


def test_header_exports_and_bindings():
    import __graft_entry__ as g
    g.build()
    from rucene_amd import _lib
    L = C.CDLL(_lib.lib_path())
    header = open(os.path.join(ROOT, "include", "rucene_gpu.h")).read()
    for n in ("rgpu_docset_head", "rgpu_search_batch_required_set", "rgpu_search_batch_device_required_set"):
        assert n in _lib.EXPORTS and hasattr(L, n) and (n + "(") in header, n
    assert _lib.lib().rgpu_abi_version() == 6
    G = _lib.lib()
    n, card = C.c_int32(), C.c_int64()
    assert G.rgpu_docset_head(None, None, 1, None, C.byref(n), C.byref(card)) == -2
    assert G.rgpu_search_batch_required_set(None, None, None, 0, None, 0, 10, None, None) == -2
    assert G.rgpu_search_batch_device_required_set(None, None, None, 0, None, 0, 10, None, None, None) == -2


def test_cpp_mirror_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/required_set_demo.cpp (MatchAllDocsQuery, FilteredQuery over should-only queries and required_sets of
    csrc/host/gpu_index_searcher.hpp) links against the C ABI on a CPU-only box, warnings as errors; running it needs a GPU
    (tests/test_gpu_required_set.py)."""
    import subprocess
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "required_set_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "required_set_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_mirror_routing_rules():
    """The refusal and opt-in table of GpuIndexSearcher._peel: with required_sets off every shape is UnsupportedOperation, as it has
    been; with it on the shapes whose only required clauses are doc sets come back as the SHOULD side plus the sets."""
    import rucene_amd
    from rucene_amd.searcher import CachedFilter, FilterQuery, GpuIndexSearcher, _RequiredSet
    T, Bq, P, All = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery, rucene_amd.MatchAllDocsQuery
    R = rucene_amd.IntPoint.new_range_query
    off, on = GpuIndexSearcher.__new__(GpuIndexSearcher), GpuIndexSearcher.__new__(GpuIndexSearcher)
    on.required_sets = True
    for g in (off, on):
        g._points = {"n": (4, [])}
    F, X = CachedFilter(on, []), CachedFilter(on, [])
    star = All()
    shapes = {
        "b c #F": Bq.build([], [T(1), T(2)], filters=[F]),
        "#F": Bq.build([], [], filters=[F]),
        "range": R("n", 1, 5),
        "+range b c": Bq.build([R("n", 1, 5)], [T(1), T(2)]),
        "-X": Bq.build([], [], must_nots=[X]),
        "-t": Bq.build([], [], must_nots=[T(3)]),
        "#F -t -X": Bq.build([], [], filters=[F], must_nots=[T(3), X]),
        "+*:* b c": Bq.build([star], [T(1), T(2)]),
        "*:*": star,
        "b #F": Bq.build([], [T(1)], filters=[F]),
        "FilterQuery(b c #F, X)": FilterQuery(Bq.build([], [T(1), T(2)], filters=[F]), [X]),
    }
    for name, q in shapes.items():
        if name == "-t":   # (no doc set in it: with the option off it packs to the OR of MUST_NOT clauses only that matches nothing)
            assert off._peel(q, build=False) == (q, ([], []))
        else:
            with pytest.raises(rucene_amd.RgpuError) as e:
                off._peel(q, build=False)
            assert e.value.status == -5, name
        rest, (f, x) = on._peel(q, build=False)
        assert isinstance(rest, _RequiredSet), name
        want_shoulds = {"b c #F": [1, 2], "+range b c": [1, 2], "+*:* b c": [1, 2], "b #F": [1], "FilterQuery(b c #F, X)": [1, 2]}.get(name, [])
        assert [c.term for c in rest.shoulds] == want_shoulds, name
        assert len(f) >= 1, name   # (a query of exclusions alone: build()'s MatchAllDocsQuery)
    rest, (f, x) = on._peel(shapes["-t"], build=False)
    assert isinstance(f[0], All) and [c.term for c in x] == [3]
    rest, (f, x) = on._peel(shapes["#F -t -X"], build=False)
    assert f == [F] and x[0] is X and x[1].term == 3
    rest, (f, x) = on._peel(shapes["FilterQuery(b c #F, X)"], build=False)
    assert f == [F, X] and x == []
    # "b c -X": the masked disjunction (no MatchAllDocsQuery beside SHOULD clauses)
    q = Bq.build([], [T(1), T(2)], must_nots=[X])
    with pytest.raises(rucene_amd.RgpuError) as e:
        off._peel(q, build=False)
    assert e.value.status == -5
    rest, (f, x) = on._peel(q, build=False)
    assert isinstance(rest, Bq) and [c.term for c in rest.should_queries] == [1, 2] and f == [] and x == [X] and rest.min_should_match == 1
    # queries with a required clause of their own go the way they went, option or not
    for g in (off, on):
        rest, (f, x) = g._peel(Bq.build([T(1)], [T(2)], filters=[F], must_nots=[X]), build=False)
        assert isinstance(rest, Bq) and f == [F] and x == [X]
        plain = Bq.build([T(1)], [T(2)])
        assert g._peel(plain) == (plain, ([], []))
    # still refused with the option on
    refused = [Bq.build([], [T(1), T(2)], filters=[F], must_nots=[X], min_should_match=2),    # an exclusion beside min_should_match >= 2
               Bq.build([], [T(1), T(2)], filters=[F], must_nots=[T(3)], min_should_match=2),
               Bq.build([], [T(1), T(2)], must_nots=[X], min_should_match=2),
               Bq.build([], [T(1), P([1, 2])], filters=[F]),                                  # a phrase on the SHOULD side
               Bq.build([], [T(1), Bq.build([T(2), T(3)], [])], filters=[F]),                 # a nested clause there
               Bq.build([], [T(1), T(2, 0.0)], filters=[F]), Bq.build([], [T(1, -1.0)], filters=[F]),   # a SHOULD clause of boost <= 0
               Bq.build([], [], filters=[F], must_nots=[P([1, 2])])]
    for q in refused:
        with pytest.raises(rucene_amd.RgpuError) as e:
            on._peel(q, build=False)
        assert e.value.status == -5, q
    # min_should_match without an exclusion is accepted and has no effect
    rest, _ = on._peel(Bq.build([], [T(1), T(2)], filters=[F], min_should_match=2), build=False)
    assert isinstance(rest, _RequiredSet) and len(rest.shoulds) == 2
    # MatchAllDocsQuery is a MUST clause or a query, nothing else; build() leaves a MUST_NOT-only tree as it was given
    for bad in (lambda: Bq.build([T(1)], [star]), lambda: Bq.build([T(1)], [], filters=[star])):
        with pytest.raises(rucene_amd.RgpuError):
            bad()
    assert Bq.build([star], []) is star and star.extract_terms() == []
