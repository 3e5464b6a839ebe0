"""Parity at every edge of MUST + SHOULD trees (`-m gpu`): k_search_and<..., HAS_OPT> and the sequential scan k_req_opt_scan behind it,
which serve "+a b" (ReqOptScorer), "+a +(b c)" and "+a +(+b +c)". The fixtures of tests/opt_spectrum.py put a sequence on either side
of every edge of the reference's doc-to-doc rule - 99 | 100 | 101 docs scored before a low one, a state that skipped docs must not
move, dead lead postings (a doc another MUST clause lacks, a MUST_NOT doc, a deleted doc) that must not count, optional misses that
must, the 101st scored match at lead record 127 | 128 | 129 and 191 | 192 | 193, lead doc_freqs 1, 2, 127, 128, 129 and 257, a doc with
2 * req == sum / num exactly, a doc between the f32 and the f64 mean, a second leaf whose scorer starts afresh - and an optional
clause of every kind behind every lead shape of tests/and_spectrum.py: walked, bitmap, four-bit array, overflow lists, singletons,
absent terms, filter false positives, a MUST term again, a term twice, three clause orders, nine, ten and sixteen clauses.

Everything goes through GpuIndexSearcher.search_batch and the C ABI against the oracle (Searcher.search_opt, with the rule and - under
req_opt_rule = -1 - with exact=True) and OptRef: doc ids, score bits, -1 padding and hit counts exact; rows of ten or more present
optional clauses under the heap-order rule of oracle/parity.py with hit counts and skip decisions exact; nested trees against
_conjunction_with_a_nested_child. Knob invariance comes on top: the same bytes alone, in batches of 1, 4, 5 and all, beside TERM, AND
and OR rows, under every knob set. Which kernel answered is read from the library's counters. tests/test_opt_spectrum_cpu.py proves
the fixtures, the reference and that each of eleven mutants of the rule changes a row here."""
import numpy as np
import pytest

import and_spectrum as as_
import opt_spectrum as os_
import segment_spectrum as ss
import test_gpu_and_spectrum as tga
from opt_spectrum import Query
from test_gpu_norm_spectrum import _assert_row
from test_gpu_parity import _check_nested_rows, _conjunction_with_a_nested_child

pytestmark = pytest.mark.gpu

RULE_CONTEXTS = {"default": {}, "bpi1": dict(and_blocks_per_item=1), "walk": dict(and_bitmaps=-1)}
FAMILY_KS = (10, 129)


@pytest.fixture(scope="module")
def ctxs():
    """get(knob set, always_add): one context per knob set of test_gpu_and_spectrum.py and of RULE_CONTEXTS, with the reference's rule
    (default) or with req_opt_rule = -1."""
    import os

    import rucene_amd
    made = {}

    def get(name, always_add=False):
        if (name, always_add) not in made:
            knobs = dict(tga.KNOBS[name] if name in tga.KNOBS else RULE_CONTEXTS[name])
            if always_add:
                knobs["req_opt_rule"] = -1
            env = tga.ENV.get(name, {})
            os.environ.update(env)
            try:
                made[(name, always_add)] = rucene_amd.Context(profile_kernels=True, **knobs)
            finally:
                for key in env:
                    del os.environ[key]
        return made[(name, always_add)]
    yield get
    for c in made.values():
        c.close()


def _gpu_leaf(fx):
    import rucene_amd
    return rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, doc_base=fx.doc_base, live_docs=fx.live_docs,
                                 sum_total_term_freq=fx.sttf)


def _gpu_query(q):
    import rucene_amd
    T = rucene_amd.TermQuery
    return rucene_amd.BooleanQuery.build([T(t) for t in q.must], [T(t) for t in q.should], filters=[T(t) for t in q.filt], must_nots=[T(t) for t in q.must_not])


def _nested_query(r):
    import rucene_amd
    T, B = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    clauses = [T(t) for t in r.musts]
    clauses.insert(r.at, B.build([], [T(t) for t in r.inner]) if r.is_or else B.build([T(t) for t in r.inner], []))
    return B.build(clauses, [], must_nots=[T(t) for t in r.nots])


def _search(g, queries, k):
    hits, totals = g.search_batch([_nested_query(q) if isinstance(q, os_.Nested) else _gpu_query(q) for q in queries], k)
    assert hits.shape == (len(queries), k) and len(totals) == len(queries)
    return hits, totals


def _launches(c, name):
    st = c.kernel_stats()
    return st[name]["launches"] if name in st else 0


_searchers, _refs, _rows = {}, {}, {}


def _osr(oracle, leaves):
    key = tuple(leaf.key for leaf in leaves)
    if key not in _searchers:
        _searchers[key] = oracle.Searcher([leaf.oracle_segment(oracle) for leaf in leaves])
    return _searchers[key]


def _ref(oracle, leaves, i=0):
    key = (tuple(leaf.key for leaf in leaves), i)
    if key not in _refs:
        _refs[key] = os_.OptRef(oracle, leaves[i], _osr(oracle, leaves))
    return _refs[key]


def _want(oracle, leaves, q, k, exact=False):
    """The oracle's row of a MUST + SHOULD query (a plain one through segment_spectrum.oracle_rows), once per (index, query, k, mode)."""
    key = (tuple(leaf.key for leaf in leaves), q, k, exact)
    if key not in _rows:
        osr = _osr(oracle, leaves)
        row = os_.oracle_row(oracle, osr, q, k, exact) if q.should and q.must else ss.oracle_rows(oracle, osr, [q], k)[0]
        for a in row[:2]:
            a.setflags(write=False)
        _rows[key] = row
    return _rows[key]


def _check_rows(oracle, leaves, queries, hits, totals, k, exact, what):
    for i, q in enumerate(queries):
        _assert_row(hits[i], totals[i], _want(oracle, leaves, q, k, exact), (what, k, i, q))


def _same_rows(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.asarray(a[1]).tolist() == np.asarray(b[1]).tolist()


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
NEIGHBOURS = [Query(must=(os_.R_THIRD,)), Query(must=(os_.R_HOLD, os_.R_THIRD)), Query(should=(os_.R_THIRD, os_.R_BAN)), Query(must=(os_.R_ALL,), must_not=(os_.R_BAN,))]
RULE_COMBOS = [(c, n, lv, v) for c in RULE_CONTEXTS for n in os_.NORMS for lv in os_.LIVE for v in os_.VERSIONS]


@pytest.mark.parametrize("knobs,norms,live,version", RULE_COMBOS, ids=["%s-%s-%s-v%d" % c for c in RULE_COMBOS])
def test_rule_sequences(ctxs, oracle, knobs, norms, live, version):
    """Every sequence alone, all in one batch, in batches of 4 and 5 (the scan runs one wavefront per query, four to a workgroup) and
    beside TERM, AND, OR and MUST_NOT rows, at k in {1, 10, 64, 65, 128, 129, 300} - above 128 the scan runs once per pass under a
    ceiling, and the state must be the same in every pass: each row against the oracle and OptRef, bit for bit, and the same bytes
    whatever the batch. With req_opt_rule = -1: the oracle's exact=True rows, and no scan."""
    import rucene_amd
    fx = os_.RuleLeaf(norms, live, version)
    ref = _ref(oracle, [fx])
    names, queries = list(os_.rule_queries()), list(os_.rule_queries().values())
    c = ctxs(knobs)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    try:
        c.kernel_stats_reset()
        for k in os_.KS:
            what = (knobs, norms, live, version)
            together = _search(g, queries, k)
            _check_rows(oracle, [fx], queries, *together, k, False, what)
            for i, q in enumerate(queries):
                _assert_row(together[0][i], together[1][i], ref.row(q, k), (what, k, names[i], "OptRef"))
                alone = _search(g, [q], k)
                assert _same_rows(alone, (together[0][i:i + 1], together[1][i:i + 1])), (what, k, names[i], "alone")
            for size in (os_.WG_WAVES, os_.WG_WAVES + 1):
                for at in range(0, len(queries), size):
                    part = _search(g, queries[at:at + size], k)
                    assert _same_rows(part, (together[0][at:at + size], together[1][at:at + size])), (what, k, size, at)
            beside = [x for i, q in enumerate(queries) for x in ([q] + [NEIGHBOURS[i % len(NEIGHBOURS)]] * (i % 3))]
            rows = [j for j, x in enumerate(beside) if x.should and x.must]
            hits, totals = _search(g, beside, k)
            _check_rows(oracle, [fx], beside, hits, totals, k, False, what + ("beside",))
            assert _same_rows((hits[rows], totals[rows]), together), (what, k, "beside TERM, AND and OR rows")
        assert _launches(c, "k_req_opt_scan") > 0
    finally:
        leaf.segment.close()
    c = ctxs(knobs, always_add=True)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    try:
        c.kernel_stats_reset()
        for k in os_.KS:
            hits, totals = _search(g, queries, k)
            _check_rows(oracle, [fx], queries, hits, totals, k, True, (knobs, norms, live, version, "always add"))
            for i, q in enumerate(queries):
                _assert_row(hits[i], totals[i], ref.row(q, k, exact=True), (knobs, k, names[i], "OptRef, exact"))
        assert _launches(c, "k_req_opt_scan") == 0 and _launches(c, "k_search_and") > 0
    finally:
        leaf.segment.close()


TWO_COMBOS = [("default", "rank", "none", 1), ("bpi1", "raw", "seeded", 0), ("walk", "none", "seeded", 1), ("default", "rank", "seeded", 0)]


@pytest.mark.parametrize("knobs,norms,live,version", TWO_COMBOS, ids=["%s-%s-%s-v%d" % c for c in TWO_COMBOS])
def test_every_leaf_has_a_scorer_of_its_own(ctxs, oracle, knobs, norms, live, version):
    """Two leaves: leaf B's first 101 scored docs take the optional sum whatever leaf A left behind - TWO's LOWs in front of B, and every
    other sequence a second time."""
    import rucene_amd
    fxs = [os_.RuleLeaf(norms, live, version), os_.RuleLeaf(norms, live, version, which="B", doc_base=os_.R_MAX_DOC)]
    refs = [_ref(oracle, fxs, 0), _ref(oracle, fxs, 1)]
    queries = list(os_.rule_queries().values())
    for always_add in (False, True):
        leaves = [_gpu_leaf(fx) for fx in fxs]           # (a segment belongs to the context that searched it first)
        try:
            g = rucene_amd.GpuIndexSearcher(leaves, ctx=ctxs(knobs, always_add))
            for k in os_.KS:
                hits, totals = _search(g, queries, k)
                _check_rows(oracle, fxs, queries, hits, totals, k, always_add, (knobs, norms, live, version, always_add))
                for i, q in enumerate(queries):
                    _assert_row(hits[i], totals[i], os_.index_row(refs, q, k, exact=always_add), (knobs, k, i, "OptRef over two leaves"))
        finally:
            for leaf in leaves:
                leaf.segment.close()
    d, sc, total = _want(oracle, fxs, os_.rule_queries()["TWO"], 300)
    assert total == 241 and (d >= os_.R_MAX_DOC).sum() == 120


# ---- HAS_OPT at the edges of k_search_and ---------------------------------------------------------------------------------------------
def _check_ten(oracle, fx, q, row, total, k, exact, what):
    """A row of ten or more present optional clauses: the hit count exact (oracle and set algebra), doc ids and scores under the
    heap-order rule against the oracle's complete row, and every returned doc on the side of the rule OptRef puts it."""
    from oracle import parity
    ref = _ref(oracle, [fx])
    docs, final, skipped, req, opt, _ = ref.walk(q, exact=exact)
    full = _want(oracle, [fx], q, docs.size + 1, exact)
    assert total == full[2] == docs.size == as_.ref_docs(fx, Query(must=q.must, must_not=q.must_not)).size, (what, "hit count")
    parity.check_heap_order_opt_row(full[0], full[1], row["doc"], row["score"], total, k, what=str(what))
    n = min(k, docs.size)
    at = np.searchsorted(docs, row["doc"][:n])
    assert (docs[at] == row["doc"][:n]).all()
    took = row["score"][:n] > 1.25 * req[at]                                   # (the optional sum is at least half the required one)
    assert (took == ~skipped[at]).all(), (what, "skip decisions")
    assert np.allclose(row["score"][:n], final[at], rtol=1e-5, atol=0), (what, "clause-order sums")


@pytest.mark.parametrize("knobs,norms,live,version", tga.COMBOS, ids=["%s-%s-%s-v%d" % c for c in tga.COMBOS])
def test_optional_families(ctxs, oracle, knobs, norms, live, version):
    """MUST + SHOULD and MUST + SHOULD + MUST_NOT families, the rows of ten, ten-less-one and sixteen optional clauses and the nested
    trees, each in a batch of its own and all dealt into one with the plain, NOT and FILTER families, at k = 10 and 129: with the rule
    against search_opt, under req_opt_rule = -1 - the run that puts optional clauses behind the survivor queue - against exact=True."""
    import rucene_amd
    fx = as_.Leaf(norms, live, version)
    both, at, fams = os_.mixed()
    queued = os_.queue_rows(fx, os_.WITH_OPT, tga.AND_BITMAPS[knobs])
    if tga.AND_BITMAPS[knobs] == 0:         # the queue carries survivors behind these leads: the path is taken
        assert {as_.Q_LEAD, as_.S_LEAD} | set(as_.G_LEADS) <= {as_.lead_of(fx, Query(must=os_.WITH_OPT[i].must)) for i in queued}
    docs_of = lambda t: (lambda d: d[fx.alive[d]].astype(np.int32))(fx.lists[t][0])   # noqa: E731
    for always_add in (False, True):
        c = ctxs(knobs, always_add)
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
        what = (knobs, norms, live, version, "always add" if always_add else "rule")
        try:
            c.kernel_stats_reset()
            for k in FAMILY_KS:
                apart = {}
                for name, fam in os_.OPT_FAMILIES.items():
                    apart[name] = _search(g, fam, k)
                    _check_rows(oracle, [fx], fam, *apart[name], k, always_add, what + (name,))
                    for i, q in enumerate(fam):
                        assert apart[name][1][i] == as_.ref_docs(fx, Query(must=q.must, must_not=q.must_not)).size, (what, name, i, "set algebra")
                ten = _search(g, os_.TEN, k)
                _assert_row(ten[0][1], ten[1][1], _want(oracle, [fx], os_.TEN_ONE_ABSENT, k, always_add), what + ("ten named, nine present",))
                for i in (0, 2):
                    _check_ten(oracle, fx, os_.TEN[i], ten[0][i], ten[1][i], k, always_add, what + ("ten or more", i, k))
                expect = [_nested_want(oracle, fx, docs_of, r, k) for r in os_.NESTED]
                nested = _check_nested_rows(g, [_nested_query(r) for r in os_.NESTED], expect, os_.NESTED, k)
                hits, totals = _search(g, both + os_.TEN + os_.NESTED, k)
                for name in fams:
                    if name in apart:
                        assert _same_rows((hits[at[name]], totals[at[name]]), apart[name]), (what, k, name, "mixed batch against its own")
                    else:
                        tga._check_exact(oracle, fx, fams[name], hits[at[name]], totals[at[name]], k, what + (name, "mixed"))
                n = len(both)
                assert _same_rows((hits[n:n + 3], totals[n:n + 3]), ten) and _same_rows((hits[n + 3:], totals[n + 3:]), nested), (what, k, "mixed")
            assert (_launches(c, "k_req_opt_scan") > 0) == (not always_add)
            fp = leaf.segment.footprint()
            seen = both + os_.TEN + [Query(must=r.musts + r.inner, must_not=r.nots) for r in os_.NESTED]
            assert (fp["doc_bitmap_terms"], fp["doc_bitmap_refused"]) == os_.bitmap_terms(fx, seen, tga.AND_BITMAPS[knobs]), (what, fp)
        finally:
            leaf.segment.close()


_nested_rows = {}


def _nested_want(oracle, fx, docs_of, r, k):
    key = (fx.key, r, k)
    if key not in _nested_rows:
        _nested_rows[key] = _conjunction_with_a_nested_child(oracle, _osr(oracle, [fx]), docs_of, fx.df, list(r.musts), list(r.inner), r.is_or, list(r.nots), r.at, k)
    return _nested_rows[key]


def test_rows_do_not_depend_on_the_knobs(ctxs, oracle):
    """Every knob set of the conjunction suite: the optional families' rows are the oracle's and OptRef's, and the same bytes, in both modes."""
    import rucene_amd
    fx = as_.Leaf("rank", "seeded", 1)
    queries = os_.ALL_OPT + [os_.TEN_ONE_ABSENT]
    for always_add in (False, True):
        rows = {}
        for knobs in tga.KNOBS:
            leaf = _gpu_leaf(fx)
            g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(knobs, always_add))
            try:
                rows[knobs] = {k: _search(g, queries, k) for k in (10, 65, 129)}
            finally:
                leaf.segment.close()
        ref = _ref(oracle, [fx])
        for k, got in rows["default"].items():
            _check_rows(oracle, [fx], queries, *got, k, always_add, ("default", always_add))
            for i, q in enumerate(queries):
                _assert_row(got[0][i], got[1][i], ref.row(q, k, exact=always_add), (k, i, q, always_add, "OptRef"))
            for knobs in tga.KNOBS:
                assert _same_rows(got, rows[knobs][k]), (k, knobs, always_add)


def test_membership_bits_are_never_built_for_an_optional_clause(ctxs, oracle):
    """ensure_memb_only_locked is asked for the second cheapest MUST clause: an optional clause of 512 to bitmap_min_df_and - 1 docs is
    walked behind any lead (k_bitmap_memb does not run), a denser one gets its bitmap; the same clause under MUST gets its bits."""
    import rucene_amd
    fx = as_.Leaf()
    c = ctxs("default")
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    try:
        c.kernel_stats_reset()
        queries = [Query(must=(as_.CORE_LEAD,), should=(as_.C_512,)), Query(must=(as_.LEAD_128, as_.EVERY), should=(as_.C_1171,)),
                   Query(must=(as_.CORE_LEAD, as_.C_1172), should=(as_.C_512, as_.C_1171)), Query(must=(as_.Q_LEAD,), should=(as_.C_1171, as_.C_1172))]
        assert not any(as_.wants_memb_only(fx, Query(must=q.must)) for q in queries)
        hits, totals = _search(g, queries, 10)
        _check_rows(oracle, [fx], queries, hits, totals, 10, False, "optional clauses in the membership-only range")
        fp = leaf.segment.footprint()
        assert _launches(c, "k_bitmap_memb") == 0 and (fp["doc_bitmap_terms"], fp["doc_bitmap_refused"]) == os_.bitmap_terms(fx, queries) == (2, 0)
        must = [Query(must=(as_.CORE_LEAD, as_.C_512), should=(as_.EVERY,))]
        assert as_.wants_memb_only(fx, Query(must=must[0].must))
        hits, totals = _search(g, must, 10)
        _check_rows(oracle, [fx], must, hits, totals, 10, False, "the same clause under MUST")
        assert _launches(c, "k_bitmap_memb") == 1
        # ... and once its bits exist, the optional clause's answers are still the oracle's
        hits, totals = _search(g, queries, 129)
        _check_rows(oracle, [fx], queries, hits, totals, 129, False, "after the bits were built")
    finally:
        leaf.segment.close()
