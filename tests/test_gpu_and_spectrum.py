"""Parity at every edge of the conjunction kernel k_search_and (`-m gpu`), which answers every AND, MUST + MUST_NOT and FILTER query.
The fixtures of tests/and_spectrum.py put a list or a query on either side of each threshold that kernel and its host rules branch
on: the clause behind the lead walked | membership bits alone | a bitmap | a bitmap with the four-bit array (doc_freq 511 | 512,
1171 | 1172, 2343 | 2344 on a leaf of 300 007 docs), a lead of 127 | 128 docs, 4096 | 4097 postings of freq >= 255, candidates at
bit 0 and 31, nibble 0 and 7, doc 0 and max_doc - 1, freq 14 | 15 and 254 | 255 | 256, 1 to 9 lead blocks per item, 0 | 1 | 127 |
128 survivors waiting and 639 of the queue's 640 cells, a lead freq of 2^20 - 1 | 2^20, lead items of 60 to 130 blocks, filter
false positives under MUST, MUST_NOT and in a VInt tail, every block edge of a walked clause, the register window's 62 | 63 | 64th
slot, find_block_wave's first look and 64-ary rounds on a leaf of 4300 one-bit blocks, walked clauses at clause positions 1, 2, 62
and 63, singletons, tail-only leads, df 0, equal doc_freqs in all six orders, k 64 | 65 and 128 | 129, a 1100-doc plateau, and batches
of 2047 | 2048 | 2049 work items around one round of the XCD remap.

Everything goes through GpuIndexSearcher.search_batch and the C ABI, against the oracle: doc ids, score bits, -1 padding and hit
counts exact, hit counts also against the numpy set algebra; plain MUST, MUST + MUST_NOT and MUST + FILTER families each in a batch of
its own and dealt into one batch (so that plain queries run in the HAS_NOT instantiation) with byte-identical rows; the same rows
under every knob set (and_bitmaps -1 | 0 | 4, and_blocks_per_item 1 | 3 | 200 | auto, RGPU_AND_MEMB_ONLY=0). Which path answered is
read from the library's own counters. tests/test_and_spectrum_cpu.py proves the fixtures and the oracle's rows on the CPU.

Not reached: the `ti_start == 2` branch (survivors popped with their first-clause freq already known) needs the four-bit array as
the batched probe's source, which only RGPU_AND_PROBE=1 variant builds ask; the default build probes the membership bits, so every
survivor carries code 15 and asks the first clause again."""
import os

import numpy as np
import pytest

import and_spectrum as as_
from and_spectrum import C_511, C_512, C_1171, C_1172, CORE_LEAD, LEAD_127, LEAD_128, OVF_CAP, OVF_OVER, Query
from test_gpu_norm_spectrum import _assert_row
from test_gpu_or_spectrum import _gpu_leaf

pytestmark = pytest.mark.gpu

KNOBS = {"default": {}, "walk": dict(and_bitmaps=-1), "quarter": dict(and_bitmaps=4), "bpi1": dict(and_blocks_per_item=1), "bpi3": dict(and_blocks_per_item=3),
         "bpi200": dict(and_blocks_per_item=200), "walk200": dict(and_bitmaps=-1, and_blocks_per_item=200), "no-memb": {}}
ENV = {"no-memb": {"RGPU_AND_MEMB_ONLY": "0"}}
AND_BITMAPS = {name: kw.get("and_bitmaps", 0) for name, kw in KNOBS.items()}
# (knobs, norms, live, .doc version): rank norms without deletions under every knob set; every other value of every axis at least once
COMBOS = [(name, "rank", "none", 1) for name in KNOBS] + [
    ("default", "raw", "none", 1), ("default", "none", "seeded", 1), ("default", "rank", "seeded", 0), ("walk", "raw", "seeded", 0),
    ("quarter", "none", "none", 0), ("bpi1", "rank", "seeded", 1), ("bpi3", "raw", "none", 0), ("bpi200", "none", "seeded", 1),
    ("walk200", "rank", "seeded", 1), ("no-memb", "rank", "seeded", 0)]


@pytest.fixture(scope="module")
def ctxs():
    import rucene_amd
    made = {}

    def get(name):
        if name not in made:
            env = ENV.get(name, {})
            os.environ.update(env)
            try:
                made[name] = rucene_amd.Context(profile_kernels=True, **KNOBS[name])
            finally:
                for key in env:
                    del os.environ[key]
        return made[name]
    yield get
    for c in made.values():
        c.close()


_searchers, _rows = {}, {}


def _osr(oracle, leaf):
    if leaf.key not in _searchers:
        _searchers[leaf.key] = oracle.Searcher([leaf.oracle_segment(oracle)])
    return _searchers[leaf.key]


def _want(oracle, leaf, queries, k):
    """The oracle's rows and the set algebra's hit counts, computed once per (leaf, query, k) and shared by every test."""
    missing = [q for q in dict.fromkeys(queries) if (leaf.key, q, k) not in _rows]
    if missing:
        for q, row in zip(missing, as_.oracle_rows(oracle, _osr(oracle, leaf), missing, k)):
            for a in row[:2]:
                a.setflags(write=False)
            _rows[(leaf.key, q, k)] = (row, as_.ref_docs(leaf, q))
    return [_rows[(leaf.key, q, k)] for q in queries]


def _gpu_query(q):
    import rucene_amd
    T = rucene_amd.TermQuery
    return rucene_amd.BooleanQuery.build([T(t) for t in q.must], [], filters=[T(t) for t in q.filt], must_nots=[T(t) for t in q.must_not])


def _search(g, queries, k):
    hits, totals = g.search_batch([_gpu_query(q) for q in queries], k)
    assert hits.shape == (len(queries), k) and len(totals) == len(queries)
    return hits, totals


def _check_exact(oracle, leaf, queries, hits, totals, k, what):
    """Doc ids, score bits, -1 in the unused slots and the hit count, as the oracle has them; the hit count as the set algebra has it."""
    for i, (q, (want, docs)) in enumerate(zip(queries, _want(oracle, leaf, queries, k))):
        _assert_row(hits[i], totals[i], want, (what, k, i, q))
        assert totals[i] == docs.size, (what, k, i, q, "hit count against the set algebra")


def _same_rows(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.asarray(a[1]).tolist() == np.asarray(b[1]).tolist()


def _launches(c, name):
    st = c.kernel_stats()
    return st[name]["launches"] if name in st else 0


def _decoded(c):
    return c.last_search_counters()["blocks_decoded"]


# ---- the families, knob set by knob set ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs,norms,live,version", COMBOS, ids=["%s-%s-%s-v%d" % c for c in COMBOS])
def test_families(ctxs, oracle, knobs, norms, live, version):
    """Plain MUST, MUST + MUST_NOT and MUST + FILTER queries each in a batch of its own and all three dealt into one, at k in
    {1, 10, 64, 65, 128, 129, 300}: every row against the oracle, and the mixed batch's rows byte for byte those of the separate ones."""
    import rucene_amd
    fx = as_.Leaf(norms, live, version)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(knobs))
    both, at = as_.mixed()
    try:
        for k in as_.KS:
            what = (knobs, norms, live, version)
            apart = {}
            for name, fam in as_.FAMILIES.items():
                apart[name] = _search(g, fam, k)
                _check_exact(oracle, fx, fam, *apart[name], k, what + (name,))
            hits, totals = _search(g, both, k)
            for name in as_.FAMILIES:
                assert _same_rows((hits[at[name]], totals[at[name]]), apart[name]), (what, k, name, "mixed batch against its own")
        fp = leaf.segment.footprint()
        assert (fp["doc_bitmap_terms"], fp["doc_bitmap_refused"]) == as_.bitmap_terms(fx, as_.ALL_QUERIES, AND_BITMAPS[knobs]), (knobs, fp)
    finally:
        leaf.segment.close()


@pytest.mark.parametrize("norms,live,version", [("rank", "none", 1), ("raw", "seeded", 0)], ids=["v1", "raw-deletions-legacy"])
def test_rows_do_not_depend_on_the_knobs(ctxs, oracle, norms, live, version):
    """Bitmaps for every clause that may have one, for none, for the densest alone; 1, 3, 200 and the library's own number of lead
    blocks per item; membership bits switched off: the rows of the mixed batch are the same bytes."""
    import rucene_amd
    fx = as_.Leaf(norms, live, version)
    both, _ = as_.mixed()
    rows = {}
    for knobs in KNOBS:
        leaf = _gpu_leaf(fx)
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(knobs))
        try:
            rows[knobs] = {k: _search(g, both, k) for k in (10, 65, 129)}
        finally:
            leaf.segment.close()
    for k, got in rows["default"].items():
        _check_exact(oracle, fx, both, *got, k, ("default", norms, live, version))
        for knobs in KNOBS:
            assert _same_rows(got, rows[knobs][k]), (k, knobs, norms, live, version)


# ---- the collector ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", ["default", "bpi1", "bpi3", "bpi200", "walk"])
def test_a_plateau_of_tied_scores_across_item_edges(ctxs, oracle, knobs):
    """1100 docs of one score in items of 1, 3, 8 and 200 lead blocks: every k cuts the tie at the k-th doc, in two and three passes
    beyond 128; next to it queries with fewer hits than k."""
    import rucene_amd
    fx = as_.Leaf()
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs(knobs))
    queries = [Query(must=(as_.CONST, as_.EVERY)), Query(must=(as_.TAIL_2, as_.EVERY)), Query(must=(as_.CONST, as_.EVERY, as_.EVERY)),
               Query(must=(as_.SING_EVEN, as_.EVERY)), Query(must=(as_.CONST,), must_not=(as_.SING_MISS,)), Query(must=(CORE_LEAD, as_.ABSENT))]
    try:
        for k in as_.KS:
            hits, totals = _search(g, queries, k)
            _check_exact(oracle, fx, queries, hits, totals, k, knobs)
            for i in (0, 2, 4):
                assert totals[i] == 1100 and hits[i]["doc"].tolist() == list(range(as_.CONST_LO, as_.CONST_LO + k)), (knobs, k, i)
                assert np.unique(hits[i]["score"].view(np.int32)).size == 1
            assert totals[1] == 2 and totals[3] == 1 and totals[5] == 0 and (hits[5]["doc"] == -1).all()
    finally:
        leaf.segment.close()


# ---- the launch's shape -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [2047, 2048, 2049, 5000])
def test_batches_around_one_round_of_the_xcd_remap(ctxs, oracle, n_items):
    """One lead block per item: batches of 2047 | 2048 | 2049 and 5000 work items - one round of the remap is 8 chunks x 64 workgroups x
    4 wavefronts = 2048 items - and every query of them exact."""
    import rucene_amd
    fx = as_.Leaf()
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctxs("bpi1"))
    queries = as_.batch_of_items(fx, n_items)
    assert sum(as_.items_of(fx, q, 1) for q in queries) == n_items
    try:
        for k in (10, 129):
            hits, totals = _search(g, queries, k)
            _check_exact(oracle, fx, queries, hits, totals, k, n_items)
    finally:
        leaf.segment.close()


# ---- which path answered ------------------------------------------------------------------------------------------------------------
def test_host_rules_decide_the_path(ctxs, oracle):
    """From the library's own counters, on fresh segments: blocks_decoded is the lead's FullBlocks when every clause behind the lead
    has a bitmap and exceeds them when the first one is membership-only or walked; k_bitmap_memb runs for a first clause of 512 to
    bitmap_min_df_and - 1 docs behind a lead of 128 or more, and never with the switch off; doc_bitmap_terms / doc_bitmap_refused
    count what the doc_freq rules and BITMAP_OVF_CAP predict."""
    import rucene_amd
    fx = as_.Leaf()
    q = lambda *m: Query(must=m)   # noqa: E731
    c = ctxs("default")
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    try:
        bitmapped = [x for x in as_.PLAIN + as_.WITH_NOT if as_.all_bitmaps_behind_the_lead(fx, x) and not as_.matches_nothing(fx, x)]
        assert len(bitmapped) >= 40 and not any(as_.wants_memb_only(fx, x) for x in bitmapped)
        c.kernel_stats_reset()
        hits, totals = _search(g, bitmapped, 10)
        _check_exact(oracle, fx, bitmapped, hits, totals, 10, "bitmaps behind the lead")
        assert _decoded(c) == sum(fx.full_blocks(as_.lead_of(fx, x)) for x in bitmapped)
        assert _launches(c, "k_bitmap_memb") == 0 and _launches(c, "k_bitmap_build") > 0
        fp = leaf.segment.footprint()
        assert (fp["doc_bitmap_terms"], fp["doc_bitmap_refused"]) == as_.bitmap_terms(fx, bitmapped)
        # (query, more blocks decoded than the lead's) - one query per launch, in this order
        steps = [(q(LEAD_127, C_512), True), (q(LEAD_128, C_512), True), (q(CORE_LEAD, C_512), True), (q(CORE_LEAD, C_511), True), (q(CORE_LEAD, C_1171), True),
                 (q(CORE_LEAD, C_1172), False), (q(CORE_LEAD, OVF_OVER), True), (q(CORE_LEAD, OVF_CAP), False), (q(CORE_LEAD, as_.HALF_B, OVF_OVER), True)]
        done, memb = list(bitmapped), set()
        for x, more in steps:
            hits, totals = _search(g, [x], 10)
            _check_exact(oracle, fx, [x], hits, totals, 10, x)
            lead_blocks = fx.full_blocks(as_.lead_of(fx, x))
            assert more == (not as_.all_bitmaps_behind_the_lead(fx, x))
            assert (_decoded(c) > lead_blocks) == more and _decoded(c) >= lead_blocks, (x, _decoded(c), lead_blocks)
            done.append(x)
            if as_.wants_memb_only(fx, x):
                memb.add(as_.required(fx, x)[1][0])
            fp = leaf.segment.footprint()
            assert _launches(c, "k_bitmap_memb") == len(memb) and (fp["doc_bitmap_terms"], fp["doc_bitmap_refused"]) == as_.bitmap_terms(fx, done), (x, fp)
        assert memb == {C_512, C_1171} and fp["doc_bitmap_refused"] == 1
    finally:
        leaf.segment.close()
    c = ctxs("no-memb")
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    try:
        c.kernel_stats_reset()
        queries = [q(LEAD_128, C_512), q(CORE_LEAD, C_1171), q(CORE_LEAD, C_512, as_.EVERY)]
        hits, totals = _search(g, queries, 10)
        _check_exact(oracle, fx, queries, hits, totals, 10, "no-memb")
        assert _launches(c, "k_bitmap_memb") == 0 and all(as_.wants_memb_only(fx, x) for x in queries)
    finally:
        leaf.segment.close()


@pytest.mark.parametrize("knobs", ["walk200", "walk"])
@pytest.mark.parametrize("live,version", [("none", 1), ("seeded", 0)], ids=["v1", "deletions-legacy"])
def test_walked_clauses_decode_the_blocks_the_model_names(ctxs, oracle, knobs, live, version):
    """Every clause walked, one item per query: blocks_decoded is the lead's FullBlocks plus, per lead vector and clause, the clause's
    FullBlocks whose doc range holds a candidate still alive - counted by tests/and_spectrum.py from the lists. The count does not
    depend on where the items are cut (a lead block is a vector of its own either way): the same with the library's item size."""
    import rucene_amd
    fx = as_.Leaf("rank", live, version)
    c = ctxs(knobs)
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    try:
        for name, fam in as_.FAMILIES.items():
            fam = [x for x in fam if knobs == "walk" or as_.items_of(fx, x, 200) <= 1]
            hits, totals = _search(g, fam, 10)
            _check_exact(oracle, fx, fam, hits, totals, 10, (knobs, name))
            assert _decoded(c) == sum(as_.walked_trace(fx, x)[0] for x in fam), name
        fp = leaf.segment.footprint()
        assert fp["doc_bitmap_terms"] == fp["doc_bitmap_refused"] == 0 and _launches(c, "k_bitmap_memb") == 0
    finally:
        leaf.segment.close()


# ---- the big leaf -------------------------------------------------------------------------------------------------------------------
def test_find_block_wave_on_4300_blocks(ctxs, oracle):
    """The every-doc list of the 550 475-doc leaf, walked: leads whose second block lies 0 to 64 + 4097 clause blocks behind the
    first one's, near the directory's end, and in the VInt tail. Rows exact, and exactly two clause blocks decoded per lead block pair."""
    import rucene_amd
    fx = as_.Leaf(big=True)
    c = ctxs("walk")
    leaf = _gpu_leaf(fx)
    g = rucene_amd.GpuIndexSearcher([leaf], ctx=c)
    try:
        for k in (10, 300):
            hits, totals = _search(g, as_.BIG_QUERIES, k)
            _check_exact(oracle, fx, as_.BIG_QUERIES, hits, totals, k, "big leaf")
        hits, totals = _search(g, as_.BIG_QUERIES, 10)
        assert _decoded(c) == sum(as_.walked_trace(fx, x)[0] for x in as_.BIG_QUERIES)
        for x in as_.BIG_QUERIES:             # one query per launch: its own count
            _search(g, [x, x], 10)
            assert _decoded(c) == 2 * as_.walked_trace(fx, x)[0], as_.BIG_NAMES[x.must[0]]
    finally:
        leaf.segment.close()
