"""Same kernels, same number of launches per call (`-m gpu`): one fixed batch through each entry point that shares the candidate
stage, the match stage and the collectors - rgpu_search_phrase_batch, rgpu_search_phrase_bool_batch, rgpu_search_phrase_or_batch,
the conjunction rows of rgpu_docset_collect_batch and rgpu_rescore_phrase_batch - at k = 10 and k = 129, on a packed and on a legacy
segment. The {launch name: launches} map of every call is compared with tests/golden/launch_sequence.json, which was recorded by
this very test body at the commit BEFORE the entry points came to share their stages: the parity suites see what a call returns,
this sees what it launched.

Only the launches the entry points themselves issue are compared. What prepares a segment's terms, builds doc bitmaps or stages
arrays (PREPARATION) runs once per segment or depends on what the context has staged before: those counts would tie a key to the
calls made in front of it, so they are left out of both sides and every key holds whatever order the tests run in.

(To record: RGPU_LAUNCH_SEQUENCE_WRITE=<file> writes the maps there instead of asserting. rgpu_docset_collect_batch takes no k: its
batch is recorded once per segment format, under "-".)"""
import json
import os

import pytest

import docset as ds
import phrase_bool as pb
import phrase_or as po
import phrase_rescore as pr
import phrase_spectrum as ps

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequence.json")
KS = (10, 129)
FORMATS = (("packed", 1), ("legacy", 0))
PREPARATION = ("k_skip_dir", "k_block_headers", "k_scan_rows", "k_prepare_blocks", "k_prepare_norms", "k_chunk_frontiers", "k_stage_copy",
               "k_decode_terms", "k_bitmap_build")
_seen = {}


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()
    if os.environ.get("RGPU_LAUNCH_SEQUENCE_WRITE"):
        with open(os.environ["RGPU_LAUNCH_SEQUENCE_WRITE"], "w") as f:
            json.dump(_seen, f, indent=1, sort_keys=True)
            f.write("\n")


def _launches(ctx, call):
    ctx.kernel_stats_reset()
    call()
    return {n: v["launches"] for n, v in ctx.kernel_stats().items() if v["launches"] and n not in PREPARATION}


def _settle(entry, fmt, k, st):
    key = "%s/%s/k=%s" % (entry, fmt, k)
    print(key, st)
    assert st, key   # an empty map must not pass for a recorded one
    if os.environ.get("RGPU_LAUNCH_SEQUENCE_WRITE"):
        _seen[key] = st
        return
    with open(GOLDEN) as f:
        want = json.load(f)
    assert key in want and st == want[key], (key, st, want.get(key))


def _bool_index(oracle, ctx, fx, version):
    import rucene_amd
    ix = pb.Index(oracle, [fx], version=version)
    leaves = ix.gpu_leaves()
    return ix, leaves, rucene_amd.GpuIndexSearcher(leaves, ctx=ctx)


def _close(ix, leaves):
    for leaf in leaves:
        if leaf.segment is not None:
            leaf.segment.close()
    ix.close()


@pytest.mark.parametrize("fmt,version", FORMATS)
@pytest.mark.parametrize("name", ["main", "groups"])
def test_phrase_bool(ctx, oracle, name, fmt, version):
    fx, queries = (pb.main(), pb.MAIN_QUERIES) if name == "main" else (pb.groups(), pb.GROUP_QUERIES)
    ix, leaves, g = _bool_index(oracle, ctx, fx, version)
    try:
        for k in KS:
            st = _launches(ctx, lambda: g.search_batch([q.build() for q in queries], k))
            assert pb.CANDIDATES in st and pb.SCORE in st and ps.COLLECT in st, st
            _settle("phrase_bool:" + name, fmt, k, st)
    finally:
        _close(ix, leaves)


@pytest.mark.parametrize("fmt,version", FORMATS)
def test_phrase_or(ctx, oracle, fmt, version):
    ix, leaves, g = _bool_index(oracle, ctx, po.main(), version)
    try:
        for k in KS:
            st = _launches(ctx, lambda: g.search_batch([q.build(raw=True) for q in po.MAIN_QUERIES], k))
            assert po.CANDIDATES in st and po.WINDOWS in st, st
            _settle("phrase_or", fmt, k, st)
    finally:
        _close(ix, leaves)


@pytest.mark.parametrize("fmt,version", FORMATS)
def test_phrase(ctx, oracle, fmt, version):
    """the first served case of the placement segment: its exact and its slop-1 query in one batch"""
    import rucene_amd
    fx = ps.segment("place")
    case = next(c for c in fx.cases if all(q.error is None for q in c.queries) and {q.slop for q in c.queries} == {0, 1})
    queries = [rucene_amd.PhraseQuery(q.terms, q.positions, slop=q.slop) for q in case.queries]
    ix = fx.index(oracle, version)
    leaf = ps.leaf_of(ix, len(fx.postings), fx.norms, fx.max_doc, fx.doc_count, fx.sum_ttf)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        for k in KS:
            st = _launches(ctx, lambda: g.search_phrase_batch(queries, k))
            assert "k_search_and(phrase candidates)" in st and ps.COLLECT in st and (ps.MERGE in st) == (k <= ps.PASS_K), st
            _settle("phrase", fmt, k, st)
    finally:
        leaf.segment.close()
        ix.close()


@pytest.mark.parametrize("fmt,version", FORMATS)
def test_docset_conjunctions(ctx, fmt, version):
    import rucene_amd
    from rucene_amd import _lib as gpu
    fx = ds.collect_leaf(version)
    seg = rucene_amd.Segment(ctx, fx.seg.doc_bytes, fx.norms, fx.max_doc, live_docs=None, index_options=2)
    try:
        _w, _idf, cache = gpu.bm25_compute_weight(1.2, 0.75, 1000, 1000, 60000, [10], 1.0)
        qs, ts = ds.pack(fx.terms, ds.COLLECT_ANDS, gpu, sim_table=ctx.sim_table(cache, 1.2))
        sets = []
        st = _launches(ctx, lambda: sets.extend(seg.docset_collect_batch(qs, ts)))
        for s in sets:
            s.close()
        assert "k_search_and(doc set candidates)" in st and "k_docset_from_emitted" in st, st
        _settle("docset", fmt, "-", st)
    finally:
        seg.close()


@pytest.mark.parametrize("fmt,version", FORMATS)
def test_phrase_rescore(ctx, oracle, fmt, version):
    import rucene_amd
    fx = pr.membership()
    ix = fx.index(oracle, version=version, woven=False)
    leaf = pr.leaf_of(ix, fx)
    try:
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        rows, queries = [pr.side_by_side_row()], [rucene_amd.PhraseQuery([pr.T, pr.B])]
        for k in KS:
            st = _launches(ctx, lambda: g.rescore_batch(pr.as_hits(rows, k), queries))
            assert pr.CANDIDATES in st and pr.COMBINE in st, st
            _settle("phrase_rescore", fmt, k, st)
    finally:
        leaf.segment.close()
        ix.close()
