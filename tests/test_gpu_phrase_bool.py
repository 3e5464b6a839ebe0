"""BooleanQuery with exact PhraseQuery clauses on the device (`-m gpu`): rgpu_search_phrase_bool_batch through the C ABI and through
GpuIndexSearcher.search_batch against tests/phrase_bool.py's composed reference (proven by tests/test_phrase_bool_cpu.py) — docs,
score bits, padding and total_hits equal, nowhere a tolerance. The kernel statistics of a batch say which launches answered it."""
import numpy as np
import pytest

import phrase_bool as pb

pytestmark = pytest.mark.gpu

REDO = "k_phrase_match(left by the 64-candidate kernel)"


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


class Opened:
    """An index of tests/phrase_bool.py as a GpuIndexSearcher beside its reference."""

    def __init__(self, oracle, ctx, fxs, version=1, deleted=None, **kw):
        import rucene_amd
        self.ix = pb.Index(oracle, fxs, version=version, deleted=deleted)
        self.leaves = self.ix.gpu_leaves()
        self.g = rucene_amd.GpuIndexSearcher(self.leaves, ctx=ctx, **kw)
        assert self.g._stats_leaf == 0

    def close(self):
        for leaf in self.leaves:
            if leaf.segment is not None:
                leaf.segment.close()
        self.ix.close()


def _opened(oracle, ctx, *a, **kw):
    o = Opened(oracle, ctx, *a, **kw)
    try:
        yield o
    finally:
        o.close()


@pytest.fixture(scope="module")
def main(oracle, ctx):
    yield from _opened(oracle, ctx, [pb.main()])


@pytest.fixture(scope="module")
def groups(oracle, ctx):
    yield from _opened(oracle, ctx, [pb.groups()])


def _search(ctx, o, queries, k):
    """One batch -> (hits, totals, {launch name: launches})"""
    ctx.kernel_stats_reset()
    hits, totals = o.g.search_batch([q.build() for q in queries], k)
    st = {n: v["launches"] for n, v in ctx.kernel_stats().items() if v["launches"]}
    return hits, totals, st


def _check(o, hits, totals, queries, what):
    for i, q in enumerate(queries):
        pb.check_row(hits[i], totals[i], o.ix.rows(q), (what, q))


def test_every_main_query_in_one_batch_and_alone(ctx, main):
    """Every cost case, kind of term clause, number of phrases, shared term, repeated term, gapped phrase, MUST_NOT, FILTER and
    boost-0 query of the main fixture: as one batch, and each alone (a row does not depend on its neighbours)."""
    qs = pb.MAIN_QUERIES
    hits, totals, st = _search(ctx, main, qs, 16)
    print("main", st)
    assert st.get(pb.CANDIDATES) == 1 and st.get(pb.FANOUT) == 1 and st.get(pb.SCORE) == 1, st
    assert "k_search_and(phrase candidates)" not in st
    _check(main, hits, totals, qs, "batch")
    assert sum(int(t) > 0 for t in totals) >= len(qs) - 2
    for i, q in enumerate(qs):
        h1, t1, st1 = _search(ctx, main, [q], 16)
        assert (h1[0] == hits[i]).all() and t1[0] == totals[i], q
        dead = q.name in ("a required term absent", "a phrase term absent")
        assert (pb.CANDIDATES in st1) == (pb.SCORE in st1) == (not dead), (q, st1)
        assert (pb.FANOUT in st1) == (sum(isinstance(c, pb.Ph) for c, _ in q.required()) > 1), (q, st1)


def test_one_phrase_batches_need_no_fanout_and_plane_one_reaches_the_redo_list(ctx, main):
    one = [q for q in pb.MAIN_QUERIES if sum(isinstance(c, pb.Ph) for c, _ in q.required()) == 1]
    hits, totals, st = _search(ctx, main, one, 8)
    assert pb.CANDIDATES in st and pb.SCORE in st and pb.FANOUT not in st, st
    _check(main, hits, totals, one, "one phrase")
    eleven = [q for q in pb.MAIN_QUERIES if q.name == "eleven positions in plane 1"]
    hits, totals, st = _search(ctx, main, eleven, 40)
    assert st.get(REDO) == 1 and pb.FANOUT in st, st   # doc 72 holds PC eleven times: plane 1's candidate goes to the one-candidate kernel
    _check(main, hits, totals, eleven, "eleven")
    assert pb.ELEVEN_DOC in hits[0]["doc"].tolist()


def test_group_edges(ctx, groups):
    """63, 64 and 65 candidates; a 64-slot group without survivors between two that have some; a query without candidates between
    two that have hits."""
    by = {q.name: q for q in pb.GROUP_QUERIES}
    qs = [by["63 candidates"], by["no candidate"], by["64 candidates"], by["a group without survivors"], by["no candidate"], by["65 candidates"]]
    hits, totals, st = _search(ctx, groups, qs, 130)
    assert pb.CANDIDATES in st and pb.SCORE in st and pb.FANOUT not in st, st
    _check(groups, hits, totals, qs, "groups")
    assert totals.tolist() == [32, 0, 50, 128, 0, 65]


@pytest.mark.parametrize("name,k", [("63 candidates", 1), ("63 candidates", 31), ("63 candidates", 32), ("63 candidates", 33), ("236 hits", 64),
                                    ("236 hits", 65), ("236 hits", 128), ("236 hits", 129), ("236 hits", 300)])
def test_k_ladder(ctx, groups, name, k):
    q = [x for x in pb.GROUP_QUERIES if x.name == name]
    hits, totals, _ = _search(ctx, groups, q, k)
    _check(groups, hits, totals, q, ("k", k))


@pytest.mark.parametrize("deleted", ["one", "all"])
def test_live_docs(ctx, oracle, deleted):
    """A deleted doc that matches everything (doc 72, the best hit; 254, the last posting of a block) is not collected and not counted;
    a leaf whose docs are all deleted has no hits."""
    gone = {pb.ELEVEN_DOC, 254} if deleted == "one" else set(range(pb.MAIN_DOCS))
    for o in _opened(oracle, ctx, [pb.main()], deleted=[gone]):
        qs = pb.ORDER_CASES + [q for q in pb.MAIN_QUERIES if q.name in ("two phrases sharing PB", "three MUST_NOT", "FILTER phrase")]
        hits, totals, st = _search(ctx, o, qs, 16)
        _check(o, hits, totals, qs, ("deleted", deleted))
        if deleted == "all":
            assert not totals.any() and (hits["doc"] == -1).all()
        else:
            assert totals.any() and not (set(hits["doc"].ravel().tolist()) & gone)


def test_three_leaves(ctx, oracle):
    """Doc bases; a leaf without a phrase term, a leaf without a MUST term; a query whose cost order differs between two leaves
    (weights from the statistics leaf, order from each leaf's own doc freqs)."""
    for o in _opened(oracle, ctx, pb.leaves()):
        hits, totals, st = _search(ctx, o, pb.LEAF_QUERIES, 24)
        assert st.get(pb.CANDIDATES) == 2 and st.get(pb.SCORE) == 2, st   # (the third leaf: every query dead, nothing launched)
        _check(o, hits, totals, pb.LEAF_QUERIES, "leaves")
        assert (hits[0]["doc"] >= pb.MAIN_DOCS).any() and (hits[0]["doc"][hits[0]["doc"] >= 0] < 2 * pb.MAIN_DOCS).all()


def test_legacy_doc_format(ctx, oracle):
    for o in _opened(oracle, ctx, [pb.main()], version=0):
        hits, totals, st = _search(ctx, o, pb.MAIN_QUERIES, 16)
        assert pb.CANDIDATES in st and pb.SCORE in st and "k_phrase_match" in st and "k_phrase_match_lanes" not in st, st
        _check(o, hits, totals, pb.MAIN_QUERIES, "version 0")


def test_unsupported_shapes_reach_the_cpu_fallback(ctx, oracle):
    """A sloppy clause, a phrase under SHOULD, a phrase under MUST_NOT, a SHOULD term beside a MUST phrase, five phrases: each is
    UnsupportedOperation (-5) and reaches cpu_fallback with the original query."""
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    seen = []

    def fallback(query, collector):
        seen.append(query)
        return "cpu"
    for o in _opened(oracle, ctx, [pb.main()], cpu_fallback=fallback):
        bad = [B.build([P([pb.PA, pb.PB], slop=1), T(pb.D600)], []), B.build([T(pb.D600)], [P([pb.PA, pb.PB]), T(pb.T40)]),
               B.build([T(pb.D600), T(pb.T40)], [], must_nots=[P([pb.PA, pb.PB])]), B.build([P([pb.PA, pb.PB])], [T(pb.T40)]),
               B.build([P([pb.PA, pb.PB])] * 5, [])]
        for q in bad:
            with pytest.raises(rucene_amd.RgpuError) as e:
                o.g.search_batch([q], 4)
            assert e.value.status == pb.UNSUPPORTED
            assert o.g.search(q, rucene_amd.TopDocsCollector(4)) == "cpu" and seen[-1] is q
        ok = pb.MAIN_QUERIES[0]
        coll = rucene_amd.TopDocsCollector(4)
        o.g.search(ok.build(), coll)
        d, s = o.ix.rows(ok)
        assert [x for x, _ in coll.top_docs().score_docs()] == d[:4].tolist() and coll.top_docs().total_hits() == d.size


def _raw(o, qs, ps, pts, ts, k, hits=None, totals=None, seg=None):
    from rucene_amd import _lib as gpu
    hits = np.full((qs.size, k), 7, dtype=np.int64).view(gpu.HIT_DTYPE).reshape(qs.size, k) if hits is None else hits
    totals = np.full(qs.size, -9, dtype=np.int64) if totals is None else totals
    rc = gpu.lib().rgpu_search_phrase_bool_batch((seg or o.leaves[0].segment)._h, qs.ctypes.data, qs.size, ps.ctypes.data, ps.size, pts.ctypes.data, pts.size,
                                                 ts.ctypes.data if ts.size else None, ts.size, k, hits.ctypes.data, totals.ctypes.data)
    return rc, hits, totals


def test_the_c_abi_itself_and_its_refusals(ctx, oracle, main):
    """rgpu_search_phrase_bool_batch on buffers of the caller's: the rows of the reference; a refused call writes nothing."""
    from rucene_amd import _lib as gpu
    o = main
    queries = pb.MAIN_QUERIES
    packed = o.g.pack_phrase_bool([q.build() for q in queries], o.leaves[0])
    rc, hits, totals = _raw(o, *packed, 16)
    assert rc == 0
    _check(o, hits, totals, queries, "C ABI")

    def refused(want, change, k=8):
        qs, ps, pts, ts = [a.copy() for a in o.g.pack_phrase_bool([q.build() for q in queries[:6]], o.leaves[0])]
        change(qs, ps, pts, ts)
        rc, hits, totals = _raw(o, qs, ps, pts, ts, k)
        assert rc == want, (rc, want)
        assert (hits.view(np.int64) == 7).all() and (totals == -9).all()
    refused(pb.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["phrase_slot"].__setitem__((0, 0), 3))     # out of range (3 required clauses)
    refused(pb.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["phrase_slot"].__setitem__((1, 0), -1))
    refused(pb.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["first_term"].__setitem__(5, ts.size))       # clause range outside terms[]
    refused(pb.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: ps["n_terms"].__setitem__(0, 1))                # check_phrase_query
    refused(pb.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: ts["sim_table"].__setitem__(0, 1 << 20))
    refused(pb.UNSUPPORTED, lambda qs, ps, pts, ts: ps["slop"].__setitem__(2, 1))
    refused(pb.UNSUPPORTED, lambda qs, ps, pts, ts: qs["n_phrases"].__setitem__(0, 5))
    refused(pb.UNSUPPORTED, lambda qs, ps, pts, ts: qs["n_phrases"].__setitem__(0, 0))
    refused(pb.UNSUPPORTED, lambda qs, ps, pts, ts: None, k=1025)     # k above RGPU_MAX_K
    # two phrases on one slot
    two = [q for q in queries if q.name == "two phrases sharing PB"]
    qs, ps, pts, ts = o.g.pack_phrase_bool([q.build() for q in two], o.leaves[0])
    qs["phrase_slot"][0, 1] = qs["phrase_slot"][0, 0]
    rc, hits, totals = _raw(o, qs, ps, pts, ts, 8)
    assert rc == pb.ILLEGAL_ARGUMENT and (hits.view(np.int64) == 7).all()
    # no .pos attached
    bare = pb.Index(oracle, [pb.main()])
    leaf = bare.gpu_leaves()[0]
    seg = gpu.Segment(ctx, leaf.doc_bytes, leaf.norms, leaf.max_doc, 0, None, leaf.index_options)
    try:
        rc, hits, totals = _raw(o, *packed, 8, seg=seg)
        assert rc == pb.ILLEGAL_STATE and (hits.view(np.int64) == 7).all() and (totals == -9).all()
    finally:
        seg.close()
        bare.close()


def test_a_mixed_batch_keeps_row_order(ctx, main):
    """Term, boolean, phrase and phrase-bool queries in one search_batch call: every row is what it is alone, in its place."""
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    o = main
    by = {q.name: q for q in pb.MAIN_QUERIES}
    mixed = [by["five clauses"].build(), T(pb.T40), P([pb.PA, pb.PB]), B.build([T(pb.T40), T(pb.D600)], []), by["two phrases sharing PB"].build(),
             B.build([], [T(pb.R20), T(pb.S)]), P([pb.PB, pb.PC]), by["three MUST_NOT"].build()]
    ctx.kernel_stats_reset()
    hits, totals = o.g.search_batch(mixed, 12)
    st = {n for n, v in ctx.kernel_stats().items() if v["launches"]}
    assert pb.CANDIDATES in st and pb.SCORE in st and "k_search_and(phrase candidates)" in st, st
    for i, q in enumerate(mixed):
        h1, t1 = o.g.search_batch([q], 12)
        assert (h1[0] == hits[i]).all() and t1[0] == totals[i], i
    for i, name in ((0, "five clauses"), (4, "two phrases sharing PB"), (7, "three MUST_NOT")):
        pb.check_row(hits[i], totals[i], o.ix.rows(by[name]), ("mixed", name))
    ph, pt = o.g.search_phrase_batch([mixed[2], mixed[6]], 12)
    assert (ph[0] == hits[2]).all() and (ph[1] == hits[6]).all() and pt.tolist() == [totals[2], totals[6]]


def test_cpp_host_mirror_gives_the_same_rows(ctx, main, tmp_path):
    """GpuIndexSearcher::search_many (csrc/host/gpu_index_searcher.hpp) with PhraseBooleanQuery rows beside a PhraseQuery and a
    TermQuery row: tests/cpp/phrase_bool_demo.cpp over the same files prints the reference's rows for every main query, in order."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    o, fx = main, main.ix.fxs[0]
    exe = str(tmp_path / "phrase_bool_demo")
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "cpp", "phrase_bool_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    doc_bytes, pos_bytes = o.ix.ixs[0].files()
    leaf = o.leaves[0]
    for name, blob in (("doc", doc_bytes), ("pos", pos_bytes), ("norms", fx.norms.tobytes()), ("terms", leaf.terms.tobytes()),
                       ("tpos", leaf.term_positions.tobytes())):
        (tmp_path / (name + ".bin")).write_bytes(bytes(blob))

    def clause(occur, c):
        if isinstance(c, pb.Ph):
            return "%s:p:%s:%s:%r" % (occur, ",".join(map(str, c.terms)), ",".join(map(str, pb.phrase_positions(c))), float(c.boost))
        return "%s:t:%d" % (occur, c)
    lines = [" ".join([clause("m", c) for c in q.musts] + [clause("f", c) for c in q.filters] + [clause("n", t) for t in q.must_nots]) for q in pb.MAIN_QUERIES]
    lines += ["plain p:%d,%d:0,1:1.0" % (pb.PA, pb.PB), "plain t:%d" % pb.T40]
    (tmp_path / "queries.txt").write_text("\n".join(lines) + "\n")
    k = 16
    out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.doc_count), str(fx.sum_ttf), str(k)], text=True).strip().splitlines()
    assert len(out) == len(lines) + 1 and out[-1] == "fallback 1", out[-3:]
    import rucene_amd
    plain, plain_totals = o.g.search_batch([rucene_amd.PhraseQuery([pb.PA, pb.PB]), rucene_amd.TermQuery(pb.T40)], k)
    for i, line in enumerate(out[:-1]):
        parts = line.split()
        assert parts[0] == "row" and int(parts[1]) == i
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        if i < len(pb.MAIN_QUERIES):
            d, s = o.ix.rows(pb.MAIN_QUERIES[i])
            total = d.size
        else:
            row = plain[i - len(pb.MAIN_QUERIES)]
            d, s, total = row["doc"][row["doc"] >= 0], row["score"][row["doc"] >= 0], int(plain_totals[i - len(pb.MAIN_QUERIES)])
        n = min(k, d.size)
        assert int(parts[2]) == total, (i, line)
        assert got == list(zip(d[:n].tolist(), np.asarray(s[:n], dtype=np.float32).view(np.uint32).tolist())), (i, line)
