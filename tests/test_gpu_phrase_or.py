"""BooleanQuery of SHOULD / MUST_NOT clauses with exact PhraseQuery clauses among the SHOULD ones on the device (`-m gpu`):
rgpu_search_phrase_or_batch through the C ABI, through GpuIndexSearcher.search_batch and through the C++ mirror, against
tests/phrase_or.py's composed reference (proven by tests/test_phrase_or_cpu.py) — docs, score bits, padding and total_hits equal,
nowhere a tolerance. The kernel statistics of a batch say which launches answered it."""
import numpy as np
import pytest

import phrase_bool as pb
import phrase_or as po

pytestmark = pytest.mark.gpu

KNOBS = {"default": {}, "small-items": dict(and_blocks_per_item=1), "w256": dict(or_window_docs=256)}


@pytest.fixture(scope="module")
def contexts():
    import rucene_amd
    made = {}

    def get(name):
        if name not in made:
            made[name] = rucene_amd.Context(profile_kernels=True, **KNOBS[name])
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(contexts):
    return contexts("default")


class Opened:
    """An index of tests/phrase_bool.py's kind as a GpuIndexSearcher beside its reference."""

    def __init__(self, oracle, ctx, fxs, version=1, deleted=None, **kw):
        import rucene_amd
        self.ctx = ctx
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
    yield from _opened(oracle, ctx, [po.main()])


@pytest.fixture(scope="module")
def pbmain(oracle, ctx):
    yield from _opened(oracle, ctx, [pb.main()])


def _search(o, queries, k, raw=True):
    """One batch -> (hits, totals, {launch name: launches})"""
    o.ctx.kernel_stats_reset()
    hits, totals = o.g.search_batch([q.build(raw=raw) for q in queries], k)
    st = {n: v["launches"] for n, v in o.ctx.kernel_stats().items() if v["launches"]}
    return hits, totals, st


def _check(o, hits, totals, queries, what):
    for i, q in enumerate(queries):
        po.check_row(hits[i], totals[i], po.rows(o.ix, q), (what, q))


def _answered_by_the_new_path(st, calls=1, passes=1):
    """the candidate conjunction once per call, the five run-building launches and the window kernel once per pass; no phrase collector"""
    assert st.get(po.CANDIDATES) == calls, st
    for name in po.RUN_KERNELS + (po.WINDOWS,):
        assert st.get(name) == calls * passes, (name, st)
    assert "k_search_and(phrase candidates)" not in st and "k_phrase_collect" not in st and pb.CANDIDATES not in st, st


def test_every_main_query_in_one_batch_and_alone(main):
    """Every bucket, window, min_should_match, MUST_NOT and absent-clause query of the main fixture: as one batch, and each alone (a
    row does not depend on its neighbours)."""
    qs = po.MAIN_QUERIES
    hits, totals, st = _search(main, qs, 16)
    print("main", st)
    _answered_by_the_new_path(st)
    _check(main, hits, totals, qs, "batch")
    for i, q in enumerate(qs):
        h1, t1, st1 = _search(main, [q], 16)
        assert (h1[0] == hits[i]).all() and t1[0] == totals[i], q
        if q.name == "every clause absent":
            assert po.CANDIDATES not in st1 and po.WINDOWS not in st1 and t1[0] == 0, st1
        else:
            _answered_by_the_new_path(st1)


def test_append_order_does_not_show(oracle, contexts):
    """One lead block per conjunction item: the wide phrase's 405 candidates are appended by four wavefronts in whatever order they
    finish. The run — and with it every row — is the reference's, and the same call made twice returns identical bytes."""
    for o in _opened(oracle, contexts("small-items"), [po.main()]):
        k = 500
        first = _search(o, po.ORDER_QUERIES, k)
        _answered_by_the_new_path(first[2], passes=4)   # k = 500: four passes of 128, one match stage
        assert first[2].get("k_phrase_match_lanes") == 1, first[2]
        _check(o, first[0], first[1], po.ORDER_QUERIES, "order")
        assert first[1].tolist() == [len(set(po.WIDE_MATCHES) | set(o.ix.fxs[0].docs_of(po.T300))), len(po.WIDE_MATCHES)]
        for _ in range(2):
            again = _search(o, po.ORDER_QUERIES, k)
            assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_bucket_edges(main):
    """0, 1, 63, 64 and 65 matches in one bucket; an empty bucket between two full ones; candidates without a match; cost 1 and 2;
    matches at B - 1, B, 2B - 1, doc 0 and max_doc - 1 (the wide phrase, alone and beside a term)."""
    qs = po.BUCKET_QUERIES + po.ORDER_QUERIES
    hits, totals, st = _search(main, qs, 80)
    _answered_by_the_new_path(st)
    _check(main, hits, totals, qs, "buckets")
    by = {q.name: i for i, q in enumerate(qs)}
    assert [int(totals[by["%d matches in bucket 1" % n]]) for n in (0, 1, 63, 64, 65)] == [5, 6, 70, 71, 72]
    assert totals[by["an empty bucket between two full ones"]] == 2048 + 2 and totals[by["candidates, no match, alone"]] == 0
    assert totals[by["cost 1 alone"]] == 1 and hits[by["cost 1 alone"]]["doc"][0] == 1500 and totals[by["cost 2"]] == 7
    full, total = main.g.search_batch([po.Q([po.FULL]).build(raw=True)], 1024)
    po.check_row(full[0], total[0], po.rows(main.ix, po.Q([po.FULL])), "the full buckets, every hit")
    wide = set(main.g.search_batch([po.Q([po.WIDE]).build(raw=True)], 512)[0][0]["doc"].tolist())
    assert set(po.WIDE_EDGES) <= wide and wide - {-1} == set(po.WIDE_MATCHES)


def test_window_edges_and_a_dense_clause(oracle, contexts):
    """or_window_docs = 256: a phrase match on a window's last doc (255) and on the next window's first (256); a dense term clause
    (decoded inside the window kernel) beside the phrase's run."""
    for o in _opened(oracle, contexts("w256"), [po.main()]):
        qs = po.WINDOW_QUERIES + po.MSM_QUERIES + po.NOT_QUERIES
        for k in (24, 300):
            hits, totals, st = _search(o, qs, k)
            _answered_by_the_new_path(st, passes=(k + 127) // 128)
            _check(o, hits, totals, qs, ("w256", k))
        docs = o.g.search_batch([po.Q([po.WIDE, po.T5]).build()], 512)[0][0]["doc"].tolist()
        assert {255, 256} <= set(docs)


def test_sum_order_shared_terms_gaps_and_boost_zero(pbmain):
    """P T T, T P T, T T P over the order-sensitive clauses of tests/phrase_bool.py; the same phrase twice; two phrases sharing a
    term; a gapped phrase; a boost-0 phrase whose phrase-only docs are hits scoring +0.0; nine clauses of which four are phrases; a
    doc with eleven positions (the one-candidate match kernel)."""
    qs = po.PB_QUERIES
    hits, totals, st = _search(pbmain, qs, 40)
    _answered_by_the_new_path(st)
    assert st.get("k_phrase_match(left by the 64-candidate kernel)") == 1, st
    _check(pbmain, hits, totals, qs, "pb")
    rows = [hits[i][:int(min(40, totals[i]))] for i in range(3)]
    assert sorted(rows[0]["doc"].tolist()) == sorted(rows[1]["doc"].tolist()) == sorted(rows[2]["doc"].tolist())
    assert rows[0].tobytes() != rows[1].tobytes() or rows[0].tobytes() != rows[2].tobytes()   # the order shows in the bits
    for i, q in enumerate(qs):
        h1, t1, _ = _search(pbmain, [q], 40)
        assert (h1[0] == hits[i]).all() and t1[0] == totals[i], q
    zero = [i for i, q in enumerate(qs) if q.name == "boost 0: the phrase-only docs count"][0]
    row = hits[zero][:int(totals[zero])]
    only = set(pbmain.ix.clause_scores(0, pb.AB)) - set(pbmain.ix.clause_scores(0, pb.R20))
    assert only <= set(row["doc"].tolist()) and all(s.view(np.uint32) == 0 for d, s in zip(row["doc"], row["score"]) if d in only)


@pytest.mark.parametrize("deleted", ["none", "first", "last", "all"])
def test_deleted_phrase_only_docs(oracle, ctx, deleted):
    """Deletions among the docs only the phrase holds: none, the first (doc 21: 0 and 14 are T5's too), the last (max_doc - 1), all of
    them. A deleted match is not collected and not counted."""
    gone = {"none": set(), "first": {po.PHRASE_ONLY[0]}, "last": {po.PHRASE_ONLY[-1]}, "all": set(po.PHRASE_ONLY)}[deleted]
    assert deleted == "none" or (gone and po.PHRASE_ONLY[-1] == po.MAIN_DOCS - 1)
    for o in _opened(oracle, ctx, [po.main()], deleted=[gone]):
        qs = [po.Q([po.WIDE, po.T5]), po.Q([po.WIDE]), po.Q([po.T5, po.WIDE, po.C65], [po.NOT1]), po.Q([po.WIDE, po.DENSE], msm=2)]
        hits, totals, st = _search(o, qs, 512)
        _answered_by_the_new_path(st, passes=4)
        _check(o, hits, totals, qs, ("deleted", deleted))
        assert not (set(hits["doc"].ravel().tolist()) & gone)
        assert totals[0] == len(set(po.WIDE_MATCHES) | set(po.T5_DOCS)) - len(gone) and totals[1] == len(po.WIDE_MATCHES) - len(gone)


def test_three_leaves(oracle, ctx):
    """Doc bases; a leaf that lacks the term clause, a leaf that lacks a phrase term (the phrase drops out, the term clause stays), a
    leaf that lacks every clause (nothing launched there)."""
    for o in _opened(oracle, ctx, pb.leaves()):
        hits, totals, st = _search(o, po.LEAF_QUERIES, 48)
        # (the third leaf lacks PA: no phrase exists there — no candidates, no run to build, the term clauses alone go through the windows)
        assert st.get(po.CANDIDATES) == 2 and all(st.get(n) == 2 for n in po.RUN_KERNELS) and st.get(po.WINDOWS) == 3, st
        _check(o, hits, totals, po.LEAF_QUERIES, "leaves")
        assert (hits[0]["doc"] >= 2 * pb.MAIN_DOCS).any() and (hits[0]["doc"] >= pb.MAIN_DOCS).any()
        hits, totals, st = _search(o, po.LEAF_QUERIES[1:2], 48)
        _answered_by_the_new_path(st, calls=2)       # the third leaf holds neither phrase: no launch
        _check(o, hits, totals, po.LEAF_QUERIES[1:2], "a leaf without every clause")
        assert (hits[0]["doc"][hits[0]["doc"] >= 0] < 2 * pb.MAIN_DOCS).all()


@pytest.mark.parametrize("k", [1, 100, 128, 129])
def test_k_ladder(main, k):
    """k = 1; k above the hit count (72 hits); k = 128 (one pass) and 129 (two) on a query with more than 2000 hits."""
    qs = [po.Q([po.C65, po.T5]), po.Q([po.WIDE, po.DENSE], [po.NOT1])]
    hits, totals, st = _search(main, qs, k)
    _answered_by_the_new_path(st, passes=(k + 127) // 128)
    _check(main, hits, totals, qs, ("k", k))
    assert totals[0] == 72 and totals[1] > 2000


def test_legacy_doc_format(oracle, ctx):
    for o in _opened(oracle, ctx, [po.main()], version=0):
        qs = po.MAIN_QUERIES
        hits, totals, st = _search(o, qs, 130)
        _answered_by_the_new_path(st, passes=2)
        assert "k_phrase_match" in st and "k_phrase_match_lanes" not in st, st
        _check(o, hits, totals, qs, "version 0")
    for o in _opened(oracle, ctx, [pb.main()], version=0):
        hits, totals, st = _search(o, po.PB_QUERIES, 16)
        _check(o, hits, totals, po.PB_QUERIES, "version 0, pb")


def test_unsupported_shapes_reach_the_cpu_fallback_and_served_ones_do_not(oracle, ctx):
    """A sloppy SHOULD phrase, ten SHOULD clauses with a phrase, a phrase under MUST_NOT, five phrases: each is UnsupportedOperation (-5)
    and reaches cpu_fallback with the original query; a served disjunction is answered on the device through search()."""
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    seen = []

    def fallback(query, collector):
        seen.append(query)
        return "cpu"
    for o in _opened(oracle, ctx, [po.main()], cpu_fallback=fallback):
        ph = P([po.W1, po.W2])
        bad = [B.build([], [P([po.W1, po.W2], slop=1), T(po.T5)]), B.build([], [ph] + [T(po.T5)] * 9), B.build([], [T(po.T5), T(po.T300)], must_nots=[ph]),
               B.build([], [ph, T(po.T5)], must_nots=[ph]), B.build([], [ph] * 5)]
        for q in bad:
            with pytest.raises(rucene_amd.RgpuError) as e:
                o.g.search_batch([q], 4)
            assert e.value.status == po.UNSUPPORTED
            assert o.g.search(q, rucene_amd.TopDocsCollector(4)) == "cpu" and seen[-1] is q
        n_seen = len(seen)
        ok = po.Q([po.WIDE, po.T5], [po.NOT1], name="served")
        coll = rucene_amd.TopDocsCollector(6)
        o.g.search(ok.build(), coll)
        d, s = po.rows(o.ix, ok)
        assert [x for x, _ in coll.top_docs().score_docs()] == d[:6].tolist() and coll.top_docs().total_hits() == d.size and len(seen) == n_seen


def _raw(o, qs, ps, pts, ts, k, seg=None):
    from rucene_amd import _lib as gpu
    hits = np.full((qs.size, k), 7, dtype=np.int64).view(gpu.HIT_DTYPE).reshape(qs.size, k)
    totals = np.full(qs.size, -9, dtype=np.int64)
    rc = gpu.lib().rgpu_search_phrase_or_batch((seg or o.leaves[0].segment)._h, qs.ctypes.data, qs.size, ps.ctypes.data, ps.size, pts.ctypes.data, pts.size,
                                               ts.ctypes.data if ts.size else None, ts.size, k, hits.ctypes.data, totals.ctypes.data)
    return rc, hits, totals


def test_the_c_abi_itself_and_its_refusals(ctx, oracle, main):
    """rgpu_search_phrase_or_batch on buffers of the caller's: the rows of the reference; a refused call writes nothing."""
    from rucene_amd import _lib as gpu
    o = main
    queries = po.MAIN_QUERIES
    packed = o.g.pack_phrase_or([q.build(raw=True) for q in queries], o.leaves[0])
    rc, hits, totals = _raw(o, *packed, 16)
    assert rc == 0
    _check(o, hits, totals, queries, "C ABI")
    head = [po.Q([po.WIDE, po.T300, po.DENSE]), po.Q([po.T5, po.C65], [po.NOT1]), po.Q([po.C63, po.C64, po.T5], msm=2)]

    def refused(want, change, k=8):
        qs, ps, pts, ts = [a.copy() for a in o.g.pack_phrase_or([q.build(raw=True) for q in head], o.leaves[0])]
        change(qs, ps, pts, ts)
        rc, hits, totals = _raw(o, qs, ps, pts, ts, k)
        assert rc == want, (rc, want)
        assert (hits.view(np.int64) == 7).all() and (totals == -9).all()
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["phrase_slot"].__setitem__((0, 0), 3))     # out of range (3 SHOULD clauses)
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["phrase_slot"].__setitem__((1, 0), -1))
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["phrase_slot"].__setitem__((2, 1), 0))     # named twice
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["first_term"].__setitem__(2, ts.size))      # clause range outside terms[]
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["first_phrase"].__setitem__(2, ps.size - 1))
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["n_must_not"].__setitem__(0, -1))
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["min_should_match"].__setitem__(1, 256))
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: qs["min_should_match"].__setitem__(1, -1))
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: ps["n_terms"].__setitem__(0, 1))               # check_phrase_query
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: ps["sim_table"].__setitem__(1, 1 << 20))
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: ts["sim_table"].__setitem__(0, 1 << 20))
    refused(po.ILLEGAL_ARGUMENT, lambda qs, ps, pts, ts: None, k=0)
    refused(po.UNSUPPORTED, lambda qs, ps, pts, ts: ps["slop"].__setitem__(2, 1))
    refused(po.UNSUPPORTED, lambda qs, ps, pts, ts: qs["n_phrases"].__setitem__(0, 5))
    refused(po.UNSUPPORTED, lambda qs, ps, pts, ts: qs["n_phrases"].__setitem__(0, 0))
    refused(po.UNSUPPORTED, lambda qs, ps, pts, ts: None, k=1025)     # k above RGPU_MAX_K
    many = [po.Q([po.WIDE] + [po.T5] * 8), po.Q([po.C65, po.T300])]
    qs, ps, pts, ts = o.g.pack_phrase_or([q.build(raw=True) for q in many], o.leaves[0])
    rc, hits, totals = _raw(o, qs, ps, pts, ts, 8)
    assert rc == 0                                                    # nine SHOULD clauses are served ...
    qs["first_term"][1], qs["n_terms"][1] = 0, 9                      # ... a phrase beside nine terms is not
    rc, hits, totals = _raw(o, qs, ps, pts, ts, 8)
    assert rc == po.UNSUPPORTED and (hits.view(np.int64) == 7).all() and (totals == -9).all()
    # no .pos attached
    bare = pb.Index(oracle, [po.main()])
    leaf = bare.gpu_leaves()[0]
    seg = gpu.Segment(ctx, leaf.doc_bytes, leaf.norms, leaf.max_doc, 0, None, leaf.index_options)
    try:
        rc, hits, totals = _raw(o, *packed, 8, seg=seg)
        assert rc == po.ILLEGAL_STATE and (hits.view(np.int64) == 7).all() and (totals == -9).all()
    finally:
        seg.close()
        bare.close()


def test_a_doc_that_holds_a_phrase_term_1025_times_refuses_the_call_whole(oracle, ctx):
    """The match stage's verdict comes before the disjunction runs: RGPU_ERR_UNSUPPORTED, nothing written, and the context answers
    the next batch."""
    import rucene_amd
    for o in _opened(oracle, ctx, [po.heavy()]):
        bad = [po.Q([po.H3, po.HEAVY]), po.Q([po.HEAVY, po.H3])]
        rc, hits, totals = _raw(o, *o.g.pack_phrase_or([q.build(raw=True) for q in bad], o.leaves[0]), 8)
        assert rc == po.UNSUPPORTED and (hits.view(np.int64) == 7).all() and (totals == -9).all()
        with pytest.raises(rucene_amd.RgpuError) as e:
            o.g.search_batch([bad[0].build()], 8)
        assert e.value.status == po.UNSUPPORTED
        hits, totals = o.g.search_batch([rucene_amd.TermQuery(po.H3)], 8)
        assert totals[0] == 10
    for o in _opened(oracle, ctx, [po.main()]):
        q = [po.Q([po.C1, po.T5])]
        hits, totals, st = _search(o, q, 8)
        _check(o, hits, totals, q, "after a refusal")


def test_a_mixed_batch_keeps_row_order(main):
    """Term, boolean, phrase, required-phrase and phrase-disjunction queries in one search_batch call: every row is what it is alone."""
    import rucene_amd
    T, B, P = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.PhraseQuery
    o = main
    by = {q.name: q for q in po.MAIN_QUERIES}
    names = {0: "a dense term beside the phrase", 3: "msm 2 of 3", 6: "MUST_NOT removes phrase-only docs"}
    mixed = [by[names[0]].build(), T(po.T300), P([po.W1, po.W2]), by[names[3]].build(), B.build([T(po.T300), P([po.W1, po.W2])], []),
             B.build([], [T(po.T5), T(po.DENSE)]), by[names[6]].build(), B.build([], [P([po.C65A, po.C65B])])]
    o.ctx.kernel_stats_reset()
    hits, totals = o.g.search_batch(mixed, 12)
    st = {n for n, v in o.ctx.kernel_stats().items() if v["launches"]}
    assert {po.CANDIDATES, pb.CANDIDATES, "k_search_and(phrase candidates)", po.WINDOWS} <= st and set(po.RUN_KERNELS) <= st, st
    for i, q in enumerate(mixed):
        h1, t1 = o.g.search_batch([q], 12)
        assert (h1[0] == hits[i]).all() and t1[0] == totals[i], i
    for i, name in names.items():
        po.check_row(hits[i], totals[i], po.rows(o.ix, by[name]), ("mixed", name))
    # a lone SHOULD phrase is the PhraseQuery itself (BooleanQuery::build): the phrase search's row, equal to the one-child disjunction's
    one, one_total = o.g.search_batch([po.Q([po.C65]).build(raw=True)], 12)
    assert (one[0] == hits[7]).all() and one_total[0] == totals[7] == 67


def test_cpp_host_mirror_gives_the_same_rows(main, tmp_path):
    """GpuIndexSearcher::search_many (csrc/host/gpu_index_searcher.hpp) with PhraseDisjunctionQuery rows beside a PhraseQuery and a
    TermQuery row: tests/cpp/phrase_or_demo.cpp over the same files prints the reference's rows for every main query, in order."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    o, fx = main, main.ix.fxs[0]
    exe = str(tmp_path / "phrase_or_demo")
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "cpp", "phrase_or_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    doc_bytes, pos_bytes = o.ix.ixs[0].files()
    leaf = o.leaves[0]
    for name, blob in (("doc", doc_bytes), ("pos", pos_bytes), ("norms", fx.norms.tobytes()), ("terms", leaf.terms.tobytes()),
                       ("tpos", leaf.term_positions.tobytes())):
        (tmp_path / (name + ".bin")).write_bytes(bytes(blob))

    def clause(occur, c):
        if isinstance(c, po.Ph):
            return "%s:p:%s:%s:%r" % (occur, ",".join(map(str, c.terms)), ",".join(map(str, pb.phrase_positions(c))), float(c.boost))
        return "%s:t:%d" % (occur, c)
    queries = po.MAIN_QUERIES
    lines = [" ".join(["msm:%d" % q.msm] + [clause("s", c) for c in q.shoulds] + [clause("n", t) for t in q.must_nots]) for q in queries]
    lines += ["plain p:%d,%d:0,1:1.0" % (po.W1, po.W2), "plain t:%d" % po.T300]
    (tmp_path / "queries.txt").write_text("\n".join(lines) + "\n")
    k = 16
    out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.doc_count), str(fx.sum_ttf), str(k)], text=True).strip().splitlines()
    assert len(out) == len(lines) + 1 and out[-1] == "fallback 2", out[-3:]
    import rucene_amd
    plain, plain_totals = o.g.search_batch([rucene_amd.PhraseQuery([po.W1, po.W2]), rucene_amd.TermQuery(po.T300)], k)
    for i, line in enumerate(out[:-1]):
        parts = line.split()
        assert parts[0] == "row" and int(parts[1]) == i
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        if i < len(queries):
            d, s = po.rows(o.ix, queries[i])
            total = d.size
        else:
            row = plain[i - len(queries)]
            d, s, total = row["doc"][row["doc"] >= 0], row["score"][row["doc"] >= 0], int(plain_totals[i - len(queries)])
        n = min(k, d.size)
        assert int(parts[2]) == total, (i, line)
        assert got == list(zip(d[:n].tolist(), np.asarray(s[:n], dtype=np.float32).view(np.uint32).tolist())), (i, line)
