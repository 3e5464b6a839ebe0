"""MUST + SHOULD trees with exact PhraseQuery clauses on the device (`-m gpu`): rgpu_search_phrase_opt_batch through the C ABI and
through GpuIndexSearcher(optional_phrases=True) against tests/phrase_opt.py's composed reference (proven by
tests/test_phrase_opt_cpu.py) - docs, score bits, {-1, 0} padding and total_hits equal, nowhere a tolerance. Queries without a phrase
are also compared with rgpu_search_batch's RGPU_OP_WITH_SHOULD rows, in both rule modes. The kernel statistics of a batch say which
launches answered it."""
import os
import subprocess

import numpy as np
import pytest

import phrase_bool as pb
import phrase_opt as po
import phrase_rescore as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_exact():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True, req_opt_rule=-1)
    yield c
    c.close()


class Opened:
    """An index of tests/phrase_bool.py's kind as a GpuIndexSearcher(optional_phrases=True) beside its reference."""

    def __init__(self, oracle, ctx, fxs, version=1, deleted=None, **kw):
        import rucene_amd
        self.ctx = ctx
        self.ix = pb.Index(oracle, fxs, version=version, deleted=deleted)
        self.leaves = self.ix.gpu_leaves()
        kw.setdefault("optional_phrases", True)
        self.g = rucene_amd.GpuIndexSearcher(self.leaves, ctx=ctx, **kw)
        assert self.g._stats_leaf == 0

    def call(self, queries, k, leaf=0, **kw):
        """the C ABI call itself on one leaf -> (hits, totals, {launch name: launches})"""
        self.ctx.kernel_stats_reset()
        packed = self.g.pack_phrase_opt([q.build() for q in queries], self.leaves[leaf])
        hits, totals = self.leaves[leaf].segment.search_phrase_opt_batch(*packed, k, **kw)
        return hits, totals, {n: v["launches"] for n, v in self.ctx.kernel_stats().items() if v["launches"]}

    def search(self, queries, k):
        """GpuIndexSearcher.search_batch -> (hits, totals, {launch name: launches})"""
        self.ctx.kernel_stats_reset()
        hits, totals = self.g.search_batch([q.build() for q in queries], k)
        return hits, totals, {n: v["launches"] for n, v in self.ctx.kernel_stats().items() if v["launches"]}

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
def main_exact(oracle, ctx_exact):
    yield from _opened(oracle, ctx_exact, [pb.main()])


@pytest.fixture(scope="module")
def groups(oracle, ctx):
    yield from _opened(oracle, ctx, [pb.groups()])


@pytest.fixture(scope="module")
def join(oracle, ctx):
    yield from _opened(oracle, ctx, [po.join()])


def _rule_index(oracle, ctx, which="A"):
    parts = [po.rule(w) for w in which]
    return _opened(oracle, ctx, [fx for fx, _ in parts], deleted=[d for _, d in parts])


@pytest.fixture(scope="module")
def rule(oracle, ctx):
    yield from _rule_index(oracle, ctx)


@pytest.fixture(scope="module")
def rule_exact(oracle, ctx_exact):
    yield from _rule_index(oracle, ctx_exact)


def _check(o, hits, totals, queries, what, exact=False):
    for i, q in enumerate(queries):
        pb.check_row(hits[i], totals[i], po.rows(o.ix, q, exact=exact), (what, q))


def _n_phrases(q, side):
    return sum(isinstance(c, pb.Ph) for c in side)


# ---- tree shapes, presence ------------------------------------------------------------------------------------------------------------
def test_every_main_query_in_one_batch_and_alone(main):
    """Every tree shape and presence case of the main fixture: as one batch, and each alone (a row does not depend on its
    neighbours). The launches that answer are the candidate conjunction under its own name, the join and the scan."""
    qs = po.MAIN_QUERIES
    hits, totals, st = main.call(qs, 16)
    print("main", st)
    assert st.get(po.CANDIDATES) == 1 and st.get(po.JOIN) == 1 and st.get(po.SCAN) == 1 and st.get(po.SCORE) == 1 and st.get(po.FANOUT) == 1, st
    assert st.get(po.SEED) == 1 and st.get("k_score_terms") == 1 and st.get("k_phrase_run_sort") == 1, st
    assert "k_search_and(phrase-bool candidates)" not in st and "k_search_and(phrase-or candidates)" not in st and "k_or_windows" not in st
    _check(main, hits, totals, qs, "batch")
    for i, q in enumerate(qs):
        h1, t1, st1 = main.call([q], 16)
        assert (h1[0] == hits[i]).all() and t1[0] == totals[i], q
        dead = q.name in ("an absent required term", "a required phrase lacking a term")
        assert (po.CANDIDATES in st1) == (po.JOIN in st1) == (po.SCAN in st1) == (not dead), (q, st1)
        assert (po.SEED in st1) == (not dead and _n_phrases(q, q.musts + q.filters) == 0), (q, st1)
        assert (po.FANOUT in st1) == (not dead and _n_phrases(q, q.musts + q.filters) > 1), (q, st1)


def test_main_queries_without_the_rule(main_exact):
    qs = po.MAIN_QUERIES
    hits, totals, st = main_exact.call(qs, 16)
    assert st.get(po.JOIN) == 1 and st.get(po.SCAN) == 1, st
    _check(main_exact, hits, totals, qs, "req_opt_rule = -1", exact=True)


def test_every_optional_clause_absent_is_the_phrase_bool_row(main):
    """With every optional clause absent there is no ReqOptScorer: the row is rgpu_search_phrase_bool_batch's for the required side."""
    import rucene_amd
    q = [x for x in po.PRESENCE if x.name == "every optional clause absent"][0]
    hits, totals, _ = main.call([q], 40)
    plain = rucene_amd.GpuIndexSearcher(main.leaves, ctx=main.ctx)
    bh, bt = plain.search_batch([q.req().build()], 40)
    assert totals[0] == bt[0] > 0 and (hits[0] == bh[0]).all()


def test_nine_optional_clauses_and_a_tenth_refused(main):
    hits, totals, st = main.call([po.NINE], 20)
    _check(main, hits, totals, [po.NINE], "nine")
    import rucene_amd
    with pytest.raises(rucene_amd.RgpuError) as e:
        main.search([po.TEN], 20)
    assert e.value.status == po.UNSUPPORTED


# ---- join edges -----------------------------------------------------------------------------------------------------------------------
def test_join_edges(join):
    """Required runs of 63 | 64 | 65 and 127 | 128 | 129 records against optional runs of 0, 1 and 63 | 64 | 65 entries; a required doc
    equal to an optional run's first and last entry; optional runs wholly before and wholly behind the required docs; a required doc
    between two neighbouring optional entries; eight runs behind one required run; phrase runs on either side."""
    qs = po.JOIN_QUERIES
    hits, totals, st = join.call(qs, 130)
    assert st.get(po.JOIN) == 1 and st.get(po.SCAN) == 2 and st.get(po.CANDIDATES) == 1, st   # (k = 130: two passes of the scan)
    _check(join, hits, totals, qs, "join")
    by = {q.name: int(t) for q, t in zip(qs, totals)}
    assert by["64 x 64"] == 64 and by["optional run of 0"] == 129 and by["wholly behind"] == 65 and by["first and last entry"] == 63
    for i, q in enumerate(qs):   # alone: every query is the batch's first, its runs start at slot 0
        h1, t1, _ = join.call([q], 130)
        assert (h1[0] == hits[i]).all() and t1[0] == totals[i], q


def test_group_edges(groups):
    """63 | 64 | 65 required candidates against an optional phrase; a required phrase whose middle 64-slot group has no survivor; a
    query whose optional run lies behind every required doc; a required lead the phrase never meets."""
    qs = po.GROUP_QUERIES
    hits, totals, st = groups.call(qs, 130)
    _check(groups, hits, totals, qs, "groups")
    assert totals.tolist()[:3] == [63, 64, 65]


# ---- arithmetic, leaves, mirrors ------------------------------------------------------------------------------------------------------
def test_three_leaves_through_the_searcher_and_the_flag_off(oracle, ctx):
    """Three leaves through GpuIndexSearcher(optional_phrases=True): doc bases, a required cost order that differs between two
    leaves beside three optional addends, a leaf without a MUST term, a leaf without a phrase term. The same trees with the flag
    off are UnsupportedOperation, as they have been."""
    import rucene_amd
    for o in _opened(oracle, ctx, pb.leaves()):
        hits, totals, st = o.search(po.LEAF_QUERIES, 24)
        assert st.get(po.CANDIDATES) == 2 and st.get(po.JOIN) == 2 and st.get(po.SCAN) == 2, st   # (the third leaf: every query dead)
        _check(o, hits, totals, po.LEAF_QUERIES, "leaves")
        assert all(int(t) > 0 for t in totals)
        # mixed with the other kinds of a batch, rows keep their places
        mixed = [po.LEAF_QUERIES[0], pb.LEAF_QUERIES[0], po.LEAF_QUERIES[2]]
        h2, t2, _ = o.search(mixed, 24)
        assert (h2[0] == hits[0]).all() and (h2[2] == hits[2]).all() and t2[0] == totals[0]
        pb.check_row(h2[1], t2[1], o.ix.rows(pb.LEAF_QUERIES[0]), "phrase-bool row in a mixed batch")
        off = rucene_amd.GpuIndexSearcher(o.leaves, ctx=ctx)
        for q in po.LEAF_QUERIES + po.SHAPES[:5]:
            with pytest.raises(rucene_amd.RgpuError) as e:
                off.search_batch([q.build()], 8)
            assert e.value.status == po.UNSUPPORTED, q
        # search(): one query through the collector, and what the call cannot express goes to cpu_fallback
        seen = []
        fb = rucene_amd.GpuIndexSearcher(o.leaves, ctx=ctx, optional_phrases=True, cpu_fallback=lambda q, c: seen.append(q))
        fb.search(po.TEN.build(), rucene_amd.TopDocsCollector(5))
        assert len(seen) == 1


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def test_rule_fixtures(rule):
    """The 100th | 101st | 102nd scored doc before a low one; a skipped doc that the optional PHRASE holds scores req alone; deleted
    and MUST_NOT docs among the first 100 leave the state alone; skipped docs do not enter the mean."""
    qs = list(po.RULE_QUERIES.values())
    hits, totals, st = rule.call(qs, 160)
    assert st.get(po.JOIN) == 1 and st.get(po.SCAN) == 2, st   # k = 160: two ceiling passes of the scan over one set of records
    _check(rule, hits, totals, qs, "rule")
    for q in qs:
        assert po.skipped_docs(rule.ix, q), q


def test_rule_fixtures_without_the_rule(rule_exact):
    qs = list(po.RULE_QUERIES.values())
    hits, totals, _ = rule_exact.call(qs, 160)
    _check(rule_exact, hits, totals, qs, "rule off", exact=True)
    on = po.rows(rule_exact.ix, qs[2])
    assert hits[2]["score"][:on[1].size].view(np.uint32).tolist() != on[1][:160].view(np.uint32).tolist()


def test_a_doc_that_doubles_to_the_mean_exactly_is_not_skipped(oracle, ctx):
    """EQUAL: 2 * req == mean in f32 at the 102nd doc - the strict `<` lets it take the optional phrase's score."""
    for o in _opened(oracle, ctx, [po.equal()]):
        q = [po.EQUAL_QUERY]
        hits, totals, _ = o.call(q, 120)
        _check(o, hits, totals, q, "equal")
        loose = po.rows(o.ix, q[0], le=True)
        assert hits[0]["score"][:loose[1].size].view(np.uint32).tolist() != loose[1][:120].view(np.uint32).tolist()


def test_second_leaf_starts_afresh(oracle, ctx):
    for o in _rule_index(oracle, ctx, "AB"):
        qs = [po.RULE_QUERIES["S101"], po.RULE_QUERIES["DEAD"]]
        hits, totals, st = o.search(qs, 300)
        _check(o, hits, totals, qs, "two leaves")
        carried = po.rows(o.ix, qs[0], carry=True)
        assert hits[0]["score"][:carried[1].size].view(np.uint32).tolist() != carried[1][:300].view(np.uint32).tolist()


# ---- cross-check with RGPU_OP_WITH_SHOULD ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["rule", "exact"])
def test_phraseless_queries_return_the_rows_of_with_should(main, main_exact, rule, rule_exact, mode):
    """A query with no phrase at all is the tree RGPU_OP_WITH_SHOULD serves: rgpu_search_batch's rows, bit for bit, in both rule modes
    (the flag-off searcher packs them as it always has)."""
    import rucene_amd
    on_main, on_rule = (main, rule) if mode == "rule" else (main_exact, rule_exact)
    for o, queries in ((on_main, po.PHRASELESS), (on_rule, [po.RULE_PHRASELESS, po.Q([po.KEEP], [po.EVERY, po.OPT60])])):
        hits, totals, st = o.call(queries, 130)
        assert po.SEED in st and "k_phrase_match_lanes" not in st, st
        _check(o, hits, totals, queries, ("phrase-less", mode), exact=mode == "exact")
        plain = rucene_amd.GpuIndexSearcher(o.leaves, ctx=o.ctx)
        wh, wt = plain.search_batch([q.build() for q in queries], 130)
        assert wt.tolist() == totals.tolist() and wh["doc"].tolist() == hits["doc"].tolist()
        assert wh["score"].view(np.uint32).tolist() == hits["score"].view(np.uint32).tolist()


# ---- the collector --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 235, 236, 237, 128, 129, 1024])
def test_k_ladder(groups, k):
    q = [x for x in po.GROUP_QUERIES if x.name == "236 hits"]
    hits, totals, st = groups.call(q, k)
    assert int(totals[0]) == 236
    assert st.get(po.SCAN) == (k + 127) // 128 and st.get(po.JOIN) == 1, st
    _check(groups, hits, totals, q, ("k", k))


def test_a_plateau_of_tied_scores_cut_by_k(rule):
    """S101's 101 HIGH docs score alike (one level, one optional score): k cuts the plateau, the lower doc ids stay."""
    q = [po.RULE_QUERIES["S101"]]
    for k in (7, 100, 101, 102):
        hits, totals, _ = rule.call(q, k)
        _check(rule, hits, totals, q, ("plateau", k))
    d, s = po.rows(rule.ix, q[0])
    assert np.unique(s[:101].view(np.uint32)).size == 1 and d[:101].tolist() == sorted(d[:101].tolist())


# ---- segment variants -----------------------------------------------------------------------------------------------------------------
def _variant(norms):
    key = "po-main-" + norms
    if key not in pr._built:
        fx = pr.Fixture(key, pb.MAIN_DOCS, pb.MAIN_TERMS, pb._main_holdings(), 21, norms=norms != "none")
        if norms == "raw":
            fx.norms[:] = np.random.default_rng(5).integers(30, 140, size=fx.max_doc).astype(np.uint8)   # 65 or more distinct bytes
            assert np.unique(fx.norms).size > 64
        pr._built[key] = fx
    return pr._built[key]


@pytest.mark.parametrize("version,norms", [(0, "rank"), (1, "raw"), (0, "raw"), (1, "none"), (0, "none")])
def test_segment_variants(oracle, ctx, version, norms):
    """Both .doc formats; rank, raw and no norms."""
    fx = pb.main() if norms == "rank" else _variant(norms)
    for o in _opened(oracle, ctx, [fx], version=version, deleted=[{pb.ELEVEN_DOC, 254}]):
        qs = po.SHAPES[:8] + po.PRESENCE[-2:] + po.PHRASELESS[:2]
        hits, totals, st = o.call(qs, 20)
        assert po.JOIN in st and po.SCAN in st, st
        _check(o, hits, totals, qs, (version, norms))
        assert not (set(hits["doc"].ravel().tolist()) & {pb.ELEVEN_DOC, 254})


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(main, oracle, ctx):
    """Every refusal returns its code and writes nothing; the sibling calls refuse what they refused."""
    import rucene_amd
    from rucene_amd import _lib
    seg, leaf = main.leaves[0].segment, main.leaves[0]
    base = main.g.pack_phrase_opt([po.SHAPES[3].build(), po.SHAPES[0].build()], leaf)
    seg.search_phrase_opt_batch(*base, 8)

    def refused(status, mutate=None, k=8, packed=None, on=None):
        qs, ps, pts, ts = [a.copy() for a in (packed or base)]
        if mutate:
            mutate(qs, ps, pts, ts)
        hits = np.full((qs.size, max(k, 1)), 7, dtype=np.int64).view(_lib.HIT_DTYPE).reshape(qs.size, -1)
        totals = np.full(qs.size, -9, dtype=np.int64)
        before = hits.copy()
        main.ctx.kernel_stats_reset()
        with pytest.raises(rucene_amd.RgpuError) as e:
            (on or seg).search_phrase_opt_batch(qs, ps, pts, ts, k, hits=hits, totals=totals)
        assert e.value.status == status, (e.value, status)
        assert (hits == before).all() and (totals == -9).all()
        return {n for n, v in main.ctx.kernel_stats().items() if v["launches"]}

    def setf(name, value, row=0):
        def go(qs, ps, pts, ts):
            qs[row][name] = value
        return go

    def slop(i):
        def go(qs, ps, pts, ts):
            ps[i]["slop"] = 1
        return go
    U, A = po.UNSUPPORTED, po.ILLEGAL_ARGUMENT
    for status, mutate in ((U, slop(0)), (U, slop(1)), (U, setf("n_opt_terms", 9)), (U, setf("n_req_phrases", 5)), (U, setf("n_opt_phrases", 5)),
                           (A, setf("n_req_terms", 0, 1)), (A, setf("n_opt_phrases", 0, 1)), (A, setf("req_phrase_slot", [3, 0, 0, 0])),
                           (A, setf("opt_phrase_slot", [2, 0, 0, 0])), (A, setf("first_phrase", 2)), (A, setf("first_term", 7, 1)), (A, setf("n_must_not", -1)),
                           (A, setf("n_req_terms", -1)), (A, setf("min_should_match", 256)), (A, setf("min_should_match", -1))):
        assert not refused(status, mutate), (status, mutate)
    assert not refused(U, k=_lib.MAX_K + 1)
    assert not refused(A, k=0)

    def bad_table(qs, ps, pts, ts):
        ts[0]["sim_table"] = 99
    assert not refused(A, bad_table)

    def bad_phrase_table(qs, ps, pts, ts):
        ps[1]["sim_table"] = -1
    assert not refused(A, bad_phrase_table)
    # more than RGPU_MAX_QUERY_TERMS distinct terms
    many = po.Q([po.AB], [po.T40], must_nots=[po.N1] * 1)
    packed = [a.copy() for a in main.g.pack_phrase_opt([many.build()], leaf)]
    ts = np.concatenate([packed[3]] + [packed[3][-1:]] * 64)
    for i in range(64):
        ts[2 + i]["state"]["doc_start_fp"] += 1000 + i    # (distinct by Term equality; refused before anything is read through them)
    packed[0][0]["n_must_not"] = 65
    assert not refused(U, packed=(packed[0], packed[1], packed[2], ts))
    # no positions attached while a phrase is named: IllegalState
    bare = _lib.Segment(ctx, leaf.doc_bytes, leaf.norms, leaf.max_doc, 0, None, 3)
    try:
        assert not refused(po.ILLEGAL_STATE, on=bare)
    finally:
        bare.close()
    # the existing calls' refusals are unchanged
    plain = rucene_amd.GpuIndexSearcher(main.leaves, ctx=ctx)
    for q in (po.SHAPES[2], po.SHAPES[0]):
        with pytest.raises(rucene_amd.RgpuError) as e:
            plain.pack_phrase_bool([q.build()], leaf)
        assert e.value.status == U
    with pytest.raises(rucene_amd.RgpuError) as e:
        plain.pack_phrase_or([po.SHAPES[0].build()], leaf)
    assert e.value.status == U


def test_a_doc_holding_a_phrase_term_more_than_1024_times_is_refused_whole(oracle, ctx):
    import rucene_amd
    X, Y, L = 0, 1, 2
    h = {d: {X: [1], Y: [2], L: [5]} for d in range(70)}
    h[40] = {X: list(range(0, 2060, 2)), Y: [2061], L: [2070]}   # X 1030 times in one doc
    fx = pr.Fixture("po-over-cap", 80, 3, h, 51)
    for o in _opened(oracle, ctx, [fx]):
        q = po.Q([L], [pb.Ph((X, Y))])
        packed = o.g.pack_phrase_opt([q.build()], o.leaves[0])
        from rucene_amd import _lib
        hits = np.full((1, 8), 7, dtype=np.int64).view(_lib.HIT_DTYPE).reshape(1, -1)
        totals = np.full(1, -9, dtype=np.int64)
        before = hits.copy()
        with pytest.raises(rucene_amd.RgpuError) as e:
            o.leaves[0].segment.search_phrase_opt_batch(*packed, 8, hits=hits, totals=totals)
        assert e.value.status == po.UNSUPPORTED and (hits == before).all() and totals[0] == -9


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------------
def test_cpp_demo_rows_equal_the_python_mirror(main, tmp_path):
    """GpuIndexSearcher::search_many (csrc/host/gpu_index_searcher.hpp, optional_phrases) with PhraseOptionalQuery rows beside a
    PhraseQuery and a TermQuery row: tests/cpp/phrase_opt_demo.cpp over the same files prints the Python mirror's rows (which are the
    reference's) for every main query, in order; with the flag off it refuses every such row; a sloppy and a ten-clause query reach the
    CPU fallback."""
    import rucene_amd
    o, fx = main, main.ix.fxs[0]
    exe = str(tmp_path / "phrase_opt_demo")
    libdir = os.path.join(ROOT, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "phrase_opt_demo.cpp"),
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
    queries = po.MAIN_QUERIES
    lines = [" ".join(["msm:%d" % q.msm] + [clause("m", c) for c in q.musts] + [clause("f", c) for c in q.filters] + [clause("s", c) for c in q.shoulds] +
                      [clause("n", t) for t in q.must_nots]) for q in queries]
    lines += ["plain p:%d,%d:0,1:1.0" % (po.PA, po.PB), "plain t:%d" % po.T129]
    (tmp_path / "queries.txt").write_text("\n".join(lines) + "\n")
    k = 16
    out = subprocess.check_output([exe, str(tmp_path), str(fx.max_doc), str(fx.doc_count), str(fx.sum_ttf), str(k)], text=True).strip().splitlines()
    assert len(out) == len(lines) + 2 and out[-2] == "off %d" % len(queries) and out[-1] == "fallback 2", out[-3:]
    mine, mine_totals, _ = o.search(queries, k)
    plain, plain_totals = o.g.search_batch([rucene_amd.PhraseQuery([po.PA, po.PB]), rucene_amd.TermQuery(po.T129)], k)
    for i, line in enumerate(out[:-2]):
        parts = line.split()
        assert parts[0] == "row" and int(parts[1]) == i
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        row, total = (mine[i], mine_totals[i]) if i < len(queries) else (plain[i - len(queries)], plain_totals[i - len(queries)])
        d, s = row["doc"][row["doc"] >= 0], row["score"][row["doc"] >= 0]
        assert int(parts[2]) == int(total), (i, line)
        assert got == list(zip(d.tolist(), np.asarray(s, dtype=np.float32).view(np.uint32).tolist())), (i, line)
        if i < len(queries):
            pb.check_row(row, total, po.rows(o.ix, queries[i]), ("python mirror", queries[i]))
