"""Doc sets as the only required clause on the GPU (`-m gpu`): rgpu_docset_head against numpy, rgpu_search_batch_required_set
against the reference tests/required_set.py composes from the oracle's parts (tests/test_required_set_cpu.py proves that it IS
the reference's ReqOptScorer search), and the Python mirror's required_sets option over four leaves.

Rows of fewer than ten present SHOULD clauses are held bit for bit; twelve clauses under oracle/parity.py's heap-order rule, as
every masked disjunction of that width is."""
import numpy as np
import pytest

import required_set as rs
import segment_spectrum as ss
from test_gpu_segment_spectrum import _gpu_leaf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


class _Case:
    """One fixture leaf on the GPU with its searcher (for pack) and the oracle over the same files"""

    def __init__(self, c, oracle, fx):
        import rucene_amd
        self.fx = fx
        self.leaf = _gpu_leaf(fx)
        self.g = rucene_amd.GpuIndexSearcher([self.leaf], ctx=c)
        self.seg = self.leaf.segment
        self.osr = oracle.Searcher([fx.oracle_segment(oracle)])
        self.oracle = oracle

    def pack(self, rows):
        """rows: tuples of SHOULD term ids, () = no optional side -> (rgpu_query[], rgpu_query_term[])"""
        import rucene_amd
        from rucene_amd import _lib as gpu
        T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
        some = [i for i, r in enumerate(rows) if r]
        qs = np.zeros(len(rows), dtype=gpu.QUERY_DTYPE)
        qs["op"] = gpu.OP_OR
        ts = np.zeros(0, dtype=gpu.QUERY_TERM_DTYPE)
        if some:
            qs[some], ts = self.g.pack([T(rows[i][0]) if len(rows[i]) == 1 else Bq([], [T(t) for t in rows[i]], 1) for i in some], self.leaf)
        return qs, ts

    def docset(self, mask):
        return self.seg.docset_from_words(ss.live_words(mask))

    def want(self, mask, row, k):
        return rs.composed(self.oracle, self.osr, [(0, mask & self.fx.alive)], row, k)

    def check(self, mask, rows, k, what, alone=()):
        """one batch on `mask` against the composed reference, row by row; the rows named in `alone` again as batches of one"""
        s = self.docset(mask)
        try:
            qs, ts = self.pack(rows)
            hits, totals = self.seg.search_batch_required_set(s, qs, ts, k)
            for i, row in enumerate(rows):
                rs.assert_row(hits[i], totals[i], self.want(mask, row, k), (what, k, row))
            for i in alone:
                q1, t1 = self.pack([rows[i]])
                h1, n1 = self.seg.search_batch_required_set(s, q1, t1, k)
                assert h1[0].tobytes() == hits[i].tobytes() and n1[0] == totals[i], (what, k, rows[i], "alone")
            return hits, totals
        finally:
            s.close()

    def close(self):
        self.seg.close()


@pytest.fixture(scope="module")
def big(ctx, oracle):
    case = _Case(ctx, oracle, rs.Big("rank", 1))
    yield case
    case.close()


@pytest.fixture(scope="module")
def big_without_seq(ctx, oracle):
    """BIG with every SEQ doc deleted: a set that holds them loses them through live AND set"""
    case = _Case(ctx, oracle, rs.Big("rank", 1, alive=~rs.seq_mask()))
    yield case
    case.close()


# ---- rgpu_docset_head -------------------------------------------------------------------------------------------------------------
def _assert_head(seg, s, m, n, what):
    docs, card = seg.docset_head(s, n)
    want = np.flatnonzero(m)
    assert card == want.size, (what, n, "cardinality", card, want.size)
    assert docs.tolist() == want[:n].tolist(), (what, n, docs.tolist()[:8], want[:8].tolist())


@pytest.mark.parametrize("n", rs.HEAD_NS)
def test_docset_head_against_numpy(ctx, big, n):
    """The empty set, doc 0, the last doc, every doc, every second doc, bits 63 | 64, the edge between two chunks with rank n - 1 | n
    on either side of it, a set in the last chunk alone, |M| = n - 1 | n | n + 1 - on a leaf of three whole chunks and a last one
    of two words. Then other n on the same set: smaller ones are prefixes, a larger one rebuilds the head."""
    import rucene_amd
    seg = big.seg
    for name, m in rs.head_sets(n).items():
        s = big.docset(m)
        before = s.nbytes
        _assert_head(seg, s, m, n, name)
        assert s.nbytes > before   # the head is counted in rgpu_docset_bytes
        for other in (0, 1, n + 1 if n < 1024 else 1000, 1024, 10):
            _assert_head(seg, s, m, other, (name, "after", n))
        s.close()
    s = big.docset(np.ones(rs.BIG_MAX_DOC, bool))
    for bad, status in ((-1, -2), (1025, -5)):
        with pytest.raises(rucene_amd.RgpuError) as e:
            seg.docset_head(s, bad)
        assert e.value.status == status
    s.close()


@pytest.mark.parametrize("gone", ["first doc", "rank n - 1", "first chunk", "the whole set"])
def test_docset_head_under_deletions(ctx, gone):
    """live AND set: the set's first doc, its doc at rank n - 1, the whole first chunk, every doc of the set deleted"""
    import rucene_amd
    fx = rs.Big("rank", 1)
    for n in (1, 65, 1024):
        spread = rs.head_sets(n)["spread"]
        alive = rs.head_deletions(spread, n)[gone]
        seg = rucene_amd.Segment(ctx, fx.seg.doc_bytes, fx.norms, fx.max_doc, live_docs=ss.live_words(alive))
        try:
            for name, m in rs.head_sets(n).items():
                s = seg.docset_from_words(ss.live_words(m))
                for ask in (n, 0, 1024, 64):
                    _assert_head(seg, s, m & alive, ask, (gone, name))
                assert s.cardinality == int(m.sum())   # the set itself keeps its deleted docs
                s.close()
        finally:
            seg.close()


def test_head_is_built_once_per_set(ctx, big):
    """Steady state: a second call on the same set launches neither k_docset_chunk_counts nor k_docset_select_head - nor does a
    smaller k; a larger k rebuilds. The fill runs once per call."""
    m = rs.placement_mask("behind")
    s = big.docset(m)
    qs, ts = big.pack([(rs.T[10],), ()])

    def launches():
        st = ctx.kernel_stats()
        return [st.get(n, {"launches": 0})["launches"] for n in ("k_docset_chunk_counts", "k_docset_head_scan", "k_docset_select_head", "k_required_set_fill")]
    ctx.kernel_stats_reset()
    first = big.seg.search_batch_required_set(s, qs, ts, 64)
    assert launches() == [1, 1, 1, 1]
    again = big.seg.search_batch_required_set(s, qs, ts, 64)
    big.seg.search_batch_required_set(s, qs, ts, 10)
    big.seg.docset_head(s, 64)
    assert launches() == [1, 1, 1, 3]
    assert first[0].tobytes() == again[0].tobytes() and first[1].tolist() == again[1].tolist()
    big.seg.search_batch_required_set(s, qs, ts, 65)
    assert launches() == [2, 2, 2, 4]
    s.close()


# ---- the search call --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", rs.PLACEMENTS + ("deleted",))
@pytest.mark.parametrize("k", rs.KS)
def test_rows_at_every_size_of_the_scored_side(big, big_without_seq, k, placement):
    """O holds 0, 1, k - 1, k, k + 1 docs - inside the first k docs of M (the fill skips them), entirely behind the head, entirely
    outside M, or deleted (the row is pure fill) - at k = 1, 10, 64, 65, 128, 129, 1024, all sizes in one batch and two of them alone"""
    case = big_without_seq if placement == "deleted" else big
    m = rs.placement_mask("inside" if placement == "deleted" else placement)
    rows = [(rs.T[n],) for n in rs.sizes_of(k)]
    hits, totals = case.check(m, rows, k, placement, alone=(0, len(rows) - 1))
    assert (totals == int((m & case.fx.alive).sum())).all()
    assert (hits["doc"][:, k - 1] >= 0).all()   # M is larger than k: every row is full
    if placement in ("outside", "deleted"):
        assert (hits["score"] == 0).all() and (hits["doc"] == hits["doc"][0]).all()


@pytest.mark.parametrize("k", [10, 129, 1024])
def test_clause_counts_absent_terms_and_the_ignored_msm_byte(big, k):
    """An absent SHOULD term alone and beside a present one, two and nine clauses bit for bit, a row without an optional side, rows
    mixed in one batch each equal to itself alone; an msm byte of 2 changes nothing"""
    m = np.random.default_rng([rs.BIG_MAX_DOC, 85]).random(rs.BIG_MAX_DOC) < 0.05
    m[rs.SEQ[:40]] = True
    absent = rs.T[0]
    rows = [(absent,), (absent, rs.R[0]), (rs.R[0], rs.R[1]), tuple(rs.R[:9]), (), (rs.T[10], rs.R[2]), (absent, absent), tuple(rs.R[3:8]) + (absent,)]
    hits, totals = big.check(m, rows, k, "clauses", alone=range(len(rows)))
    assert (hits["score"][0] == 0).all() and hits[0].tobytes() == hits[4].tobytes() == hits[6].tobytes()   # nothing scored: the head of M
    s = big.docset(m)
    qs, ts = big.pack(rows)
    qs["op"] |= 2 << 8
    h2, t2 = big.seg.search_batch_required_set(s, qs, ts, k)
    assert h2.tobytes() == hits.tobytes() and t2.tolist() == totals.tolist()
    s.close()


@pytest.mark.parametrize("k", [10, 128, 1024])
def test_twelve_clauses_under_the_heap_order_rule(big, oracle, k):
    """Ten and twelve present clauses: the reference sums them in heap order, the masked call in clause order - the scored part of
    the row under oracle/parity.py's rule against the oracle on live docs M, the fill behind it exact"""
    from oracle import parity
    m = np.random.default_rng([rs.BIG_MAX_DOC, 86]).random(rs.BIG_MAX_DOC) < 0.05
    has = rs.has_table(big.fx)
    osr_m = oracle.Searcher([oracle.Segment(big.fx.seg.doc_bytes, big.fx.norms, big.fx.max_doc, big.fx.seg.terms, live_docs=ss.live_words(m),
                                            sum_total_term_freq=big.fx.sttf)])
    rows = [tuple(rs.R[:12]), tuple(rs.R[:10])]
    s = big.docset(m)
    qs, ts = big.pack(rows)
    hits, totals = big.seg.search_batch_required_set(s, qs, ts, k)
    s.close()
    for i, row in enumerate(rows):
        o = m & has[list(row)].any(axis=0)
        n_o = min(int(o.sum()), k)
        assert int(o.sum()) > 128 and totals[i] == int(m.sum())
        d, sc, total = osr_m.search(oracle.OP_OR, list(row), k, tie_mode=oracle.TIE_CANONICAL)
        assert d.size == n_o and total == int(o.sum())
        scored_docs = np.where(np.arange(k) < n_o, hits[i]["doc"], -1)
        parity.check_heap_order_row(osr_m, oracle.OP_OR, list(row), scored_docs, hits[i]["score"], total, d, sc, d.size, total, rtol=1e-5,
                                    what="required set, %d clauses, k %d" % (len(row), k))
        np.testing.assert_allclose(hits[i]["score"][:n_o], sc, rtol=1e-5, atol=0)
        fill = np.flatnonzero(m & ~o)[:k - n_o]
        assert hits[i]["doc"][n_o:].tolist() == fill.tolist() and (hits[i]["score"][n_o:].view(np.int32) == 0).all()
    assert k != 1024 or n_o < k   # (the deepest k reaches the fill)


def test_small_sets(big):
    """|M| = 0, 1 and fewer than k: the rows end in padding, total_hits is |M|"""
    rows = [(rs.T[1],), (), (rs.R[0], rs.R[1]), (rs.T[65],)]
    for docs in ([], [int(rs.SEQ[0])], [3], [0, int(rs.SEQ[0]), int(rs.SEQ[1]), rs.CHUNK_DOCS, rs.BIG_MAX_DOC - 1], list(range(100, 109))):
        m = np.zeros(rs.BIG_MAX_DOC, bool)
        m[docs] = True
        for k in (1, 10, 129):
            hits, totals = big.check(m, rows, k, ("small", len(docs)))
            assert (totals == len(docs)).all() and ((hits["doc"] >= 0).sum(axis=1) == min(len(docs), k)).all()


@pytest.mark.parametrize("norms,version", [("rank", 0), ("raw", 1), ("raw", 0), ("none", 1)])
def test_norm_modes_and_doc_formats(ctx, oracle, norms, version):
    """RANK, RAW and no norms; the current and the legacy .doc format"""
    case = _Case(ctx, oracle, rs.Big(norms, version))
    try:
        m = rs.placement_mask("inside") | (np.random.default_rng([rs.BIG_MAX_DOC, 87]).random(rs.BIG_MAX_DOC) < 0.03)
        rows = [(rs.T[10],), (rs.R[0], rs.R[1]), tuple(rs.R[:9]), (), (rs.T[129], rs.R[4])]
        for k in (10, 129):
            case.check(m, rows, k, (norms, version))
    finally:
        case.close()


def _device_rows(nq, k):
    import torch
    return torch.full((nq, k), -3, dtype=torch.int64, device="cuda"), torch.full((nq,), -3, dtype=torch.int64, device="cuda")


def test_device_form_and_lifetime(ctx, big):
    """The enqueue-only form on a stream of the caller's returns the blocking call's rows; rgpu_docset_free right behind it waits"""
    import torch
    from rucene_amd import _lib as gpu
    m = rs.placement_mask("inside")
    rows = [(rs.T[n],) for n in (0, 9, 11)] + [(), (rs.R[0], rs.R[1])]
    qs, ts = big.pack(rows)
    for k in (10, 129):
        s = big.docset(m)
        want = big.seg.search_batch_required_set(s, qs, ts, k)
        stream = torch.cuda.Stream()
        hits, totals = _device_rows(len(rows), k)
        torch.cuda.synchronize()
        big.seg.search_batch_device_required_set(s, qs, ts, k, hits.data_ptr(), totals.data_ptr(), stream=stream.cuda_stream)
        s.close()   # returns when the search has finished reading the set and its head
        got = hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(-1, k)
        assert got.tobytes() == want[0].tobytes() and totals.cpu().numpy().tolist() == want[1].tolist()


def test_abi_refusals(ctx, big):
    import rucene_amd
    from rucene_amd import _lib as gpu
    m = rs.placement_mask("inside")
    s = big.docset(m)
    rows = [(rs.R[0], rs.R[1]), (rs.T[10],), ()]
    qs, ts = big.pack(rows)
    big.seg.search_batch_required_set(s, qs, ts, 10)

    def refused(change=None, terms=None, k=10, docset=None, seg=None):
        q2, t2 = qs.copy(), (ts if terms is None else terms).copy()
        if change:
            change(q2, t2)
        with pytest.raises(rucene_amd.RgpuError) as e:
            (seg or big.seg).search_batch_required_set(docset or s, q2, t2, k)
        return e.value.status

    def set_(row, field, value):
        def go(q, _t):
            q[row][field] = value
        return go

    def weight(i, value):
        def go(_q, t):
            t[i]["weight"] = value
        return go
    assert refused(set_(0, "n_must_not", 1)) == -5                                   # MUST_NOT clauses are folded into the set
    assert refused(set_(0, "n_must_not", gpu.not_with_demote(0, 1))) == -5           # a demote byte
    assert refused(set_(0, "op", gpu.OP_AND)) == -5 and refused(set_(0, "op", gpu.OP_DISMAX)) == -5
    assert refused(set_(1, "op", gpu.OP_TERM | (1 << 16))) == -5                     # RGPU_OP_WITH_SHOULD
    assert refused(set_(0, "op", gpu.OP_OR | gpu.OP_SHOULD_REQUIRED)) == -5 and refused(set_(0, "op", gpu.OP_OR | gpu.OP_NESTED_MUST)) == -5
    for w in (0.0, -1.0, float("nan"), float("inf")):                                # a SHOULD clause's weight is finite and > 0
        assert refused(weight(1, w)) == -5, w
    assert refused(set_(0, "op", 7)) == -2 and refused(set_(0, "n_terms", 70)) == -2 and refused(set_(0, "first_term", ts.size)) == -2
    assert refused(set_(1, "n_terms", 2)) == -2                                      # RGPU_OP_TERM has one clause
    assert refused(k=0) == -2 and refused(k=1025) == -5
    other = rucene_amd.Segment(ctx, big.fx.seg.doc_bytes, big.fx.norms, big.fx.max_doc)
    try:
        assert refused(seg=other) == -2                                              # a set of another segment
        with pytest.raises(rucene_amd.RgpuError) as e:
            other.docset_head(s, 10)
        assert e.value.status == -2
    finally:
        other.close()
    big.seg.search_batch_required_set(s, qs, ts, 10)                                   # and nothing is left behind by the refusals
    s.close()


# ---- the Python mirror --------------------------------------------------------------------------------------------------------------
def _int_values(v):
    """IntPoint::encode_dimension of many values: the sign bit flipped, big-endian"""
    return (np.asarray(v, np.int64).astype(np.uint32) ^ np.uint32(0x80000000)).astype(">u4").view(np.uint8).reshape(-1, 4)


@pytest.fixture(scope="module")
def index(oracle):
    """Four leaves: leaf 0's sets are smaller than k (the fill goes on in leaf 1), leaf 1 is BIG, leaf 2's filter is empty"""
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    fxs = ss._based([rs.Small(40, "seeded", salt=1), rs.Big("rank", 1), rs.Small(8193, "first", salt=2), rs.Small(129, "none", salt=3)])
    fallen = []
    leaves = [_gpu_leaf(fx) for fx in fxs]
    on = rucene_amd.GpuIndexSearcher(leaves, ctx=c, required_sets=True)
    off = rucene_amd.GpuIndexSearcher(leaves, ctx=c, cpu_fallback=lambda q, coll: fallen.append(q) or "cpu")
    osr = oracle.Searcher([fx.oracle_segment(oracle) for fx in fxs])
    rng = np.random.default_rng(88)
    f_masks = [np.zeros(fx.max_doc, bool) for fx in fxs]
    f_masks[0][[1, 5, 9, 20, 33, 34, 39]] = True
    f_masks[1] = rs.placement_mask("behind")
    f_masks[3][::3] = True
    x_masks = [rng.random(fx.max_doc) < 0.3 for fx in fxs]
    points = [(np.arange(fx.max_doc, dtype=np.int32), _int_values(np.arange(fx.max_doc) % 1000 - 500)) for fx in fxs]
    for g in (on, off):
        g.attach_points("n", points)
    yield {"fxs": fxs, "on": on, "off": off, "osr": osr, "fallen": fallen, "f": f_masks, "x": x_masks, "has": [rs.has_table(fx) for fx in fxs]}
    c.close()


def _shapes(g, ix):
    """name -> (query, per-leaf M without live docs, SHOULD term ids)"""
    import rucene_amd
    T, Bq, All = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.MatchAllDocsQuery
    fxs = ix["fxs"]
    F = g.filter_from_bits([ss.live_words(m) for m in ix["f"]])
    X = g.filter_from_bits([ss.live_words(m) for m in ix["x"]])
    rng_q = rucene_amd.IntPoint.new_range_query("n", -500, -401)
    in_range = [np.arange(fx.max_doc) % 1000 < 100 for fx in fxs]
    every = [np.ones(fx.max_doc, bool) for fx in fxs]
    b, c_ = rs.R[0], rs.R[1]
    t = rs.R[3]
    return {
        "b c #F": (Bq.build([], [T(b), T(c_)], filters=[F]), ix["f"], (b, c_)),
        "b #F": (Bq.build([], [T(rs.T[10])], filters=[F]), ix["f"], (rs.T[10],)),
        "nine clauses #F": (Bq.build([], [T(r) for r in rs.R[:9]], filters=[F]), ix["f"], tuple(rs.R[:9])),
        "#F": (Bq.build([], [], filters=[F]), ix["f"], ()),
        "range": (rng_q, in_range, ()),
        "+range b c": (Bq.build([rng_q], [T(b), T(c_)]), in_range, (b, c_)),
        "+range #F b": (Bq.build([rng_q], [T(b)], filters=[F]), [a & f for a, f in zip(in_range, ix["f"])], (b,)),
        "-X": (Bq.build([], [], must_nots=[X]), [~x for x in ix["x"]], ()),
        "-t": (Bq.build([], [], must_nots=[T(t)]), [~h[t] for h in ix["has"]], ()),
        "#F -t -X b": (Bq.build([], [T(b)], filters=[F], must_nots=[T(t), X]), [f & ~h[t] & ~x for f, h, x in zip(ix["f"], ix["has"], ix["x"])], (b,)),
        "+*:* b c": (Bq.build([All()], [T(b), T(c_)]), every, (b, c_)),
        "+*:* b c, msm 2": (Bq.build([All()], [T(b), T(c_)], min_should_match=2), every, (b, c_)),
        "*:*": (All(), every, ()),
    }


def _want(ix, masks, shoulds, k):
    fxs = ix["fxs"]
    return rs.composed(ix["oracle"], ix["osr"], [(fx.doc_base, m & fx.alive) for fx, m in zip(fxs, masks)], shoulds, k)


@pytest.mark.parametrize("k", [10, 129])
def test_mirror_serves_every_shape(index, oracle, k):
    """Every shape of the option through search_batch (one mixed batch, plain rows in between) and through search: leaf 0's M is
    smaller than k, so the zero-score fill continues in leaf 1; leaf 2's filter is empty; totals are summed over the leaves"""
    import rucene_amd
    T = rucene_amd.TermQuery
    ix = dict(index, oracle=oracle)
    g = ix["on"]
    shapes = _shapes(g, ix)
    names = list(shapes)
    batch = [T(rs.R[0])] + [shapes[n][0] for n in names] + [T(rs.R[1])]
    hits, totals = g.search_batch(batch, k)
    plain = g.search_batch([T(rs.R[0]), T(rs.R[1])], k)
    assert hits[0].tobytes() == plain[0][0].tobytes() and hits[-1].tobytes() == plain[0][1].tobytes()
    for i, name in enumerate(names):
        _q, masks, shoulds = shapes[name]
        want = _want(ix, masks, shoulds, k)
        rs.assert_row(hits[i + 1], totals[i + 1], want, (name, k))
        coll = rucene_amd.TopDocsCollector(k)
        g.search(shapes[name][0], coll)
        top = coll.top_docs()
        assert top.total_hits() == want[2] and [d for d, _ in top.score_docs()] == want[0].tolist(), (name, k, "search")
    d, s, total = _want(ix, ix["f"], (), 10)
    assert total == sum(int((m & fx.alive).sum()) for m, fx in zip(ix["f"], ix["fxs"])) and d[-1] >= ix["fxs"][1].doc_base > d[0]


def test_should_clauses_beside_an_excluded_set_are_searched_masked(index, oracle):
    """"b c -X" with the option on: the disjunction's docs outside X (the oracle on live docs without X), not every doc outside X"""
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    ix, g = index, index["on"]
    X = g.filter_from_bits([ss.live_words(m) for m in ix["x"]])
    b, c_ = rs.R[0], rs.R[1]
    osr = oracle.Searcher([oracle.Segment(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, doc_base=fx.doc_base, live_docs=ss.live_words(fx.alive & ~x),
                                          sum_total_term_freq=fx.sttf) for fx, x in zip(ix["fxs"], ix["x"])])
    for k in (10, 129):
        hits, totals = g.search_batch([Bq.build([], [T(b), T(c_)], must_nots=[X])], k)
        d, s, total = osr.search(oracle.OP_OR, [b, c_], k, tie_mode=oracle.TIE_CANONICAL)
        rs.assert_row(hits[0], totals[0], (d.astype(np.int64), s, total), ("b c -X", k))


def test_option_off_refuses_as_before(index):
    """Without required_sets the same queries are UnsupportedOperation (-5) in search_batch and reach cpu_fallback in search"""
    import rucene_amd
    T = rucene_amd.TermQuery
    ix = index
    g, fallen = ix["off"], ix["fallen"]
    for name, (q, _m, _s) in _shapes(g, dict(ix)).items():
        if name == "-t":   # (no doc set in it: the OR of MUST_NOT clauses only, which matches nothing, as it has)
            continue
        del fallen[:]
        assert g.search(q, rucene_amd.TopDocsCollector(10)) == "cpu" and fallen == [q], name
        with pytest.raises(rucene_amd.RgpuError) as e:
            g.search_batch([T(rs.R[0]), q], 10)
        assert e.value.status == -5, name


def test_cpp_demo_rows_equal_the_python_mirror(index, tmp_path):
    """tests/cpp/required_set_demo.cpp: rucene::MatchAllDocsQuery / FilteredQuery with GpuIndexSearcher::required_sets through
    csrc/host/gpu_index_searcher.hpp on the same four leaves - the lines it prints are the Python mirror's rows, which the tests above
    hold against the composed reference; with the option off the shapes reach its cpu_fallback."""
    import os
    import subprocess
    import rucene_amd
    from rucene_amd.searcher import FilterQuery
    T, Bq, All = rucene_amd.TermQuery, rucene_amd.BooleanQuery, rucene_amd.MatchAllDocsQuery
    ix, g = index, index["on"]
    fxs = ix["fxs"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "required_set_demo")
    libdir = os.path.join(root, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "cpp", "required_set_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    b, c_, nine = rs.R[0], rs.R[1], rs.R[2]
    args = [exe, str(tmp_path), str(len(fxs)), str(b), str(c_), str(nine)]
    for i, fx in enumerate(fxs):
        d = tmp_path / ("leaf%d" % i)
        d.mkdir()
        for name, blob in (("doc", fx.seg.doc_bytes), ("norms", fx.norms), ("terms", np.ascontiguousarray(fx.seg.terms, dtype=rucene_amd.TERM_STATE_DTYPE)),
                           ("live", np.zeros(0, np.uint64) if fx.live_docs is None else fx.live_docs),
                           ("f", ss.live_words(ix["f"][i])), ("x", ss.live_words(ix["x"][i]))):
            (d / (name + ".bin")).write_bytes(np.asarray(blob).tobytes())
        args += [str(fx.max_doc), str(fx.sttf)]
    out = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "fallback ok", lines
    F = g.filter_from_bits([ss.live_words(m) for m in ix["f"]])
    X = g.filter_from_bits([ss.live_words(m) for m in ix["x"]])
    bc = [T(b), T(c_)]
    queries = [Bq.build([], bc, filters=[F]), Bq.build([], [], filters=[F]), Bq.build([], [], must_nots=[X]), Bq.build([], bc, filters=[F], must_nots=[X]),
               All(), Bq.build([], [T(nine + i) for i in range(9)], filters=[F]), Bq.build([], bc, must_nots=[X]), FilterQuery(All(), [F]), T(b)]
    hits, totals = g.search_batch(queries, 10)
    rows = lines[:-1]
    assert len(rows) == len(queries) + 1
    for i, line in enumerate(rows):
        j = i if i < len(queries) else 0              # the last line: row 0 through search() and a collector
        parts = line.split()
        assert parts[0] == "required" and int(parts[1]) == i and int(parts[2]) == totals[j], line
        got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
        n = min(10, int(totals[j]))
        assert [x[0] for x in got] == hits[j]["doc"][:n].tolist(), line
        assert [x[1] for x in got] == hits[j]["score"][:n].view(np.uint32).tolist(), line
    assert totals[1] == sum(int((m & fx.alive).sum()) for m, fx in zip(ix["f"], fxs)) and totals[4] == sum(int(fx.alive.sum()) for fx in fxs)


def test_excluded_term_sets_are_memoised_and_bounded(index):
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    g = index["on"]
    g._not_filters.clear()
    g.ctx.kernel_stats_reset()
    q = Bq.build([], [], must_nots=[T(rs.R[4]), T(rs.R[5])])
    first = g.search_batch([q], 10)
    lists = g.ctx.kernel_stats()["k_docset_lists"]["launches"]
    again = g.search_batch([q], 10)
    assert g.ctx.kernel_stats()["k_docset_lists"]["launches"] == lists and len(g._not_filters) == 1
    assert first[0].tobytes() == again[0].tobytes()
    g.range_filter_capacity = 2
    try:
        for t in rs.R[6:10]:
            g.search_batch([Bq.build([], [], must_nots=[T(t)])], 10)
        assert len(g._not_filters) == 2
    finally:
        del g.range_filter_capacity
