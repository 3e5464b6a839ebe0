"""Parity over every packed bit width and block alignment (`-m gpu`), all bit-exact. The fixture of tests/bit_spectrum.py (proven on the
CPU by tests/test_bit_spectrum_cpu.py) puts FullBlocks on every doc width 0..27 and freq width 0..31 at all 16 byte misalignments,
on 169 (doc width, freq width) pairs and on all-equal streams with VInts of 1..3 (doc) and 1..5 (freq) bytes, in BP128 and legacy
.doc files. Decode: first touch (file -> k_prepare_blocks -> output), second touch (block store -> k_decode_terms), permuted,
after prepare_terms; advance around every block's first and last doc; search (TERM, AND, OR, MUST_NOT at k = 10 and 100) against the
oracle under the knob sets that route the work through each kernel family. A decode mismatch is reported by cell (widths, VInt
lengths, misalignment), so a failure names the shape.

The decode items also run on the WIDE segment (max_doc 2^31 - 1, no norms: doc widths 28..31, the 4-byte all-equal doc VInt) and,
with 33 000 small terms behind the spectrum lists, through a bulk first touch planned by host threads; decode_positions and two- and
three-term phrases (exact, slop 2) run over position-delta blocks of width 0 (1- and 2-byte VInt) and 1..31.

Search says nothing about freq width 1: such a block needs freqs of 0 (no writer produces them), its postings sit on byte-0 docs and
stay below every top k except the block's plant, a posting of freq 1 on an ordinary doc; decode and advance cover the shape."""
import numpy as np
import pytest

import bit_spectrum as bs
from test_gpu_norm_spectrum import _assert_row, _context, _run_term

pytestmark = pytest.mark.gpu

VERSIONS = [1, 0]
IDS = ["bp128", "legacy"]
KS = (10, 100)


@pytest.fixture(scope="module")
def fx():
    return bs.search_fixture()


_oracle_rows = {}


def _wanted(oracle, fx, version, k):
    """The oracle's rows for fx.queries(), once per (version, k)."""
    if (version, k) not in _oracle_rows:
        seg = fx.seg[version]
        osr = oracle.Searcher([oracle.Segment(seg.doc_bytes, seg.norms, bs.MAX_DOC, seg.terms, sum_total_term_freq=bs.STTF)])
        specs = fx.queries(oracle)
        ops = [oracle.OP_AND if (op == oracle.OP_TERM and neg) else op for op, _, neg in specs]
        offs = np.concatenate([[0], np.cumsum([len(p) for _, p, _ in specs])]).astype(np.int32)
        noffs = np.concatenate([[0], np.cumsum([len(n) for _, _, n in specs])]).astype(np.int32)
        tids = np.concatenate([np.asarray(p, np.int64) for _, p, _ in specs])
        nids = np.concatenate([np.asarray(n, np.int64) for _, _, n in specs] + [np.zeros(0, np.int64)])
        cd, cs, cc, ct, _, _ = osr.search_batch(ops, offs, tids, k, tie_mode=oracle.TIE_CANONICAL, threads=8, not_offsets=noffs, not_ids=nids)
        _oracle_rows[(version, k)] = [(cd[i, :int(cc[i])], cs[i, :int(cc[i])], int(ct[i])) for i in range(len(specs))]
    return _oracle_rows[(version, k)]


def _gpu_queries(oracle, specs):
    import rucene_amd
    T, Bq = rucene_amd.TermQuery, rucene_amd.BooleanQuery
    out = []
    for op, pos, neg in specs:
        nots = [T(t) for t in neg]
        if op == oracle.OP_TERM and not neg:
            out.append(T(pos[0]))
        elif op == oracle.OP_OR:
            out.append(Bq.build([], [T(t) for t in pos], must_nots=nots))
        else:
            out.append(Bq.build([T(t) for t in pos], [], must_nots=nots))
    return out


def _searcher(fx, version, ctx):
    import rucene_amd
    seg = fx.seg[version]
    leaf = rucene_amd.LeafReader(seg.doc_bytes, seg.norms, bs.MAX_DOC, seg.terms, sum_total_term_freq=bs.STTF)
    return rucene_amd.GpuIndexSearcher([leaf], ctx=ctx), leaf


def _segment(fx, version, ctx):
    import rucene_amd
    seg = fx.seg[version]
    return rucene_amd.Segment(ctx, seg.doc_bytes, seg.norms, bs.MAX_DOC)


def _assert_lists(fx, version, order, docs, freqs, what):
    """Decoded postings of the terms `order` against the built arrays; a mismatch is told by the cells of the blocks it is in."""
    cells = fx.cells[version]
    bad = []
    o = 0
    for t in order:
        d, f = fx.lists[t]
        gd, gf = docs[o:o + d.size], freqs[o:o + d.size]
        o += d.size
        wrong = np.flatnonzero((gd != d) | (gf != f))
        for blk in np.unique(wrong // 128)[:4]:
            at = int(wrong[wrong // 128 == blk][0])
            cell = cells[(cells["term"] == t) & (cells["block"] == blk)]
            shape = {n: int(cell[n][0]) for n in ("bd", "dvl", "bf", "fvl", "mis")} if cell.size else "the VInt tail"
            bad.append((int(t), int(blk), shape, "posting", at, "doc", int(gd[at]), int(d[at]), "freq", int(gf[at]), int(f[at])))
    assert o == docs.size
    assert not bad, (what, len(bad), "blocks differ; (term, block, cell, first difference: got, want)", bad[:12])


# ---- decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_decode_first_touch_second_touch_and_permuted(fx, version):
    ctx = _context()
    try:
        gseg = _segment(fx, version, ctx)
        terms = fx.seg[version].terms
        order = np.arange(len(fx.lists))
        docs, freqs = gseg.decode_terms(terms)
        assert ctx.kernel_stats()["k_prepare_blocks"]["launches"] > 0
        _assert_lists(fx, version, order, docs, freqs, "first touch (file -> k_prepare_blocks)")
        ctx.kernel_stats_reset()
        docs, freqs = gseg.decode_terms(terms)
        st = ctx.kernel_stats()
        assert st["k_decode_terms"]["launches"] > 0 and st.get("k_prepare_blocks", {"launches": 0})["launches"] == 0
        _assert_lists(fx, version, order, docs, freqs, "second touch (block store -> k_decode_terms)")
        perm = np.random.default_rng(5).permutation(len(fx.lists))
        docs, freqs = gseg.decode_terms(terms[perm])
        _assert_lists(fx, version, perm, docs, freqs, "permuted")
        # a first touch in another order and term by term: other neighbours in a prepare item, other store rows
        gseg2 = _segment(fx, version, ctx)
        docs, freqs = gseg2.decode_terms(terms[perm])
        _assert_lists(fx, version, perm, docs, freqs, "first touch, permuted")
        gseg3 = _segment(fx, version, ctx)
        for t in fx.steered[::9] + [0, 1]:
            docs, freqs = gseg3.decode_terms(terms[t])
            _assert_lists(fx, version, [t], docs, freqs, "first touch, one term")
    finally:
        ctx.close()


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_five_byte_all_equal_freq_at_every_misalignment(fx, version):
    """128 equal freqs >= 2^28: an all-equal freq stream whose VInt has five bytes (the directory header word has no field for its
    length). At all 16 misalignments, and where its fifth byte is the last byte of the span a prepare has to stage
    ((misalignment + 2 + doc stream bytes + 4) % 16 == 0) behind each kind of doc stream."""
    cells = fx.cells[version]
    fifth = cells[(cells["bf"] == 0) & (cells["fvl"] == 5)]
    assert set(fifth["mis"].tolist()) == set(range(16))
    ctx = _context()
    try:
        gseg = _segment(fx, version, ctx)
        terms = fx.seg[version].terms
        wrong = []
        for t in np.unique(fifth["term"]):
            docs, freqs = gseg.decode_terms(terms[t])
            d, f = fx.lists[t]
            assert (docs == d).all(), t
            for c in fifth[fifth["term"] == t]:
                b = int(c["block"])
                want, got = f[128 * b:128 * b + 128], freqs[128 * b:128 * b + 128]
                assert (want == want[0]).all() and want[0] >= 2 ** 28
                q = int(c["mis"]) + 2 + (16 * int(c["bd"]) if c["bd"] else int(c["dvl"]))
                if not (got == want).all():
                    wrong.append({"term": int(t), "block": b, "mis": int(c["mis"]), "bd": int(c["bd"]), "dvl": int(c["dvl"]),
                                  "fifth byte last staged": (q + 4) % 16 == 0, "got": int(got[0]), "want": int(want[0])})
        print("5-byte all-equal freq VInt:", fifth.size, "blocks,", len(wrong), "wrong; misalignments of the wrong ones:",
              sorted({w["mis"] for w in wrong}))
        assert not wrong, wrong[:16]
    finally:
        ctx.close()


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_prepare_terms_in_one_call_then_decode(fx, version):
    ctx = _context()
    try:
        terms = fx.seg[version].terms
        gseg = _segment(fx, version, ctx)
        gseg.prepare_terms(terms)
        ctx.kernel_stats_reset()
        docs, freqs = gseg.decode_terms(terms)
        assert ctx.kernel_stats().get("k_prepare_blocks", {"launches": 0})["launches"] == 0
        _assert_lists(fx, version, np.arange(len(fx.lists)), docs, freqs, "prepare_terms")
    finally:
        ctx.close()


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_bulk_first_touch_planned_by_host_threads(fx, version, monkeypatch):
    """The long and steered lists in front of 33 000 two- and three-posting terms, decoded in file order on a fresh segment: the plan
    of that first touch is made by several host threads (prepare_bulk_plans), by one thread it is not; the same postings."""
    import rucene_amd
    seg, n, fill = bs.bulk_segment(fx, version)
    want_fill_d = np.concatenate([d for d, _ in fill])
    want_fill_f = np.concatenate([f for _, f in fill])
    n_spec = int(seg.terms["doc_freq"][:n].sum())
    ctx = _context()
    try:
        for threads, bulk in (("5", 1), ("1", 0)):
            monkeypatch.setenv("RGPU_HOST_THREADS", threads)
            ctx.kernel_stats_reset()
            gseg = rucene_amd.Segment(ctx, seg.doc_bytes, None, bs.MAX_DOC)
            docs, freqs = gseg.decode_terms(seg.terms)
            assert ctx.kernel_stats().get("prepare_bulk_plans", {"launches": 0})["launches"] == bulk, threads
            _assert_lists(fx, version, np.arange(n), docs[:n_spec], freqs[:n_spec], "bulk first touch, RGPU_HOST_THREADS=" + threads)
            assert (docs[n_spec:] == want_fill_d).all() and (freqs[n_spec:] == want_fill_f).all(), threads
            gseg.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_wide_segment_decodes(version):
    """max_doc 2^31 - 1, no norms: doc widths 28..31 and the all-equal doc block of a 4-byte VInt, under packed and all-equal freqs:
    first touch, second touch, permuted, a first touch in permuted order, and after prepare_terms."""
    import rucene_amd
    w = bs.wide_fixture()
    seg = w.seg[version]
    order = np.arange(len(w.lists))
    perm = np.random.default_rng(6).permutation(len(w.lists))
    ctx = _context()
    try:
        gseg = rucene_amd.Segment(ctx, seg.doc_bytes, None, bs.WIDE_MAX_DOC)
        for what, o in (("first touch", order), ("second touch", order), ("permuted", perm)):
            docs, freqs = gseg.decode_terms(seg.terms[o])
            _assert_lists(w, version, o, docs, freqs, "WIDE " + what)
        gseg2 = rucene_amd.Segment(ctx, seg.doc_bytes, None, bs.WIDE_MAX_DOC)
        docs, freqs = gseg2.decode_terms(seg.terms[perm])
        _assert_lists(w, version, perm, docs, freqs, "WIDE first touch, permuted")
        gseg3 = rucene_amd.Segment(ctx, seg.doc_bytes, None, bs.WIDE_MAX_DOC)
        gseg3.prepare_terms(seg.terms)
        docs, freqs = gseg3.decode_terms(seg.terms)
        _assert_lists(w, version, order, docs, freqs, "WIDE prepare_terms")
        for t in range(len(w.lists)):   # advance on both sides of the wide delta
            d, f = w.lists[t]
            targets = np.unique(np.clip(np.concatenate([d[::16].astype(np.int64) - 1, d[::16], d[::16].astype(np.int64) + 1, [0, bs.WIDE_MAX_DOC - 1]]), 0, bs.WIDE_MAX_DOC - 1))
            got_d, got_f = gseg.advance(seg.terms[t], targets.astype(np.int32))
            idx = np.searchsorted(d, targets, side="left")
            ok = idx < d.size
            assert (got_d[~ok] == 0x7fffffff).all() and (got_d[ok] == d[idx[ok]]).all() and (got_f[ok] == f[idx[ok]]).all(), ("WIDE advance", t)
    finally:
        ctx.close()


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_advance_around_every_spectrum_block(fx, oracle, version):
    ctx = _context()
    try:
        gseg = _segment(fx, version, ctx)
        terms = fx.seg[version].terms
        for t in list(range(fx.n_long)) + fx.steered:
            docs, freqs = fx.lists[t]
            nb = docs.size // 128
            edge = np.concatenate([docs[0:128 * nb:128], docs[127:128 * nb:128]]).astype(np.int64)
            targets = np.unique(np.clip(np.concatenate([edge - 1, edge, edge + 1, [0, int(docs[-1]), int(docs[-1]) + 1, bs.MAX_DOC - 1]]), 0, bs.MAX_DOC - 1))
            got_d, got_f = gseg.advance(terms[t], targets.astype(np.int32))
            idx = np.searchsorted(docs, targets, side="left")
            ok = idx < docs.size
            assert (got_d[~ok] == oracle.NO_MORE_DOCS).all(), t
            bad = np.flatnonzero(ok)[(got_d[ok] != docs[idx[ok]]) | (got_f[ok] != freqs[idx[ok]])]
            if bad.size:
                cells = fx.cells[version]
                blk = int(idx[bad[0]]) // 128
                cell = cells[(cells["term"] == t) & (cells["block"] == blk)]
                raise AssertionError(("advance", t, "target", int(targets[bad[0]]), "got", int(got_d[bad[0]]), int(got_f[bad[0]]), "want",
                                      int(docs[idx[bad[0]]]), int(freqs[idx[bad[0]]]), "cell", cell))
    finally:
        ctx.close()


# ---- search -----------------------------------------------------------------------------------------------------------------------
KNOBS = {"default": dict(), "and-no-bitmaps": dict(and_bitmaps=-1), "k_or_wide": dict(or_bitmaps=-1, or_wide_window_docs=2048),
         "k_or_windows": dict(or_wide=-1), "raw-norms": dict(raw_norms=True), "small-items": dict(blocks_per_item=3, and_blocks_per_item=1)}


@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_search_rows_under_every_knob_set(fx, oracle, version, knobs):
    """TERM over every list, 2- and 3-clause AND, OR of 2..8 clauses, MUST_NOT: docs, f32 score bits and totals are the oracle's. The
    first rows of a steered or long term are its plants - the posting of the largest freq of every spectrum block (CPU-proven in
    float64) -, so a block-max word built from a wrongly decoded freq, or a wrong doc id, loses a winner."""
    specs = fx.queries(oracle)
    ctx = _context(**KNOBS[knobs])
    try:
        g, leaf = _searcher(fx, version, ctx)
        queries = _gpu_queries(oracle, specs)
        for k in KS:
            want = _wanted(oracle, fx, version, k)
            hits, totals = g.search_batch(queries, k)
            for i, spec in enumerate(specs):
                _assert_row(hits[i], totals[i], want[i], (IDS[1 - version], knobs, k, spec))
        hits, _ = g.search_batch(queries[:fx.n_steered_end], 100)
        for t in list(range(fx.n_long)) + fx.steered:
            plants = fx.info[t]["plants"]
            assert set(hits[t]["doc"][:plants.size].tolist()) == set(plants.tolist()), (knobs, t, "the plants are not the first rows")
    finally:
        ctx.close()


TERM_KNOBS = {"query": {}, "query-2-waves": {"RGPU_TERM_QUERY_WAVES": "2"}, "items": {"RGPU_TERM_KERNEL": "items"}}


@pytest.mark.parametrize("knobs", list(TERM_KNOBS))
@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_fused_term_call_per_query_and_items_kernels(fx, oracle, version, knobs):
    specs = fx.queries(oracle)
    n_terms = len(fx.lists)
    assert all(specs[t] == (oracle.OP_TERM, [t], []) for t in range(n_terms))
    ctx = _context(TERM_KNOBS[knobs])
    try:
        g, leaf = _searcher(fx, version, ctx)
        ids = list(range(n_terms))
        for k in KS:
            want = _wanted(oracle, fx, version, k)
            for fused in (True, False):
                rows, totals = _run_term(g, leaf, ids, k, fused)
                for t in ids:
                    _assert_row(rows[t], totals[t], want[t], (IDS[1 - version], knobs, k, "fused" if fused else "two calls", t))
        st = ctx.kernel_stats()
        ran = "term_query_launches" in st and st["term_query_launches"]["launches"] > 0
        assert ran == (knobs != "items"), (knobs, ran)
    finally:
        ctx.close()


# ---- positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_position_blocks_of_every_width(oracle, version):
    """decode_positions over .pos blocks of width 0 (1- and 2-byte VInt) and 1..31 and the VInt block behind them, a mismatch told
    by the block's shape; two- and three-term phrases, exact and slop 2, whose every doc is one such block: the oracle's rows."""
    import rucene_amd
    p = bs.positions_fixture()
    seg = p.seg[version]
    ctx = _context()
    try:
        leaf = rucene_amd.LeafReader.from_synthetic_positions(seg)
        leaf.doc_count, leaf.sum_total_term_freq = p.doc_count, p.sum_ttf
        g = rucene_amd.GpuIndexSearcher([leaf], ctx=ctx)
        leaf.segment.attach_positions(leaf.pos_bytes)   # (as the searcher does before a leaf's first phrase search)
        leaf._pos_attached = True
        want = p.flat_positions()
        for what in ("first touch", "second touch"):
            got = leaf.segment.decode_positions(seg.terms, leaf.term_positions)
            assert got.size == want.size
            wrong = np.flatnonzero(got != want)
            if wrong.size:
                starts = np.concatenate([[0], np.cumsum(seg.terms["total_term_freq"])])
                t = int(np.searchsorted(starts, wrong[0], side="right") - 1)
                blk = int(wrong[0] - starts[t]) // 128
                cell = p.cells[version][(p.cells[version]["term"] == t) & (p.cells[version]["block"] == blk)]
                raise AssertionError((what, "term", t, "block", blk, "cell (term, block, width, VInt length, misalignment)", cell, "got", int(got[wrong[0]]), "want", int(want[wrong[0]]), wrong.size))
        one = leaf.segment.decode_positions(seg.terms[p.THIRD], leaf.term_positions[p.THIRD])
        assert one.tolist() == [q for _, ps in p.postings[p.THIRD] for q in ps]
        ix = oracle.PositionsIndex.from_files(seg.doc_bytes, seg.pos_bytes, seg.terms, leaf.term_positions)
        queries = [rucene_amd.PhraseQuery(t, slop=sl) for t, sl in p.phrases]
        matched = 0
        for k in KS:
            hits, totals = g.search_phrase_batch(queries, k)
            for i, q in enumerate(queries):
                row = ix.phrase_search(q.terms, k, p.norms, bs.POS_MAX_DOC, p.doc_count, p.sum_ttf, slop=q.slop)
                _assert_row(hits[i], totals[i], row, (IDS[1 - version], "phrase", q.terms, q.slop, k))
                matched += row[2]
        assert matched > 500
        ix.close()
    finally:
        ctx.close()
