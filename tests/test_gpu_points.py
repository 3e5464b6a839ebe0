"""Point ranges on the GPU through the C ABI (`-m gpu`): rgpu_points_attach / rgpu_docset_from_point_ranges against the numpy model
of tests/points.py - every segment size, field shape, key width and kind of range under the forced scatter (path 1), the forced scan
(path 2) and the library's own choice (path 0), with byte-identical words; the launches behind path 0 from rgpu_kernel_stats; batches
of 1, 16 and 17 ranges; the refusals; and end to end through GpuIndexSearcher and the raw masked call, bit for bit against
rgpu_search_batch on a twin segment uploaded with live AND set(model) - the method of tests/test_gpu_docset.py."""
import os
import subprocess

import numpy as np
import pytest

import points as pt
import segment_spectrum as ss
from test_gpu_segment_spectrum import _gpu_leaf

pytestmark = pytest.mark.gpu

PATHS = (1, 2, 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import rucene_amd
    c = rucene_amd.Context(profile_kernels=True)
    yield c
    c.close()


def _segment(c, fx, live_docs=None):
    import rucene_amd
    return rucene_amd.Segment(c, fx.seg.doc_bytes, fx.norms, fx.max_doc, live_docs=live_docs)


def _launches(c, *names):
    st = c.kernel_stats()
    return [st[n]["launches"] if n in st else 0 for n in names]


def _check_sets(sets, max_doc, docs, rows, ranges, what):
    assert len(sets) == len(ranges)
    for s, (name, lo, hi) in zip(sets, ranges):
        want = pt.model_mask(max_doc, docs, rows, lo, hi)
        got = s.words()
        assert got.size == (max_doc + 63) // 64
        bits = np.unpackbits(got.view(np.uint8), bitorder="little")
        assert (got == ss.live_words(want)).all(), (what, name, "docs differing", np.flatnonzero(bits[:max_doc] != want)[:10], "bits past max_doc", int(bits[max_doc:].sum()))
        assert s.cardinality == int(bits.sum()) == int(want.sum()), (what, name)
        s.close()


def _sweep(c, seg, max_doc, width, shape, plateau=1):
    docs, values = pt.field(max_doc, width, shape, plateau)
    rows = pt.value_rows(values)
    pts = seg.attach_points(width, docs, values)
    info = pts.info()
    assert info["n_points"] == docs.size and info["doc_count"] == np.unique(docs).size and info["bytes_per_dim"] == width
    assert info["dense"] == int(docs.size == max_doc and np.unique(docs).size == max_doc), (shape, info)
    assert info["hbm_bytes"] >= docs.size * (width + 4)
    if rows:
        assert info["min_value"] == min(rows) and info["max_value"] == max(rows)
    ranges = pt.ranges_for(values, width)
    for path in PATHS:
        _check_sets(pts.range_docsets([(lo, hi) for _, lo, hi in ranges], path), max_doc, docs, rows, ranges, (max_doc, width, shape, plateau, "path", path))
    pts.close()


@pytest.mark.parametrize("width", pt.WIDTHS)
@pytest.mark.parametrize("max_doc", pt.SIZES)
def test_every_shape_size_and_range_under_every_path(ctx, max_doc, width):
    """dense, sparse, multi-valued, no point and one point at every segment size: the sets of every kind of range equal the model
    under the forced scatter, the forced scan and the library's choice; no bit at or past max_doc; the cardinality is the popcount."""
    seg = _segment(ctx, ss.Leaf(max_doc, "rank", "none"))
    try:
        for shape in pt.SHAPES + pt.INNER_SHAPES + ("none", "one"):   # (-inner: the ranges below the minimum / above the maximum exist)
            _sweep(ctx, seg, max_doc, width, shape)
    finally:
        seg.close()


@pytest.mark.parametrize("width", pt.WIDTHS)
@pytest.mark.parametrize("plateau", pt.PLATEAUS)
def test_plateaus_of_equal_keys_on_a_bound(ctx, plateau, width):
    """1, 64, 65 and 1000 equal keys sitting exactly on the lower and on the upper bound (tests/points.py ranges_for)"""
    seg = _segment(ctx, ss.Leaf(8193, "rank", "none"))
    try:
        for shape in ("dense", "sparse", "multi"):
            _sweep(ctx, seg, 8193, width, shape, plateau)
    finally:
        seg.close()


@pytest.mark.parametrize("width", pt.WIDTHS)
def test_points_on_deleted_docs_are_in_the_set(ctx, width):
    fx = ss.Leaf(8193, "rank", "seeded")
    seg = _segment(ctx, fx, live_docs=fx.live_docs)
    try:
        assert int(fx.alive.sum()) < fx.max_doc
        for shape in ("dense", "multi"):
            _sweep(ctx, seg, fx.max_doc, width, shape)
    finally:
        seg.close()


def test_the_launch_behind_the_library_s_choice(ctx):
    """path 0: a scatter for a narrow range, the scan for a wide one, no launch for an empty one, the every-doc form for a covering
    range on a dense field - and the scan, not the every-doc form, for [min, max] on a sparse field."""
    max_doc = 8193
    seg = _segment(ctx, ss.Leaf(max_doc, "rank", "none"))
    try:
        for width in pt.WIDTHS:
            for shape in ("dense", "sparse"):
                docs, values = pt.field(max_doc, width, shape)
                rows = pt.value_rows(values)
                srt = sorted(rows)
                pts = seg.attach_points(width, docs, values)
                cases = {"narrow": (srt[10], srt[10]), "wide": (srt[len(srt) // 4], srt[-1]),
                         "empty": (pt.be(5, width), pt.be(4, width)), "covering": (srt[0], srt[-1]), "whole type": (pt.type_min(width), pt.type_max(width))}
                for name, (lo, hi) in cases.items():
                    ctx.kernel_stats_reset()
                    (s,) = pts.range_docsets([(lo, hi)], 0)
                    scatter, scan, combine = _launches(ctx, "k_docset_from_docs", "k_points_scan", "k_docset_combine")
                    want = pt.model_mask(max_doc, docs, rows, lo, hi)
                    assert (s.words() == ss.live_words(want)).all() and s.cardinality == int(want.sum()), (width, shape, name)
                    assert combine == 1, (width, shape, name)
                    if name == "narrow":
                        assert (scatter, scan) == (1, 0) and 0 < want.sum() <= 4, (width, shape, name)
                    elif name == "empty":
                        assert (scatter, scan) == (0, 0) and want.sum() == 0
                    elif name == "wide" or shape == "sparse":
                        assert (scatter, scan) == (0, 1), (width, shape, name)
                        assert want.sum() < max_doc or shape == "dense"
                    else:   # covering a dense field: every doc, neither kernel
                        assert (scatter, scan) == (0, 0) and want.all(), (width, shape, name)
                    s.close()
                pts.close()
    finally:
        seg.close()


@pytest.mark.parametrize("width", pt.WIDTHS)
def test_batches_of_1_16_and_17_ranges(ctx, width):
    max_doc = 8193
    seg = _segment(ctx, ss.Leaf(max_doc, "rank", "none"))
    try:
        for shape in ("dense", "multi"):
            docs, values = pt.field(max_doc, width, shape)
            rows = pt.value_rows(values)
            srt = sorted(set(rows))
            pts = seg.attach_points(width, docs, values)
            # a mix: narrow, wide, empty and covering ranges, every one with a name of its own
            kinds = [("narrow %d" % i, srt[(i * 37) % (len(srt) - 3)], srt[(i * 37) % (len(srt) - 3) + 2]) for i in range(6)] + \
                    [("wide %d" % i, srt[len(srt) // (i + 3)], srt[-1 - i]) for i in range(6)] + \
                    [("empty", pt.be(9, width), pt.be(8, width)), ("covering", srt[0], srt[-1]), ("whole type", pt.type_min(width), pt.type_max(width)),
                     ("gap", pt.be(int.from_bytes(pt.plateau_value(width), "big") + 1, width), pt.be(int.from_bytes(pt.plateau_value(width), "big") + 7, width)),
                     ("one value", srt[7], srt[7])]
            assert len(kinds) == 17
            for n in (1, 16, 17):
                mix = [kinds[(3 * i) % 17] for i in range(n)]
                for path in PATHS:
                    _check_sets(pts.range_docsets([(lo, hi) for _, lo, hi in mix], path), max_doc, docs, rows, mix, (width, shape, n, "path", path))
                # n ranges with a match each under the forced scan: one launch per 16
                full = [k for k in kinds if not k[0].startswith(("empty", "gap"))]
                full = (full * 2)[:n]
                ctx.kernel_stats_reset()
                sets = pts.range_docsets([(lo, hi) for _, lo, hi in full], 2)
                assert _launches(ctx, "k_points_scan", "k_docset_from_docs") == [2 if n == 17 else 1, 0], (width, shape, n)
                _check_sets(sets, max_doc, docs, rows, full, (width, shape, n, "forced scan"))
                ctx.kernel_stats_reset()
                sets = pts.range_docsets([(lo, hi) for _, lo, hi in full], 1)
                assert _launches(ctx, "k_points_scan", "k_docset_from_docs") == [0, n], (width, shape, n)
                _check_sets(sets, max_doc, docs, rows, full, (width, shape, n, "forced scatter"))
            pts.close()
    finally:
        seg.close()


def test_refusals(ctx):
    import ctypes as C
    import rucene_amd
    from rucene_amd import _lib as gpu
    fx = ss.Leaf(129, "rank", "none")
    seg, other = _segment(ctx, fx), _segment(ctx, ss.Leaf(129, "rank", "none", salt=1))
    try:
        docs, values = pt.field(129, 4, "dense")
        for width in (0, 1, 3, 5, 16, -4):
            with pytest.raises(rucene_amd.RgpuError) as e:
                seg.attach_points(width, docs[:2], np.zeros(2 * max(width, 0), np.uint8))
            assert e.value.status == -2, width
        for bad in ([0, 129], [-1], [2**31 - 1]):
            with pytest.raises(rucene_amd.RgpuError) as e:
                seg.attach_points(4, np.array(bad, np.int32), np.zeros((len(bad), 4), np.uint8))
            assert e.value.status == -2, bad
        L = gpu.lib()
        h = C.c_void_p(0)
        d = np.array([129], np.int32)
        assert L.rgpu_points_attach(seg._h, 4, d.ctypes.data, np.zeros(4, np.uint8).ctypes.data, 1, C.byref(h)) == -2 and not h.value   # no handle is returned
        assert L.rgpu_points_attach(None, 4, None, None, 0, C.byref(h)) == -2 and not h.value
        pts = seg.attach_points(4, docs, values)
        r = gpu.point_ranges([(pt.type_min(4), pt.type_max(4))], 4)
        out = (C.c_void_p * 2)()
        assert L.rgpu_docset_from_point_ranges(None, r.ctypes.data, 1, 0, out) == -2
        for n, path in ((0, 0), (-1, 0), (1, 3), (1, -1)):
            out[0] = 7
            assert L.rgpu_docset_from_point_ranges(pts._h, r.ctypes.data, n, path, out) == -2, (n, path)
        assert L.rgpu_docset_from_point_ranges(pts._h, None, 1, 0, out) == -2 and L.rgpu_docset_from_point_ranges(pts._h, r.ctypes.data, 1, 0, None) == -2
        with pytest.raises(rucene_amd.RgpuError) as e:                      # bounds of another width
            pts.range_docsets([(pt.type_min(8), pt.type_max(8))])
        assert e.value.status == -2
        # the points of one segment make sets of that segment: another segment's masked search refuses them
        (s,) = pts.range_docsets([(pt.type_min(4), pt.type_max(4))])
        assert s.cardinality == 129
        g = rucene_amd.GpuIndexSearcher([_gpu_leaf(fx)], ctx=ctx)
        qs, ts = g.pack([rucene_amd.TermQuery(ss.EVERY)], g.leaves[0])
        with pytest.raises(rucene_amd.RgpuError) as e:
            other.search_batch_masked(s, qs, ts, 10)
        assert e.value.status == -2
        hits, totals = seg.search_batch_masked(s, qs, ts, 10)
        assert totals[0] == 129
        g.leaves[0].segment.close()
        assert "doc_bitmap_bytes" in seg.footprint() and not any("point" in k for k in seg.footprint())   # outside the footprint: rgpu_points_info.hbm_bytes
    finally:
        seg.close()
        other.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _twin_leaf(fx, mask):
    import rucene_amd
    return rucene_amd.LeafReader(fx.seg.doc_bytes, fx.norms, fx.max_doc, fx.seg.terms, doc_base=fx.doc_base, live_docs=ss.live_words(fx.alive & mask),
                                 sum_total_term_freq=fx.sttf)


def _same(a, b, what):
    assert a[0]["doc"].tolist() == b[0]["doc"].tolist(), (what, "docs")
    assert a[0]["score"].view(np.int32).tolist() == b[0]["score"].view(np.int32).tolist(), (what, "score bits")
    assert np.asarray(a[1]).tolist() == np.asarray(b[1]).tolist(), (what, "totals")


def _range_cases(fxs, fields):
    """[(name, query with range clauses, the query without them, mask per leaf)] over leaves that hold `fields` (None: not in the leaf)"""
    import rucene_amd
    from rucene_amd import BooleanQuery as Bq, TermQuery as T
    p8, p4 = [f and f["date"] for f in fields], [f and f["price"] for f in fields]
    first = next(f for f in fields if f)
    v4, v8 = sorted(pt.value_rows(first["price"][2])), sorted(pt.value_rows(first["date"][2]))
    r1 = rucene_amd.PointRangeQuery("price", v4[len(v4) // 5], v4[(4 * len(v4)) // 5])          # wide, IntPoint-sized
    r2 = rucene_amd.PointRangeQuery("date", v8[len(v8) // 2], v8[len(v8) // 2 + 40])            # narrow, LongPoint-sized
    r3 = rucene_amd.PointRangeQuery("date", pt.type_min(8), v8[len(v8) // 3])

    def mask(r, held):
        return [np.zeros(fx.max_doc, bool) if h is None else pt.model_mask(fx.max_doc, h[1], pt.value_rows(h[2]), r.lower, r.upper) for fx, h in zip(fxs, held)]
    m1, m2, m3 = mask(r1, p4), mask(r2, p8), mask(r3, p8)
    both = Bq.build([T(ss.EVERY), T(ss.EVEN)], [])
    return r1, r2, r3, [
        ("+a +range", Bq.build([T(ss.EVERY), r1], []), T(ss.EVERY), m1),
        ("+a +range (narrow)", Bq.build([r2, T(ss.CONST)], []), T(ss.CONST), m2),
        ("+a +b #range -range2", Bq.build([T(ss.EVERY), T(ss.EVEN)], [], filters=[r1], must_nots=[r2]), both, [a & ~b for a, b in zip(m1, m2)]),
        ("+a b c #range", Bq.build([T(ss.EVERY)], [T(ss.LAST), T(ss.FIFTH)], filters=[r3]), Bq.build([T(ss.EVERY)], [T(ss.LAST), T(ss.FIFTH)]), m3),
        ("+a -range", Bq.build([T(ss.EVEN)], [], must_nots=[r1]), T(ss.EVEN), [~a for a in m1]),
        ("+a +range +range3", Bq.build([T(ss.EVERY), r1, r3], []), T(ss.EVERY), [a & b for a, b in zip(m1, m3)]),
        # the range as the ONLY MUST clause beside a FILTER term and a SHOULD term: min_should_match stays 0, b stays optional.
        # The rest is written here as the required zero-boost clause a FILTER term is, not as _peel forms it
        ("+range #a b", Bq.build([r1], [T(ss.FIFTH)], filters=[T(ss.EVEN)]), Bq.build([T(ss.EVEN, 0.0)], [T(ss.FIFTH)]), m1)]


def test_end_to_end_on_one_leaf(ctx):
    import rucene_amd
    from rucene_amd import BooleanQuery as Bq, TermQuery as T
    from rucene_amd.searcher import FilterQuery
    fx = ss.Leaf(3001, "rank", "seeded", salt=31)
    fields = pt.leaf_points(fx)
    g = rucene_amd.GpuIndexSearcher([_gpu_leaf(fx)], ctx=ctx)
    twins = []
    try:
        for name, (width, docs, values) in fields.items():
            g.attach_points(name, [(docs, values)])
        r1, r2, r3, cases = _range_cases([fx], [fields])
        f1 = g.range_filter(r1)
        assert f1 is g.range_filter(rucene_amd.PointRangeQuery("price", r1.lower, r1.upper)) and f1.cardinality() == int(cases[0][3][0].sum())
        or3 = Bq.build([], [T(ss.FIRST), T(ss.LAST), T(ss.SOMETIMES)])
        dismax = rucene_amd.DisjunctionMaxQuery([T(ss.EVEN), T(ss.FIFTH), T(ss.LAST)], 0.3)
        boosting = rucene_amd.BoostingQuery.build(T(ss.EVERY), T(ss.EVEN), 0.5)
        m1, m3 = cases[0][3], cases[3][3]
        cases += [("FilterQuery(a b c, [range])", FilterQuery(or3, [f1]), or3, m1),
                  ("dismax under a range", FilterQuery(dismax, [g.range_filter(r3)]), dismax, m3),
                  ("boosting under a range", FilterQuery(boosting, [f1]), boosting, m1)]
        for k in (10, 129):
            hits, totals = g.search_batch([c[1] for c in cases], k)
            for i, (name, _q, rest, mask) in enumerate(cases):
                twin = rucene_amd.GpuIndexSearcher([_twin_leaf(fx, mask[0])], ctx=ctx)
                twins.append(twin)
                want = twin.search_batch([rest], k)
                _same((hits[i:i + 1], totals[i:i + 1]), want, (name, k))
                assert totals[i] > 0, name
                if name == "+range #a b":   # every doc of a inside the range, with or without b (numpy, not the twin)
                    assert totals[i] == int((fx.has[ss.EVEN] & mask[0] & fx.alive).sum()) > int((fx.has[ss.EVEN] & fx.has[ss.FIFTH] & mask[0] & fx.alive).sum())
                # the raw masked call with the set the C ABI built
                _peeled, (f, x) = g._peel(_q)
                _key, sets = g._mask(f, x)
                qs, ts = g.pack([rest], g.leaves[0])
                _same(g.leaves[0].segment.search_batch_masked(sets[0], qs, ts, k), twin.leaves[0].segment.search_batch(qs, ts, k), (name, k, "raw"))
        # deleted docs are in the set, and the masked search dropped them above
        assert f1.cardinality() > int((cases[0][3][0] & fx.alive).sum())
    finally:
        for t in twins:
            t.leaves[0].segment.close()
        g.leaves[0].segment.close()


def test_three_leaves_the_middle_one_without_the_field_and_the_memo(ctx):
    import rucene_amd
    fxs = ss._based([ss.Leaf(1025, "rank", "seeded", salt=32), ss.Leaf(3001, "rank", "first", salt=32), ss.Leaf(129, "rank", "none", salt=32)])
    fields = [pt.leaf_points(fxs[0]), None, pt.leaf_points(fxs[2], salt=1)]
    fallen = []
    g = rucene_amd.GpuIndexSearcher([_gpu_leaf(fx) for fx in fxs], ctx=ctx, cpu_fallback=lambda q, coll: fallen.append(q) or "cpu")
    twins = []
    try:
        for name in ("price", "date"):
            g.attach_points(name, [None if f is None else (f[name][1], f[name][2]) for f in fields])
        r1, r2, r3, cases = _range_cases(fxs, fields)
        queries = [c[1] for c in cases]
        ctx.kernel_stats_reset()
        for k in (10, 129):
            hits, totals = g.search_batch(queries, k)
            for i, (name, _q, rest, mask) in enumerate(cases):
                twin = rucene_amd.GpuIndexSearcher([_twin_leaf(fx, m) for fx, m in zip(fxs, mask)], ctx=ctx)
                twins.append(twin)
                _same((hits[i:i + 1], totals[i:i + 1]), twin.search_batch([rest], k), (name, k))
                in_middle = (hits[i]["doc"] >= fxs[1].doc_base) & (hits[i]["doc"] < fxs[2].doc_base)
                if name == "+a -range":   # nothing is excluded under MUST_NOT in the leaf without the field
                    assert totals[i] >= int((fxs[1].has[ss.EVEN] & fxs[1].alive).sum()) > 0
                else:                      # and nothing matches there under MUST / FILTER
                    assert not in_middle.any(), name
        names = ("k_points_scan", "k_docset_from_docs", "k_docset_combine")
        before = _launches(ctx, *names)
        assert before[0] + before[1] > 0 and len(g._range_filters) == 3
        g.search_batch(queries, 10)                                        # the memo: the same ranges build no new set
        assert _launches(ctx, *names) == before
        # a refused row builds nothing, wherever it stands in the batch: the whole batch is checked first
        new_range = rucene_amd.IntPoint.new_range_query("price", -7, 7)
        with pytest.raises(rucene_amd.RgpuError) as e:
            g.search_batch([rucene_amd.BooleanQuery.build([rucene_amd.TermQuery(ss.EVERY), new_range], []), r1], 10)
        assert e.value.status == -5 and _launches(ctx, *names) == before and len(g._range_filters) == 3
        # the memo is bounded: with room for one range, the next batch keeps the most recently used one and builds the others anew
        g.range_filter_capacity = 1
        hits1, totals1 = g.search_batch(queries, 10)
        assert len(g._range_filters) == 3 and _launches(ctx, *names) != before
        g.drop_range_filters()
        assert not g._range_filters and not g._masks
        hits2, totals2 = g.search_batch(queries, 10)
        _same((hits1, totals1), (hits2, totals2), "after the memo was emptied")
        g.range_filter_capacity = 256
        # shapes that are not served reach the CPU path
        from rucene_amd import BooleanQuery as Bq, TermQuery as T
        for q in (r1, Bq.build([r1], [T(ss.EVERY), T(ss.LAST)]), Bq.build([T(ss.EVERY)], [], filters=[rucene_amd.IntPoint.new_range_query("weight", 1, 2)])):
            del fallen[:]
            assert g.search(q, rucene_amd.TopDocsCollector(10)) == "cpu" and fallen == [q]
    finally:
        for t in twins:
            for leaf in t.leaves:
                leaf.segment.close()
        for leaf in g.leaves:
            leaf.segment.close()


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------
def test_cpp_demo_rows_equal_the_python_mirror(ctx, tmp_path):
    """tests/cpp/points_demo.cpp: rucene::PointRangeQuery through attach_points / range_filter / search of
    csrc/host/gpu_index_searcher.hpp on one leaf - the lines it prints are the Python mirror's rows (held against the twin above)."""
    import rucene_amd
    from rucene_amd import BooleanQuery as Bq, TermQuery as T
    fx = ss.Leaf(3001, "rank", "seeded", salt=31)
    fields = pt.leaf_points(fx)
    exe = str(tmp_path / "points_demo")
    libdir = os.path.join(ROOT, "rucene_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "points_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    for name, blob in (("doc", fx.seg.doc_bytes), ("norms", fx.norms), ("terms", np.ascontiguousarray(fx.seg.terms, dtype=rucene_amd.TERM_STATE_DTYPE)),
                       ("live", fx.live_docs), ("price_docs", fields["price"][1]), ("price_values", fields["price"][2]),
                       ("date_docs", fields["date"][1]), ("date_values", fields["date"][2])):
        (tmp_path / (name + ".bin")).write_bytes(np.ascontiguousarray(blob).tobytes())
    r1, r2, r3, cases = _range_cases([fx], [fields])
    bounds = "".join(b.hex() for b in (r1.lower, r1.upper, r2.lower, r2.upper, r3.lower, r3.upper))
    out = subprocess.run([exe, str(tmp_path), str(fx.max_doc), str(fx.sttf), bounds], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.strip().splitlines()
    assert lines[0].split() == ["cardinality", str(int(cases[0][3][0].sum())), str(int(cases[1][3][0].sum())), str(int(cases[3][3][0].sum()))], lines[0]
    assert lines[-1] == "fallback ok", lines
    g = rucene_amd.GpuIndexSearcher([_gpu_leaf(fx)], ctx=ctx)
    try:
        for name, (width, docs, values) in fields.items():
            g.attach_points(name, [(docs, values)])
        hits, totals = g.search_batch([c[1] for c in cases], 10)
        rows = lines[1:-1]
        assert len(rows) == len(cases)
        for i, line in enumerate(rows):
            parts = line.split()
            assert parts[0] == "points" and int(parts[1]) == i and int(parts[2]) == totals[i], line
            got = [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in parts[3:]]
            n = min(10, int(totals[i]))
            assert [x[0] for x in got] == hits[i]["doc"][:n].tolist(), line
            assert [x[1] for x in got] == hits[i]["score"][:n].view(np.uint32).tolist(), line
    finally:
        g.leaves[0].segment.close()
