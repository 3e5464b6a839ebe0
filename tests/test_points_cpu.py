"""Point ranges without a GPU: the encoders against values written out by hand, the fixtures and their numpy model (tests/points.py),
the mirror's routing of PointRangeQuery clauses, the struct layouts against a C compile of the header, the host plan
(csrc/host/points_plan.hpp) under the sanitizers, and the C++ demo's build. The GPU side is tests/test_gpu_points.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import points as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- encoders -------------------------------------------------------------------------------------------------------------------
def test_encoders_against_values_written_out_by_hand():
    from rucene_amd import DoublePoint, FloatPoint, IntPoint, LongPoint
    assert [IntPoint.encode(v).hex() for v in (-2**31, -1, 0, 1, 2**31 - 1)] == ["00000000", "7fffffff", "80000000", "80000001", "ffffffff"]
    assert [LongPoint.encode(v).hex() for v in (-2**63, -1, 0, 1, 2**63 - 1)] == \
        ["0000000000000000", "7fffffffffffffff", "8000000000000000", "8000000000000001", "ffffffffffffffff"]
    inf, nan = float("inf"), float("nan")
    f32_min_positive = struct.unpack(">f", bytes.fromhex("00800000"))[0]
    # f32: -inf = ff800000 -> sortable int 0x807fffff ^ ... : bits ^ 0x7fffffff for negatives, then the sign flip of the int
    assert [FloatPoint.encode(v).hex() for v in (-inf, -1.5, -0.0, 0.0, f32_min_positive, inf, nan)] == \
        ["007fffff", "403fffff", "7fffffff", "80000000", "80800000", "ff800000", "ffc00000"]
    f64_min_positive = struct.unpack(">d", bytes.fromhex("0010000000000000"))[0]
    assert [DoublePoint.encode(v).hex() for v in (-inf, -1.5, -0.0, 0.0, f64_min_positive, inf, nan)] == \
        ["000fffffffffffff", "4007ffffffffffff", "7fffffffffffffff", "8000000000000000", "8010000000000000", "fff0000000000000", "fff8000000000000"]


def test_byte_order_is_numeric_order():
    from rucene_amd import DoublePoint, FloatPoint, IntPoint, LongPoint
    rng = np.random.default_rng(3)
    ints = sorted({-2**31, -1, 0, 1, 2**31 - 1} | {int(x) for x in rng.integers(-2**31, 2**31, 200)})
    assert [IntPoint.encode(v) for v in ints] == sorted(IntPoint.encode(v) for v in ints)
    longs = sorted({-2**63, -1, 0, 1, 2**63 - 1} | {int(x) for x in rng.integers(-2**63, 2**63 - 1, 200)})
    assert [LongPoint.encode(v) for v in longs] == sorted(LongPoint.encode(v) for v in longs)
    floats = [float("-inf"), -3.4e38, -1.5, -1e-40, -0.0, 0.0, 1e-45, 1.17549435e-38, 1.5, 3.4e38, float("inf")]
    for P in (FloatPoint, DoublePoint):
        enc = [P.encode(v) for v in floats]
        assert enc == sorted(enc) and len(set(enc)) == len(enc)        # strictly ascending: -0.0 before +0.0
        drawn = sorted(float(np.float32(x)) for x in rng.normal(0, 1e3, 200))
        assert [P.encode(v) for v in drawn] == sorted(P.encode(v) for v in drawn)
        assert P.encode(float("nan")) > P.encode(float("inf"))          # the NaN of Rust's f32::NAN / f64::NAN sorts last
    assert len(IntPoint.encode(0)) == len(FloatPoint.encode(0.0)) == 4 and len(LongPoint.encode(0)) == len(DoublePoint.encode(0.0)) == 8
    q = IntPoint.new_range_query("price", -5, 7)
    assert (q.field, q.lower, q.upper, q.extract_terms()) == ("price", IntPoint.encode(-5), IntPoint.encode(7), [])
    e = LongPoint.new_exact_query("date", 9)
    assert e.lower == e.upper == LongPoint.encode(9)


# ---- fixtures and model -----------------------------------------------------------------------------------------------------------
def test_the_model_and_the_fixtures():
    """The model on a field small enough to write out; every shape holds what its name promises."""
    docs = np.array([2, 0, 2, 4], np.int32)
    values = np.array([[0, 0, 0, 9], [0x80, 0, 0, 0], [0x7f, 0xff, 0xff, 0xff], [0xff, 0xff, 0xff, 0xff]], np.uint8)
    assert pt.model_mask(5, docs, values, b"\x00\x00\x00\x09", b"\x00\x00\x00\x09").tolist() == [False, False, True, False, False]
    assert pt.model_mask(5, docs, values, b"\x7f\xff\xff\xff", b"\x80\x00\x00\x00").tolist() == [True, False, True, False, False]
    assert pt.model_mask(5, docs, values, b"\x00\x00\x00\x0a", b"\x7f\xff\xff\xfe").sum() == 0          # inside a gap
    assert pt.model_mask(5, docs, values, b"\x80\x00\x00\x00", b"\x00\x00\x00\x00").sum() == 0          # lower > upper
    assert pt.model_mask(5, docs, values, b"\x00" * 4, b"\xff" * 4).tolist() == [True, False, True, False, True]
    assert pt.model_words(65, np.array([64], np.int32), values[:1], b"\x00" * 4, b"\xff" * 4).tolist() == [0, 1]
    for width in pt.WIDTHS:
        for max_doc in pt.SIZES:
            d, v = pt.field(max_doc, width, "dense")
            assert sorted(d.tolist()) == list(range(max_doc)) and v.shape == (max_doc, width)
            d, v = pt.field(max_doc, width, "sparse")
            assert {0, max_doc - 1} <= set(d.tolist()) and np.unique(d).size == d.size and (max_doc < 4 or d.size < max_doc)
            d, v = pt.field(max_doc, width, "multi")
            counts = np.bincount(d, minlength=max_doc)
            assert d.size > max_doc or max_doc > 400
            if max_doc >= 129:
                assert {2, 64, 65, 200} <= {int(c) - (1 if doc % 7 == 0 else 0) - (2 if doc in (max_doc // 2, max_doc // 5) else 0) for doc, c in enumerate(counts) if c}
            lo, hi = pt.inout_range(width)
            rows = [r for dd, r in zip(d.tolist(), pt.value_rows(v)) if dd == max_doc // 2]
            assert any(lo <= r <= hi for r in rows) and any(r > hi for r in rows)                           # one inside, one outside
            assert sum(1 for dd, r in zip(d.tolist(), pt.value_rows(v)) if dd == max_doc // 5 and r == pt.plateau_value(width)) >= 2
        for plateau in pt.PLATEAUS:
            d, v = pt.field(8193, width, "dense", plateau)
            assert sum(1 for r in pt.value_rows(v) if r == pt.plateau_value(width)) == plateau
            names = [n for n, _, _ in pt.ranges_for(v, width)]
            for need in ("lower > upper", "plateau as lower bound", "plateau as upper bound", "[min, max]", "inside a gap", "across the sign flip"):
                assert need in names
            rows = pt.value_rows(v)
            assert pt.type_min(width) in rows and pt.type_max(width) in rows                               # the type's minimum and maximum
            for name, lo, hi in pt.ranges_for(v, width):
                n = pt.model_mask(8193, d, rows, lo, hi).sum()
                if name in ("lower > upper", "inside a gap", "just above the plateau"):
                    assert n == 0, name
                if name in ("plateau value alone",):
                    assert n == plateau
                if name in ("plateau as lower bound", "plateau as upper bound"):
                    assert n >= plateau
                if name in ("[min, max]", "the whole type"):
                    assert n == 8193
        assert pt.field(64, width, "none")[0].size == 0 and pt.field(64, width, "one")[0].tolist() == [63]
        # the inner variants hold neither end of the type, so both outside ranges exist on fields of real sizes and match nothing
        for shape, plain in zip(pt.INNER_SHAPES, pt.SHAPES):
            for max_doc in (129, 8193):
                d, v = pt.field(max_doc, width, shape)
                d0, _ = pt.field(max_doc, width, plain)
                rows = pt.value_rows(v)
                assert sorted(d.tolist()) == sorted(d0.tolist()) and pt.type_min(width) not in rows and pt.type_max(width) not in rows
                by_name = {n: (lo, hi) for n, lo, hi in pt.ranges_for(v, width)}
                for need in ("below the minimum", "above the maximum"):
                    assert need in by_name and pt.model_mask(max_doc, d, rows, *by_name[need]).sum() == 0, (shape, need)
                assert pt.model_mask(max_doc, d, rows, *by_name["[min, max]"]).sum() == np.unique(d).size
                assert pt.model_mask(max_doc, d, rows, pt.type_min(width), min(rows)).sum() >= 1                # the bound itself is inside


# ---- the mirror's routing ---------------------------------------------------------------------------------------------------------
class _FakeSets:
    cardinality = 0


def _searcher_without_a_gpu():
    """A GpuIndexSearcher whose range filters are made without a device: enough for build / _peel decisions"""
    import rucene_amd
    from rucene_amd.searcher import CachedFilter, GpuIndexSearcher
    g = GpuIndexSearcher.__new__(GpuIndexSearcher)
    g.leaves, g._masks, g._range_filters = [object()], {}, {}
    g._points = {"price": (4, [None]), "date": (8, [None])}
    made = []

    def fake(queries, path=0):
        out = []
        for q in queries:
            if q.field not in g._points:
                raise rucene_amd.RgpuError(-5, "no points")
            if len(q.lower) != g._points[q.field][0]:
                raise rucene_amd.RgpuError(-2, "width")
            key = (q.field, q.lower, q.upper)
            if key not in g._range_filters:
                g._range_filters[key] = CachedFilter(g, [_FakeSets()])
                made.append(key)
            out.append(g._range_filters[key])
        return out
    return g, fake, made


def test_mirror_routing_rules():
    import rucene_amd
    from rucene_amd import BooleanQuery as Bq, IntPoint, LongPoint, PhraseQuery, TermQuery as T
    from rucene_amd.searcher import FilterQuery, GpuIndexSearcher
    g, fake, made = _searcher_without_a_gpu()
    real = GpuIndexSearcher._range_filters_for
    r1, r2 = IntPoint.new_range_query("price", 10, 20), LongPoint.new_range_query("date", -5, 5)
    # the length check and the unknown field are the real method's (they come before any device work)
    with pytest.raises(rucene_amd.RgpuError) as e:
        real(g, [rucene_amd.PointRangeQuery("price", b"\x00" * 8, b"\xff" * 8)])
    assert e.value.status == -2
    with pytest.raises(rucene_amd.RgpuError) as e:
        real(g, [IntPoint.new_range_query("nowhere", 1, 2)])
    assert e.value.status == -5
    with pytest.raises(rucene_amd.RgpuError) as e:                               # two dimensions of 4 bytes: the CPU path
        real(g, [rucene_amd.PointRangeQuery("price", b"\x00" * 8, b"\xff" * 8, num_dims=2)])
    assert e.value.status == -5
    with pytest.raises(rucene_amd.RgpuError) as e:
        rucene_amd.PointRangeQuery("price", b"\x00" * 7, b"\xff" * 7, num_dims=2)
    assert e.value.status == -2
    with pytest.raises(rucene_amd.RgpuError) as e:
        rucene_amd.PointRangeQuery("price", b"\x00" * 4, b"\xff" * 8)
    assert e.value.status == -2
    g._range_filters_for = fake
    # +a +range: the range is a filter, the rest is the term
    rest, (f, x) = g._peel(Bq.build([T(1), r1], []))
    assert isinstance(rest, T) and rest.term == 1 and f == [g._range_filters[("price", r1.lower, r1.upper)]] and x == []
    # +a #range -range2
    rest, (f, x) = g._peel(Bq.build([T(1)], [], filters=[r1], must_nots=[r2]))
    assert isinstance(rest, T) and rest.term == 1 and len(f) == 1 and len(x) == 1 and f[0] is not x[0]
    assert x == [g._range_filters[("date", r2.lower, r2.upper)]] and len(made) == 2
    # the memo: the same bounds again make nothing new, under MUST or FILTER
    rest, (f2, _) = g._peel(Bq.build([T(1), T(2)], [T(3)], filters=[IntPoint.new_range_query("price", 10, 20)]))
    assert f2 == f and len(made) == 2 and isinstance(rest, Bq) and [c.term for c in rest.must_queries] == [1, 2] and len(rest.should_queries) == 1
    # +range #a b: the range was the only MUST clause; what is left keeps the query's min_should_match (0: b stays optional),
    # where build() alone would give "#a b" the default 1 of a query without MUST clauses
    q = Bq.build([r1], [T(3)], filters=[T(2)])
    assert q.min_should_match == 0
    rest, (f3, x3) = g._peel(q)
    assert isinstance(rest, Bq) and rest.min_should_match == 0 and rest.must_queries == [] and [c.term for c in rest.filter_queries] == [2]
    assert [c.term for c in rest.should_queries] == [3] and f3 == f and x3 == []
    assert Bq.build([], [T(3)], filters=[T(2)]).min_should_match == 1                       # (the spelling without a MUST clause)
    rest, _ = g._peel(Bq.build([r1, r2], [T(3), T(4)], filters=[T(2)], min_should_match=2))   # an explicit one is kept as well
    assert rest.min_should_match == 2
    # FilterQuery(b c, [range filter]) as with any CachedFilter
    cf = fake([r1])[0]
    inner = Bq.build([], [T(2), T(3)])
    rest, (f, x) = g._peel(FilterQuery(inner, [cf]))
    assert rest is inner and f == [cf] and x == []
    # a query without such clauses takes the path it takes today
    plain = Bq.build([T(1), T(2)], [T(3)], must_nots=[T(4)])
    t1 = T(1)
    assert g._peel(plain) == (plain, ([], [])) and g._peel(t1) == (t1, ([], []))
    # the unchanged refusals
    refused = [Bq.build([r1], [T(2), T(3)]),                                     # +range b c
               r1, Bq.build([r1], []), Bq.build([], [], filters=[r1]),           # a lone range, however it is spelt
               Bq.build([T(1)], [T(2), T(3)], must_nots=[r2], min_should_match=2),  # -range beside min_should_match 2
               Bq.build([PhraseQuery([1, 2])], [], filters=[r1]),                 # beside a phrase
               Bq.build([T(1), r1], [PhraseQuery([1, 2])]),
               FilterQuery(PhraseQuery([1, 2]), [cf])]
    fresh = [IntPoint.new_range_query("price", 100 + i, 200 + i) for i in range(3)]       # ranges no earlier query has built
    refused += [Bq.build([fresh[0]], [T(2), T(3)]), Bq.build([PhraseQuery([1, 2])], [], filters=[fresh[1]]),
                Bq.build([T(1)], [T(2), T(3)], must_nots=[fresh[2]], min_should_match=2)]
    n_made = len(made)
    for q in refused:
        for build_sets in (True, False):
            with pytest.raises(rucene_amd.RgpuError) as e:
                g._peel(q, build_sets)
            assert e.value.status == -5, str(q)
    assert len(made) == n_made                                                   # a refused shape builds no set
    rest, (fq, _) = g._peel(Bq.build([T(1), fresh[0]], []), build=False)         # the dry pass of search_batch: checked, nothing built
    assert rest.term == 1 and fq == [fresh[0]] and len(made) == n_made
    with pytest.raises(rucene_amd.RgpuError) as e:                               # a range under SHOULD
        Bq.build([T(1)], [T(2), r1])
    assert e.value.status == -5
    with pytest.raises(rucene_amd.RgpuError) as e:
        Bq.build([], [r1, r2])
    assert e.value.status == -5
    with pytest.raises(rucene_amd.RgpuError) as e:                               # packing a range as a clause is never tried
        GpuIndexSearcher._flatten(g, Bq.build([T(1), r1], []))
    assert e.value.status == -5
    # a wrong width among a query's clauses: IllegalArgument from the real check, before anything is built
    g._range_filters_for = lambda qs, path=0: real(g, qs, path)
    with pytest.raises(rucene_amd.RgpuError) as e:
        g._peel(Bq.build([T(1)], [], filters=[LongPoint.new_range_query("price", 1, 2)]))
    assert e.value.status == -2


# ---- header, exports, layouts -----------------------------------------------------------------------------------------------------
def test_header_exports_and_struct_layouts(tmp_path):
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from rucene_amd import _lib
    L = C.CDLL(_lib.lib_path())
    for name in ("rgpu_points_attach", "rgpu_points_get_info", "rgpu_points_free", "rgpu_docset_from_point_ranges"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert _lib.lib().rgpu_abi_version() == 6 and C.sizeof(_lib._Config) == 68
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "rucene_gpu.h"), "int main(void) {"]
    structs = {"rgpu_points_info": _lib.POINTS_INFO_DTYPE, "rgpu_point_range": _lib.POINT_RANGE_DTYPE}
    for name, dt in structs.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (name, name))
        lines += ['  printf(" %s=%%zu", offsetof(%s, %s));' % (f, name, f) for f in dt.names]
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-o", exe, str(src)])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    for line, (name, dt) in zip(out, structs.items()):
        parts = line.split()
        assert parts[0] == name and int(parts[1]) == dt.itemsize, line
        assert parts[2:] == ["%s=%d" % (f, dt.fields[f][1]) for f in dt.names], line
    # argument errors need no device
    G = _lib.lib()
    out_h = C.c_void_p(1)
    assert G.rgpu_points_attach(None, 4, None, None, 0, C.byref(out_h)) == -2
    assert G.rgpu_points_get_info(None, None) == -2
    assert G.rgpu_docset_from_point_ranges(None, None, 1, 0, None) == -2
    G.rgpu_points_free(None)
    r = _lib.point_ranges([(b"\x00\x00\x00\x01", b"\x00\x00\x00\x02")], 4)
    assert r[0]["lower"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and r[0]["upper"].tolist() == [0, 0, 0, 2, 0, 0, 0, 0]
    with pytest.raises(_lib.RgpuError) as e:
        _lib.point_ranges([(b"\x00" * 4, b"\x00" * 8)], 4)
    assert e.value.status == -2


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/points_plan_test.cpp: keys, the two sort orders, dense detection, bounds on plateaus of equal keys, the nothing /
    every-doc / scatter / scan decisions and the passes of 16 of csrc/host/points_plan.hpp, as a stand-alone program built with
    -fsanitize=address,undefined."""
    exe = str(tmp_path / "points_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "points_plan_test.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("points_plan_test OK"), out.stdout


def test_cpp_mirror_demo_compiles_without_a_gpu(tmp_path):
    """tests/cpp/points_demo.cpp (PointRangeQuery / attach_points / range_filter of csrc/host/gpu_index_searcher.hpp) links against the
    C ABI on a CPU-only box, warnings as errors; running it needs a GPU (tests/test_gpu_points.py)."""
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "rucene_amd")
    exe = str(tmp_path / "points_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "points_demo.cpp"),
                           "-L" + libdir, "-lrucene_gpu", "-lrucene_indexgen", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
