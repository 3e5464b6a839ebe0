"""Fixtures for point ranges - numeric range filters built as doc sets (plain Python, no GPU).

The reference is model_mask(): for every point `lower <= value <= upper` on the RAW bytes (Python's bytes comparison is the unsigned
lexicographic one of point_range_query.rs:626-640), OR-ed into a bool array over the leaf's docs; model_words() packs it as
FixedBitSet words. It knows nothing of keys, sorting, density or paths.

A field is (docs int32[n], values uint8[n, width]) in SHUFFLED order, as an IntersectVisitor may see it. Shapes:
  dense     one point per doc
  sparse    every third doc, plus the first and the last doc
  multi     docs holding 2, 64, 65 and 200 points (one doc's run crosses lane, wavefront and workgroup edges of the doc-ordered scan),
            a doc with one point inside and one outside RANGE_INOUT, a doc holding one value twice, every seventh doc one point
  none/one  n_points 0 and 1
  *-inner   the three shapes above without the type's minimum and maximum among their values: only then do the ranges "below the
            minimum" and "above the maximum" exist (ranges_for), and they run on fields of real sizes
Values are drawn from a pool that holds the type's minimum and maximum, both sides of the sign flip (0x7f ff.. / 0x80 00..), a
plateau value PLATEAU repeated `plateau` times, and seeded values that leave gaps."""
import numpy as np

import segment_spectrum as ss

SIZES = (1, 63, 64, 65, 127, 128, 129, 8193)   # word, wavefront and last-word edges of a set
WIDTHS = (4, 8)
SHAPES = ("dense", "sparse", "multi")
INNER_SHAPES = ("dense-inner", "sparse-inner", "multi-inner")   # no value within 16 of either end of the type
PLATEAUS = (1, 64, 65, 1000)


def be(value, width):
    return int(value).to_bytes(width, "big")


def type_min(width):
    return b"\x00" * width


def type_max(width):
    return b"\xff" * width


def plateau_value(width):
    return be(0x80 << (8 * (width - 1)) | 0x1234, width)     # just above the sign flip


def inout_range(width):
    """RANGE_INOUT: the multi field's split doc holds one point inside and one just above it"""
    return be(0x40 << (8 * (width - 1)), width), be((0x40 << (8 * (width - 1))) + 10, width)


def _pool(rng, width, n, plateau, extremes=True):
    """n values (bytes rows): the specials once each as far as n goes, `plateau` copies of the plateau value, seeded values else;
    extremes=False: nothing within 16 of the type's minimum or maximum"""
    top = 1 << (8 * width)
    specials = [0, top - 1, (top >> 1) - 1, top >> 1, (top >> 1) + 1, 1] if extremes else [(top >> 1) - 1, top >> 1, (top >> 1) + 1, 16, top - 17]
    vals = [int.from_bytes(plateau_value(width), "big")] * min(plateau, n)
    vals += specials[:max(0, n - len(vals))]
    # seeded values on a coarse grid (gaps between neighbours), over the whole type and densely around the sign flip
    while len(vals) < n:
        if rng.random() < 0.5:
            vals.append(int(rng.integers(0, 1 << 20)) * (top >> 20))
        else:
            vals.append((top >> 1) + (int(rng.integers(0, 4001)) - 2000) * 16)
    vals = [v % top for v in vals]
    if not extremes:
        vals = [min(max(v, 16), top - 17) for v in vals]
    order = rng.permutation(n)
    return np.frombuffer(b"".join(be(vals[i], width) for i in order), np.uint8).reshape(n, width).copy()


def field(max_doc, width, shape, plateau=1):
    """-> (docs int32[n], values uint8[n, width]) in shuffled order"""
    extremes = not shape.endswith("-inner")
    shape = shape[:-len("-inner")] if not extremes else shape
    rng = np.random.default_rng([max_doc, width, SHAPES.index(shape) if shape in SHAPES else 9, plateau, 71 if extremes else 72])
    if shape == "none":
        return np.zeros(0, np.int32), np.zeros((0, width), np.uint8)
    if shape == "one":
        return np.array([max_doc - 1], np.int32), np.frombuffer(plateau_value(width), np.uint8).reshape(1, width).copy()
    if shape == "dense":
        docs = np.arange(max_doc, dtype=np.int32)
        values = _pool(rng, width, max_doc, plateau, extremes)
    elif shape == "sparse":
        docs = np.unique(np.concatenate([np.arange(0, max_doc, 3), [0, max_doc - 1]])).astype(np.int32)
        values = _pool(rng, width, docs.size, plateau, extremes)
    else:
        assert shape == "multi"
        at = [0, max_doc // 3, (2 * max_doc) // 3, max_doc - 1]
        docs = np.concatenate([np.full(n, d) for d, n in zip(at, (2, 64, 65, 200))] + [np.arange(0, max_doc, 7)]).astype(np.int32)
        values = _pool(rng, width, docs.size, plateau, extremes)
        lo, hi = inout_range(width)
        split, twice = max_doc // 2, max_doc // 5
        extra_docs = np.array([split, split, twice, twice], np.int32)
        above = be(int.from_bytes(hi, "big") + 1, width)
        extra = np.frombuffer(lo + above + plateau_value(width) * 2, np.uint8).reshape(4, width)
        docs, values = np.concatenate([docs, extra_docs]), np.concatenate([values, extra])
    order = rng.permutation(docs.size)
    return docs[order].copy(), values[order].copy()


def value_rows(values):
    return [bytes(r) for r in np.asarray(values, np.uint8)]


def model_mask(max_doc, docs, values, lower, upper):
    rows = values if isinstance(values, list) else value_rows(values)
    lower, upper = bytes(lower), bytes(upper)
    inside = np.fromiter((lower <= v <= upper for v in rows), bool, count=len(rows))
    m = np.zeros(max_doc, bool)
    m[np.asarray(docs)[inside]] = True
    return m


def model_words(max_doc, docs, values, lower, upper):
    return ss.live_words(model_mask(max_doc, docs, values, lower, upper))


def ranges_for(values, width):
    """[(name, lower, upper)] over a field's values: every kind of range the issue names"""
    rows = sorted(set(value_rows(values)))
    out = [("lower > upper", be(5, width), be(4, width)), ("the whole type", type_min(width), type_max(width)),
           ("plateau value alone", plateau_value(width), plateau_value(width)),
           ("plateau as lower bound", plateau_value(width), be(int.from_bytes(plateau_value(width), "big") + 5000, width)),
           ("plateau as upper bound", be(int.from_bytes(plateau_value(width), "big") - 5000, width), plateau_value(width)),
           ("just above the plateau", be(int.from_bytes(plateau_value(width), "big") + 1, width), be(int.from_bytes(plateau_value(width), "big") + 7, width)),
           ("across the sign flip", be((0x80 << (8 * (width - 1))) - 1, width), be(0x80 << (8 * (width - 1)), width)),
           ("the negative half", type_min(width), be((0x80 << (8 * (width - 1))) - 1, width)),
           ("in / out", ) + inout_range(width)]
    if rows:
        lo, hi = rows[0], rows[-1]
        out += [("[min, max]", lo, hi), ("min alone", lo, lo), ("max alone", hi, hi)]
        if lo != type_min(width):
            out.append(("below the minimum", type_min(width), be(int.from_bytes(lo, "big") - 1, width)))
        if hi != type_max(width):
            out.append(("above the maximum", be(int.from_bytes(hi, "big") + 1, width), type_max(width)))
        for a, b in zip(rows, rows[1:]):
            if int.from_bytes(b, "big") - int.from_bytes(a, "big") >= 3:
                out.append(("inside a gap", be(int.from_bytes(a, "big") + 1, width), be(int.from_bytes(b, "big") - 1, width)))
                break
        mid = rows[len(rows) // 2]
        out += [("lower half", lo, mid), ("upper half", mid, hi), ("a few values", rows[len(rows) // 3], rows[min(len(rows) - 1, len(rows) // 3 + 3)])]
    return out


# ---- the end-to-end leaf: ss.Leaf's postings with a dense 4-byte "price" and a sparse 8-byte "date" beside them ----------------------
def leaf_points(fx, salt=0):
    """{field: (width, docs, values)} for a segment_spectrum leaf: "price" dense IntPoint-like, "date" multi-valued LongPoint-like"""
    d4, v4 = field(fx.max_doc, 4, "dense", plateau=1 + salt)
    d8, v8 = field(fx.max_doc, 8, "multi", plateau=1 + salt)
    return {"price": (4, d4, v4), "date": (8, d8, v8)}
