// The host plan of the point-range entry points (rgpu_points_attach, rgpu_docset_from_point_ranges): the decisions that can be wrong
// without a GPU, in plain C++17 with no device dependency (tests/cpp/points_plan_test.cpp runs it under the sanitizers).
//   * keys: the sortable bytes of a one-dimensional point (IntPoint / LongPoint / FloatPoint / DoublePoint::encode_dimension) loaded
//     big-endian into an unsigned integer — an unsigned compare is then the reference's byte compare (point_range_query.rs:626-640);
//   * attach: the points of one field of one segment in two orders — by (doc, key) for the scan, by (key, doc) for the scatter; the
//     sorted keys stay on the host, so a range's slice [i0, i1) of the value order is two binary searches and i1 - i0 is the exact
//     number of matching points before anything is launched. A field is DENSE when it has exactly one point per doc of the segment:
//     then point i of the doc order belongs to doc i and the doc ids need not be stored;
//   * per range of a call: nothing to launch (no point inside), every doc (a dense field's whole value span is covered: the
//     reference's all_docs_match, point_range_query.rs:531-549), the value-ordered scatter (one atomic per matching point) or the
//     doc-ordered scan (one pass over the column, shared by up to 16 ranges);
//   * the scan's passes of 16 ranges.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../../include/rucene_gpu.h"

namespace rgpu_host {

constexpr int POINTS_RANGES_PER_PASS = 16;  // == POINTS_SCAN_RANGES of kernels/points.hpp

// What one scattered point costs, in column bytes of the scan: the doc-ordered scan streams this many bytes of the column in the time
// the value-ordered scatter sets one matching point (its atomic into the set). Under path = 0 a range is scanned when its matches,
// at this price, cost at least one pass over the column: matches * 200 >= n_points * (bytes per key + 4 bytes per doc id unless dense).
// Measured on a 10 M-doc leaf where the medians of the two forced paths meet (point ranges): a dense 4-byte field at
// 1.9 % of its points (4 / 200 = 2 %), a sparse 8-byte field at 5.9 % (12 / 200 = 6 %).
constexpr int64_t POINTS_SCAN_BYTES_PER_SCATTERED_POINT = 200;

inline uint64_t points_key(const uint8_t* bytes, int bytes_per_dim) {
  uint64_t k = 0;
  for (int i = 0; i < bytes_per_dim; ++i) k = (k << 8) | bytes[i];
  return k;
}
inline void points_key_bytes(uint64_t key, int bytes_per_dim, uint8_t* out) {
  for (int i = bytes_per_dim - 1; i >= 0; --i) { out[i] = (uint8_t)(key & 0xff); key >>= 8; }
}

struct PointsColumns {
  int32_t max_doc = 0, bytes_per_dim = 0;
  int64_t n_points = 0, doc_count = 0;   // doc_count: distinct docs holding a point
  bool dense = false;
  std::vector<uint64_t> keys_by_doc;     // order (doc, key)
  std::vector<int32_t> docs_by_doc;      // ascending, not strictly (kept on the host also when dense)
  std::vector<uint64_t> keys_sorted;     // order (key, doc): stays on the host
  std::vector<int32_t> docs_by_value;
  uint64_t min_key = 0, max_key = 0;     // of a field with points
};

// RGPU_OK, or RGPU_ERR_ILLEGAL_ARGUMENT (bytes_per_dim other than 4 / 8, a doc outside [0, max_doc), a negative count): `out` is then unspecified
inline int32_t points_build(int32_t max_doc, int32_t bytes_per_dim, const int32_t* docs, const uint8_t* values, int64_t n_points, PointsColumns& out) {
  if ((bytes_per_dim != 4 && bytes_per_dim != 8) || n_points < 0 || max_doc < 0 || (n_points > 0 && (!docs || !values))) return RGPU_ERR_ILLEGAL_ARGUMENT;
  for (int64_t i = 0; i < n_points; ++i) if (docs[i] < 0 || docs[i] >= max_doc) return RGPU_ERR_ILLEGAL_ARGUMENT;
  const size_t n = (size_t)n_points;
  std::vector<uint64_t> keys(n);
  for (size_t i = 0; i < n; ++i) keys[i] = points_key(values + i * (size_t)bytes_per_dim, bytes_per_dim);
  std::vector<int64_t> order(n);
  std::iota(order.begin(), order.end(), (int64_t)0);
  out = PointsColumns();
  out.max_doc = max_doc;
  out.bytes_per_dim = bytes_per_dim;
  out.n_points = n_points;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return docs[a] != docs[b] ? docs[a] < docs[b] : keys[(size_t)a] < keys[(size_t)b]; });
  out.keys_by_doc.resize(n);
  out.docs_by_doc.resize(n);
  for (size_t i = 0; i < n; ++i) { out.keys_by_doc[i] = keys[(size_t)order[i]]; out.docs_by_doc[i] = docs[order[i]]; }
  for (size_t i = 0; i < n; ++i) if (i == 0 || out.docs_by_doc[i] != out.docs_by_doc[i - 1]) ++out.doc_count;
  out.dense = n_points == (int64_t)max_doc && out.doc_count == n_points;   // (then docs_by_doc[i] == i)
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return keys[(size_t)a] != keys[(size_t)b] ? keys[(size_t)a] < keys[(size_t)b] : docs[a] < docs[b]; });
  out.keys_sorted.resize(n);
  out.docs_by_value.resize(n);
  for (size_t i = 0; i < n; ++i) { out.keys_sorted[i] = keys[(size_t)order[i]]; out.docs_by_value[i] = docs[order[i]]; }
  if (n > 0) { out.min_key = out.keys_sorted.front(); out.max_key = out.keys_sorted.back(); }
  return RGPU_OK;
}

// the bytes one pass of the scan reads: the keys, and the doc ids unless the field is dense
inline int64_t points_scan_bytes(const PointsColumns& C) { return C.n_points * (C.bytes_per_dim + (C.dense ? 0 : 4)); }

enum PointsAnswer : int32_t {
  POINTS_NOTHING = 0,   // no point inside (lower > upper included): the empty set, no launch
  POINTS_EVERY_DOC = 1, // a dense field's [min, max] is covered: every doc of the segment
  POINTS_SCATTER = 2,   // k_docset_from_docs over docs_by_value[i0, i1)
  POINTS_SCAN = 3,      // k_points_scan over the doc order
};
struct PointsRangePlan {
  uint64_t lower = 0, upper = 0;
  int64_t i0 = 0, i1 = 0;   // the range's slice of the value order: i1 - i0 points match
  PointsAnswer answer = POINTS_NOTHING;
};

// [i0, i1) of keys_sorted with lower <= key <= upper (both ends inclusive: a plateau of equal keys on a bound is inside)
inline void points_bounds(const std::vector<uint64_t>& keys_sorted, uint64_t lower, uint64_t upper, int64_t& i0, int64_t& i1) {
  if (lower > upper) { i0 = i1 = 0; return; }
  i0 = std::lower_bound(keys_sorted.begin(), keys_sorted.end(), lower) - keys_sorted.begin();
  i1 = std::upper_bound(keys_sorted.begin(), keys_sorted.end(), upper) - keys_sorted.begin();
}

// path: 0 = chosen per range — the scatter below the crossover (POINTS_SCAN_BYTES_PER_SCATTERED_POINT), the scan at or above it (a call with two or more ranges at or above
// it scans them together: that is the same rule, the pass is shared); 1 = always the scatter; 2 = always the scan. A range without a
// matching point launches nothing under every path; the every-doc form is taken under path 0 only (a forced path runs its kernel).
inline std::vector<PointsRangePlan> plan_point_ranges(const PointsColumns& C, const rgpu_point_range* ranges, int32_t n_ranges, int32_t path) {
  std::vector<PointsRangePlan> plans((size_t)std::max(n_ranges, 0));
  const int64_t column_bytes = points_scan_bytes(C);
  for (int32_t r = 0; r < n_ranges; ++r) {
    PointsRangePlan& P = plans[(size_t)r];
    P.lower = points_key(ranges[r].lower, C.bytes_per_dim);
    P.upper = points_key(ranges[r].upper, C.bytes_per_dim);
    points_bounds(C.keys_sorted, P.lower, P.upper, P.i0, P.i1);
    const int64_t m = P.i1 - P.i0;
    if (m == 0) P.answer = POINTS_NOTHING;
    else if (path == 1) P.answer = POINTS_SCATTER;
    else if (path == 2) P.answer = POINTS_SCAN;
    else if (C.dense && P.lower <= C.min_key && P.upper >= C.max_key) P.answer = POINTS_EVERY_DOC;
    else P.answer = m * POINTS_SCAN_BYTES_PER_SCATTERED_POINT >= column_bytes ? POINTS_SCAN : POINTS_SCATTER;
  }
  return plans;
}

// the ranges the scan answers, in caller order, in passes of POINTS_RANGES_PER_PASS (one launch each)
inline std::vector<std::vector<int32_t>> points_scan_passes(const std::vector<PointsRangePlan>& plans) {
  std::vector<std::vector<int32_t>> passes;
  for (size_t r = 0; r < plans.size(); ++r) {
    if (plans[r].answer != POINTS_SCAN) continue;
    if (passes.empty() || (int)passes.back().size() == POINTS_RANGES_PER_PASS) passes.emplace_back();
    passes.back().push_back((int32_t)r);
  }
  return passes;
}

// keys of the doc order a scan launch may load: whole chunks of 64 lanes x 16 bytes. A dense field's column also covers the docs up
// to the end of the last u64 word of a set (the kernel writes every word), zero-filled.
inline int64_t points_padded_count(int64_t n_points, int32_t max_doc, int32_t bytes_per_dim, bool dense) {
  const int64_t chunk = 64 * (16 / bytes_per_dim);
  const int64_t cover = dense ? (((int64_t)max_doc + 63) / 64) * 64 : n_points;
  return std::max<int64_t>(chunk, (cover + chunk - 1) / chunk * chunk);
}

}  // namespace rgpu_host
