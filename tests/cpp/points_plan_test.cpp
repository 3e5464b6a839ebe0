// csrc/host/points_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_points_cpu.py): the keys,
// the two sort orders of an attach, dense detection, a range's bounds on plateaus of equal keys, the nothing / every-doc / scatter /
// scan decisions under the three paths, and the grouping of the scanned ranges into passes of 16.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rucene_amd/csrc/host/points_plan.hpp"

using namespace rgpu_host;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static std::vector<uint8_t> bytes_of(const std::vector<uint64_t>& keys, int width) {
  std::vector<uint8_t> out(keys.size() * (size_t)width);
  for (size_t i = 0; i < keys.size(); ++i) points_key_bytes(keys[i], width, out.data() + i * (size_t)width);
  return out;
}
static rgpu_point_range range(uint64_t lo, uint64_t hi, int width) {
  rgpu_point_range r;
  std::memset(&r, 0xee, sizeof r);   // the bytes behind bytes_per_dim are not read
  points_key_bytes(lo, width, r.lower);
  points_key_bytes(hi, width, r.upper);
  return r;
}

static void test_keys() {
  const uint8_t b4[4] = {0x80, 0x00, 0x01, 0xff};
  CHECK(points_key(b4, 4) == 0x800001ffull);
  const uint8_t b8[8] = {0xff, 0, 0, 0, 0, 0, 0, 0x01};
  CHECK(points_key(b8, 8) == 0xff00000000000001ull);
  uint8_t back[8];
  points_key_bytes(0xff00000000000001ull, 8, back);
  CHECK(std::memcmp(back, b8, 8) == 0);
  points_key_bytes(0x800001ffull, 4, back);
  CHECK(std::memcmp(back, b4, 4) == 0);
  // byte order is key order: 0x00ff.. < 0x0100..
  const uint8_t lo[4] = {0x00, 0xff, 0xff, 0xff}, hi[4] = {0x01, 0x00, 0x00, 0x00};
  CHECK(points_key(lo, 4) < points_key(hi, 4));
}

static void test_build_orders_and_density() {
  for (int width : {4, 8}) {
    // docs out of order, doc 2 twice (once with one value twice), doc 1 absent
    const std::vector<int32_t> docs = {3, 0, 2, 2, 2, 4};
    const std::vector<uint64_t> keys = {50, 70, 90, 10, 90, 70};
    const std::vector<uint8_t> vals = bytes_of(keys, width);
    PointsColumns C;
    CHECK(points_build(5, width, docs.data(), vals.data(), 6, C) == RGPU_OK);
    CHECK(C.n_points == 6 && C.doc_count == 4 && !C.dense && C.bytes_per_dim == width && C.max_doc == 5);
    CHECK((C.docs_by_doc == std::vector<int32_t>{0, 2, 2, 2, 3, 4}));
    CHECK((C.keys_by_doc == std::vector<uint64_t>{70, 10, 90, 90, 50, 70}));
    CHECK((C.keys_sorted == std::vector<uint64_t>{10, 50, 70, 70, 90, 90}));
    CHECK((C.docs_by_value == std::vector<int32_t>{2, 3, 0, 4, 2, 2}));
    CHECK(C.min_key == 10 && C.max_key == 90);
    // dense: one point per doc, given in any order
    const std::vector<int32_t> d2 = {2, 0, 1};
    const std::vector<uint8_t> v2 = bytes_of({7, 9, 8}, width);
    CHECK(points_build(3, width, d2.data(), v2.data(), 3, C) == RGPU_OK);
    CHECK(C.dense && C.doc_count == 3 && (C.keys_by_doc == std::vector<uint64_t>{9, 8, 7}) && (C.docs_by_doc == std::vector<int32_t>{0, 1, 2}));
    // as many points as docs but one doc twice: not dense
    const std::vector<int32_t> d3 = {0, 0, 2};
    CHECK(points_build(3, width, d3.data(), v2.data(), 3, C) == RGPU_OK && !C.dense && C.doc_count == 2);
    // fewer points than docs
    CHECK(points_build(4, width, d2.data(), v2.data(), 3, C) == RGPU_OK && !C.dense);
    // nothing
    CHECK(points_build(4, width, nullptr, nullptr, 0, C) == RGPU_OK && C.n_points == 0 && !C.dense && C.keys_sorted.empty());
    // refusals
    const std::vector<int32_t> bad = {0, 3};
    CHECK(points_build(3, width, bad.data(), v2.data(), 2, C) == RGPU_ERR_ILLEGAL_ARGUMENT);
    const std::vector<int32_t> neg = {-1};
    CHECK(points_build(3, width, neg.data(), v2.data(), 1, C) == RGPU_ERR_ILLEGAL_ARGUMENT);
  }
  PointsColumns C;
  const int32_t d = 0;
  const uint8_t v[16] = {0};
  for (int width : {0, 1, 2, 3, 5, 16}) CHECK(points_build(1, width, &d, v, 1, C) == RGPU_ERR_ILLEGAL_ARGUMENT);
  CHECK(points_build(1, 4, &d, v, -1, C) == RGPU_ERR_ILLEGAL_ARGUMENT);
}

static void test_bounds_on_plateaus() {
  for (size_t plateau : {(size_t)1, (size_t)64, (size_t)65, (size_t)1000}) {
    std::vector<uint64_t> keys = {5, 6};
    keys.insert(keys.end(), plateau, 100);
    keys.push_back(200);
    int64_t i0, i1;
    points_bounds(keys, 100, 150, i0, i1);   // the plateau as lower bound
    CHECK(i0 == 2 && i1 == 2 + (int64_t)plateau);
    points_bounds(keys, 7, 100, i0, i1);     // as upper bound
    CHECK(i0 == 2 && i1 == 2 + (int64_t)plateau);
    points_bounds(keys, 100, 100, i0, i1);   // lower == upper
    CHECK(i1 - i0 == (int64_t)plateau);
    points_bounds(keys, 101, 199, i0, i1);   // inside a gap
    CHECK(i1 == i0);
    points_bounds(keys, 101, 100, i0, i1);   // lower > upper
    CHECK(i1 == i0);
    points_bounds(keys, 0, 4, i0, i1);       // below the minimum
    CHECK(i1 == i0);
    points_bounds(keys, 201, ~0ull, i0, i1); // above the maximum
    CHECK(i1 == i0);
    points_bounds(keys, 0, ~0ull, i0, i1);
    CHECK(i0 == 0 && i1 == (int64_t)keys.size());
  }
  int64_t i0 = 9, i1 = 9;
  points_bounds({}, 0, ~0ull, i0, i1);
  CHECK(i0 == 0 && i1 == 0);
}

static void test_decisions() {
  // a dense field of 6400 docs, key = doc; and a sparse one (every second doc)
  const int32_t n = 6400;
  std::vector<int32_t> docs(n);
  std::vector<uint64_t> keys(n);
  for (int32_t i = 0; i < n; ++i) { docs[(size_t)i] = i; keys[(size_t)i] = 1000 + (uint64_t)i; }
  for (int width : {4, 8}) {
    const std::vector<uint8_t> vals = bytes_of(keys, width);
    PointsColumns D, S;
    CHECK(points_build(n, width, docs.data(), vals.data(), n, D) == RGPU_OK && D.dense);
    std::vector<int32_t> sdocs;
    for (int32_t i = 0; i < n; ++i) sdocs.push_back(i - (i & 1));   // every even doc twice
    CHECK(points_build(n, width, sdocs.data(), vals.data(), n, S) == RGPU_OK && !S.dense && S.doc_count == n / 2);
    // matches at the crossover of the dense field: the least m with m * price >= n * width
    const int64_t at = ((int64_t)n * width + POINTS_SCAN_BYTES_PER_SCATTERED_POINT - 1) / POINTS_SCAN_BYTES_PER_SCATTERED_POINT;
    CHECK(points_scan_bytes(D) == (int64_t)n * width && points_scan_bytes(S) == (int64_t)n * (width + 4));
    const std::vector<rgpu_point_range> rs = {
        range(0, 999, width),                               // below the minimum
        range(1000, 1000 + n - 1, width),                   // exactly [min, max]
        range(0, 0xffffffffull, width),                     // wider than [min, max]
        range(1000, 1000 + (uint64_t)at - 2, width),        // one match short of the crossover
        range(1000, 1000 + (uint64_t)at - 1, width),        // at the crossover
        range(2000, 1999, width),                           // lower > upper
        range(1001, 1000 + n - 1, width),                   // all but one
        range(1500, 1500, width)};                          // one value
    const PointsAnswer want_auto_dense[] = {POINTS_NOTHING, POINTS_EVERY_DOC, POINTS_EVERY_DOC, POINTS_SCATTER, POINTS_SCAN, POINTS_NOTHING, POINTS_SCAN, POINTS_SCATTER};
    const std::vector<PointsRangePlan> P = plan_point_ranges(D, rs.data(), (int32_t)rs.size(), 0);
    for (size_t r = 0; r < rs.size(); ++r) CHECK(P[r].answer == want_auto_dense[r]);
    CHECK(P[1].i0 == 0 && P[1].i1 == n && P[3].i1 - P[3].i0 == at - 1 && P[4].i1 - P[4].i0 == at && P[7].i1 - P[7].i0 == 1);
    // a sparse field never takes the every-doc form
    const std::vector<PointsRangePlan> Q = plan_point_ranges(S, rs.data(), (int32_t)rs.size(), 0);
    CHECK(Q[1].answer == POINTS_SCAN && Q[2].answer == POINTS_SCAN && Q[0].answer == POINTS_NOTHING && Q[7].answer == POINTS_SCATTER);
    // its crossover lies higher: every point also costs the scan its doc id
    const int64_t sat = ((int64_t)n * (width + 4) + POINTS_SCAN_BYTES_PER_SCATTERED_POINT - 1) / POINTS_SCAN_BYTES_PER_SCATTERED_POINT;
    const rgpu_point_range edge[2] = {range(1000, 1000 + (uint64_t)sat - 2, width), range(1000, 1000 + (uint64_t)sat - 1, width)};
    const std::vector<PointsRangePlan> E2 = plan_point_ranges(S, edge, 2, 0);
    CHECK(sat > at && E2[0].answer == POINTS_SCATTER && E2[1].answer == POINTS_SCAN && E2[1].i1 - E2[1].i0 == sat);
    // forced paths: their kernel for every range with a match, nothing to launch otherwise
    for (int path : {1, 2}) {
      const std::vector<PointsRangePlan> F = plan_point_ranges(D, rs.data(), (int32_t)rs.size(), path);
      for (size_t r = 0; r < rs.size(); ++r)
        CHECK(F[r].answer == (want_auto_dense[r] == POINTS_NOTHING ? POINTS_NOTHING : (path == 1 ? POINTS_SCATTER : POINTS_SCAN)));
    }
    // passes: 17 scanned ranges among others -> 16 + 1, caller order kept
    std::vector<rgpu_point_range> many;
    for (int i = 0; i < 20; ++i) many.push_back(i % 7 == 3 ? range(5, 1, width) : range(1000, 1000 + (uint64_t)i, width));
    const std::vector<PointsRangePlan> M = plan_point_ranges(D, many.data(), 20, 2);
    const std::vector<std::vector<int32_t>> passes = points_scan_passes(M);
    CHECK(passes.size() == 2 && passes[0].size() == 16 && passes[1].size() == 1);
    CHECK(passes[0][0] == 0 && passes[0][3] == 4 && passes[1][0] == 19);   // rows 3, 10, 17 launch nothing
    CHECK(points_scan_passes(plan_point_ranges(D, many.data(), 20, 1)).empty());
    CHECK(points_scan_passes(plan_point_ranges(D, many.data(), 16, 2)).size() == 1);
  }
  PointsColumns E;
  CHECK(points_build(10, 4, nullptr, nullptr, 0, E) == RGPU_OK);
  const rgpu_point_range all = range(0, 0xffffffffull, 4);
  for (int path : {0, 1, 2}) CHECK(plan_point_ranges(E, &all, 1, path)[0].answer == POINTS_NOTHING);
}

static void test_padding() {
  CHECK(points_padded_count(0, 10, 4, false) == 256 && points_padded_count(0, 10, 8, false) == 128);
  CHECK(points_padded_count(256, 300, 4, false) == 256 && points_padded_count(257, 300, 4, false) == 512);
  CHECK(points_padded_count(129, 129, 8, true) == 256);     // three u64 words = 192 docs -> two chunks of 128
  CHECK(points_padded_count(8193, 8193, 4, true) == 8448);  // 129 words = 8256 docs -> 33 chunks of 256
  CHECK(points_padded_count(1, 1, 4, true) == 256);
}

int main() {
  test_keys();
  test_build_orders_and_density();
  test_bounds_on_plateaus();
  test_decisions();
  test_padding();
  std::printf("points_plan_test OK\n");
  return 0;
}
