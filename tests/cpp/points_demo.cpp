// The C++ host mirror's point ranges (rucene_amd/csrc/host/gpu_index_searcher.hpp: PointRangeQuery, IntPoint / LongPoint / FloatPoint /
// DoublePoint, attach_points, range_filter, range_clauses) over ONE docs-and-freqs leaf handed over as raw files:
// <dir>/{doc,norms,terms,live}.bin as tests/cpp/docset_demo.cpp reads them, and <dir>/{price,date}_{docs,values}.bin — the (doc, value)
// pairs of a dense 4-byte field and a multi-valued 8-byte field. Command line: "<dir> <max_doc> <sum_total_term_freq> <bounds>", bounds =
// the hex of r1.lower r1.upper (4 bytes each, price), r2.lower r2.upper r3.lower r3.upper (8 bytes each, date). Prints
//   cardinality <r1> <r2> <r3>
//   points <i> <total_hits> <doc>:<score-bits> ...
// for the seven range queries of tests/test_gpu_points.py (_range_cases) through search_many, then checks that the shapes the GPU path does
// not serve reach the cpu_fallback hook, that a wrong width is an argument error and that the encoders give the bytes written out by hand.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../rucene_amd/csrc/host/gpu_index_searcher.hpp"

enum { EVERY, FIRST, LAST, EVEN, FIFTH, ABSENT, SOMETIMES, CONST };  // tests/segment_spectrum.py

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static std::vector<uint8_t> unhex(const std::string& s, size_t at, size_t n) {
  std::vector<uint8_t> out;
  for (size_t i = 0; i < n; ++i) out.push_back(static_cast<uint8_t>(std::stoul(s.substr(2 * (at + i), 2), nullptr, 16)));
  return out;
}
static std::string hex(const std::vector<uint8_t>& b) {
  std::string s;
  char two[3];
  for (uint8_t x : b) { std::snprintf(two, sizeof two, "%02x", x); s += two; }
  return s;
}
static void print_line(size_t i, const rucene::TopDocs& top) {
  std::printf("points %zu %lld", i, (long long)top.total_hits());
  for (const rucene::ScoreDoc& d : top.score_docs()) {
    uint32_t bits;
    std::memcpy(&bits, &d.score, 4);
    std::printf(" %d:%08x", d.doc, bits);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc != 5 || std::strlen(argv[4]) != 80) return 1;
  try {
    // the encoders, against bytes written out by hand (core/util/numeric.rs:163-218)
    if (hex(IntPoint::encode(-1)) != "7fffffff" || hex(IntPoint::encode(INT32_MIN)) != "00000000" || hex(LongPoint::encode(1)) != "8000000000000001" ||
        hex(FloatPoint::encode(-0.0f)) != "7fffffff" || hex(FloatPoint::encode(0.0f)) != "80000000" || hex(FloatPoint::encode(-1.5f)) != "403fffff" ||
        hex(DoublePoint::encode(-1.5)) != "4007ffffffffffff" || hex(DoublePoint::encode(0.0)) != "8000000000000000") {
      std::printf("an encoder is off\n");
      return 1;
    }
    const std::string dir = argv[1];
    const std::vector<uint8_t> doc = slurp(dir + "/doc.bin"), norms = slurp(dir + "/norms.bin"), terms = slurp(dir + "/terms.bin"), live = slurp(dir + "/live.bin");
    const std::vector<uint8_t> price_docs = slurp(dir + "/price_docs.bin"), price_values = slurp(dir + "/price_values.bin");
    const std::vector<uint8_t> date_docs = slurp(dir + "/date_docs.bin"), date_values = slurp(dir + "/date_values.bin");
    LeafReader leaf;
    leaf.doc_bytes = doc.data();
    leaf.doc_len = doc.size();
    leaf.norms = norms.data();
    leaf.max_doc = std::atoi(argv[2]);
    leaf.doc_base = 0;
    leaf.doc_count = leaf.max_doc;
    leaf.sum_total_term_freq = std::atoll(argv[3]);
    leaf.live_docs = live.empty() ? nullptr : reinterpret_cast<const uint64_t*>(live.data());
    leaf.terms = reinterpret_cast<const rgpu_term_state*>(terms.data());
    leaf.n_terms = static_cast<int64_t>(terms.size() / sizeof(rgpu_term_state));
    GpuIndexSearcher searcher({leaf});
    searcher.attach_points("price", 4, {LeafPoints::of(reinterpret_cast<const int32_t*>(price_docs.data()), price_values.data(), static_cast<int64_t>(price_docs.size() / 4))});
    searcher.attach_points("date", 8, {LeafPoints::of(reinterpret_cast<const int32_t*>(date_docs.data()), date_values.data(), static_cast<int64_t>(date_docs.size() / 4))});

    const std::string b = argv[4];
    const PointRangeQuery r1("price", unhex(b, 0, 4), unhex(b, 4, 4)), r2("date", unhex(b, 8, 8), unhex(b, 16, 8)), r3("date", unhex(b, 24, 8), unhex(b, 32, 8));
    const CachedFilter f1 = searcher.range_filter(r1);
    if (searcher.range_filter(PointRangeQuery("price", r1.lower, r1.upper)).id != f1.id) { std::printf("the memo made a second filter\n"); return 1; }
    std::printf("cardinality %lld %lld %lld\n", (long long)searcher.filter_cardinality(f1), (long long)searcher.filter_cardinality(searcher.range_filter(r2)),
                (long long)searcher.filter_cardinality(searcher.range_filter(r3)));

    auto T = [](std::initializer_list<int> ids) {
      std::vector<TermQuery> out;
      for (int t : ids) out.emplace_back(static_cast<int64_t>(t));
      return out;
    };
    const TermQuery every(static_cast<int64_t>(EVERY)), constant(static_cast<int64_t>(CONST)), even(static_cast<int64_t>(EVEN));
    const std::unique_ptr<Query> both = BooleanQuery::build(T({EVERY, EVEN}), {});
    const std::unique_ptr<Query> opt = BooleanQuery::build(T({EVERY}), T({LAST, FIFTH}));
    std::vector<FilteredQuery> fq;
    fq.push_back(searcher.range_clauses(every, {&r1}));             // +a +range
    fq.push_back(searcher.range_clauses(constant, {&r2}));          // +range +a (narrow)
    fq.push_back(searcher.range_clauses(*both, {&r1}, {&r2}));      // +a +b #range -range2
    fq.push_back(searcher.range_clauses(*opt, {&r3}));              // +a b c #range
    fq.push_back(searcher.range_clauses(even, {}, {&r1}));          // +a -range
    fq.push_back(searcher.range_clauses(every, {&r1, &r3}));        // +a +range +range3
    const std::unique_ptr<Query> filt_opt = BooleanQuery::build({}, T({FIFTH}), 0, {}, T({EVEN}));
    fq.push_back(searcher.range_clauses(*filt_opt, {&r1}));         // +range #a b: b stays optional (min_should_match 0)
    std::vector<const Query*> batch;
    for (const FilteredQuery& q : fq) batch.push_back(&q);
    const std::vector<TopDocs> rows = searcher.search_many(batch, 10);
    for (size_t i = 0; i < rows.size(); ++i) print_line(i, rows[i]);

    // ---- what is not served reaches the CPU path; a wrong width is an argument error
    int fallen = 0;
    searcher.cpu_fallback = [&](const Query&, TopDocsCollector&) { ++fallen; };
    TopDocsCollector collector(10);
    const std::unique_ptr<Query> or3 = BooleanQuery::build({}, T({FIRST, LAST, SOMETIMES}));
    const PhraseQuery phrase(T({EVERY, EVEN}));
    searcher.search(r1, collector);                                        // a lone range
    searcher.search(searcher.range_clauses(*or3, {&r1}), collector);       // +range b c
    searcher.search(searcher.range_clauses(phrase, {&r1}), collector);     // beside a phrase
    if (fallen != 3) { std::printf("cpu_fallback reached %d times, not 3\n", fallen); return 1; }
    bool unknown = false, width = false, dims = false;
    try { searcher.range_filter(PointRangeQuery("price", r2.lower, r2.upper, 2)); } catch (const Error& e) { dims = e.kind == RGPU_ERR_UNSUPPORTED; }
    if (!dims) { std::printf("a two-dimensional range was not refused\n"); return 1; }
    try { searcher.range_filter(IntPoint::new_range_query("weight", 1, 2)); } catch (const Error& e) { unknown = e.kind == RGPU_ERR_UNSUPPORTED; }
    try { searcher.range_filter(LongPoint::new_range_query("price", 1, 2)); } catch (const Error& e) { width = e.kind == RGPU_ERR_ILLEGAL_ARGUMENT; }
    if (!unknown || !width) { std::printf("an unknown field / a wrong width was not refused as it should be\n"); return 1; }
    // the memo can be emptied: the same range is then built anew, under a new id
    searcher.drop_range_filters();
    if (searcher.range_filter(r1).id == f1.id) { std::printf("drop_range_filters kept a filter\n"); return 1; }
    std::printf("fallback ok\n");
  } catch (const rucene::Error& e) {
    std::printf("error %d: %s\n", e.kind, e.what());
    return 1;
  }
  return 0;
}
