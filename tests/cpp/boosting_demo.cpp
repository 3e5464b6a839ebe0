// The C++ host mirror's BoostingQuery (rucene_amd/csrc/host/gpu_index_searcher.hpp) over a docs-and-freqs field handed over as raw
// files: <dir>/{doc,norms,terms}.bin (terms = rgpu_term_state[], the vocabulary of tests/segment_spectrum.py) and
// "<max_doc> <doc_count> <sum_total_term_freq>" on the command line. Prints, for a fixed list of queries and k = 10,
//   boosting <i> <total_hits> <doc>:<score-bits> ...
// through search_many (one mixed batch: the queries below and a TermQuery between them) and, for the last line, through
// search() with a collector; then checks that what the GPU path does not serve reaches the cpu_fallback hook.
// tests/test_gpu_boosting.py compares the lines with the Python mirror's rows on the same leaf.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../rucene_amd/csrc/host/gpu_index_searcher.hpp"

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void print_line(size_t i, const rucene::TopDocs& top) {
  std::printf("boosting %zu %lld", i, (long long)top.total_hits());
  for (const rucene::ScoreDoc& d : top.score_docs()) {
    uint32_t bits;
    std::memcpy(&bits, &d.score, 4);
    std::printf(" %d:%08x", d.doc, bits);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc != 5) return 1;
  try {
    const std::string dir = argv[1];
    const std::vector<uint8_t> doc = slurp(dir + "/doc.bin"), norms = slurp(dir + "/norms.bin"), terms = slurp(dir + "/terms.bin");
    LeafReader leaf;
    leaf.doc_bytes = doc.data();
    leaf.doc_len = doc.size();
    leaf.norms = norms.data();
    leaf.max_doc = std::atoi(argv[2]);
    leaf.doc_count = std::atoll(argv[3]);
    leaf.sum_total_term_freq = std::atoll(argv[4]);
    leaf.terms = reinterpret_cast<const rgpu_term_state*>(terms.data());
    leaf.n_terms = static_cast<int64_t>(terms.size() / sizeof(rgpu_term_state));
    GpuIndexSearcher searcher({leaf});

    auto T = [](std::initializer_list<int> ids) {
      std::vector<TermQuery> out;
      for (int t : ids) out.emplace_back(static_cast<int64_t>(t));
      return out;
    };
    auto term = [](int t) { return std::shared_ptr<const Query>(new TermQuery(static_cast<int64_t>(t))); };
    auto boolean = [](std::vector<TermQuery> musts, std::vector<TermQuery> shoulds, int msm = 0, std::vector<TermQuery> nots = {}) {
      return std::shared_ptr<const Query>(BooleanQuery::build(std::move(musts), std::move(shoulds), msm, std::move(nots)));
    };
    std::vector<std::unique_ptr<Query>> qs;
    qs.emplace_back(new BoostingQuery(term(0), term(3), 0.1f));                                        // TERM, demoted by a dense term
    qs.emplace_back(new BoostingQuery(term(4), term(1), 0.5f));                                        // ... by a singleton
    qs.emplace_back(new TermQuery(static_cast<int64_t>(6)));                                           // (a mixed batch)
    qs.emplace_back(new BoostingQuery(boolean(T({0, 3, 7}), {}), boolean({}, T({5, 4})), 0.5f));       // AND, a union with an absent term
    qs.emplace_back(new BoostingQuery(boolean({}, T({3, 4, 6}), 2), term(0), 0.99999994f));            // OR msm 2, every hit demoted
    qs.emplace_back(new BoostingQuery(boolean({}, T({0, 2, 3, 4, 5, 6, 7, 3, 4}), 0, T({1})), boolean({}, T({3, 4})), 0.1f));
    qs.emplace_back(new BoostingQuery(term(0), term(5), 0.5f));                                        // the negative has no posting: no hit
    std::vector<const Query*> ptrs;
    for (auto& q : qs) ptrs.push_back(q.get());
    const std::vector<TopDocs> got = searcher.search_many(ptrs, 10);
    for (size_t i = 0; i < got.size(); ++i) print_line(i, got[i]);
    TopDocsCollector coll(10);
    searcher.search(*qs[0], coll);
    print_line(got.size(), coll.top_docs());
    // what the GPU path does not serve: UnsupportedOperation, i.e. the cpu_fallback hook when it is set
    std::vector<std::unique_ptr<Query>> declined;
    declined.emplace_back(new BoostingQuery(term(0), term(3), 1.0f));
    declined.emplace_back(new BoostingQuery(term(0), term(3), 0.0f));
    declined.emplace_back(new BoostingQuery(boolean(T({0}), T({3})), term(4), 0.5f));                  // MUST + SHOULD positive
    declined.emplace_back(new BoostingQuery(term(0), boolean(T({3, 4}), {}), 0.5f));                   // a conjunction as the negative
    declined.emplace_back(new BoostingQuery(std::shared_ptr<const Query>(new DisjunctionMaxQuery(T({3, 4}), 0.1f)), term(0), 0.5f));
    for (auto& q : declined) {
      bool threw = false;
      try { searcher.search(*q, coll); } catch (const Error& e) { threw = e.kind == RGPU_ERR_UNSUPPORTED; }
      if (!threw) return 3;
    }
    int fell_back = 0;
    searcher.cpu_fallback = [&](const Query&, TopDocsCollector&) { ++fell_back; };
    for (auto& q : declined) searcher.search(*q, coll);
    if (fell_back != static_cast<int>(declined.size())) return 4;
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
