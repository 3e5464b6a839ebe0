// The C++ host mirror's DisjunctionMaxQuery (rucene_amd/csrc/host/gpu_index_searcher.hpp) over a docs-and-freqs field handed
// over as raw files: <dir>/{doc,norms,terms}.bin (terms = rgpu_term_state[], the vocabulary of tests/segment_spectrum.py) and
// "<max_doc> <doc_count> <sum_total_term_freq>" on the command line. Prints, for a fixed list of queries and k = 10,
//   dismax <i> <total_hits> <doc>:<score-bits> ...
// through search_many (one mixed batch: the queries below and a TermQuery between them) and, for the last line, through
// search() with a collector. tests/test_gpu_dismax.py compares the lines with the Python mirror's rows on the same leaf.
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
  std::printf("dismax %zu %lld", i, (long long)top.total_hits());
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
    std::vector<std::unique_ptr<Query>> qs;
    qs.emplace_back(new DisjunctionMaxQuery(T({4}), 0.5f));                                  // one disjunct, kept as a dismax
    qs.emplace_back(new DisjunctionMaxQuery(T({3, 4}), 0.0f));
    qs.emplace_back(new TermQuery(static_cast<int64_t>(6)));                                 // (a mixed batch)
    qs.emplace_back(new DisjunctionMaxQuery(T({4, 4}), 0.1f));
    qs.emplace_back(new DisjunctionMaxQuery(T({0, 1, 2, 3, 4, 5, 6, 7, 3}), 0.1f));
    qs.emplace_back(new DisjunctionMaxQuery(T({1, 2, 4, 5, 6, 5, 1, 2, 4, 5, 5, 5}), 1.0f));  // 12 disjuncts, the absent one repeats
    qs.emplace_back(new DisjunctionMaxQuery(T({5, 5}), 0.1f));
    std::vector<const Query*> ptrs;
    for (auto& q : qs) ptrs.push_back(q.get());
    const std::vector<TopDocs> got = searcher.search_many(ptrs, 10);
    for (size_t i = 0; i < got.size(); ++i) print_line(i, got[i]);
    // DisjunctionMaxQuery::build: a lone disjunct is that query; search() with a collector
    std::unique_ptr<Query> lone = DisjunctionMaxQuery::build(T({4}), 0.5f);
    if (!dynamic_cast<const TermQuery*>(lone.get())) return 3;
    TopDocsCollector coll(10);
    searcher.search(*qs[1], coll);
    print_line(got.size(), coll.top_docs());
    bool threw = false;
    try { DisjunctionMaxQuery empty({}, 0.1f); } catch (const Error& e) { threw = e.kind == RGPU_ERR_ILLEGAL_ARGUMENT; }
    if (!threw) return 4;
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
