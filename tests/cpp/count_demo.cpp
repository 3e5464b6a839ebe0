// The C++ host mirror's hit counts (rucene_amd/csrc/host/gpu_index_searcher.hpp: count, count_many, cpu_count_fallback) over
// docs-and-freqs leaves handed over as raw files: <dir>/leaf<i>/{doc,norms,terms,live}.bin (terms = rgpu_term_state[], the vocabulary
// of tests/count.py; live.bin empty = no deletions) and, on the command line, "<dir> <n_leaves>" followed by
// "<max_doc> <sum_total_term_freq>" per leaf. Prints
//   count <i> <n>
// for a batch through count_many, then the same rows one by one through count() with MatchAllDocsQuery last, checks that a phrase
// reaches the cpu_count_fallback hook, and ends with "count_demo OK". tests/test_gpu_count.py compares the lines with the model.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../rucene_amd/csrc/host/gpu_index_searcher.hpp"

enum { EDGE, BLK, SPARSE, TAIL0, TAIL1, TAIL127, S0, SW1, SW, SLAST, ABSENT, A, B, C };  // tests/count.py

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc < 3) return 1;
  const int n_leaves = std::atoi(argv[2]);
  if (n_leaves < 1 || argc != 3 + 2 * n_leaves) return 1;
  try {
    const std::string dir = argv[1];
    std::vector<std::vector<uint8_t>> docs, norms, terms, lives;
    std::vector<LeafReader> leaves;
    int32_t base = 0;
    for (int i = 0; i < n_leaves; ++i) {
      const std::string at = dir + "/leaf" + std::to_string(i);
      docs.push_back(slurp(at + "/doc.bin"));
      norms.push_back(slurp(at + "/norms.bin"));
      terms.push_back(slurp(at + "/terms.bin"));
      lives.push_back(slurp(at + "/live.bin"));
    }
    for (int i = 0; i < n_leaves; ++i) {
      LeafReader leaf;
      leaf.doc_bytes = docs[(size_t)i].data();
      leaf.doc_len = docs[(size_t)i].size();
      leaf.norms = norms[(size_t)i].data();
      leaf.max_doc = std::atoi(argv[3 + 2 * i]);
      leaf.doc_base = base;
      leaf.doc_count = leaf.max_doc;
      leaf.sum_total_term_freq = std::atoll(argv[4 + 2 * i]);
      leaf.live_docs = lives[(size_t)i].empty() ? nullptr : reinterpret_cast<const uint64_t*>(lives[(size_t)i].data());
      leaf.terms = reinterpret_cast<const rgpu_term_state*>(terms[(size_t)i].data());
      leaf.n_terms = static_cast<int64_t>(terms[(size_t)i].size() / sizeof(rgpu_term_state));
      base += leaf.max_doc;
      leaves.push_back(leaf);
    }
    GpuIndexSearcher searcher(leaves);
    auto T = [](std::initializer_list<int> ids) {
      std::vector<TermQuery> out;
      for (int t : ids) out.emplace_back(static_cast<int64_t>(t));
      return out;
    };
    // the rows of tests/test_gpu_count.py::test_cpp_demo, in its order
    std::vector<std::unique_ptr<Query>> owned;
    owned.push_back(std::make_unique<TermQuery>(static_cast<int64_t>(A)));
    owned.push_back(BooleanQuery::build(T({A, C}), {}));
    owned.push_back(BooleanQuery::build({}, T({A, B, C}), 2));
    owned.push_back(BooleanQuery::build({}, T({A, B}), 0, T({C})));
    owned.push_back(BooleanQuery::build(T({C}), {}, 0, T({A})));
    owned.push_back(BooleanQuery::build({}, T({EDGE, SPARSE, SLAST, ABSENT})));
    owned.push_back(std::make_unique<TermQuery>(static_cast<int64_t>(ABSENT)));
    std::vector<const Query*> rows;
    for (const std::unique_ptr<Query>& q : owned) rows.push_back(q.get());
    const std::vector<int64_t> counts = searcher.count_many(rows);
    for (size_t i = 0; i < counts.size(); ++i) std::printf("count %zu %lld\n", i, (long long)counts[i]);
    for (size_t i = 0; i < rows.size(); ++i)
      if (searcher.count(*rows[i]) != counts[i]) { std::printf("count() and count_many() differ on row %zu\n", i); return 1; }
    std::printf("count %zu %lld\n", rows.size(), (long long)searcher.count(MatchAllDocsQuery()));
    // what the GPU path refuses reaches the hook; without one the error comes back
    const PhraseQuery phrase(T({A, B}));
    bool threw = false;
    try { (void)searcher.count(phrase); } catch (const Error& e) { threw = e.kind == RGPU_ERR_UNSUPPORTED; }
    int seen = 0;
    searcher.cpu_count_fallback = [&](const Query&) { ++seen; return (int64_t)41; };
    if (!threw || searcher.count(phrase) != 41 || seen != 1) { std::printf("the fallback hook was not reached\n"); return 1; }
    std::printf("count_demo OK\n");
  } catch (const Error& e) {
    std::printf("error %d: %s\n", e.kind, e.what());
    return 1;
  }
  return 0;
}
