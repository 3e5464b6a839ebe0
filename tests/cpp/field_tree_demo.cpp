// The C++ host mirror's routing of cross-field query-string trees (rucene_amd/csrc/host/gpu_index_searcher.hpp: MultiFieldQuery's sum
// groups and must_should form, GpuIndexSearcher::field_trees) over a three-field leaf handed over as raw files, as
// tests/cpp/cross_field_demo.cpp takes them: <dir>/doc.bin, <dir>/norms<f>.bin, <dir>/terms<f>.bin per field f = 0, 1, 2, then
// "<max_doc>" and "<sum_total_term_freq>" per field, then the term ids the queries name: title's a b c, body's a b c, tags' a.
// Prints, for a fixed list of queries and k = 10,
//   tree <i> <total_hits> <doc>:<score-bits> ...
// through search_many with field_trees on, and a last line with what a default searcher does with the first tree.
// tests/test_gpu_field_tree.py compares the lines with tests/field_tree.py.
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
  std::printf("tree %zu %lld", i, (long long)top.total_hits());
  for (const rucene::ScoreDoc& d : top.score_docs()) {
    uint32_t bits;
    std::memcpy(&bits, &d.score, 4);
    std::printf(" %d:%08x", d.doc, bits);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc != 13) return 1;
  try {
    const std::string dir = argv[1];
    const std::vector<uint8_t> doc = slurp(dir + "/doc.bin");
    std::vector<uint8_t> norms[3], terms[3];
    for (int f = 0; f < 3; ++f) {
      norms[f] = slurp(dir + "/norms" + std::to_string(f) + ".bin");
      terms[f] = slurp(dir + "/terms" + std::to_string(f) + ".bin");
    }
    const char* names[3] = {"title", "body", "tags"};
    LeafReader leaf;
    leaf.field = names[0];
    leaf.doc_bytes = doc.data();
    leaf.doc_len = doc.size();
    leaf.norms = norms[0].data();
    leaf.max_doc = std::atoi(argv[2]);
    leaf.doc_count = leaf.max_doc;
    leaf.sum_total_term_freq = std::atoll(argv[3]);
    leaf.terms = reinterpret_cast<const rgpu_term_state*>(terms[0].data());
    leaf.n_terms = static_cast<int64_t>(terms[0].size() / sizeof(rgpu_term_state));
    for (int f = 1; f < 3; ++f) {
      ExtraField x;
      x.name = names[f];
      x.field_number = f;
      x.norms = norms[f].empty() ? nullptr : norms[f].data();
      x.doc_count = leaf.max_doc;
      x.sum_total_term_freq = std::atoll(argv[3 + f]);
      x.terms = reinterpret_cast<const rgpu_term_state*>(terms[f].data());
      x.n_terms = static_cast<int64_t>(terms[f].size() / sizeof(rgpu_term_state));
      leaf.extra_fields.push_back(x);
    }
    int id[7];
    for (int i = 0; i < 7; ++i) id[i] = std::atoi(argv[6 + i]);
    auto T = [&](int f, int t) { return TermQuery(static_cast<int64_t>(t), 1.0f).in(f == 0 ? "" : names[f]); };
    using M = MultiFieldQuery;
    auto word = [&](int w) { return M::sum_of({T(0, id[w]), T(1, id[3 + w])}, 1); };   // (title:w body:w)
    std::vector<std::unique_ptr<Query>> qs;
    qs.emplace_back(M::must_should({word(0)}, {word(1)}).release());                                 // "b +a"
    qs.emplace_back(M::should({word(1), word(2)}, 1).release());                                     // "b c"
    qs.emplace_back(M::must_should({word(0), M::term(T(2, id[6]))}, {word(1), word(2)}, 0, {T(1, id[5])}).release());
    qs.emplace_back(M::all_must({word(1), word(2)}).release());                                      // "+b +c"
    qs.emplace_back(M::should({M::dismax({T(0, id[1]), T(1, id[4])}, 0.3f), M::term(T(2, id[6]))}).release());   // the old call's
    std::vector<const Query*> ptrs;
    for (auto& q : qs) ptrs.push_back(q.get());
    GpuIndexSearcher searcher({leaf});
    int fell_back = 0, refused = 0;
    searcher.cpu_fallback = [&](const Query&, TopDocsCollector&) { ++fell_back; };
    TopDocsCollector coll(10);
    searcher.search(*qs[0], coll);   // without the flag: the CPU searcher's
    try { searcher.search_many({qs[1].get()}, 10); } catch (const Error& e) { refused += e.kind == RGPU_ERR_UNSUPPORTED; }
    searcher.field_trees = true;
    const std::vector<TopDocs> got = searcher.search_many(ptrs, 10);
    for (size_t i = 0; i < got.size(); ++i) print_line(i, got[i]);
    std::unique_ptr<M> nested2 = M::should({M::sum_of({T(0, id[0]), T(1, id[3])}, 2)});
    try { searcher.search_many({nested2.get()}, 10); } catch (const Error& e) { refused += e.kind == RGPU_ERR_UNSUPPORTED; }
    std::printf("fallback %d refused %d\n", fell_back, refused);
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
