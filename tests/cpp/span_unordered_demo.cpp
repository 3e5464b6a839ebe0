// The C++ host mirror's UNORDERED SpanNearQuery over SpanTermQuery clauses (rucene_amd/csrc/host/gpu_index_searcher.hpp:
// GpuIndexSearcher::unordered_spans -> rgpu_search_span_unordered_batch) over a positions field handed over as raw files:
// <dir>/{doc,pos,norms,terms,tpos,live}.bin (terms = rgpu_term_state[], tpos = rgpu_term_positions[], live = u64 words, empty: no
// deletions), "<max_doc> <doc_count> <sum_total_term_freq> <k>" on the command line and the queries in <dir>/queries.txt, one per line:
//   <slop> <boost> <t,t,..>          the clauses' term ids in clause order
// Prints, for the whole batch in ONE search_many call:   row <i> <total_hits> <doc>:<score-bits> ...
// then "single <total_hits> <doc>:<score-bits> ..." for the first query through search(query, collector),
// and then "refused <a> <b> <c> <d> <e>": UnsupportedOperation for an unordered near on a searcher with the flag off (a), a nested span
// clause with it on (b), an unordered near under a FilteredQuery (c), SpanNearQuery::check_served() itself, which keeps refusing
// unordered near (d), and an unordered near in a rescore request (e); "built <f>": a one-clause SpanNearQuery is IllegalArgument
// when it is made (f).
// tests/test_gpu_span_unordered.py compares the lines with the model of tests/span_unordered.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../rucene_amd/csrc/host/gpu_index_searcher.hpp"

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string part;
  while (std::getline(ss, part, sep)) out.push_back(part);
  return out;
}
static void print_row(const char* head, const rucene::TopDocs& row) {
  std::printf("%s %lld", head, (long long)row.total_hits());
  for (const rucene::ScoreDoc& d : row.score_docs()) {
    uint32_t bits;
    std::memcpy(&bits, &d.score, 4);
    std::printf(" %d:%08x", d.doc, bits);
  }
  std::printf("\n");
}

template <typename Fn>
static int refused(Fn&& fn, int kind = RGPU_ERR_UNSUPPORTED) {
  try {
    fn();
  } catch (const rucene::Error& e) {
    return e.kind == kind ? 1 : 0;
  }
  return 0;
}

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc != 6) return 1;
  try {
    const std::string dir = argv[1];
    const std::vector<uint8_t> doc = slurp(dir + "/doc.bin"), pos = slurp(dir + "/pos.bin"), norms = slurp(dir + "/norms.bin"),
                               terms = slurp(dir + "/terms.bin"), tpos = slurp(dir + "/tpos.bin"), live = slurp(dir + "/live.bin");
    LeafReader leaf;
    leaf.index_options = 3;
    leaf.doc_bytes = doc.data();
    leaf.doc_len = doc.size();
    leaf.pos_bytes = pos.data();
    leaf.pos_len = pos.size();
    leaf.norms = norms.data();
    leaf.max_doc = std::atoi(argv[2]);
    leaf.doc_count = std::atoll(argv[3]);
    leaf.sum_total_term_freq = std::atoll(argv[4]);
    std::vector<uint64_t> live_words(live.size() / 8);
    if (!live.empty()) std::memcpy(live_words.data(), live.data(), live_words.size() * 8);
    leaf.live_docs = live_words.empty() ? nullptr : live_words.data();
    const size_t k = static_cast<size_t>(std::atoi(argv[5]));
    leaf.terms = reinterpret_cast<const rgpu_term_state*>(terms.data());
    leaf.n_terms = static_cast<int64_t>(terms.size() / sizeof(rgpu_term_state));
    leaf.term_positions = reinterpret_cast<const rgpu_term_positions*>(tpos.data());
    GpuIndexSearcher searcher({leaf});
    searcher.unordered_spans = true;

    std::vector<std::unique_ptr<SpanNearQuery>> made;
    std::vector<const Query*> batch;
    std::ifstream in(dir + "/queries.txt");
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      const std::vector<std::string> parts = split(line, ' ');
      std::vector<SpanTermQuery> clauses;
      for (const std::string& t : split(parts[2], ',')) clauses.emplace_back(TermQuery(static_cast<int64_t>(std::atoll(t.c_str()))));
      made.emplace_back(new SpanNearQuery(std::move(clauses), std::atoi(parts[0].c_str()), false, static_cast<float>(std::atof(parts[1].c_str()))));
      batch.push_back(made.back().get());
    }
    const std::vector<TopDocs> got = searcher.search_many(batch, k);
    for (size_t i = 0; i < got.size(); ++i) {
      char head[32];
      std::snprintf(head, sizeof head, "row %zu", i);
      print_row(head, got[i]);
    }
    TopDocsCollector collector(k);
    searcher.search(*made[0], collector);
    print_row("single", collector.top_docs());

    const std::vector<SpanTermQuery> two{SpanTermQuery(TermQuery(int64_t(0))), SpanTermQuery(TermQuery(int64_t(1)))};
    const SpanNearQuery unordered(two, 1, false);
    SpanNearQuery outer(two, 1, false);
    outer.add_nested(unordered);
    const CachedFilter F = searcher.filter_from_docs({0});
    const FilteredQuery filtered = FilteredQuery::filter_query(unordered, {F});
    searcher.unordered_spans = false;
    const int a = refused([&] { searcher.search_many({&unordered}, k); });
    searcher.unordered_spans = true;
    const int b = refused([&] { searcher.search_many({&outer}, k); });
    const int c = refused([&] { searcher.search_many({&filtered}, k); });
    const int d = refused([&] { unordered.check_served(); });
    RescoreRequest req;
    req.query = &unordered;
    const int e = refused([&] { searcher.rescore({got[0]}, {req}, k); });
    std::printf("refused %d %d %d %d %d\n", a, b, c, d, e);
    const int f = refused([&] { SpanNearQuery one({SpanTermQuery(TermQuery(int64_t(0)))}); (void)one; }, RGPU_ERR_ILLEGAL_ARGUMENT);
    std::printf("built %d\n", f);
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
