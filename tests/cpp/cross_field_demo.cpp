// The C++ host mirror's cross-field routing (rucene_amd/csrc/host/gpu_index_searcher.hpp) over a three-field leaf handed over as raw
// files: <dir>/doc.bin (ONE .doc file), <dir>/norms<f>.bin and <dir>/terms<f>.bin (rgpu_term_state[]) per field f = 0, 1, 2 (a norms
// file of zero bytes: the field omits norms), and on the command line "<max_doc>" then "<sum_total_term_freq>" per field - the leaf of
// tests/test_gpu_cross_field.py (title, body, tags). Prints, for a fixed list of queries and k = 10,
//   cross <i> <total_hits> <doc>:<score-bits> ...
// through search_many (one mixed batch: cross-field rows and a primary-field row between them) and, for the last lines, through
// search() with a collector and through the CPU fallback (which also takes phrase, phrase-boolean and span trees that name a further field). tests/test_gpu_cross_field.py compares the lines with tests/cross_field.py.
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
  std::printf("cross %zu %lld", i, (long long)top.total_hits());
  for (const rucene::ScoreDoc& d : top.score_docs()) {
    uint32_t bits;
    std::memcpy(&bits, &d.score, 4);
    std::printf(" %d:%08x", d.doc, bits);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc != 6) return 1;
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
    GpuIndexSearcher searcher({leaf});

    auto T = [&](int f, int t, float boost = 1.0f) { return TermQuery(static_cast<int64_t>(t), boost).in(f == 0 ? "" : names[f]); };
    using M = MultiFieldQuery;
    std::vector<std::unique_ptr<Query>> qs;
    qs.emplace_back(new DisjunctionMaxQuery({T(0, 0), T(1, 1)}, 0.1f));                                   // title:a | body:a
    qs.emplace_back(M::should({M::dismax({T(0, 0), T(1, 1)}, 0.0f), M::dismax({T(0, 4), T(1, 3)}, 1.0f)}).release());  // the multi-field query
    qs.emplace_back(new TermQuery(static_cast<int64_t>(0)));                                               // (a primary-field row: where it went)
    qs.emplace_back(new TermQuery(T(1, 1)));                                                               // a lone TermQuery of another field
    qs.emplace_back(BooleanQuery::build({T(0, 0), T(1, 1), T(1, 3)}, {}).release());                       // MUST: the leaf's cost order
    qs.emplace_back(BooleanQuery::build({}, {T(0, 0), T(1, 1)}, 0, {T(2, 0)}).release());                   // MUST_NOT in a third field
    qs.emplace_back(M::all_must({M::dismax({T(0, 3), T(1, 2)}, 0.1f), M::term(T(0, 4)), M::term(T(2, 1))}).release());
    qs.emplace_back(M::should({M::dismax({T(0, 0), T(1, 1)}, 0.0f), M::term(T(2, 0)), M::term(T(0, 3))}, 2).release());
    qs.emplace_back(M::should({M::dismax({T(0, 5), T(1, 4)}, 0.1f)}).release());                           // absent everywhere
    std::vector<const Query*> ptrs;
    for (auto& q : qs) ptrs.push_back(q.get());
    const std::vector<TopDocs> got = searcher.search_many(ptrs, 10);
    for (size_t i = 0; i < got.size(); ++i) print_line(i, got[i]);
    TopDocsCollector coll(10);
    searcher.search(*qs[1], coll);
    print_line(got.size(), coll.top_docs());
    // what the call cannot express, and every path but search, is the CPU searcher's
    int fell_back = 0;
    searcher.cpu_fallback = [&](const Query&, TopDocsCollector&) { ++fell_back; };
    std::unique_ptr<Query> req_opt = BooleanQuery::build({T(1, 1)}, {T(0, 0)});
    searcher.search(*req_opt, coll);
    std::vector<TermQuery> ten(10, T(1, 1));
    DisjunctionMaxQuery wide(ten, 0.1f);
    searcher.search(wide, coll);
    // a phrase, a boolean over a phrase, a disjunction over a phrase and a span query hold TermQuery members too: a further field in
    // any of them is the CPU searcher's, never the primary field's postings under another name
    PhraseBooleanQuery phrase_bool;
    phrase_bool.must(PhraseQuery({T(0, 0), T(0, 4)})).must(T(1, 1));
    searcher.search(phrase_bool, coll);
    PhraseDisjunctionQuery phrase_or;
    phrase_or.should(PhraseQuery({T(0, 0), T(0, 4)})).should(T(0, 3)).must_not(T(1, 1));
    searcher.search(phrase_or, coll);
    searcher.search(PhraseQuery({T(1, 1), T(0, 4)}), coll);
    searcher.search(SpanNearQuery({SpanTermQuery(T(0, 0)), SpanTermQuery(T(1, 1))}, 2), coll);
    bool rescore_refused = false;
    try {
      RescoreRequest rr;
      const TermQuery other = T(1, 1);
      rr.query = &other;
      searcher.rescore({got[0]}, {rr}, 10);
    } catch (const Error& e) { rescore_refused = e.kind == RGPU_ERR_UNSUPPORTED; }
    int64_t counted = -1;
    searcher.cpu_count_fallback = [&](const Query&) { return static_cast<int64_t>(-7); };
    counted = searcher.count(T(1, 1));
    bool refused = false;
    try { searcher.cache_filter(T(1, 1)); } catch (const Error& e) { refused = e.kind == RGPU_ERR_UNSUPPORTED; }
    bool unknown = false;
    try { searcher.search_many({std::unique_ptr<Query>(new TermQuery(TermQuery(static_cast<int64_t>(0)).in("nope"))).get()}, 10); }
    catch (const Error& e) { unknown = e.kind == RGPU_ERR_ILLEGAL_ARGUMENT; }
    std::printf("fallback %d count %lld cache_filter %d unknown %d rescore %d\n", fell_back, (long long)counted, refused ? 1 : 0, unknown ? 1 : 0,
                rescore_refused ? 1 : 0);
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
