// The C++ host mirror's filtered exact phrases (rucene_amd/csrc/host/gpu_index_searcher.hpp: FilteredQuery over PhraseQuery /
// PhraseBooleanQuery / PhraseDisjunctionQuery with GpuIndexSearcher::filtered_phrases on -> rgpu_search_phrase_batch_masked,
// rgpu_search_phrase_bool_batch_masked, rgpu_search_phrase_or_batch_masked) over a positions field handed over as raw files:
// <dir>/{doc,pos,norms,terms,tpos,live}.bin (terms = rgpu_term_state[], tpos = rgpu_term_positions[], live = u64 words, empty: no
// deletions), the docs of two cached filters in <dir>/f.txt and <dir>/x.txt (one id per line),
// "<max_doc> <doc_count> <sum_total_term_freq> <k>" on the command line and the queries in <dir>/queries.txt, one per line:
//   <mode> <kind> <clause> ...
//   mode   fq: FilterQuery(Q, F)   cl: Q's clauses, #F, -X   cf: Q's clauses, #F   cx: Q's clauses, -X   un: Q alone
//   kind   p: a PhraseQuery (one clause p:<t,t,..>:<pos,pos,..>:<boost>)
//          b: a PhraseBooleanQuery (m:t:<term> f:t:<term> n:t:<term> m:p:... f:p:...)
//          o<msm>: a PhraseDisjunctionQuery (s:t:<term> s:p:... n:t:<term>)
// Prints, for the whole batch in ONE search_many call:   row <i> <total_hits> <doc>:<score-bits> ...
// and then "refused <a> <b> <c>": a sloppy phrase under a filter is UnsupportedOperation with the opt-in on (a), "a b" c #F likewise
// (b), and an exact filtered phrase is UnsupportedOperation with the opt-in off (c).
// tests/test_gpu_phrase_masked.py compares the lines with the rows of the unmasked queries on a twin segment.
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
static std::vector<int64_t> docs_of(const std::string& path) {
  std::vector<int64_t> out;
  std::ifstream f(path);
  long long d;
  while (f >> d) out.push_back(d);
  return out;
}
static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string part;
  while (std::getline(ss, part, sep)) out.push_back(part);
  return out;
}
static rucene::PhraseQuery phrase_of(const std::vector<std::string>& f, size_t at, int32_t slop = 0) {  // f[at] = terms, f[at + 1] = positions, f[at + 2] = boost
  std::vector<rucene::TermQuery> terms;
  std::vector<int32_t> positions;
  for (const std::string& t : split(f[at], ',')) terms.emplace_back(static_cast<int64_t>(std::atoll(t.c_str())));
  for (const std::string& p : split(f[at + 1], ',')) positions.push_back(std::atoi(p.c_str()));
  return rucene::PhraseQuery(std::move(terms), std::move(positions), static_cast<float>(std::atof(f[at + 2].c_str())), slop);
}
static rucene::TermQuery term_of(const std::vector<std::string>& f) { return rucene::TermQuery(static_cast<int64_t>(std::atoll(f[2].c_str()))); }

template <typename Fn>
static int refused(Fn&& fn) {
  try {
    fn();
  } catch (const rucene::Error& e) {
    return e.kind == RGPU_ERR_UNSUPPORTED ? 1 : 0;
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
    searcher.filtered_phrases = true;
    const CachedFilter F = searcher.filter_from_docs(docs_of(dir + "/f.txt")), X = searcher.filter_from_docs(docs_of(dir + "/x.txt"));

    std::vector<std::unique_ptr<Query>> inner, outer;
    std::vector<const Query*> batch;
    std::ifstream in(dir + "/queries.txt");
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      const std::vector<std::string> parts = split(line, ' ');
      const std::string &mode = parts[0], &kind = parts[1];
      if (kind == "p") {
        inner.emplace_back(new PhraseQuery(phrase_of(split(parts[2], ':'), 1)));
      } else if (kind == "b") {
        std::unique_ptr<PhraseBooleanQuery> q(new PhraseBooleanQuery());
        for (size_t i = 2; i < parts.size(); ++i) {
          const std::vector<std::string> f = split(parts[i], ':');
          if (f[1] == "p") {
            if (f[0] == "m") q->must(phrase_of(f, 2)); else q->filter(phrase_of(f, 2));
          } else {
            if (f[0] == "m") q->must(term_of(f)); else if (f[0] == "f") q->filter(term_of(f)); else q->must_not(term_of(f));
          }
        }
        inner.emplace_back(q.release());
      } else {
        std::unique_ptr<PhraseDisjunctionQuery> q(new PhraseDisjunctionQuery());
        q->min_should(std::atoi(kind.c_str() + 1));
        for (size_t i = 2; i < parts.size(); ++i) {
          const std::vector<std::string> f = split(parts[i], ':');
          if (f[1] == "p") q->should(phrase_of(f, 2));
          else if (f[0] == "s") q->should(term_of(f));
          else q->must_not(term_of(f));
        }
        inner.emplace_back(q.release());
      }
      const Query& q = *inner.back();
      if (mode == "un") { batch.push_back(&q); continue; }
      if (mode == "fq") outer.emplace_back(new FilteredQuery(FilteredQuery::filter_query(q, {F})));
      else if (mode == "cl") outer.emplace_back(new FilteredQuery(FilteredQuery::clauses(q, {F}, {X})));
      else if (mode == "cf") outer.emplace_back(new FilteredQuery(FilteredQuery::clauses(q, {F})));
      else outer.emplace_back(new FilteredQuery(FilteredQuery::clauses(q, {}, {X})));
      batch.push_back(outer.back().get());
    }
    const std::vector<TopDocs> got = searcher.search_many(batch, k);
    for (size_t i = 0; i < got.size(); ++i) {
      std::printf("row %zu %lld", i, (long long)got[i].total_hits());
      for (const ScoreDoc& d : got[i].score_docs()) {
        uint32_t bits;
        std::memcpy(&bits, &d.score, 4);
        std::printf(" %d:%08x", d.doc, bits);
      }
      std::printf("\n");
    }
    const PhraseQuery sloppy({TermQuery(int64_t(0)), TermQuery(int64_t(1))}, {}, 1.0f, 1), exact({TermQuery(int64_t(0)), TermQuery(int64_t(1))});
    PhraseDisjunctionQuery either;
    either.should(exact).should(TermQuery(int64_t(2)));
    const FilteredQuery fs = FilteredQuery::filter_query(sloppy, {F}), fe = FilteredQuery::filter_query(exact, {F}), fo = FilteredQuery::clauses(either, {F});
    const int a = refused([&] { searcher.search_many({&fs}, k); });
    const int b = refused([&] { searcher.search_many({&fo}, k); });
    searcher.filtered_phrases = false;
    const int c = refused([&] { searcher.search_many({&fe}, k); });
    std::printf("refused %d %d %d\n", a, b, c);
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
