// The C++ host mirror's MUST + SHOULD path over phrases (rucene_amd/csrc/host/gpu_index_searcher.hpp PhraseOptionalQuery ->
// rgpu_search_phrase_opt_batch, GpuIndexSearcher::optional_phrases) over a positions field handed over as raw files:
// <dir>/{doc,pos,norms,terms,tpos}.bin (terms = rgpu_term_state[], tpos = rgpu_term_positions[]), "<max_doc> <doc_count>
// <sum_total_term_freq> <k>" on the command line and the queries in <dir>/queries.txt, one per line, clauses separated by blanks:
//   msm:<n>                                                   min_should_match as given to BooleanQuery::build
//   m:t:<term>   f:t:<term>   s:t:<term>   n:t:<term>          a MUST / FILTER / SHOULD / MUST_NOT term clause
//   m:p:<t,t,..>:<pos,pos,..>:<boost>   f:p:...   s:p:...      a MUST / FILTER / SHOULD phrase clause
// A line that starts with "plain " holds one PhraseQuery (p:...) or TermQuery (t:<term>): the mixed batch keeps row order.
// Prints, for the whole batch in ONE search_many call:   row <i> <total_hits> <doc>:<score-bits> ...
// then "off <n>": how many of the rows a searcher WITHOUT optional_phrases refuses as UnsupportedOperation, and "fallback <n>": how
// many of a sloppy and a ten-clause query reach the CPU fallback. tests/test_gpu_phrase_opt.py compares the lines with the Python mirror's rows.
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
static rucene::PhraseQuery phrase_of(const std::vector<std::string>& f, size_t at) {  // f[at] = terms, f[at + 1] = positions, f[at + 2] = boost
  std::vector<rucene::TermQuery> terms;
  std::vector<int32_t> positions;
  for (const std::string& t : split(f[at], ',')) terms.emplace_back(static_cast<int64_t>(std::atoll(t.c_str())));
  for (const std::string& p : split(f[at + 1], ',')) positions.push_back(std::atoi(p.c_str()));
  return rucene::PhraseQuery(std::move(terms), std::move(positions), static_cast<float>(std::atof(f[at + 2].c_str())));
}

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc != 6) return 1;
  try {
    const std::string dir = argv[1];
    const std::vector<uint8_t> doc = slurp(dir + "/doc.bin"), pos = slurp(dir + "/pos.bin"), norms = slurp(dir + "/norms.bin"),
                               terms = slurp(dir + "/terms.bin"), tpos = slurp(dir + "/tpos.bin");
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
    const size_t k = static_cast<size_t>(std::atoi(argv[5]));
    leaf.terms = reinterpret_cast<const rgpu_term_state*>(terms.data());
    leaf.n_terms = static_cast<int64_t>(terms.size() / sizeof(rgpu_term_state));
    leaf.term_positions = reinterpret_cast<const rgpu_term_positions*>(tpos.data());
    GpuIndexSearcher searcher({leaf});
    searcher.optional_phrases = true;

    std::vector<std::unique_ptr<Query>> queries;
    std::ifstream in(dir + "/queries.txt");
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      const std::vector<std::string> clauses = split(line, ' ');
      if (clauses[0] == "plain") {
        const std::vector<std::string> f = split(clauses[1], ':');
        if (f[0] == "p") queries.emplace_back(new PhraseQuery(phrase_of(f, 1)));
        else queries.emplace_back(new TermQuery(static_cast<int64_t>(std::atoll(f[1].c_str()))));
        continue;
      }
      std::unique_ptr<PhraseOptionalQuery> q(new PhraseOptionalQuery());
      for (const std::string& c : clauses) {
        const std::vector<std::string> f = split(c, ':');
        if (f[0] == "msm") {
          q->min_should(std::atoi(f[1].c_str()));
        } else if (f[1] == "p") {
          if (f[0] == "m") q->must(phrase_of(f, 2)); else if (f[0] == "f") q->filter(phrase_of(f, 2)); else q->should(phrase_of(f, 2));
        } else {
          const TermQuery t(static_cast<int64_t>(std::atoll(f[2].c_str())));
          if (f[0] == "m") q->must(t); else if (f[0] == "f") q->filter(t); else if (f[0] == "s") q->should(t); else q->must_not(t);
        }
      }
      queries.emplace_back(q.release());
    }
    std::vector<const Query*> batch;
    for (auto& q : queries) batch.push_back(q.get());
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
    // with the flag off every such row is UnsupportedOperation, as it has been
    searcher.optional_phrases = false;
    int off = 0;
    for (const Query* q : batch) {
      if (!dynamic_cast<const PhraseOptionalQuery*>(q)) continue;
      try {
        searcher.search_many({q}, k);
      } catch (const rucene::Error& e) {
        off += e.kind == RGPU_ERR_UNSUPPORTED ? 1 : 0;
      }
    }
    std::printf("off %d\n", off);
    searcher.optional_phrases = true;
    // a sloppy clause and a tenth SHOULD clause are UnsupportedOperation and reach the CPU fallback with the query
    PhraseOptionalQuery sloppy, ten;
    sloppy.must(TermQuery(int64_t(2))).should(PhraseQuery({TermQuery(int64_t(0)), TermQuery(int64_t(1))}, {}, 1.0f, 1));
    ten.must(TermQuery(int64_t(2))).should(PhraseQuery({TermQuery(int64_t(0)), TermQuery(int64_t(1))}, {}, 1.0f, 0));
    for (int i = 0; i < 9; ++i) ten.should(TermQuery(int64_t(2)));
    const Query* seen = nullptr;
    searcher.cpu_fallback = [&](const Query& q, TopDocsCollector&) { seen = &q; };
    TopDocsCollector coll(k);
    int fell = 0;
    searcher.search(sloppy, coll);
    fell += seen == &sloppy ? 1 : 0;
    searcher.search(ten, coll);
    fell += seen == &ten ? 1 : 0;
    std::printf("fallback %d\n", fell);
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
