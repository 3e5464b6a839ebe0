// The C++ host mirror's QueryRescorer with PhraseQuery rows (rucene_amd/csrc/host/gpu_index_searcher.hpp: rescore ->
// rgpu_rescore_phrase_batch) over a positions field handed over as raw files: <dir>/{doc,pos,norms,terms,tpos}.bin (terms =
// rgpu_term_state[], tpos = rgpu_term_positions[]), <dir>/rows.txt and "<max_doc> <doc_count> <sum_total_term_freq>" on the
// command line. rows.txt, one first-pass row and its request per line:
//   <kind> <slop> <n_terms> <term>... <mode> <query_weight> <rescore_weight> <window> <n_hits> <doc>:<score-bits>...
// kind: p = PhraseQuery, t = TermQuery (n_terms = 1), a = all-MUST BooleanQuery. Prints, per row,
//   rescore <i> <doc>:<score-bits> ...
// tests/test_gpu_phrase_rescore.py compares the lines with the Python mirror's rows.
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

int main(int argc, char** argv) {
  using namespace rucene;
  if (argc != 5) return 1;
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
    leaf.terms = reinterpret_cast<const rgpu_term_state*>(terms.data());
    leaf.n_terms = static_cast<int64_t>(terms.size() / sizeof(rgpu_term_state));
    leaf.term_positions = reinterpret_cast<const rgpu_term_positions*>(tpos.data());
    GpuIndexSearcher searcher({leaf});

    std::vector<std::unique_ptr<Query>> seconds;
    std::vector<RescoreRequest> reqs;
    std::vector<TopDocs> first;
    size_t k = 1;
    std::ifstream rows(dir + "/rows.txt");
    std::string line;
    while (std::getline(rows, line)) {
      if (line.empty()) continue;
      std::istringstream in(line);
      std::string kind;
      int slop = 0, n_terms = 0, mode = 0, window = 0, n_hits = 0;
      float qw = 1.0f, rw = 1.0f;
      in >> kind >> slop >> n_terms;
      std::vector<TermQuery> ts;
      for (int i = 0; i < n_terms; ++i) { long long t; in >> t; ts.emplace_back(t); }
      in >> mode >> qw >> rw >> window >> n_hits;
      std::vector<ScoreDoc> docs;
      for (int i = 0; i < n_hits; ++i) {
        std::string cell;
        in >> cell;
        const size_t colon = cell.find(':');
        const uint32_t bits = static_cast<uint32_t>(std::strtoul(cell.substr(colon + 1).c_str(), nullptr, 16));
        float score;
        std::memcpy(&score, &bits, 4);
        docs.push_back(ScoreDoc{std::atoi(cell.substr(0, colon).c_str()), score});
      }
      if (!in) return 3;
      if (kind == "p") seconds.emplace_back(new PhraseQuery(ts, {}, 1.0f, slop));
      else if (kind == "t") seconds.emplace_back(new TermQuery(ts[0]));
      else seconds.push_back(BooleanQuery::build(ts, {}));
      RescoreRequest r;
      r.query = seconds.back().get();
      r.query_weight = qw;
      r.rescore_weight = rw;
      r.mode = static_cast<rgpu_rescore_mode>(mode);
      r.window_size = window;
      reqs.push_back(r);
      k = std::max(k, docs.size());
      first.emplace_back(static_cast<int64_t>(docs.size()), std::move(docs));
    }
    const std::vector<TopDocs> pass2 = searcher.rescore(first, reqs, k);
    for (size_t i = 0; i < pass2.size(); ++i) {
      std::printf("rescore %zu", i);
      for (const ScoreDoc& d : pass2[i].score_docs()) {
        uint32_t bits;
        std::memcpy(&bits, &d.score, 4);
        std::printf(" %d:%08x", d.doc, bits);
      }
      std::printf("\n");
    }
  } catch (const rucene::Error& e) {
    std::fprintf(stderr, "rucene::Error kind=%d: %s\n", e.kind, e.what());
    return 2;
  }
  return 0;
}
