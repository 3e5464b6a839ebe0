// The C++ host mirror's cached filters (rucene_amd/csrc/host/gpu_index_searcher.hpp: CachedFilter, FilteredQuery, cache_filter,
// filter_from_docs, filter_from_bits) over docs-and-freqs leaves handed over as raw files: <dir>/leaf<i>/{doc,norms,terms,live}.bin
// (terms = rgpu_term_state[], the vocabulary of tests/segment_spectrum.py; live.bin empty = no deletions) and, on the command line,
// "<dir> <n_leaves>" followed by "<max_doc> <sum_total_term_freq>" per leaf. Prints
//   cardinality <cache_filter> <filter_from_docs> <filter_from_bits>
//   docset <i> <total_hits> <doc>:<score-bits> ...
// for a mixed batch through search_many (rows of four combinations of sets beside unfiltered rows) and, for the last line, row 0 through
// search() with a collector; then checks that the shapes the GPU path does not serve reach the cpu_fallback hook.
// tests/test_gpu_docset_mirror.py compares the lines with the Python mirror's rows on the same leaves.
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
static void print_line(size_t i, const rucene::TopDocs& top) {
  std::printf("docset %zu %lld", i, (long long)top.total_hits());
  for (const rucene::ScoreDoc& d : top.score_docs()) {
    uint32_t bits;
    std::memcpy(&bits, &d.score, 4);
    std::printf(" %d:%08x", d.doc, bits);
  }
  std::printf("\n");
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
    // ---- three ways to the same filter, and two more filters
    const TermQuery even(static_cast<int64_t>(EVEN)), fifth(static_cast<int64_t>(FIFTH));
    const CachedFilter f = searcher.cache_filter(even);
    const CachedFilter x = searcher.cache_filter(fifth);
    const std::unique_ptr<Query> some_or_last = BooleanQuery::build({}, T({SOMETIMES, LAST}), 0, T({FIRST}));
    const CachedFilter f2 = searcher.cache_filter(*some_or_last);
    std::vector<int64_t> even_docs;
    std::vector<std::vector<uint64_t>> even_words;
    std::vector<const uint64_t*> even_ptrs;
    for (const LeafReader& l : leaves) {
      even_words.emplace_back(static_cast<size_t>((l.max_doc + 63) / 64), 0ull);
      for (int32_t d = l.max_doc - 1; d >= 0; --d)
        if (d % 2 == 0) {   // EVEN: every second doc; handed over in descending order, some of them twice
          even_docs.push_back(l.doc_base + d);
          if (d % 6 == 0) even_docs.push_back(l.doc_base + d);
          even_words.back()[static_cast<size_t>(d >> 6)] |= 1ull << (d & 63);
        }
    }
    for (const auto& w : even_words) even_ptrs.push_back(w.data());
    const CachedFilter by_docs = searcher.filter_from_docs(even_docs);
    const CachedFilter by_bits = searcher.filter_from_bits(even_ptrs);
    std::printf("cardinality %lld %lld %lld\n", (long long)searcher.filter_cardinality(f), (long long)searcher.filter_cardinality(by_docs),
                (long long)searcher.filter_cardinality(by_bits));

    // ---- a mixed batch: four combinations of sets and unfiltered rows, not grouped
    const TermQuery every(static_cast<int64_t>(EVERY)), constant(static_cast<int64_t>(CONST));
    const std::unique_ptr<Query> and2 = BooleanQuery::build(T({EVERY, CONST}), {});
    const std::unique_ptr<Query> or3 = BooleanQuery::build({}, T({FIRST, LAST, SOMETIMES}));
    const std::unique_ptr<Query> opt = BooleanQuery::build(T({EVERY}), T({LAST, SOMETIMES}));
    const DisjunctionMaxQuery dismax(T({EVEN, FIFTH, LAST}), 0.3f);
    std::vector<FilteredQuery> fq;
    fq.push_back(FilteredQuery::clauses(every, {f}));                   // 0: +every #F
    fq.push_back(FilteredQuery::clauses(*and2, {f}, {x}));              // 2: +every +const #F -X
    fq.push_back(FilteredQuery::filter_query(*or3, {by_docs}));         // 3: FilterQuery(first last sometimes, F)
    fq.push_back(FilteredQuery::clauses(even, {}, {x}));                // 4: +even -X
    fq.push_back(FilteredQuery::filter_query(every, {by_bits, f2}));    // 5: two filters
    fq.push_back(FilteredQuery::filter_query(dismax, {f}));             // 6
    fq.push_back(FilteredQuery::clauses(*opt, {f}, {x}));               // 8: MUST + SHOULD beside the sets
    fq.push_back(FilteredQuery::clauses(every, {f, f}));                // 9: the key of row 0, spelt twice
    const std::vector<const Query*> batch = {&fq[0], &constant, &fq[1], &fq[2], &fq[3], &fq[4], &fq[5], or3.get(), &fq[6], &fq[7]};
    const std::vector<TopDocs> rows = searcher.search_many(batch, 10);
    for (size_t i = 0; i < rows.size(); ++i) print_line(i, rows[i]);
    TopDocsCollector collector(10);
    searcher.search(fq[0], collector);
    print_line(rows.size(), collector.top_docs());

    // ---- what is not equivalent reaches the CPU path
    int fallen = 0;
    searcher.cpu_fallback = [&](const Query&, TopDocsCollector&) { ++fallen; };
    const PhraseQuery phrase(T({EVERY, EVEN}));
    const FilteredQuery refused[] = {FilteredQuery::clauses(*or3, {f}),               // b c #F
                                     FilteredQuery::clauses(*or3, {}, {x}),           // no required clause of its own
                                     FilteredQuery::filter_query(phrase, {f}),        // a filtered phrase
                                     FilteredQuery::clauses(phrase, {f})};
    for (const FilteredQuery& q : refused) searcher.search(q, collector);
    if (fallen != 4) { std::printf("cpu_fallback reached %d times, not 4\n", fallen); return 1; }
    searcher.drop_filter(by_docs);
    bool gone = false;
    try { searcher.search_many({&fq[2]}, 10); } catch (const Error& e) { gone = e.kind == RGPU_ERR_ILLEGAL_ARGUMENT; }
    if (!gone) { std::printf("a dropped filter was still served\n"); return 1; }
    std::printf("fallback ok\n");
  } catch (const rucene::Error& e) {
    std::printf("error %d: %s\n", e.kind, e.what());
    return 1;
  }
  return 0;
}
