// The host plan of the doc-set entry points (rgpu_docset_from_words, rgpu_docset_collect_batch) and of the C++ mirror's filtered
// batches: the decisions that can be wrong without a GPU, in plain C++17 with no device dependency
// (tests/cpp/docset_plan_test.cpp runs it under the sanitizers).
//   * the words of a set: ceil(max_doc / 64) u64, no bit at or past max_doc (FixedBitSet's invariant) — from_words checks the last one;
//   * per query of collect_batch (the query cache's fill, search/cache/query_cache.rs:301-372 — nothing is scored, live docs are not
//     consulted): what is refused; which clauses exist in the leaf (a term of doc_freq 0 has no scorer: a MUST clause then kills the
//     conjunction, boolean_query.rs:201-207, a SHOULD or MUST_NOT clause drops out, :217-252); the DISTINCT terms; for a conjunction
//     the stable cost order ConjunctionScorer::new uses (conjunction_scorer.rs:30) — its first term leads the candidate search and
//     bounds the candidates;
//   * the (row, term, items) jobs of the list kernel, setting jobs apart from clearing jobs (the clearing launch runs behind);
//   * for the mirror: a mixed batch grouped by (filter sets, exclude sets) key, caller row order kept inside each group.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../../include/rucene_gpu.h"

namespace rgpu_host {

inline int64_t docset_word_count(int32_t max_doc) { return max_doc <= 0 ? 0 : ((int64_t)max_doc + 63) / 64; }
// the bits of the LAST word that stand for docs below max_doc (every bit when max_doc is a multiple of 64)
inline uint64_t docset_tail_mask(int32_t max_doc) { return (max_doc & 63) == 0 ? ~0ull : ((1ull << (max_doc & 63)) - 1ull); }
// rgpu_docset_from_words: false when a bit at or past max_doc is set (only the last word can hold one)
inline bool docset_words_valid(const uint64_t* words, int32_t max_doc) {
  const int64_t n = docset_word_count(max_doc);
  return n == 0 || (words[n - 1] & ~docset_tail_mask(max_doc)) == 0;
}

inline bool ds_same_term(const rgpu_term_state& a, const rgpu_term_state& b) {
  return a.doc_start_fp == b.doc_start_fp && a.doc_freq == b.doc_freq && a.singleton_doc_id == b.singleton_doc_id &&
         a.total_term_freq == b.total_term_freq;
}

struct DocsetQueryPlan {
  int32_t status = RGPU_OK;  // RGPU_OK, RGPU_ERR_ILLEGAL_ARGUMENT or RGPU_ERR_UNSUPPORTED (then `why` says what, and nothing else is filled)
  const char* why = "";
  bool dead = false;         // matches nothing in this leaf: the empty set (nothing else is filled)
  bool conjunction = false;  // `positive` is conjoined (k_search_and in emit mode, which also removes `negative`); else: united, bit by bit
  std::vector<const rgpu_term_state*> positive;  // distinct terms the leaf holds; a conjunction's in stable cost order (the first leads)
  std::vector<const rgpu_term_state*> negative;  // distinct MUST_NOT terms the leaf holds
};

// `terms`: the call's array of n_terms_total clauses.
inline DocsetQueryPlan plan_docset_query(const rgpu_query& Q, const rgpu_query_term* terms, int64_t n_terms_total) {
  DocsetQueryPlan P;
  auto refuse = [&](int32_t status, const char* why) { P.status = status; P.why = why; return P; };
  const int32_t op = Q.op & 0xff, msm = (Q.op >> 8) & 0xff;
  if (op != RGPU_OP_TERM && op != RGPU_OP_AND && op != RGPU_OP_OR) return refuse(RGPU_ERR_UNSUPPORTED, "a doc set is collected from RGPU_OP_TERM, RGPU_OP_AND or RGPU_OP_OR");
  if (((uint32_t)Q.op >> 16) != 0u) return refuse(RGPU_ERR_UNSUPPORTED, "a doc set is collected from flat queries: no RGPU_OP_WITH_SHOULD, no nested clauses");
  if (msm >= 2) return refuse(RGPU_ERR_UNSUPPORTED, "a doc set is collected with min_should_match <= 1");
  if (((uint32_t)Q.n_must_not >> 16) != 0u) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "n_must_not: bits 16 and up must be zero");
  if (((Q.n_must_not >> 8) & 0xff) != 0) return refuse(RGPU_ERR_UNSUPPORTED, "a doc set is collected without demoting clauses");
  const int32_t n_not = Q.n_must_not & 0xff;
  const int32_t min_terms = (op == RGPU_OP_OR && n_not > 0) ? 0 : 1;  // (an OR of MUST_NOT clauses only has no scorer: the empty set)
  if (Q.n_terms < min_terms || Q.n_terms > RGPU_MAX_QUERY_TERMS || Q.n_terms + n_not > RGPU_MAX_QUERY_TERMS || (op == RGPU_OP_TERM && Q.n_terms != 1))
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "bad clause count");
  if (Q.first_term < 0 || (int64_t)Q.first_term + Q.n_terms + n_not > n_terms_total) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "clause range outside terms[]");
  const rgpu_query_term* mine = terms + Q.first_term;
  auto add_distinct = [](std::vector<const rgpu_term_state*>& list, const rgpu_term_state* st) {
    for (const rgpu_term_state* have : list) if (ds_same_term(*have, *st)) return false;
    list.push_back(st);
    return true;
  };
  const bool required = op != RGPU_OP_OR;
  std::vector<const rgpu_term_state*> positive, negative;
  for (int i = 0; i < Q.n_terms; ++i) {
    const rgpu_term_state* st = &mine[i].state;
    if (st->doc_freq < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative doc_freq");
    if (st->doc_freq == 0) {
      if (required) { P.dead = true; return P; }
      continue;
    }
    add_distinct(positive, st);
  }
  if (positive.empty()) { P.dead = true; return P; }
  for (int i = 0; i < n_not; ++i) {
    const rgpu_term_state* st = &mine[Q.n_terms + i].state;
    if (st->doc_freq < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative doc_freq");
    if (st->doc_freq == 0) continue;
    if (required) for (const rgpu_term_state* p : positive) if (ds_same_term(*p, *st)) { P.dead = true; return P; }  // +a -a
    add_distinct(negative, st);
  }
  P.conjunction = op == RGPU_OP_AND && positive.size() >= 2;
  if (P.conjunction) std::stable_sort(positive.begin(), positive.end(), [](const rgpu_term_state* a, const rgpu_term_state* b) { return a->doc_freq < b->doc_freq; });
  P.positive.swap(positive);
  P.negative.swap(negative);
  return P;
}

// Work items of one term in the list kernel: chunks of `blocks_per_item` 128-posting blocks; the last one also takes the VInt tail
// (a list without a full block, a singleton included, is one item)
inline int64_t docset_term_items(int32_t doc_freq, int blocks_per_item) {
  const int64_t nblocks = doc_freq >= 2 ? doc_freq / 128 : 0;
  return nblocks == 0 ? 1 : (nblocks + blocks_per_item - 1) / blocks_per_item;
}

struct DocsetListJob {
  int32_t row;                   // the query (= output set) the bits go to
  const rgpu_term_state* term;
  int64_t first_item, n_items;   // [first_item, first_item + n_items) of its launch
};
struct DocsetJobs {
  std::vector<DocsetListJob> set, clear;  // two launches: every setting job, then every clearing job
  int64_t set_items = 0, clear_items = 0;
};
// the jobs of the queries that are united bit by bit (TERM, OR, one-clause AND); conjunctions' and dead queries' rows get none
inline DocsetJobs plan_docset_jobs(const std::vector<DocsetQueryPlan>& plans, int blocks_per_item) {
  DocsetJobs J;
  for (size_t q = 0; q < plans.size(); ++q) {
    const DocsetQueryPlan& P = plans[q];
    if (P.status != RGPU_OK || P.dead || P.conjunction) continue;
    for (const rgpu_term_state* st : P.positive) {
      const int64_t n = docset_term_items(st->doc_freq, blocks_per_item);
      J.set.push_back(DocsetListJob{(int32_t)q, st, J.set_items, n});
      J.set_items += n;
    }
    for (const rgpu_term_state* st : P.negative) {
      const int64_t n = docset_term_items(st->doc_freq, blocks_per_item);
      J.clear.push_back(DocsetListJob{(int32_t)q, st, J.clear_items, n});
      J.clear_items += n;
    }
  }
  return J;
}

// ---- the mirror's filtered batches --------------------------------------------------------------------------------------------
// A query's doc-set clauses as ids of cached filters (any caller-chosen ids): FILTER sets and MUST_NOT sets. The order of the sets
// inside a side does not matter and repeats do not either (an intersection / a union), so a key is kept sorted and distinct.
struct DocsetKey {
  std::vector<uint64_t> filters, excludes;
  bool empty() const { return filters.empty() && excludes.empty(); }
  bool operator==(const DocsetKey& o) const { return filters == o.filters && excludes == o.excludes; }
};
inline DocsetKey docset_key(std::vector<uint64_t> filters, std::vector<uint64_t> excludes) {
  auto norm = [](std::vector<uint64_t>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
  norm(filters);
  norm(excludes);
  return DocsetKey{std::move(filters), std::move(excludes)};
}
struct DocsetGroup {
  DocsetKey key;
  std::vector<int32_t> rows;  // caller rows of this key, ascending
};
// groups in order of first appearance; every caller row is in exactly one group (the unfiltered rows share the empty key)
inline std::vector<DocsetGroup> group_by_docset_key(const std::vector<DocsetKey>& keys) {
  std::vector<DocsetGroup> groups;
  for (size_t r = 0; r < keys.size(); ++r) {
    size_t g = 0;
    while (g < groups.size() && !(groups[g].key == keys[r])) ++g;
    if (g == groups.size()) groups.push_back(DocsetGroup{keys[r], {}});
    groups[g].rows.push_back((int32_t)r);
  }
  return groups;
}

}  // namespace rgpu_host
