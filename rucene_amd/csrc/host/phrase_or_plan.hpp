// The host plan of rgpu_search_phrase_or_batch (BooleanQuery whose clauses are all SHOULD / MUST_NOT, exact PhraseQuery clauses among
// the SHOULD ones): the decisions that can be wrong without a GPU, in plain C++17 with no device dependency
// (tests/cpp/phrase_or_plan_test.cpp runs it under the sanitizers).
//   * the clause order: BooleanWeight::create_scorer (boolean_query.rs:217-234) hands the SHOULD scorers that exist in the leaf, in
//     query order, to ONE DisjunctionSumScorer; below ten children that is the SimpleQueue arm (disjunction_scorer.rs:41), which
//     adds a doc's children in that order (:213-225). phrase_slot[] says where among should_weights each phrase sits;
//   * which clauses exist in this leaf: a phrase with a term of doc_freq 0 has no scorer (phrase_query.rs:275-283), a term clause
//     of doc_freq 0 has none either — both drop out, min_should_match stays as it is (it then counts fewer children);
//   * dead queries: every SHOULD clause dropped -> no scorer at all (boolean_query.rs:274-276), the leaf matches nothing;
//   * each phrase's run capacity = its cost, the smallest doc_freq among its terms (phrase_scorer.rs:270-272): the candidate
//     conjunction is led by that term, so no more docs can match;
//   * the distinct MUST_NOT terms the leaf holds, and the limits.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../../include/rucene_gpu.h"

namespace rgpu_host {

constexpr int32_t PHRASE_OR_MAX_SHOULD = 9;  // ten or more children: the heap-order arm (disjunction_scorer.rs:41-45)

// Two clauses name the same postings (PhraseQuery's Term equality, as the phrase planner tells repeated terms)
inline bool po_same_term(const rgpu_term_state& a, const rgpu_term_state& b) {
  return a.doc_start_fp == b.doc_start_fp && a.doc_freq == b.doc_freq && a.singleton_doc_id == b.singleton_doc_id &&
         a.total_term_freq == b.total_term_freq;
}

struct PhraseOrPlan {
  int32_t status = RGPU_OK;  // RGPU_OK, RGPU_ERR_ILLEGAL_ARGUMENT or RGPU_ERR_UNSUPPORTED (then `why` says what, and nothing else is filled)
  const char* why = "";
  bool dead = false;         // no SHOULD clause exists in this leaf: it matches nothing (nothing else is filled)
  // DisjunctionSumScorer's children that exist in this leaf, in the order their scores are added (query order): >= 0 = SHOULD term
  // clause (index into the query's SHOULD terms), < 0 = ~(phrase index)
  std::vector<int32_t> order;
  std::vector<int32_t> capacity;                 // per phrase of the query: its run capacity (= cost), 0 when it dropped out
  std::vector<const rgpu_term_state*> must_not;  // the distinct MUST_NOT terms this leaf holds
  int32_t min_should_match = 0;                  // as given (0 and 1 collect the same docs)
};

// `phrases` / `phrase_terms` / `terms`: the call's arrays (index ranges already checked against their lengths).
inline PhraseOrPlan plan_phrase_or(const rgpu_phrase_or_query& Q, const rgpu_phrase_query* phrases, const rgpu_phrase_term* phrase_terms,
                                   const rgpu_query_term* terms) {
  PhraseOrPlan P;
  auto refuse = [&](int32_t status, const char* why) { P.status = status; P.why = why; return P; };
  if (Q.n_phrases < 1 || Q.n_phrases > RGPU_MAX_BOOL_PHRASES) return refuse(RGPU_ERR_UNSUPPORTED, "a disjunction over phrases holds 1..RGPU_MAX_BOOL_PHRASES phrases");
  if (Q.n_terms < 0 || Q.n_must_not < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative clause count");
  if (Q.min_should_match < 0 || Q.min_should_match > 255) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "min_should_match outside 0..255");
  const int64_t n_should64 = (int64_t)Q.n_phrases + Q.n_terms;
  if (n_should64 > PHRASE_OR_MAX_SHOULD) return refuse(RGPU_ERR_UNSUPPORTED, "ten or more SHOULD clauses with a phrase among them sum in heap order");
  const int n_should = (int)n_should64;
  // ---- should_weights: which clause sits at each position
  std::vector<int32_t> at_slot((size_t)n_should, INT32_MIN);
  for (int i = 0; i < Q.n_phrases; ++i) {
    const int32_t s = Q.phrase_slot[i];
    if (s < 0 || s >= n_should) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase_slot outside the SHOULD clauses");
    if (at_slot[(size_t)s] != INT32_MIN) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "two phrases on one phrase_slot");
    at_slot[(size_t)s] = ~i;
    if (phrases[Q.first_phrase + i].slop > 0) return refuse(RGPU_ERR_UNSUPPORTED, "a sloppy phrase inside a boolean query is not served");
  }
  for (int s = 0, t = 0; s < n_should; ++s) if (at_slot[(size_t)s] == INT32_MIN) at_slot[(size_t)s] = t++;
  const rgpu_query_term* mine = (int64_t)Q.n_terms + Q.n_must_not > 0 ? terms + Q.first_term : nullptr;
  // ---- the clauses that exist here, their capacities, the distinct terms
  std::vector<const rgpu_term_state*> distinct;
  auto add_distinct = [](std::vector<const rgpu_term_state*>& list, const rgpu_term_state* st) {
    for (const rgpu_term_state* have : list) if (po_same_term(*have, *st)) return false;
    list.push_back(st);
    return true;
  };
  std::vector<int32_t> order, capacity((size_t)Q.n_phrases, 0);
  for (int s = 0; s < n_should; ++s) {
    const int32_t c = at_slot[(size_t)s];
    if (c >= 0) {
      if (mine[c].state.doc_freq <= 0) continue;
      add_distinct(distinct, &mine[c].state);
      order.push_back(c);
      continue;
    }
    const rgpu_phrase_query& ph = phrases[Q.first_phrase + ~c];
    int64_t least = INT64_MAX;
    for (int i = 0; i < ph.n_terms; ++i) least = std::min<int64_t>(least, phrase_terms[ph.first_term + i].state.doc_freq);
    if (ph.n_terms < 1 || least <= 0) continue;
    for (int i = 0; i < ph.n_terms; ++i) add_distinct(distinct, &phrase_terms[ph.first_term + i].state);
    capacity[(size_t)~c] = (int32_t)least;
    order.push_back(c);
  }
  std::vector<const rgpu_term_state*> must_not;
  for (int i = 0; i < Q.n_must_not; ++i) {
    const rgpu_term_state* st = &mine[Q.n_terms + i].state;
    if (st->doc_freq <= 0) continue;
    if (add_distinct(must_not, st)) add_distinct(distinct, st);
  }
  // (the window kernel keeps one clause position per lane: SHOULD children and MUST_NOT terms together)
  if (distinct.size() > (size_t)RGPU_MAX_QUERY_TERMS || order.size() + must_not.size() > (size_t)RGPU_MAX_QUERY_TERMS)
    return refuse(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_QUERY_TERMS distinct terms in a disjunction over phrases");
  if (order.empty()) { P.dead = true; return P; }
  P.order.swap(order);
  P.capacity.swap(capacity);
  P.must_not.swap(must_not);
  P.min_should_match = Q.min_should_match;
  return P;
}

}  // namespace rgpu_host
