// The host plan of rgpu_search_phrase_bool_batch (BooleanQuery with exact PhraseQuery clauses among its required clauses): the
// decisions that can be wrong without a GPU, in plain C++17 with no device dependency (tests/cpp/phrase_bool_plan_test.cpp runs it
// under the sanitizers).
//   * the reference order: BooleanWeight::create_scorer (boolean_query.rs:196-279) hands must_weights — MUST clauses in query
//     order, then FILTER clauses — to ConjunctionScorer::new, which sorts them by cost() with a stable sort
//     (conjunction_scorer.rs:27-42) and sums their scores in that order (:87-95). A term's cost is its doc_freq in the leaf, an
//     ExactPhraseScorer's the smallest doc_freq among its terms (phrase_scorer.rs:270-272);
//   * the candidate conjunction's clause list: the DISTINCT terms of all phrases and required term clauses, rarest first
//     (+"a b" +a and +"a b" +"b c" must not hand the conjunction a term twice), and the distinct MUST_NOT terms the leaf holds;
//   * the slot layout: n_phrases planes of round_up(lead doc_freq, 64) slots, slot i of every plane the same candidate;
//   * dead queries: a phrase term or a required term absent from the leaf -> the leaf matches nothing.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../../include/rucene_gpu.h"

namespace rgpu_host {

// Two clauses name the same postings (PhraseQuery's Term equality, as the phrase planner tells repeated terms): a conjunction over
// both is the conjunction over one.
inline bool pb_same_term(const rgpu_term_state& a, const rgpu_term_state& b) {
  return a.doc_start_fp == b.doc_start_fp && a.doc_freq == b.doc_freq && a.singleton_doc_id == b.singleton_doc_id &&
         a.total_term_freq == b.total_term_freq;
}

struct PhraseBoolPlan {
  int32_t status = RGPU_OK;  // RGPU_OK, RGPU_ERR_ILLEGAL_ARGUMENT or RGPU_ERR_UNSUPPORTED (then `why` says what, and nothing else is filled)
  const char* why = "";
  bool dead = false;         // the leaf matches nothing (nothing else is filled)
  // ConjunctionScorer's children in the order their scores are added: >= 0 = required term clause (index into the query's
  // required terms), < 0 = ~(phrase index)
  std::vector<int32_t> order;
  std::vector<const rgpu_term_state*> conj;      // the candidate conjunction's clauses, rarest first (conj[0] leads it)
  std::vector<const rgpu_term_state*> must_not;  // the distinct MUST_NOT terms this leaf holds
  int32_t lead_df = 0;
  int64_t plane_slots = 0;  // slots of ONE plane: lead_df rounded up to a multiple of 64 (a 64-slot group belongs to one query)
};

inline int64_t pb_round_up_64(int64_t n) { return (n + 63) & ~(int64_t)63; }

// `phrases` / `phrase_terms` / `terms`: the call's arrays (index ranges already checked against their lengths).
inline PhraseBoolPlan plan_phrase_bool(const rgpu_phrase_bool_query& Q, const rgpu_phrase_query* phrases, const rgpu_phrase_term* phrase_terms,
                                       const rgpu_query_term* terms) {
  PhraseBoolPlan P;
  auto refuse = [&](int32_t status, const char* why) { P.status = status; P.why = why; return P; };
  if (Q.n_phrases < 1 || Q.n_phrases > RGPU_MAX_BOOL_PHRASES) return refuse(RGPU_ERR_UNSUPPORTED, "a boolean query over phrases holds 1..RGPU_MAX_BOOL_PHRASES phrases");
  if (Q.n_terms < 0 || Q.n_must_not < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative clause count");
  const int n_req = Q.n_phrases + Q.n_terms;
  // ---- must_weights: which clause sits at each position
  std::vector<int32_t> at_slot((size_t)n_req, INT32_MIN);
  for (int i = 0; i < Q.n_phrases; ++i) {
    const int32_t s = Q.phrase_slot[i];
    if (s < 0 || s >= n_req) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase_slot outside the required clauses");
    if (at_slot[(size_t)s] != INT32_MIN) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "two phrases on one phrase_slot");
    at_slot[(size_t)s] = ~i;
    if (phrases[Q.first_phrase + i].slop > 0) return refuse(RGPU_ERR_UNSUPPORTED, "a sloppy phrase inside a boolean query is not served");
  }
  for (int s = 0, t = 0; s < n_req; ++s) if (at_slot[(size_t)s] == INT32_MIN) at_slot[(size_t)s] = t++;
  const rgpu_query_term* req = Q.n_terms + Q.n_must_not > 0 ? terms + Q.first_term : nullptr;
  // ---- costs; a clause absent from the leaf kills the query there
  std::vector<int64_t> cost((size_t)n_req, 0);
  for (int s = 0; s < n_req; ++s) {
    const int32_t c = at_slot[(size_t)s];
    if (c >= 0) {
      cost[(size_t)s] = req[c].state.doc_freq;
    } else {
      const rgpu_phrase_query& ph = phrases[Q.first_phrase + ~c];
      int64_t least = INT64_MAX;
      for (int i = 0; i < ph.n_terms; ++i) least = std::min<int64_t>(least, phrase_terms[ph.first_term + i].state.doc_freq);
      cost[(size_t)s] = least;
    }
    if (cost[(size_t)s] <= 0) { P.dead = true; return P; }
  }
  // ---- the distinct terms (before anything is kept: the limit refuses the query whole)
  auto add_distinct = [](std::vector<const rgpu_term_state*>& list, const rgpu_term_state* st) {
    for (const rgpu_term_state* have : list) if (pb_same_term(*have, *st)) return;
    list.push_back(st);
  };
  for (int s = 0; s < n_req; ++s) {
    const int32_t c = at_slot[(size_t)s];
    if (c >= 0) { add_distinct(P.conj, &req[c].state); continue; }
    const rgpu_phrase_query& ph = phrases[Q.first_phrase + ~c];
    for (int i = 0; i < ph.n_terms; ++i) add_distinct(P.conj, &phrase_terms[ph.first_term + i].state);
  }
  for (int i = 0; i < Q.n_must_not; ++i)
    if (req[Q.n_terms + i].state.doc_freq > 0) add_distinct(P.must_not, &req[Q.n_terms + i].state);
  if (P.conj.size() + P.must_not.size() > (size_t)RGPU_MAX_QUERY_TERMS) {
    P.conj.clear();
    P.must_not.clear();
    return refuse(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_QUERY_TERMS distinct terms in a boolean query over phrases");
  }
  std::stable_sort(P.conj.begin(), P.conj.end(), [](const rgpu_term_state* a, const rgpu_term_state* b) { return a->doc_freq < b->doc_freq; });
  // ---- the reference order
  std::vector<int32_t> pos((size_t)n_req);
  for (int s = 0; s < n_req; ++s) pos[(size_t)s] = s;
  std::stable_sort(pos.begin(), pos.end(), [&](int32_t a, int32_t b) { return cost[(size_t)a] < cost[(size_t)b]; });
  P.order.reserve((size_t)n_req);
  for (int32_t s : pos) P.order.push_back(at_slot[(size_t)s]);
  P.lead_df = P.conj[0]->doc_freq;
  P.plane_slots = pb_round_up_64(P.lead_df);
  return P;
}

}  // namespace rgpu_host
