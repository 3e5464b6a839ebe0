// The host plan of rgpu_search_phrase_opt_batch (BooleanQuery of MUST / FILTER and SHOULD clauses with exact PhraseQuery clauses on
// either side: +a +b "a b", +"a b" c, +"a b" +c "b c" d -n #f): the decisions that can be wrong without a GPU, in plain C++17 with no
// device dependency (tests/cpp/phrase_opt_plan_test.cpp runs it under the sanitizers).
//   * the tree: BooleanWeight::create_scorer (boolean_query.rs:196-279) builds ReqOptScorer(must, DisjunctionSumScorer(should)), inside
//     a ReqNotScorer when MUST_NOT clauses exist in the leaf;
//   * the required side: must_weights - MUST clauses in query order, then FILTER clauses - go to ConjunctionScorer::new, which sorts
//     them by cost() with a stable sort (conjunction_scorer.rs:27-42) and sums their scores in that order (:87-95); a single required
//     clause is its own scorer. A term's cost is its doc_freq, an ExactPhraseScorer's the smallest doc_freq among its terms
//     (phrase_scorer.rs:270-272). req_phrase_slot[] says where among must_weights each required phrase sits;
//   * the candidate conjunction's clause list: the DISTINCT terms of all required phrases and required term clauses, rarest first,
//     and the distinct MUST_NOT terms the leaf holds;
//   * the optional side: the SHOULD scorers that exist in the leaf, in query order (disjunction_scorer.rs:211-225, the SimpleQueue arm
//     below ten children). opt_phrase_slot[] says where among should_weights each optional phrase sits. A term of doc_freq 0 and a
//     phrase that lacks a term drop out; with all of them gone the row is the required scorer's;
//   * the run capacities: the required run holds at most lead_df docs, an optional phrase's run at most its cost, an optional term's
//     its doc_freq;
//   * dead queries: a required clause absent from the leaf -> the leaf matches nothing.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../../include/rucene_gpu.h"

namespace rgpu_host {

constexpr int32_t PHRASE_OPT_MAX_SHOULD = 9;  // ten or more children: the heap-order arm (disjunction_scorer.rs:41-45)

// Two clauses name the same postings (PhraseQuery's Term equality, as the phrase planner tells repeated terms)
inline bool popt_same_term(const rgpu_term_state& a, const rgpu_term_state& b) {
  return a.doc_start_fp == b.doc_start_fp && a.doc_freq == b.doc_freq && a.singleton_doc_id == b.singleton_doc_id &&
         a.total_term_freq == b.total_term_freq;
}
inline int64_t popt_round_up_64(int64_t n) { return (n + 63) & ~(int64_t)63; }

struct PhraseOptPlan {
  int32_t status = RGPU_OK;  // RGPU_OK, RGPU_ERR_ILLEGAL_ARGUMENT or RGPU_ERR_UNSUPPORTED (then `why` says what, and nothing else is filled)
  const char* why = "";
  bool dead = false;         // a required clause is absent from the leaf: it matches nothing (nothing else is filled)
  // the required scorer's children in the order their scores are added: >= 0 = required term clause (index into the query's
  // required terms), < 0 = ~(required phrase index)
  std::vector<int32_t> req_order;
  std::vector<const rgpu_term_state*> conj;      // the candidate conjunction's clauses, rarest first (conj[0] leads it)
  std::vector<const rgpu_term_state*> must_not;  // the distinct MUST_NOT terms this leaf holds
  int32_t lead_df = 0;      // the required run's capacity
  int64_t plane_slots = 0;  // candidate slots of ONE plane: lead_df rounded up to a multiple of 64
  // the optional scorer's children that exist in this leaf, in the order their scores are added (query order): >= 0 = SHOULD term
  // clause (index into the query's optional terms), < 0 = ~(optional phrase index). Empty: no ReqOptScorer, the required scorer's row
  std::vector<int32_t> opt_order;
  std::vector<int32_t> opt_capacity;  // per optional phrase of the query: its run capacity (= cost), 0 when it dropped out
};

// The call's arrays with their lengths: every index range is checked here, before anything is read through it.
struct PhraseOptArrays {
  const rgpu_phrase_query* phrases;
  int32_t n_phrases_total;
  const rgpu_phrase_term* phrase_terms;
  int32_t n_phrase_terms_total;
  const rgpu_query_term* terms;
  int32_t n_terms_total;
};

inline PhraseOptPlan plan_phrase_opt(const rgpu_phrase_opt_query& Q, const PhraseOptArrays& a) {
  PhraseOptPlan P;
  auto refuse = [&](int32_t status, const char* why) { P = PhraseOptPlan{}; P.status = status; P.why = why; return P; };
  if (Q.n_req_phrases < 0 || Q.n_opt_phrases < 0 || Q.n_req_terms < 0 || Q.n_opt_terms < 0 || Q.n_must_not < 0)
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative clause count");
  if (Q.n_req_phrases > RGPU_MAX_BOOL_PHRASES || Q.n_opt_phrases > RGPU_MAX_BOOL_PHRASES)
    return refuse(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_BOOL_PHRASES phrases on one side of a MUST + SHOULD tree");
  if (Q.min_should_match < 0 || Q.min_should_match > 255) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "min_should_match outside 0..255");
  const int64_t n_req64 = (int64_t)Q.n_req_phrases + Q.n_req_terms, n_opt64 = (int64_t)Q.n_opt_phrases + Q.n_opt_terms;
  if (n_req64 < 1) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a MUST + SHOULD tree needs a required clause");
  if (n_opt64 < 1) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a MUST + SHOULD tree needs an optional clause");
  if (n_opt64 > PHRASE_OPT_MAX_SHOULD) return refuse(RGPU_ERR_UNSUPPORTED, "ten or more SHOULD clauses sum in heap order");
  const int64_t n_phr = (int64_t)Q.n_req_phrases + Q.n_opt_phrases;
  const int64_t n_trm = (int64_t)Q.n_req_terms + Q.n_opt_terms + Q.n_must_not;
  if (n_phr > 0 && (!a.phrases || !a.phrase_terms || Q.first_phrase < 0 || (int64_t)Q.first_phrase + n_phr > (int64_t)a.n_phrases_total))
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase range outside phrases[]");
  if (n_trm > 0 && (!a.terms || Q.first_term < 0 || (int64_t)Q.first_term + n_trm > (int64_t)a.n_terms_total))
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "clause range outside terms[]");
  if (n_req64 > RGPU_MAX_QUERY_TERMS) return refuse(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_QUERY_TERMS distinct terms in a MUST + SHOULD tree over phrases");
  const int n_req = (int)n_req64, n_opt = (int)n_opt64;
  for (int64_t i = 0; i < n_phr; ++i) {
    const rgpu_phrase_query& ph = a.phrases[Q.first_phrase + i];
    if (ph.n_terms < 2 || ph.n_terms > RGPU_MAX_PHRASE_TERMS) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a phrase has 2..RGPU_MAX_PHRASE_TERMS terms");
    if (ph.first_term < 0 || (int64_t)ph.first_term + ph.n_terms > (int64_t)a.n_phrase_terms_total)
      return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "term range outside terms[]");
    if (ph.slop < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "Slop must be >= 0");
  }
  // ---- must_weights and should_weights: which clause sits at each position
  auto place = [&](const int32_t* slot, int n_phrases, int n_clauses, std::vector<int32_t>* at_slot) -> const char* {
    at_slot->assign((size_t)n_clauses, INT32_MIN);
    for (int i = 0; i < n_phrases; ++i) {
      const int32_t s = slot[i];
      if (s < 0 || s >= n_clauses) return "a phrase slot outside its side's clauses";
      if ((*at_slot)[(size_t)s] != INT32_MIN) return "two phrases on one phrase slot";
      (*at_slot)[(size_t)s] = ~i;
    }
    for (int s = 0, t = 0; s < n_clauses; ++s) if ((*at_slot)[(size_t)s] == INT32_MIN) (*at_slot)[(size_t)s] = t++;
    return nullptr;
  };
  std::vector<int32_t> req_at, opt_at;
  if (const char* why = place(Q.req_phrase_slot, Q.n_req_phrases, n_req, &req_at)) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, why);
  if (const char* why = place(Q.opt_phrase_slot, Q.n_opt_phrases, n_opt, &opt_at)) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, why);
  for (int64_t i = 0; i < n_phr; ++i)
    if (a.phrases[Q.first_phrase + i].slop > 0) return refuse(RGPU_ERR_UNSUPPORTED, "a sloppy phrase inside a boolean query is not served");
  const rgpu_phrase_query* req_ph = n_phr > 0 ? a.phrases + Q.first_phrase : nullptr;
  const rgpu_phrase_query* opt_ph = n_phr > 0 ? req_ph + Q.n_req_phrases : nullptr;
  const rgpu_query_term* req_t = n_trm > 0 ? a.terms + Q.first_term : nullptr;
  const rgpu_query_term* opt_t = n_trm > 0 ? req_t + Q.n_req_terms : nullptr;
  const rgpu_query_term* not_t = n_trm > 0 ? opt_t + Q.n_opt_terms : nullptr;
  auto phrase_cost = [&](const rgpu_phrase_query& ph) {
    int64_t least = INT64_MAX;
    for (int i = 0; i < ph.n_terms; ++i) least = std::min<int64_t>(least, a.phrase_terms[ph.first_term + i].state.doc_freq);
    return least;
  };
  auto add_distinct = [](std::vector<const rgpu_term_state*>& list, const rgpu_term_state* st) {
    for (const rgpu_term_state* have : list) if (popt_same_term(*have, *st)) return;
    list.push_back(st);
  };
  // ---- the required side: costs (a clause absent from the leaf kills the query there), the distinct terms
  std::vector<int64_t> cost((size_t)n_req, 0);
  bool dead = false;
  std::vector<const rgpu_term_state*> conj, must_not, distinct;
  for (int s = 0; s < n_req; ++s) {
    const int32_t c = req_at[(size_t)s];
    cost[(size_t)s] = c >= 0 ? (int64_t)req_t[c].state.doc_freq : phrase_cost(req_ph[~c]);
    if (cost[(size_t)s] <= 0) dead = true;
    if (c >= 0) { add_distinct(conj, &req_t[c].state); continue; }
    for (int i = 0; i < req_ph[~c].n_terms; ++i) add_distinct(conj, &a.phrase_terms[req_ph[~c].first_term + i].state);
  }
  for (int i = 0; i < Q.n_must_not; ++i)
    if (not_t[i].state.doc_freq > 0) add_distinct(must_not, &not_t[i].state);
  // ---- the optional side: the clauses that exist here and their capacities
  std::vector<int32_t> opt_order, opt_capacity((size_t)Q.n_opt_phrases, 0);
  distinct = conj;
  for (const rgpu_term_state* st : must_not) add_distinct(distinct, st);
  for (int s = 0; s < n_opt; ++s) {
    const int32_t c = opt_at[(size_t)s];
    if (c >= 0) {
      if (opt_t[c].state.doc_freq <= 0) continue;
      add_distinct(distinct, &opt_t[c].state);
      opt_order.push_back(c);
      continue;
    }
    const rgpu_phrase_query& ph = opt_ph[~c];
    const int64_t least = phrase_cost(ph);
    if (least <= 0) continue;
    for (int i = 0; i < ph.n_terms; ++i) add_distinct(distinct, &a.phrase_terms[ph.first_term + i].state);
    opt_capacity[(size_t)~c] = (int32_t)least;
    opt_order.push_back(c);
  }
  // (before anything is kept: the limit refuses the query whole, dead in this leaf or not)
  if (distinct.size() > (size_t)RGPU_MAX_QUERY_TERMS || conj.size() + must_not.size() > (size_t)RGPU_MAX_QUERY_TERMS)
    return refuse(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_QUERY_TERMS distinct terms in a MUST + SHOULD tree over phrases");
  if (dead) { P.dead = true; return P; }
  std::stable_sort(conj.begin(), conj.end(), [](const rgpu_term_state* x, const rgpu_term_state* y) { return x->doc_freq < y->doc_freq; });
  // ---- the reference order of the required sum
  std::vector<int32_t> pos((size_t)n_req);
  for (int s = 0; s < n_req; ++s) pos[(size_t)s] = s;
  std::stable_sort(pos.begin(), pos.end(), [&](int32_t x, int32_t y) { return cost[(size_t)x] < cost[(size_t)y]; });
  P.req_order.reserve((size_t)n_req);
  for (int32_t s : pos) P.req_order.push_back(req_at[(size_t)s]);
  P.conj.swap(conj);
  P.must_not.swap(must_not);
  P.lead_df = P.conj[0]->doc_freq;
  P.plane_slots = popt_round_up_64(P.lead_df);
  P.opt_order.swap(opt_order);
  P.opt_capacity.swap(opt_capacity);
  return P;
}

}  // namespace rgpu_host
