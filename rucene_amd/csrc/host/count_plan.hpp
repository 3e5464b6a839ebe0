// The host plan of rgpu_count_batch (IndexSearcher::count, search/searcher.rs:632-654: a TotalHitCountCollector, needs_scores false)
// and of the mirrors' count(): the decisions that can be wrong without a GPU, in plain C++17 with no device dependency
// (tests/cpp/count_plan_test.cpp runs it under the sanitizers). It shares docset_plan.hpp's helpers.
// Per row: what is refused (the checks of rgpu_search_batch, less the ones on `weight` and `sim_table`, which a count ignores);
// which clauses exist in the leaf; and which of five kinds answers it:
//   ZERO      the reference builds no scorer, or one that can match nothing (boolean_query.rs:196-275): a MUST clause the leaf
//             lacks, no SHOULD clause left, fewer SHOULD clauses left than min_should_match, `+a -a`, a demoting side without a
//             posting in the leaf (boosting_query.rs:102-118) - and every row when the mask is an explicit empty set
//   DOC_FREQ  a lone present positive term, nothing present to exclude, no deletions, no set: its doc_freq (searcher.rs:640-648)
//   LIST      the same lone term under deletions or a set: its list is decoded and counted against the mask
//   CONJ      two or more distinct present MUST terms (stable cost order, conjunction_scorer.rs:30), MUST_NOT terms excluded one by one
//   WINDOWS   everything else: doc-id windows in which clauses are united or counted against the thresholds `need` / `need_not`
// min_should_match counts CLAUSES (a repeated term counts once per clause), so WINDOWS clauses carry a multiplicity.
#pragma once
#include <cstring>
#include <vector>

#include "docset_plan.hpp"

namespace rgpu_host {

enum CountKind : int32_t { COUNT_ZERO = 0, COUNT_DOC_FREQ = 1, COUNT_LIST = 2, COUNT_CONJ = 3, COUNT_WINDOWS = 4 };

struct CountClause {
  const rgpu_term_state* term;
  int32_t mult;  // clauses of the row that name this term
};

struct CountRowPlan {
  int32_t status = RGPU_OK;  // RGPU_OK, RGPU_ERR_ILLEGAL_ARGUMENT or RGPU_ERR_UNSUPPORTED (then `why` says what, and nothing else is filled)
  const char* why = "";
  CountKind kind = COUNT_ZERO;
  int64_t doc_freq = 0;                // DOC_FREQ: the answer
  std::vector<CountClause> positive;   // LIST: the one term; CONJ: distinct, stable cost order (the first leads); WINDOWS: distinct, clause order
  std::vector<CountClause> negative;   // CONJ / WINDOWS: the distinct present MUST_NOT terms
  int32_t need = 1;                    // WINDOWS: a doc stands when at least `need` positive clauses hold it ...
  int32_t need_not = 1;                // ... and fewer than `need_not` negative ones (always 1: see plan_count_query)
  bool bit_form() const { return need == 1 && need_not == 1; }
};

// what decides between DOC_FREQ and LIST, and the rule that goes before every other one
struct CountMask {
  bool deletions = false;  // the segment has live docs
  bool set = false;        // the call has a doc set
  bool empty_set = false;  // ... of cardinality 0
};

inline void count_add_clause(std::vector<CountClause>& list, const rgpu_term_state* st) {
  for (CountClause& have : list) if (ds_same_term(*have.term, *st)) { ++have.mult; return; }
  list.push_back(CountClause{st, 1});
}

// `terms`: the call's array of n_terms_total clauses.
inline CountRowPlan plan_count_query(const rgpu_query& Q, const rgpu_query_term* terms, int64_t n_terms_total, const CountMask& mask) {
  CountRowPlan P;
  auto refuse = [&](int32_t status, const char* why) { P.status = status; P.why = why; return P; };
  const int32_t NESTED = RGPU_OP_SHOULD_REQUIRED | RGPU_OP_NESTED_MUST;
  const int32_t op = Q.op & 0xff, msm = (Q.op >> 8) & 0xff, opt = (Q.op >> 16) & 0xff;
  // ---- malformed rows: what rgpu_search_batch checks, in its order
  if (op < RGPU_OP_TERM || op > RGPU_OP_DISMAX || (Q.op & ~(0xffffff | NESTED | RGPU_OP_NESTED_AT(63))) != 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "unknown query op");
  int32_t n_not = 0, n_demote = 0;
  if (op == RGPU_OP_DISMAX) {
    if ((Q.op & ~0xff) != 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "RGPU_OP_DISMAX takes no min_should_match, optional-clause or nesting bits");
    float tie;
    std::memcpy(&tie, &Q.n_must_not, sizeof tie);
    if (!(tie - tie == 0.0f)) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "RGPU_OP_DISMAX: n_must_not holds the bits of a finite f32 tie_breaker_multiplier");
  } else {
    if (((uint32_t)Q.n_must_not >> 16) != 0u) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "n_must_not: a MUST_NOT count, or RGPU_NOT_WITH_DEMOTE(n_not, n_demote) - bits 16 and up are zero");
    n_not = Q.n_must_not & 0xff;
    n_demote = (Q.n_must_not >> 8) & 0xff;
  }
  const int32_t behind = n_not + n_demote;
  if (n_demote > 0 && (opt != 0 || (Q.op & NESTED) != 0))
    return refuse(RGPU_ERR_UNSUPPORTED, "demoting clauses go with TERM, AND and OR positives, not with optional or nested clauses");
  if (((uint32_t)Q.op >> 26) != 0 && (!(Q.op & NESTED) || (int32_t)((uint32_t)Q.op >> 26) > Q.n_terms))
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "RGPU_OP_NESTED_AT goes with RGPU_OP_SHOULD_REQUIRED / RGPU_OP_NESTED_MUST: 0 .. n_terms");
  if ((Q.op & RGPU_OP_SHOULD_REQUIRED) && (op == RGPU_OP_OR || opt < 1))
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "RGPU_OP_SHOULD_REQUIRED goes with RGPU_OP_WITH_SHOULD(TERM / AND, n >= 1)");
  if ((Q.op & RGPU_OP_NESTED_MUST) && (op == RGPU_OP_OR || opt < 2 || (Q.op & RGPU_OP_SHOULD_REQUIRED)))
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "RGPU_OP_NESTED_MUST goes with RGPU_OP_WITH_SHOULD(TERM / AND, n >= 2) and without RGPU_OP_SHOULD_REQUIRED");
  if (msm > 1 && op != RGPU_OP_OR && opt == 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "min_should_match needs SHOULD clauses");
  if (opt > 0 && op == RGPU_OP_OR) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "optional SHOULD clauses go with MUST clauses (op TERM / AND)");
  const int32_t min_terms = (op == RGPU_OP_OR && behind > 0) ? 0 : 1;  // (an OR of MUST_NOT clauses only has no scorer)
  if (Q.n_terms < min_terms || Q.n_terms > RGPU_MAX_QUERY_TERMS || Q.n_terms + opt + behind > RGPU_MAX_QUERY_TERMS || (op == RGPU_OP_TERM && Q.n_terms != 1))
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "bad clause count");
  if (Q.first_term < 0 || (int64_t)Q.first_term + Q.n_terms + opt + behind > n_terms_total) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "clause range outside terms[]");
  const rgpu_query_term* mine = terms + Q.first_term;
  for (int i = 0; i < Q.n_terms + opt + behind; ++i)
    if (mine[i].state.doc_freq < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative doc_freq");
  // ---- trees a count does not serve
  if (Q.op & NESTED) return refuse(RGPU_ERR_UNSUPPORTED, "a count is taken of flat queries: no RGPU_OP_SHOULD_REQUIRED, no RGPU_OP_NESTED_MUST");
  // ---- the kind
  auto zero = [&]() { P.positive.clear(); P.negative.clear(); P.kind = COUNT_ZERO; P.need = P.need_not = 1; return P; };
  if (mask.empty_set) return P;  // ZERO
  const bool required = op == RGPU_OP_TERM || op == RGPU_OP_AND;
  int32_t pos_clauses = 0;
  for (int i = 0; i < Q.n_terms; ++i) {
    const rgpu_term_state* st = &mine[i].state;
    if (st->doc_freq == 0) {
      if (required) return zero();  // a MUST clause the leaf lacks
      continue;                // a SHOULD clause the leaf lacks drops out; min_should_match stays
    }
    count_add_clause(P.positive, st);
    ++pos_clauses;
  }
  if (P.positive.empty()) return zero();
  // (the optional clauses of RGPU_OP_WITH_SHOULD, mine[n_terms .. n_terms + opt), never change which docs match: skipped)
  const rgpu_query_term* nots = mine + Q.n_terms + opt;
  int32_t not_clauses = 0;
  for (int i = 0; i < n_not; ++i) {
    if (nots[i].state.doc_freq == 0) continue;
    count_add_clause(P.negative, &nots[i].state);
    ++not_clauses;
  }
  if (n_demote > 0) {  // BoostingQuery: no scorer in a leaf where the negative query has none
    bool any = false;
    for (int i = 0; i < n_demote; ++i) any = any || nots[n_not + i].state.doc_freq > 0;
    if (!any) return zero();
  }
  // One present MUST_NOT clause excludes its docs. Two or more are a DisjunctionSumScorer(.., false, min_should_match)
  // (boolean_query.rs:235-252), but ReqNotScorer only ever advance()s it (req_not_scorer.rs:47-78) and advance() does not look at
  // the count (disjunction_scorer.rs:75-89: only approximate_next does): a doc is excluded where ANY present MUST_NOT clause holds
  // it, whatever min_should_match says - which is what rgpu_search_batch's totals and the oracle say too. need_not stays 1.
  P.need_not = 1;
  (void)not_clauses;
  if (required) {
    P.need = (int32_t)P.positive.size();  // every distinct term
    for (const CountClause& n : P.negative) for (const CountClause& p : P.positive) if (ds_same_term(*p.term, *n.term)) return zero();  // +a -a
    for (CountClause& p : P.positive) p.mult = 1;  // (+a +a is +a)
  } else {
    P.need = (op == RGPU_OP_OR && msm >= 1) ? msm : 1;
    if (P.need > pos_clauses) return zero();
  }
  if (P.positive.size() == 1 && P.positive[0].mult >= P.need) { P.need = 1; P.positive[0].mult = 1; }  // a lone term, however often named
  if (P.positive.size() == 1 && P.negative.empty()) {
    if (!mask.deletions && !mask.set) { P.kind = COUNT_DOC_FREQ; P.doc_freq = P.positive[0].term->doc_freq; P.positive.clear(); }
    else P.kind = COUNT_LIST;
    return P;
  }
  if (required && P.positive.size() >= 2 && P.need_not == 1) {
    P.kind = COUNT_CONJ;
    std::stable_sort(P.positive.begin(), P.positive.end(), [](const CountClause& a, const CountClause& b) { return a.term->doc_freq < b.term->doc_freq; });
    for (CountClause& n : P.negative) n.mult = 1;
    P.need = 1;
    return P;
  }
  P.kind = COUNT_WINDOWS;
  if (P.need == 1) for (CountClause& p : P.positive) p.mult = 1;      // a union: once is enough
  if (P.need_not == 1) for (CountClause& n : P.negative) n.mult = 1;
  return P;
}

// ---- work items ----------------------------------------------------------------------------------------------------------------
// LIST rows: docset_term_items() chunks of blocks per term, as the doc-set list kernel.
// WINDOWS rows: an item is a run of `windows_per_item` consecutive windows of `window_docs` docs.
inline int64_t count_windows(int32_t max_doc, int32_t window_docs) { return max_doc <= 0 ? 0 : ((int64_t)max_doc + window_docs - 1) / window_docs; }
inline int64_t count_window_items(int32_t max_doc, int32_t window_docs, int32_t windows_per_item) {
  const int64_t w = count_windows(max_doc, window_docs);
  return (w + windows_per_item - 1) / windows_per_item;
}
// windows per item when nobody says: runs long enough that a clause's one search for its first block is shared by many windows,
// short enough that a batch of `rows` WINDOWS rows still fills the device (`target_items` wavefronts); 1 .. all
inline int32_t count_windows_per_item(int32_t max_doc, int32_t window_docs, int64_t rows, int64_t target_items, int32_t override_or_0) {
  const int64_t w = std::max<int64_t>(1, count_windows(max_doc, window_docs));
  if (override_or_0 > 0) return (int32_t)std::min<int64_t>(override_or_0, w);
  const int64_t items_per_row = std::max<int64_t>(1, target_items / std::max<int64_t>(1, rows));
  return (int32_t)std::max<int64_t>(1, std::min<int64_t>(w, (w + items_per_row - 1) / items_per_row));
}

}  // namespace rgpu_host
