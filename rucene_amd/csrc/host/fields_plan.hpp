// The host plan of rgpu_search_fields_batch (BooleanQuery over TermQuery / DisjunctionMaxQuery clauses whose terms live in different
// fields of one segment): the decisions that can be wrong without a GPU, in plain C++17 with no device dependency
// (tests/cpp/fields_plan_test.cpp runs it under the sanitizers).
//   * validation and every refusal of include/rucene_gpu.h, before anything is launched or written;
//   * presence per leaf: a disjunct of doc_freq 0 has no scorer (disjunction_max_query.rs:142-161), a group with no disjunct left
//     has none, a dismax group with ONE left is that TermScorer (:154); an absent MUST_NOT clause drops (boolean_query.rs:235-252);
//   * dead queries: a MUST group absent from the leaf (boolean_query.rs:203-207), no SHOULD group left (:274-277), or fewer groups
//     left than min_should_match asks for (disjunction_scorer.rs:317-329 can never be met);
//   * the summation order: clause order under SHOULD (SimpleQueue, disjunction_scorer.rs:213-225); under MUST ConjunctionScorer::new's
//     stable sort by cost (conjunction_scorer.rs:30) - a term's doc_freq, a dismax group's sum over its present disjuncts
//     (disjunction_scorer.rs:126) - whose order score() adds in (:87-95);
//   * the run capacity of every clause that is walked (doc_freq + the sentinels), the window items.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/rucene_gpu.h"

namespace rgpu_host {

constexpr int32_t FIELDS_RUN_PAD = 64;  // sentinel entries behind every run (kernels/search_or.hpp OR_RUN_PAD: k_score_terms writes them)
constexpr int32_t FIELDS_MAX_K = 128;

// What the window kernel reads (kernels/search_fields.hpp mirrors the two layouts; rgpu_api.hip asserts the sizes)
struct FieldsPlanGroup {
  int32_t first_term;  // into the plan's flat clause order
  int32_t n_terms;     // present disjuncts
  uint32_t tie_bits;
  int32_t kind;        // RGPU_GROUP_TERM: the score is the one clause's own
};
struct FieldsPlanQuery {
  int32_t first_group, n_groups;  // in summation order; 0 groups: the query matches nothing in this leaf
  int32_t first_not, n_not;       // flat clause range of the present MUST_NOT clauses
  int32_t need;                   // a hit is held by at least this many groups (MUST: all of them)
  int32_t must;                   // 1: the first group's score is taken as it is; 0: 0.0f + g
};

struct FieldsPlan {
  int32_t status = RGPU_OK;  // RGPU_OK, RGPU_ERR_ILLEGAL_ARGUMENT or RGPU_ERR_UNSUPPORTED (then `why` says what, and nothing else is filled)
  const char* why = "";
  std::vector<FieldsPlanQuery> queries;
  std::vector<FieldsPlanGroup> groups;
  std::vector<int32_t> clause_of;   // flat clause j of the plan -> index into the caller's `clauses`
  std::vector<int64_t> run_prefix;  // flat clause j -> first slot of its run; [n] = slots in all
  uint32_t fields_named = 0;        // bit f: some walked clause lives in field f
  int32_t windows_per_query = 0, windows_per_item = 0, items_per_query = 0;
  int64_t items = 0;
};

inline bool fields_finite_bits(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// Every refusal, in the caller's terms. `attached`: bit f = field slot f exists. `n_sim_tables`: tables uploaded to the context.
inline int32_t fields_validate(const rgpu_fields_query* queries, int32_t n_queries, const rgpu_field_group* groups, int32_t n_groups_total,
                               const rgpu_field_clause* clauses, int32_t n_clauses_total, int32_t k, uint32_t attached, int32_t n_sim_tables,
                               const char** why) {
  auto refuse = [&](int32_t status, const char* w) { *why = w; return status; };
  if (!queries || n_queries <= 0 || !groups || n_groups_total <= 0 || !clauses || n_clauses_total <= 0)
    return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "k must be in 1..128");
  if (k > FIELDS_MAX_K) return refuse(RGPU_ERR_UNSUPPORTED, "k must be in 1..128");
  auto clause_ok = [&](const rgpu_field_clause& c, bool scored) -> const char* {
    if (c.field < 0 || c.field >= RGPU_MAX_FIELDS || !((attached >> c.field) & 1u)) return "a clause names a field slot that is not attached";
    if (c.state.doc_freq < 0) return "negative doc_freq";
    if (scored && (c.sim_table < 0 || c.sim_table >= n_sim_tables)) return "a clause names a sim_table that was never uploaded";
    return nullptr;
  };
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_fields_query& Q = queries[q];
    if (Q.occur & RGPU_OCCUR_FILTER) return refuse(RGPU_ERR_UNSUPPORTED, "FILTER clauses are not served by the cross-field call");
    if (Q.occur == (RGPU_OCCUR_MUST | RGPU_OCCUR_SHOULD))
      return refuse(RGPU_ERR_UNSUPPORTED, "MUST and SHOULD groups in one query (ReqOptScorer) are not served by the cross-field call");
    if (Q.occur != RGPU_OCCUR_SHOULD && Q.occur != RGPU_OCCUR_MUST) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "occur must be RGPU_OCCUR_SHOULD or RGPU_OCCUR_MUST");
    if (Q.n_groups < 0 || Q.n_must_not < 0 || Q.min_should_match < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative count");
    if (Q.n_groups == 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a query of zero groups");
    if (Q.n_groups > RGPU_MAX_FIELD_GROUPS) return refuse(RGPU_ERR_UNSUPPORTED, "ten or more groups are summed in heap order by the reference");
    if (Q.first_group < 0 || (int64_t)Q.first_group + Q.n_groups > n_groups_total) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "group range outside the groups array");
    if (Q.n_must_not > 0 && (Q.first_must_not < 0 || (int64_t)Q.first_must_not + Q.n_must_not > n_clauses_total))
      return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "MUST_NOT range outside the clauses array");
    if (Q.occur == RGPU_OCCUR_SHOULD && Q.n_must_not > 0 && Q.min_should_match >= 2)
      return refuse(RGPU_ERR_UNSUPPORTED, "MUST_NOT clauses beside min_should_match >= 2 are not served by the cross-field call");
    int64_t n_clauses = Q.n_must_not;
    for (int32_t g = 0; g < Q.n_groups; ++g) {
      const rgpu_field_group& G = groups[Q.first_group + g];
      if (G.kind != RGPU_GROUP_TERM && G.kind != RGPU_GROUP_DISMAX) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "group kind must be RGPU_GROUP_TERM or RGPU_GROUP_DISMAX");
      if (G.n_terms < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative count");
      if (G.kind == RGPU_GROUP_TERM && G.n_terms != 1) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a TERM group is one clause");
      if (G.n_terms == 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a dismax group without a disjunct");
      if (G.n_terms > RGPU_MAX_GROUP_DISJUNCTS) return refuse(RGPU_ERR_UNSUPPORTED, "ten or more disjuncts are summed in heap order by the reference");
      if (G.kind == RGPU_GROUP_DISMAX && !fields_finite_bits(G.tie_bits)) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "tie_breaker_multiplier is not finite");
      if (G.first_term < 0 || (int64_t)G.first_term + G.n_terms > n_clauses_total) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "clause range outside the clauses array");
      for (int32_t i = 0; i < G.n_terms; ++i)
        if (const char* w = clause_ok(clauses[G.first_term + i], true)) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, w);
      n_clauses += G.n_terms;
    }
    if (n_clauses > RGPU_MAX_FIELDS_QUERY_CLAUSES) return refuse(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_FIELDS_QUERY_CLAUSES clauses in one query");
    for (int32_t i = 0; i < Q.n_must_not; ++i)
      if (const char* w = clause_ok(clauses[Q.first_must_not + i], false)) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, w);
  }
  return RGPU_OK;
}

// (query, range of windows) items: one per wavefront, a query's item count a multiple of `waves` so that a workgroup serves one query
inline void fields_items(int32_t max_doc, int32_t window_docs, int32_t n_queries, int32_t waves, int32_t per_item_override_or_0, FieldsPlan* P) {
  P->windows_per_query = std::max(1, (int32_t)(((int64_t)max_doc + window_docs - 1) / window_docs));
  const int64_t auto_wpi = std::max<int64_t>(1, ((int64_t)n_queries * P->windows_per_query + 131071) / 131072);
  P->windows_per_item = per_item_override_or_0 > 0 ? per_item_override_or_0 : (int32_t)auto_wpi;
  P->items_per_query = ((P->windows_per_query + P->windows_per_item - 1) / P->windows_per_item + waves - 1) / waves * waves;
  P->items = (int64_t)n_queries * P->items_per_query;
}

// The whole batch for one leaf. The arguments have passed fields_validate.
inline FieldsPlan plan_fields(const rgpu_fields_query* queries, int32_t n_queries, const rgpu_field_group* groups, const rgpu_field_clause* clauses,
                              int32_t max_doc, int32_t window_docs, int32_t waves, int32_t per_item_override_or_0 = 0) {
  FieldsPlan P;
  P.queries.resize((size_t)n_queries);
  struct Present { int32_t group; int64_t cost; };
  std::vector<Present> order;
  auto walk = [&](int32_t clause) {
    P.clause_of.push_back(clause);
    P.fields_named |= 1u << clauses[clause].field;
  };
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_fields_query& Q = queries[q];
    const bool must = Q.occur == RGPU_OCCUR_MUST;
    FieldsPlanQuery& D = P.queries[(size_t)q];
    D = FieldsPlanQuery{(int32_t)P.groups.size(), 0, (int32_t)P.clause_of.size(), 0, 1, must ? 1 : 0};
    order.clear();
    bool dead = false;
    for (int32_t g = 0; g < Q.n_groups; ++g) {
      const rgpu_field_group& G = groups[Q.first_group + g];
      int64_t cost = 0;
      int32_t present = 0;
      for (int32_t i = 0; i < G.n_terms; ++i)
        if (clauses[G.first_term + i].state.doc_freq > 0) { ++present; cost += clauses[G.first_term + i].state.doc_freq; }
      if (present > 0) order.push_back(Present{g, cost});
      else if (must) dead = true;
    }
    const int32_t need = must ? (int32_t)order.size() : std::max(1, Q.min_should_match);
    if (order.empty() || (int32_t)order.size() < need) dead = true;
    if (dead) continue;
    if (must) std::stable_sort(order.begin(), order.end(), [](const Present& a, const Present& b) { return a.cost < b.cost; });
    for (const Present& o : order) {
      const rgpu_field_group& G = groups[Q.first_group + o.group];
      FieldsPlanGroup DG{(int32_t)P.clause_of.size(), 0, G.tie_bits, G.kind};
      for (int32_t i = 0; i < G.n_terms; ++i)
        if (clauses[G.first_term + i].state.doc_freq > 0) { walk(G.first_term + i); ++DG.n_terms; }
      if (DG.n_terms == 1) DG.kind = RGPU_GROUP_TERM;  // one scorer left: DisjunctionMaxWeight hands it out as it is
      P.groups.push_back(DG);
    }
    D.n_groups = (int32_t)order.size();
    D.need = need;
    D.first_not = (int32_t)P.clause_of.size();
    for (int32_t i = 0; i < Q.n_must_not; ++i)
      if (clauses[Q.first_must_not + i].state.doc_freq > 0) { walk(Q.first_must_not + i); ++D.n_not; }
  }
  P.run_prefix.resize(P.clause_of.size() + 1);
  int64_t slots = 0;
  for (size_t j = 0; j < P.clause_of.size(); ++j) {
    P.run_prefix[j] = slots;
    slots += (int64_t)clauses[P.clause_of[j]].state.doc_freq + FIELDS_RUN_PAD;
  }
  P.run_prefix[P.clause_of.size()] = slots;
  fields_items(max_doc, window_docs, n_queries, waves, per_item_override_or_0, &P);
  return P;
}

}  // namespace rgpu_host
