// The host plan of rgpu_search_fields_tree_batch (BooleanQuery over TermQuery / DisjunctionMaxQuery / nested should-only BooleanQuery
// groups under MUST and SHOULD, the tree query_string.rs builds over several fields): plain C++17 with no device dependency
// (tests/cpp/fields_tree_plan_test.cpp runs it under the sanitizers). It reuses host/fields_plan.hpp and adds
//   * validation and every refusal of include/rucene_gpu.h, before anything is launched or written;
//   * presence per leaf: a SUM group stays ONE DisjunctionSumScorer even with one clause left (boolean_query.rs:217-234), a dismax
//     group with one left is that TermScorer; a SHOULD group without a scorer drops, a MUST group without one kills the query;
//   * the three modes: SINGLE (one side, or every SHOULD group absent: rgpu_search_fields_batch's rules), ADD (required/optional with
//     rgpu_config.req_opt_rule = -1: req + opt in the window kernel) and RULE (required/optional under req_opt_scorer.rs:41-66: one
//     record per collected hit, then k_req_opt_scan);
//   * the two summation orders: the MUST groups first, in the leaf's stable cost order (conjunction_scorer.rs:30), then the SHOULD
//     groups in clause order (SimpleQueue, disjunction_scorer.rs:213-225);
//   * the run capacity of a walked clause (fields_tree_run_slots: doc_freq + the sentinels; the call keeps ONE run per distinct
//     clause of the batch, so the prefix over them is the call's), the window items;
//   * for RULE queries the lead group - the required side's cheapest, the first in cost order - and the record region: every hit is
//     held by the lead group, so the sum of its present clauses' doc_freq bounds the records (a doc two of them hold counts twice).
#pragma once
#include "fields_plan.hpp"

namespace rgpu_host {

constexpr int32_t FIELDS_TREE_SINGLE = 0, FIELDS_TREE_ADD = 1, FIELDS_TREE_RULE = 2;

// What the window kernel reads (kernels/search_fields_tree.hpp mirrors the two layouts; api/fields_tree.hpp asserts the sizes)
struct FieldsTreePlanGroup {
  int32_t first_term;  // into the plan's flat clause order
  int32_t n_terms;     // present clauses
  uint32_t tie_bits;
  int32_t kind;        // RGPU_GROUP_TERM: the one clause's score; RGPU_GROUP_DISMAX: max + (sum - max) * tie; RGPU_GROUP_SUM: the sum
  int32_t optional;    // 1: a SHOULD group beside MUST groups - folded into the doc's optional sum, not counted
  int32_t pad;
};
struct FieldsTreePlanQuery {
  int32_t first_group, n_groups;  // in summation order; 0 groups: the query matches nothing in this leaf
  int32_t first_not, n_not;       // flat clause range of the present MUST_NOT clauses
  int32_t need;                   // a hit is held by at least this many counted groups (MUST groups: all of them)
  int32_t must;                   // 1: the first counted group's score is taken as it is; 0: 0.0f + g
  int32_t mode;                   // FIELDS_TREE_*
  int32_t lead_terms;             // RULE: present clauses of the lead group = the query's first `lead_terms` flat clauses
  int64_t rec_base;               // RULE: first record slot of the query's region; else -1
};

// slots of the {doc, score} run of a clause of `doc_freq` postings: k_score_terms closes it with FIELDS_RUN_PAD sentinels
inline int64_t fields_tree_run_slots(int32_t doc_freq) { return (int64_t)doc_freq + FIELDS_RUN_PAD; }

struct FieldsTreePlan {
  std::vector<FieldsTreePlanQuery> queries;
  std::vector<FieldsTreePlanGroup> groups;
  std::vector<int32_t> clause_of;   // flat clause j of the plan -> index into the caller's `clauses`
  std::vector<int32_t> rule_query;  // the RULE queries, ascending: k_req_opt_scan's qmap
  std::vector<int64_t> rec_prefix;  // rule query i -> first record slot; [n] = records in all: k_req_opt_scan's seq_prefix
  int32_t n_single_or_add = 0;      // queries whose rows k_merge_items folds
  int32_t windows_per_query = 0, windows_per_item = 0, items_per_query = 0;
  int64_t items = 0;
};

inline int32_t fields_tree_validate(const rgpu_fields_tree_query* queries, int32_t n_queries, const rgpu_field_tree_group* groups,
                                    int32_t n_groups_total, const rgpu_field_clause* clauses, int32_t n_clauses_total, int32_t k, uint32_t attached,
                                    int32_t n_sim_tables, const char** why) {
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
    const rgpu_fields_tree_query& Q = queries[q];
    if (Q.n_must < 0 || Q.n_should < 0 || Q.n_must_not < 0 || Q.min_should_match < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative count");
    if (Q.n_must == 0 && Q.n_should == 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a query of zero groups");
    if (Q.n_must > RGPU_MAX_FIELD_GROUPS || Q.n_should > RGPU_MAX_FIELD_GROUPS)
      return refuse(RGPU_ERR_UNSUPPORTED, "ten or more groups on a side are summed in heap order by the reference");
    const int32_t n_groups = Q.n_must + Q.n_should;
    if (Q.first_group < 0 || (int64_t)Q.first_group + n_groups > n_groups_total) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "group range outside the groups array");
    if (Q.n_must_not > 0 && (Q.first_must_not < 0 || (int64_t)Q.first_must_not + Q.n_must_not > n_clauses_total))
      return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "MUST_NOT range outside the clauses array");
    if (Q.n_must == 0 && Q.n_must_not > 0 && Q.min_should_match >= 2)
      return refuse(RGPU_ERR_UNSUPPORTED, "MUST_NOT clauses beside min_should_match >= 2 are not served by the cross-field calls");
    int64_t n_clauses = Q.n_must_not;
    for (int32_t g = 0; g < n_groups; ++g) {
      const rgpu_field_tree_group& G = groups[Q.first_group + g];
      if (G.kind != RGPU_GROUP_TERM && G.kind != RGPU_GROUP_DISMAX && G.kind != RGPU_GROUP_SUM)
        return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "group kind must be RGPU_GROUP_TERM, RGPU_GROUP_DISMAX or RGPU_GROUP_SUM");
      if (G.n_terms < 0 || G.min_should_match < 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "negative count");
      if (G.reserved != 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "rgpu_field_tree_group.reserved must be 0");
      if (G.kind != RGPU_GROUP_SUM && G.min_should_match != 0)
        return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "min_should_match of a TERM or DISMAX group must be 0");
      if (G.kind == RGPU_GROUP_TERM && G.n_terms != 1) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a TERM group is one clause");
      if (G.n_terms == 0) return refuse(RGPU_ERR_ILLEGAL_ARGUMENT, "a dismax or sum group without a clause");
      if (G.n_terms > RGPU_MAX_GROUP_DISJUNCTS) return refuse(RGPU_ERR_UNSUPPORTED, "ten or more disjuncts are summed in heap order by the reference");
      if (G.kind == RGPU_GROUP_SUM && G.min_should_match >= 2)
        return refuse(RGPU_ERR_UNSUPPORTED, "a SUM group with min_should_match >= 2: the reference's advance() ignores it while next() honours it");
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

// The whole batch for one leaf. The arguments have passed fields_tree_validate. `req_opt_rule`: rgpu_config.req_opt_rule.
inline FieldsTreePlan plan_fields_tree(const rgpu_fields_tree_query* queries, int32_t n_queries, const rgpu_field_tree_group* groups,
                                       const rgpu_field_clause* clauses, int32_t max_doc, int32_t window_docs, int32_t waves, int32_t req_opt_rule,
                                       int32_t per_item_override_or_0 = 0) {
  FieldsTreePlan P;
  P.queries.resize((size_t)n_queries);
  struct Present { int32_t group; int64_t cost; };
  std::vector<Present> req, opt;
  auto walk = [&](int32_t clause) { P.clause_of.push_back(clause); };
  int64_t records = 0;
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_fields_tree_query& Q = queries[q];
    FieldsTreePlanQuery& D = P.queries[(size_t)q];
    D = FieldsTreePlanQuery{(int32_t)P.groups.size(), 0, (int32_t)P.clause_of.size(), 0, 1, Q.n_must > 0 ? 1 : 0, FIELDS_TREE_SINGLE, 0, -1};
    req.clear();
    opt.clear();
    bool dead = false;
    for (int32_t g = 0; g < Q.n_must + Q.n_should; ++g) {
      const rgpu_field_tree_group& G = groups[Q.first_group + g];
      int64_t cost = 0;
      int32_t present = 0;
      for (int32_t i = 0; i < G.n_terms; ++i)
        if (clauses[G.first_term + i].state.doc_freq > 0) { ++present; cost += clauses[G.first_term + i].state.doc_freq; }
      const bool required = g < Q.n_must;
      if (present > 0) (required ? req : opt).push_back(Present{g, cost});
      else if (required) dead = true;
    }
    int32_t need;
    if (Q.n_must > 0) {
      need = (int32_t)req.size();
    } else {
      need = std::max(1, Q.min_should_match);
      if (opt.empty() || (int32_t)opt.size() < need) dead = true;
    }
    if (dead) { P.n_single_or_add += 1; continue; }
    std::stable_sort(req.begin(), req.end(), [](const Present& a, const Present& b) { return a.cost < b.cost; });
    const bool req_opt = !req.empty() && !opt.empty();
    D.mode = !req_opt ? FIELDS_TREE_SINGLE : req_opt_rule < 0 ? FIELDS_TREE_ADD : FIELDS_TREE_RULE;
    auto emit = [&](const Present& o, bool optional) {
      const rgpu_field_tree_group& G = groups[Q.first_group + o.group];
      FieldsTreePlanGroup DG{(int32_t)P.clause_of.size(), 0, G.tie_bits, G.kind, optional ? 1 : 0, 0};
      for (int32_t i = 0; i < G.n_terms; ++i)
        if (clauses[G.first_term + i].state.doc_freq > 0) { walk(G.first_term + i); ++DG.n_terms; }
      if (DG.n_terms == 1 && DG.kind == RGPU_GROUP_DISMAX) DG.kind = RGPU_GROUP_TERM;  // DisjunctionMaxWeight hands the one scorer out as it is
      P.groups.push_back(DG);
    };
    for (const Present& o : req) emit(o, false);
    for (const Present& o : opt) emit(o, req_opt);
    D.n_groups = (int32_t)(req.size() + opt.size());
    D.need = need;
    D.first_not = (int32_t)P.clause_of.size();
    for (int32_t i = 0; i < Q.n_must_not; ++i)
      if (clauses[Q.first_must_not + i].state.doc_freq > 0) { walk(Q.first_must_not + i); ++D.n_not; }
    if (D.mode == FIELDS_TREE_RULE) {
      D.lead_terms = P.groups[(size_t)D.first_group].n_terms;
      D.rec_base = records;
      P.rule_query.push_back(q);
      P.rec_prefix.push_back(records);
      records += req.front().cost;
    } else {
      P.n_single_or_add += 1;
    }
  }
  P.rec_prefix.push_back(records);
  FieldsPlan items;
  fields_items(max_doc, window_docs, n_queries, waves, per_item_override_or_0, &items);
  P.windows_per_query = items.windows_per_query;
  P.windows_per_item = items.windows_per_item;
  P.items_per_query = items.items_per_query;
  P.items = items.items;
  return P;
}

}  // namespace rgpu_host
