// csrc/host/fields_tree_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_field_tree_cpu.py):
// validation and every refusal, per-leaf presence, dead queries, the three modes, the two summation orders, the run capacities, the
// window items, and for required/optional queries under the rule the lead group with the record prefix k_req_opt_scan takes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../rucene_amd/csrc/host/fields_tree_plan.hpp"

using namespace rgpu_host;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Batch {
  std::vector<rgpu_fields_tree_query> queries;
  std::vector<rgpu_field_tree_group> groups;
  std::vector<rgpu_field_clause> clauses;
  int32_t clause(int32_t df, int32_t field) {
    rgpu_field_clause c{};
    c.state.doc_start_fp = 100 + (int64_t)clauses.size();
    c.state.skip_offset = -1;
    c.state.total_term_freq = df;
    c.state.doc_freq = df;
    c.state.singleton_doc_id = df == 1 ? 3 : -1;
    c.weight = 1.0f;
    c.field = field;
    clauses.push_back(c);
    return (int32_t)clauses.size() - 1;
  }
  void group(int32_t kind, std::vector<int32_t> dfs, int32_t msm = 0, float tie = 0.1f) {
    const int32_t f = (int32_t)clauses.size();
    for (size_t i = 0; i < dfs.size(); ++i) clause(dfs[i], (int32_t)(i % 2));
    groups.push_back(rgpu_field_tree_group{f, (int32_t)dfs.size(), bits(tie), kind, msm, 0});
  }
  // a query over the groups added since `first_group`: the first n_must are MUST groups
  void query(int32_t first_group, int32_t n_must, int32_t msm = 0, std::vector<int32_t> not_dfs = {}) {
    const int32_t fn = (int32_t)clauses.size();
    for (int32_t df : not_dfs) clause(df, 1);
    queries.push_back(rgpu_fields_tree_query{first_group, n_must, (int32_t)groups.size() - first_group - n_must, msm, fn, (int32_t)not_dfs.size()});
  }
  int32_t validate(int32_t k = 10, uint32_t attached = 3u, int32_t n_tables = 1) const {
    const char* why = "";
    const int32_t rc = fields_tree_validate(queries.data(), (int32_t)queries.size(), groups.data(), (int32_t)groups.size(), clauses.data(),
                                            (int32_t)clauses.size(), k, attached, n_tables, &why);
    CHECK((rc == RGPU_OK) == (why[0] == 0));
    return rc;
  }
  FieldsTreePlan plan(int32_t rule = 0, int32_t max_doc = 4099, int32_t per_item = 0) const {
    CHECK(validate() == RGPU_OK);
    return plan_fields_tree(queries.data(), (int32_t)queries.size(), groups.data(), clauses.data(), max_doc, 512, 8, rule, per_item);
  }
};

static Batch one(int32_t kind, std::vector<int32_t> dfs, int32_t n_must, int32_t gmsm = 0, int32_t msm = 0, std::vector<int32_t> nots = {}) {
  Batch b;
  b.group(kind, dfs, gmsm);
  b.query(0, n_must, msm, nots);
  return b;
}

static void refusals() {
  CHECK(one(RGPU_GROUP_SUM, {5, 7}, 0).validate() == RGPU_OK);
  CHECK(one(RGPU_GROUP_SUM, {5, 7}, 1, 1).validate() == RGPU_OK);
  CHECK(one(RGPU_GROUP_SUM, {5, 7}, 0, 2).validate() == RGPU_ERR_UNSUPPORTED);     // a nested min_should_match of 2
  CHECK(one(RGPU_GROUP_SUM, {5, 7}, 0, -1).validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
  CHECK(one(RGPU_GROUP_SUM, {}, 0).validate() == RGPU_ERR_ILLEGAL_ARGUMENT);       // a sum group without a clause
  CHECK(one(RGPU_GROUP_SUM, {1, 2, 3, 4, 5, 6, 7, 8, 9}, 0).validate() == RGPU_OK);
  CHECK(one(RGPU_GROUP_SUM, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 0).validate() == RGPU_ERR_UNSUPPORTED);
  CHECK(one(3, {5}, 0).validate() == RGPU_ERR_ILLEGAL_ARGUMENT);                  // a kind outside the three
  CHECK(one(RGPU_GROUP_TERM, {5, 6}, 0).validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
  CHECK(one(RGPU_GROUP_SUM, {5}, 0).validate(0) == RGPU_ERR_ILLEGAL_ARGUMENT);
  CHECK(one(RGPU_GROUP_SUM, {5}, 0).validate(128) == RGPU_OK);
  CHECK(one(RGPU_GROUP_SUM, {5}, 0).validate(129) == RGPU_ERR_UNSUPPORTED);
  CHECK(one(RGPU_GROUP_SUM, {5, 6}, 0).validate(10, 1u) == RGPU_ERR_ILLEGAL_ARGUMENT);   // field 1 is not attached
  CHECK(one(RGPU_GROUP_SUM, {5}, 0).validate(10, 3u, 0) == RGPU_ERR_ILLEGAL_ARGUMENT);   // no sim table
  CHECK(one(RGPU_GROUP_SUM, {5}, 0, 0, 2, {3}).validate() == RGPU_ERR_UNSUPPORTED);      // MUST_NOT beside msm 2 under SHOULD
  CHECK(one(RGPU_GROUP_SUM, {5}, 1, 0, 2, {3}).validate() == RGPU_OK);                   // ... beside a MUST group: no effect
  {
    Batch b;  // no group at all; a negative side count; ten groups on a side
    b.group(RGPU_GROUP_SUM, {5});
    b.queries.push_back(rgpu_fields_tree_query{0, 0, 0, 0, 0, 0});
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.queries[0] = rgpu_fields_tree_query{0, -1, 2, 0, 0, 0};
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.queries[0] = rgpu_fields_tree_query{0, 1, 1, 0, 0, 0};  // two groups named, one in the array
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    for (int i = 0; i < 18; ++i) b.group(RGPU_GROUP_TERM, {4});
    b.queries[0] = rgpu_fields_tree_query{0, 9, 9, 0, 0, 0};
    CHECK(b.validate() == RGPU_OK);
    b.queries[0] = rgpu_fields_tree_query{0, 10, 1, 0, 0, 0};
    CHECK(b.validate() == RGPU_ERR_UNSUPPORTED);
    b.queries[0] = rgpu_fields_tree_query{0, 1, 10, 0, 0, 0};
    CHECK(b.validate() == RGPU_ERR_UNSUPPORTED);
  }
  {
    Batch b;  // 128 clauses are served, 129 are not
    for (int g = 0; g < 14; ++g) b.group(RGPU_GROUP_SUM, {1, 2, 3, 4, 5, 6, 7, 8, 9});
    b.query(0, 7, 0, {1, 1});
    CHECK(b.validate() == RGPU_OK);
    Batch c;
    for (int g = 0; g < 14; ++g) c.group(RGPU_GROUP_SUM, {1, 2, 3, 4, 5, 6, 7, 8, 9});
    c.query(0, 7, 0, {1, 1, 1});
    CHECK(c.validate() == RGPU_ERR_UNSUPPORTED);
  }
  {
    Batch b = one(RGPU_GROUP_DISMAX, {5, 6}, 0);
    b.groups[0].tie_bits = bits(std::numeric_limits<float>::infinity());
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
  }
  {  // what the header says is 0 is 0: the reserved word, min_should_match of a TERM or DISMAX group
    Batch b = one(RGPU_GROUP_SUM, {5, 6}, 0, 1);
    b.groups[0].reserved = 1;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(one(RGPU_GROUP_DISMAX, {5, 6}, 0, 1).validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(one(RGPU_GROUP_TERM, {5}, 1, 1).validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(one(RGPU_GROUP_DISMAX, {5, 6}, 0, 0).validate() == RGPU_OK);
  }
}

static void presence_and_modes() {
  Batch b;
  // q0 "+(7 0) (3 4)": required/optional; the sum group keeps its kind with one clause left
  b.group(RGPU_GROUP_SUM, {7, 0});
  b.group(RGPU_GROUP_SUM, {3, 4});
  b.query(0, 1);
  // q1 "+(0 0) (3)": a MUST group absent: dead
  b.group(RGPU_GROUP_SUM, {0, 0});
  b.group(RGPU_GROUP_SUM, {3});
  b.query(2, 1);
  // q2 "+(5) (0)": every SHOULD group absent: the MUST side alone
  b.group(RGPU_GROUP_SUM, {5});
  b.group(RGPU_GROUP_SUM, {0});
  b.query(4, 1);
  // q3 "(0) (6 2)" msm 1: SHOULD only, an absent group drops
  b.group(RGPU_GROUP_SUM, {0});
  b.group(RGPU_GROUP_SUM, {6, 2});
  b.query(6, 0, 1);
  // q4 "(6) (2)" msm 3: unreachable
  b.group(RGPU_GROUP_SUM, {6});
  b.group(RGPU_GROUP_SUM, {2});
  b.query(8, 0, 3);
  // q5 "+t300 +(100 150) +dismax(0 120) s1 s2 -9 -0": cost order 120 (a dismax group of one: a term), 250, 300; lead = the dismax's clause
  b.group(RGPU_GROUP_TERM, {300});
  b.group(RGPU_GROUP_SUM, {100, 150});
  b.group(RGPU_GROUP_DISMAX, {0, 120});
  b.group(RGPU_GROUP_TERM, {50});
  b.group(RGPU_GROUP_SUM, {60, 70});
  b.query(10, 3, 5, {9, 0});
  // q6 "+(100 150) +t250 x": equal costs keep the clause order; the lead group has two clauses
  b.group(RGPU_GROUP_SUM, {100, 150});
  b.group(RGPU_GROUP_TERM, {250});
  b.group(RGPU_GROUP_TERM, {11});
  b.query(15, 2);
  for (int rule = 0; rule >= -1; --rule) {
    const FieldsTreePlan P = b.plan(rule);
    const int32_t both = rule < 0 ? FIELDS_TREE_ADD : FIELDS_TREE_RULE;
    CHECK(P.queries.size() == 7);
    const FieldsTreePlanQuery& q0 = P.queries[0];
    CHECK(q0.n_groups == 2 && q0.mode == both && q0.need == 1 && q0.must == 1 && q0.n_not == 0);
    CHECK(P.groups[q0.first_group].kind == RGPU_GROUP_SUM && P.groups[q0.first_group].n_terms == 1 && P.groups[q0.first_group].optional == 0);
    CHECK(P.groups[q0.first_group + 1].n_terms == 2 && P.groups[q0.first_group + 1].optional == 1);
    CHECK(P.queries[1].n_groups == 0 && P.queries[1].mode == FIELDS_TREE_SINGLE && P.queries[1].rec_base == -1);
    const FieldsTreePlanQuery& q2 = P.queries[2];
    CHECK(q2.n_groups == 1 && q2.mode == FIELDS_TREE_SINGLE && q2.must == 1 && q2.need == 1 && P.groups[q2.first_group].optional == 0);
    const FieldsTreePlanQuery& q3 = P.queries[3];
    CHECK(q3.n_groups == 1 && q3.mode == FIELDS_TREE_SINGLE && q3.must == 0 && q3.need == 1 && P.groups[q3.first_group].n_terms == 2);
    CHECK(P.queries[4].n_groups == 0);
    const FieldsTreePlanQuery& q5 = P.queries[5];
    CHECK(q5.n_groups == 5 && q5.mode == both && q5.need == 3 && q5.must == 1 && q5.n_not == 1);
    const FieldsTreePlanGroup* g5 = &P.groups[q5.first_group];
    CHECK(g5[0].kind == RGPU_GROUP_TERM && g5[0].n_terms == 1 && b.clauses[P.clause_of[g5[0].first_term]].state.doc_freq == 120);
    CHECK(g5[1].kind == RGPU_GROUP_SUM && g5[1].n_terms == 2 && g5[2].kind == RGPU_GROUP_TERM && b.clauses[P.clause_of[g5[2].first_term]].state.doc_freq == 300);
    CHECK(!g5[0].optional && !g5[1].optional && !g5[2].optional && g5[3].optional && g5[4].optional);
    CHECK(b.clauses[P.clause_of[g5[3].first_term]].state.doc_freq == 50 && g5[4].n_terms == 2);
    CHECK(q5.first_not == g5[4].first_term + 2 && b.clauses[P.clause_of[q5.first_not]].state.doc_freq == 9);
    const FieldsTreePlanQuery& q6 = P.queries[6];
    const FieldsTreePlanGroup* g6 = &P.groups[q6.first_group];
    CHECK(g6[0].kind == RGPU_GROUP_SUM && g6[1].kind == RGPU_GROUP_TERM && g6[2].optional == 1);
    // the flat clause order of a query starts with its lead group
    CHECK(g5[0].first_term < g5[1].first_term && g6[0].first_term < g6[1].first_term);
    if (rule < 0) {
      CHECK(P.rule_query.empty() && P.rec_prefix.size() == 1 && P.rec_prefix[0] == 0 && P.n_single_or_add == 7);
      CHECK(q0.rec_base == -1 && q0.lead_terms == 0);
    } else {
      CHECK(P.rule_query == (std::vector<int32_t>{0, 5, 6}) && P.n_single_or_add == 4);
      CHECK(P.rec_prefix == (std::vector<int64_t>{0, 7, 127, 377}));   // 7; 120; 100 + 150: a doc both clauses hold counts twice
      CHECK(q0.rec_base == 0 && q0.lead_terms == 1 && q5.rec_base == 7 && q5.lead_terms == 1 && q6.rec_base == 127 && q6.lead_terms == 2);
    }
    // absent clauses are not walked; a walked clause's run holds its postings and the sentinels
    for (size_t j = 0; j < P.clause_of.size(); ++j) CHECK(b.clauses[P.clause_of[j]].state.doc_freq > 0);
    CHECK(fields_tree_run_slots(0) == FIELDS_RUN_PAD && fields_tree_run_slots(300) == 300 + FIELDS_RUN_PAD);
    CHECK(fields_tree_run_slots(0x7fffffff) == (int64_t)0x7fffffff + FIELDS_RUN_PAD);
    // items: 4099 docs = 9 windows, one per item, rounded up to the eight wavefronts of a workgroup
    CHECK(P.windows_per_query == 9 && P.windows_per_item == 1 && P.items_per_query == 16 && P.items == 7 * 16);
  }
  const FieldsTreePlan P3 = b.plan(0, 4099, 3);
  CHECK(P3.windows_per_item == 3 && P3.items_per_query == 8);
  const FieldsTreePlan P1 = b.plan(0, 1, 0);
  CHECK(P1.windows_per_query == 1 && P1.items_per_query == 8);
}

int main() {
  refusals();
  presence_and_modes();
  std::printf("fields_tree_plan_test OK\n");
  return 0;
}
