// csrc/host/fields_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_cross_field_cpu.py):
// validation and every refusal, per-leaf presence, dead queries, the stable MUST cost order, the run capacities, the item counts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../rucene_amd/csrc/host/fields_plan.hpp"

using rgpu_host::FieldsPlan;
using rgpu_host::fields_validate;
using rgpu_host::plan_fields;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Batch {
  std::vector<rgpu_fields_query> queries;
  std::vector<rgpu_field_group> groups;
  std::vector<rgpu_field_clause> clauses;
  int32_t clause(int32_t df, int32_t field, int64_t fp = 100) {
    rgpu_field_clause c{};
    c.state.doc_start_fp = fp;
    c.state.skip_offset = -1;
    c.state.total_term_freq = df;
    c.state.doc_freq = df;
    c.state.singleton_doc_id = df == 1 ? 3 : -1;
    c.weight = 1.0f;
    c.sim_table = 0;
    c.field = field;
    clauses.push_back(c);
    return (int32_t)clauses.size() - 1;
  }
  // a group over the clauses added since `first`
  void group(int32_t first, int32_t kind, float tie = 0.0f) {
    groups.push_back(rgpu_field_group{first, (int32_t)clauses.size() - first, bits(tie), kind});
  }
  void term_group(int32_t df, int32_t field) { const int32_t f = clause(df, field); group(f, RGPU_GROUP_TERM); }
  void dismax_group(std::vector<int32_t> dfs, float tie = 0.1f) {
    const int32_t f = (int32_t)clauses.size();
    for (size_t i = 0; i < dfs.size(); ++i) clause(dfs[i], (int32_t)(i % 2));
    group(f, RGPU_GROUP_DISMAX, tie);
  }
  // a query over the groups added since `first_group`; MUST_NOT clauses: the dfs given, appended now
  void query(int32_t first_group, int32_t occur, int32_t msm = 0, std::vector<int32_t> not_dfs = {}) {
    const int32_t fn = (int32_t)clauses.size();
    for (int32_t df : not_dfs) clause(df, 1);
    queries.push_back(rgpu_fields_query{occur, first_group, (int32_t)groups.size() - first_group, msm, fn, (int32_t)not_dfs.size()});
  }
  int32_t validate(int32_t k = 10, uint32_t attached = 3u, int32_t n_tables = 1) const {
    const char* why = "";
    const int32_t rc = fields_validate(queries.data(), (int32_t)queries.size(), groups.data(), (int32_t)groups.size(), clauses.data(),
                                       (int32_t)clauses.size(), k, attached, n_tables, &why);
    CHECK((rc == RGPU_OK) == (why[0] == 0));
    return rc;
  }
  FieldsPlan plan(int32_t max_doc = 1000, int32_t W = 512, int32_t waves = 8, int32_t per_item = 0) const {
    CHECK(validate() == RGPU_OK);
    return plan_fields(queries.data(), (int32_t)queries.size(), groups.data(), clauses.data(), max_doc, W, waves, per_item);
  }
};

static void refusals() {
  {  // the plain multi-field query passes
    Batch b;
    b.dismax_group({5, 7});
    b.dismax_group({1, 300});
    b.query(0, RGPU_OCCUR_SHOULD);
    CHECK(b.validate() == RGPU_OK);
    CHECK(b.validate(128) == RGPU_OK);
    CHECK(b.validate(129) == RGPU_ERR_UNSUPPORTED);
    CHECK(b.validate(0) == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(b.validate(10, 1u) == RGPU_ERR_ILLEGAL_ARGUMENT);      // field 1 is not attached
    CHECK(b.validate(10, 3u, 0) == RGPU_ERR_ILLEGAL_ARGUMENT);   // no sim table was uploaded
  }
  for (int n = 9; n <= 10; ++n) {  // nine groups are served, ten are the heap arm
    Batch b;
    for (int i = 0; i < n; ++i) b.term_group(4 + i, i % 2);
    b.query(0, RGPU_OCCUR_SHOULD);
    CHECK(b.validate() == (n == 9 ? RGPU_OK : RGPU_ERR_UNSUPPORTED));
  }
  for (int n = 9; n <= 10; ++n) {  // ... and so are nine / ten disjuncts
    Batch b;
    b.dismax_group(std::vector<int32_t>((size_t)n, 6));
    b.query(0, RGPU_OCCUR_MUST);
    CHECK(b.validate() == (n == 9 ? RGPU_OK : RGPU_ERR_UNSUPPORTED));
  }
  {
    Batch b;
    b.term_group(4, 0);
    b.term_group(4, 1);
    b.query(0, RGPU_OCCUR_MUST | RGPU_OCCUR_SHOULD);
    CHECK(b.validate() == RGPU_ERR_UNSUPPORTED);  // ReqOptScorer
    b.queries[0].occur = RGPU_OCCUR_MUST | RGPU_OCCUR_FILTER;
    CHECK(b.validate() == RGPU_ERR_UNSUPPORTED);
    b.queries[0].occur = RGPU_OCCUR_FILTER;
    CHECK(b.validate() == RGPU_ERR_UNSUPPORTED);
    b.queries[0].occur = 0;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.queries[0].occur = 8;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.queries[0].occur = RGPU_OCCUR_SHOULD;
    b.queries[0].n_groups = 0;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);  // zero groups
    b.queries[0].n_groups = 3;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);  // past the groups array
    b.queries[0].n_groups = 2;
    b.groups[1].first_term = 2;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);  // past the clauses array
  }
  {  // MUST_NOT beside min_should_match >= 2: refused under SHOULD, without effect under MUST
    Batch b;
    b.term_group(4, 0);
    b.term_group(4, 1);
    b.query(0, RGPU_OCCUR_SHOULD, 2, {9});
    CHECK(b.validate() == RGPU_ERR_UNSUPPORTED);
    b.queries[0].min_should_match = 1;
    CHECK(b.validate() == RGPU_OK);
    b.queries[0].min_should_match = 2;
    b.queries[0].occur = RGPU_OCCUR_MUST;
    CHECK(b.validate() == RGPU_OK);
    b.clauses[2].field = 2;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);  // the MUST_NOT clause's field is not attached
    b.clauses[2].field = 1;
    b.clauses[2].sim_table = 77;                         // unused for a MUST_NOT clause
    CHECK(b.validate() == RGPU_OK);
    b.clauses[0].sim_table = 1;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
  }
  {  // ties and kinds
    Batch b;
    b.dismax_group({4, 5}, std::numeric_limits<float>::infinity());
    b.query(0, RGPU_OCCUR_SHOULD);
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.groups[0].tie_bits = bits(std::nanf(""));
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.groups[0].tie_bits = bits(-2.5f);
    CHECK(b.validate() == RGPU_OK);
    b.groups[0].kind = RGPU_GROUP_TERM;  // a TERM group of two clauses
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.groups[0].n_terms = 1;
    b.groups[0].tie_bits = bits(std::nanf(""));  // ignored for a TERM group
    CHECK(b.validate() == RGPU_OK);
    b.groups[0].kind = 2;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.groups[0].kind = RGPU_GROUP_DISMAX;
    b.groups[0].tie_bits = 0;
    b.groups[0].n_terms = 0;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
    b.groups[0].n_terms = 1;
    b.clauses[0].state.doc_freq = -1;
    CHECK(b.validate() == RGPU_ERR_ILLEGAL_ARGUMENT);
  }
  {  // 81 scored clauses + MUST_NOT clauses up to 128 in all
    Batch b;
    for (int g = 0; g < 9; ++g) b.dismax_group(std::vector<int32_t>(9, 3));
    b.query(0, RGPU_OCCUR_SHOULD, 0, std::vector<int32_t>(47, 2));
    CHECK(b.validate() == RGPU_OK);
    Batch c;
    for (int g = 0; g < 9; ++g) c.dismax_group(std::vector<int32_t>(9, 3));
    c.query(0, RGPU_OCCUR_SHOULD, 0, std::vector<int32_t>(48, 2));
    CHECK(c.validate() == RGPU_ERR_UNSUPPORTED);
  }
}

static void presence_and_order() {
  {  // SHOULD: clause order, absent disjuncts and groups drop, msm stays; one disjunct left = that term's scorer
    Batch b;
    b.dismax_group({0, 40, 0}, 0.5f);   // one present: a TERM group over clause 1
    b.term_group(0, 1);                  // absent
    b.dismax_group({7, 0, 9}, 0.25f);   // two present: clauses 4 and 6
    b.term_group(3, 0);
    b.query(0, RGPU_OCCUR_SHOULD, 2, {});
    const FieldsPlan P = b.plan();
    CHECK(P.queries.size() == 1 && P.queries[0].n_groups == 3 && P.queries[0].need == 2 && P.queries[0].must == 0 && P.queries[0].n_not == 0);
    CHECK((P.clause_of == std::vector<int32_t>{1, 4, 6, 7}));
    CHECK(P.groups[0].kind == RGPU_GROUP_TERM && P.groups[0].n_terms == 1 && P.groups[0].first_term == 0);
    CHECK(P.groups[1].kind == RGPU_GROUP_DISMAX && P.groups[1].n_terms == 2 && P.groups[1].first_term == 1 && P.groups[1].tie_bits == bits(0.25f));
    CHECK(P.groups[2].kind == RGPU_GROUP_TERM && P.groups[2].first_term == 3);
    CHECK((P.run_prefix == std::vector<int64_t>{0, 40 + 64, 40 + 7 + 128, 40 + 7 + 9 + 192, 40 + 7 + 9 + 3 + 256}));
    CHECK(P.fields_named == 3u);
    b.queries[0].min_should_match = 3;
    CHECK(b.plan().queries[0].n_groups == 3 && b.plan().queries[0].need == 3);
    b.queries[0].min_should_match = 4;  // n + 1: can never be met
    CHECK(b.plan().queries[0].n_groups == 0 && b.plan().clause_of.empty() && b.plan().run_prefix == std::vector<int64_t>{0});
  }
  {  // SHOULD with nothing present: dead; MUST_NOT clauses of a dead query are not walked
    Batch b;
    b.dismax_group({0, 0});
    b.query(0, RGPU_OCCUR_SHOULD, 0, {5});
    const FieldsPlan P = b.plan();
    CHECK(P.queries[0].n_groups == 0 && P.queries[0].n_not == 0 && P.clause_of.empty() && P.fields_named == 0u);
  }
  {  // MUST: an absent group kills the leaf; min_should_match has no effect
    Batch b;
    b.term_group(5, 0);
    b.dismax_group({0, 0});
    b.query(0, RGPU_OCCUR_MUST);
    CHECK(b.plan().queries[0].n_groups == 0);
    b.clauses[2].state.doc_freq = 1;
    FieldsPlan P = b.plan();
    CHECK(P.queries[0].n_groups == 2 && P.queries[0].need == 2 && P.queries[0].must == 1);
    CHECK((P.clause_of == std::vector<int32_t>{2, 0}));  // cost 1 before cost 5
    b.queries[0].min_should_match = 7;
    P = b.plan();
    CHECK(P.queries[0].n_groups == 2 && P.queries[0].need == 2);
  }
  {  // MUST: stable by cost; a dismax group's cost is the sum over its PRESENT disjuncts
    Batch b;
    b.term_group(30, 0);              // g0 cost 30
    b.dismax_group({10, 0, 20});      // g1 cost 30: equal to g0, stays behind it
    b.term_group(29, 1);              // g2 cost 29
    b.dismax_group({15, 15});         // g3 cost 30: behind g0 and g1
    b.term_group(31, 1);              // g4
    b.query(0, RGPU_OCCUR_MUST, 0, {0, 4});
    const FieldsPlan P = b.plan();
    CHECK(P.queries[0].n_groups == 5 && P.queries[0].need == 5);
    CHECK((P.clause_of == std::vector<int32_t>{4, 0, 1, 3, 5, 6, 7, 9}));  // g2, g0, g1 (present disjuncts), g3, g4, then the present MUST_NOT clause
    CHECK(P.queries[0].first_not == 7 && P.queries[0].n_not == 1);
    CHECK(P.groups[0].kind == RGPU_GROUP_TERM && P.groups[2].kind == RGPU_GROUP_DISMAX && P.groups[2].n_terms == 2 && P.groups[3].n_terms == 2);
  }
  {  // two queries: ranges follow one another; a dead one in between holds nothing
    Batch b;
    b.term_group(2, 0);
    b.query(0, RGPU_OCCUR_SHOULD);
    b.term_group(0, 1);
    b.query(1, RGPU_OCCUR_MUST);
    b.term_group(1, 1);
    b.term_group(6, 0);
    b.query(2, RGPU_OCCUR_SHOULD, 0, {8});
    const FieldsPlan P = b.plan();
    CHECK(P.queries[1].n_groups == 0 && P.queries[1].n_not == 0);
    CHECK(P.queries[2].first_group == 1 && P.queries[2].n_groups == 2 && P.queries[2].first_not == 3 && P.queries[2].n_not == 1);
    CHECK((P.clause_of == std::vector<int32_t>{0, 2, 3, 4}));
    CHECK(P.run_prefix.back() == 2 + 1 + 6 + 8 + 4 * 64);
  }
}

static void items() {
  Batch b;
  b.term_group(2, 0);
  b.query(0, RGPU_OCCUR_SHOULD);
  FieldsPlan P = b.plan(549, 512, 8);
  CHECK(P.windows_per_query == 2 && P.windows_per_item == 1 && P.items_per_query == 8 && P.items == 8);
  P = b.plan(549, 512, 8, 2);
  CHECK(P.windows_per_query == 2 && P.windows_per_item == 2 && P.items_per_query == 8);
  P = b.plan(512 * 17, 512, 8, 2);
  CHECK(P.windows_per_query == 17 && P.items_per_query == 16 && P.items == 16);  // 9 items of two windows, rounded up to whole workgroups
  P = b.plan(0, 512, 8);
  CHECK(P.windows_per_query == 1 && P.items == 8);
  P = b.plan(512, 512, 8);
  CHECK(P.windows_per_query == 1);
  P = b.plan(513, 512, 8);
  CHECK(P.windows_per_query == 2);
  P = b.plan(2147483647, 512, 8);  // no overflow at the largest segment
  CHECK(P.windows_per_query == 4194304 && P.windows_per_item == 32 && (int64_t)P.items_per_query * P.windows_per_item >= P.windows_per_query);
}

int main() {
  refusals();
  presence_and_order();
  items();
  std::printf("fields_plan_test OK\n");
  return 0;
}
