// csrc/host/count_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_count_cpu.py): every kind
// decision of a counted row (ZERO, DOC_FREQ, LIST, CONJ, WINDOWS), the thresholds `need` / `need_not` with clause multiplicities, the
// refusals, and the sizing of the window kernel's work items.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "../../rucene_amd/csrc/host/count_plan.hpp"

using namespace rgpu_host;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static rgpu_query_term term(int64_t fp, int32_t df) {
  rgpu_query_term t{};
  t.state.doc_start_fp = fp;
  t.state.skip_offset = -1;
  t.state.total_term_freq = 2 * (int64_t)df;
  t.state.doc_freq = df;
  t.state.singleton_doc_id = df == 1 ? 7 : -1;
  t.weight = 1.0f;
  return t;
}
static rgpu_query query(int32_t op, int32_t n_terms, int32_t first, int32_t n_not) {
  rgpu_query q{};
  q.op = op;
  q.n_terms = n_terms;
  q.first_term = first;
  q.n_must_not = n_not;
  return q;
}

// exactly the clauses a row may read: ASan watches both ends
struct Row {
  std::vector<rgpu_query_term> t;
  rgpu_query q;
  CountRowPlan plan(const CountMask& m = CountMask{}) const { return plan_count_query(q, t.data(), (int64_t)t.size(), m); }
};
static const rgpu_query_term a = term(100, 300), b = term(200, 5), c = term(300, 40), absent = term(400, 0), d = term(500, 1), e = term(600, 40);
// (a plan points into its row's clauses: the rows live as long as the program)
static std::deque<Row> g_rows;
static Row& row(int32_t op, std::vector<rgpu_query_term> pos, std::vector<rgpu_query_term> behind = {}, int32_t n_not = -1, int32_t n_demote = 0) {
  Row r;
  const int32_t opt = (op >> 16) & 0xff;
  const int32_t n_pos = (int32_t)pos.size() - opt;
  r.t = pos;
  r.t.insert(r.t.end(), behind.begin(), behind.end());
  if (n_not < 0) n_not = (int32_t)behind.size();
  r.q = query(op, n_pos, 0, RGPU_NOT_WITH_DEMOTE(n_not, n_demote));
  if (r.t.empty()) r.t.push_back(absent);
  g_rows.push_back(r);
  return g_rows.back();
}
static bool is(const rgpu_term_state* st, const rgpu_query_term& t) { return ds_same_term(*st, t.state); }

static void test_kinds() {
  const CountMask plain{}, deleted{true, false, false}, masked{false, true, false}, empty{false, true, true};
  // ---- a lone term
  CountRowPlan P = row(RGPU_OP_TERM, {a}).plan();
  CHECK(P.status == RGPU_OK && P.kind == COUNT_DOC_FREQ && P.doc_freq == 300 && P.positive.empty());
  CHECK(row(RGPU_OP_TERM, {a}).plan(deleted).kind == COUNT_LIST && row(RGPU_OP_TERM, {a}).plan(masked).kind == COUNT_LIST);
  P = row(RGPU_OP_TERM, {d}).plan(deleted);
  CHECK(P.kind == COUNT_LIST && P.positive.size() == 1 && is(P.positive[0].term, d) && P.negative.empty());
  CHECK(row(RGPU_OP_TERM, {a}).plan(empty).kind == COUNT_ZERO);                      // the empty set goes before every other rule
  CHECK(row(RGPU_OP_AND, {a, c}).plan(empty).kind == COUNT_ZERO && row(RGPU_OP_OR, {a, c}).plan(empty).kind == COUNT_ZERO);
  CHECK(row(RGPU_OP_TERM, {absent}).plan().kind == COUNT_ZERO);
  CHECK(row(RGPU_OP_AND, {a}).plan().kind == COUNT_DOC_FREQ && row(RGPU_OP_AND, {a, a}).plan().kind == COUNT_DOC_FREQ);        // +a +a is +a
  CHECK(row(RGPU_OP_OR, {a}).plan().kind == COUNT_DOC_FREQ && row(RGPU_OP_OR, {a, absent}).plan().doc_freq == 300);
  CHECK(row(RGPU_OP_OR_MSM(2), {a, a}).plan().kind == COUNT_DOC_FREQ);               // min_should_match counts clauses: (a, a), msm 2 is a
  CHECK(row(RGPU_OP_OR_MSM(3), {a, a}).plan().kind == COUNT_ZERO);
  CHECK(row(RGPU_OP_OR_MSM(2), {a, absent}).plan().kind == COUNT_ZERO);              // the absent clause drops out, msm stays
  CHECK(row(RGPU_OP_TERM, {a}, {absent}).plan().kind == COUNT_DOC_FREQ);             // an absent MUST_NOT clause excludes nothing
  CHECK(row(RGPU_OP_DISMAX, {a}).plan().kind == COUNT_DOC_FREQ && row(RGPU_OP_DISMAX, {absent}).plan().kind == COUNT_ZERO);
  // ---- a lone term with something to exclude: the window kernel, bit form
  P = row(RGPU_OP_TERM, {a}, {c}).plan();
  CHECK(P.kind == COUNT_WINDOWS && P.bit_form() && P.positive.size() == 1 && P.negative.size() == 1 && is(P.negative[0].term, c));
  CHECK(row(RGPU_OP_AND, {a}, {c}).plan(deleted).kind == COUNT_WINDOWS);
  CHECK(row(RGPU_OP_TERM, {a}, {a}).plan().kind == COUNT_ZERO && row(RGPU_OP_AND, {a, c}, {c}).plan().kind == COUNT_ZERO);     // +a -a
  // ---- conjunctions: distinct terms, stable cost order, MUST_NOT distinct
  P = row(RGPU_OP_AND, {a, c, b, e, c}, {d, absent, d}).plan(deleted);
  CHECK(P.kind == COUNT_CONJ && P.positive.size() == 4 && is(P.positive[0].term, b) && is(P.positive[1].term, c) && is(P.positive[2].term, e) && is(P.positive[3].term, a));
  CHECK(P.negative.size() == 1 && is(P.negative[0].term, d) && P.negative[0].mult == 1);
  CHECK(row(RGPU_OP_AND, {a, absent}).plan().kind == COUNT_ZERO && row(RGPU_OP_AND, {absent, a, c}).plan().kind == COUNT_ZERO);
  // ---- unions and thresholds
  P = row(RGPU_OP_OR, {a, b, absent, a}).plan();
  CHECK(P.kind == COUNT_WINDOWS && P.bit_form() && P.positive.size() == 2 && P.positive[0].mult == 1 && P.negative.empty());
  CHECK(row(RGPU_OP_OR_MSM(1), {a, b}).plan().bit_form() && row(RGPU_OP_DISMAX, {a, b}).plan().bit_form());
  P = row(RGPU_OP_OR_MSM(2), {a, b, a, absent}).plan();
  CHECK(P.kind == COUNT_WINDOWS && !P.bit_form() && P.need == 2 && P.need_not == 1 && P.positive.size() == 2 && is(P.positive[0].term, a) && P.positive[0].mult == 2 &&
        P.positive[1].mult == 1);
  CHECK(row(RGPU_OP_OR_MSM(3), {a, b, c}).plan().need == 3 && row(RGPU_OP_OR_MSM(4), {a, b, c}).plan().kind == COUNT_ZERO);
  CHECK(row(RGPU_OP_OR, {absent, absent}).plan().kind == COUNT_ZERO && row(RGPU_OP_OR, {}, {a}).plan().kind == COUNT_ZERO);  // no SHOULD left; MUST_NOT only
  CHECK(row(RGPU_OP_OR, {absent}, {a}).plan().kind == COUNT_ZERO);
  // MUST_NOT: every present clause excludes its docs - ReqNotScorer advance()s the prohibited disjunction, and advance() does not
  // look at min_should_match (disjunction_scorer.rs:75-89)
  P = row(RGPU_OP_OR_MSM(2), {a, b}, {c, e}).plan();
  CHECK(P.kind == COUNT_WINDOWS && P.need == 2 && P.need_not == 1 && P.negative.size() == 2);
  P = row(RGPU_OP_OR_MSM(2), {a, b}, {c, absent}).plan();
  CHECK(P.need == 2 && P.need_not == 1 && P.negative.size() == 1);                   // one present, one absent
  P = row(RGPU_OP_OR_MSM(2), {a, b}, {c, c}).plan();
  CHECK(P.need_not == 1 && P.negative.size() == 1 && P.negative[0].mult == 1);
  P = row(RGPU_OP_OR_MSM(3), {a, b, c}, {e, d}).plan();
  CHECK(P.need == 3 && P.need_not == 1 && P.negative.size() == 2);
  P = row(RGPU_OP_OR, {a, b}, {c, e}).plan();
  CHECK(P.bit_form() && P.negative.size() == 2);
  // ---- optional clauses are skipped, and their min_should_match byte with them
  P = row(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 2), {a, c, b, e}).plan();
  CHECK(P.kind == COUNT_CONJ && P.positive.size() == 2 && is(P.positive[0].term, c));
  P = row(RGPU_OP_WITH_SHOULD(RGPU_OP_TERM, 1) | (2 << 8), {a, b}).plan();
  CHECK(P.kind == COUNT_DOC_FREQ && P.doc_freq == 300);
  P = row(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 1), {a, c, b}, {e}).plan();
  CHECK(P.kind == COUNT_CONJ && P.negative.size() == 1 && is(P.negative[0].term, e));
  P = row(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 1) | (2 << 8), {a, c, b}, {e, d}).plan();
  CHECK(P.kind == COUNT_CONJ && P.positive.size() == 2 && P.negative.size() == 2);   // (the byte has no effect beside MUST clauses
  // ---- a demote byte: the leaf rule, otherwise ignored
  CHECK(row(RGPU_OP_TERM, {a}, {b}, 0, 1).plan().kind == COUNT_DOC_FREQ && row(RGPU_OP_TERM, {a}, {absent}, 0, 1).plan().kind == COUNT_ZERO);
  P = row(RGPU_OP_OR, {a, b}, {c, absent, e}, 1, 2).plan();
  CHECK(P.kind == COUNT_WINDOWS && P.negative.size() == 1 && is(P.negative[0].term, c));
  CHECK(row(RGPU_OP_AND, {a, c}, {absent, absent}, 0, 2).plan().kind == COUNT_ZERO);
  (void)plain;
}

static void test_refusals() {
  auto status = [](const Row& r) { return r.plan().status; };
  CHECK(status(row(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 1) | RGPU_OP_SHOULD_REQUIRED, {a, c, b})) == RGPU_ERR_UNSUPPORTED);
  CHECK(status(row(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 2) | RGPU_OP_NESTED_MUST, {a, c, b, e})) == RGPU_ERR_UNSUPPORTED);
  CHECK(status(row(RGPU_OP_WITH_SHOULD(RGPU_OP_OR, 1) | RGPU_OP_SHOULD_REQUIRED, {a, c, b})) == RGPU_ERR_ILLEGAL_ARGUMENT);   // malformed goes first
  CHECK(status(row(RGPU_OP_DISMAX + 1, {a})) == RGPU_ERR_ILLEGAL_ARGUMENT && status(row(RGPU_OP_OR | (1 << 30), {a, b})) == RGPU_ERR_ILLEGAL_ARGUMENT);
  CHECK(status(row(RGPU_OP_DISMAX | (1 << 8), {a, b})) == RGPU_ERR_ILLEGAL_ARGUMENT);
  CHECK(status(row(RGPU_OP_AND | (2 << 8), {a, b})) == RGPU_ERR_ILLEGAL_ARGUMENT);                   // min_should_match needs SHOULD clauses
  CHECK(status(row(RGPU_OP_WITH_SHOULD(RGPU_OP_OR, 1), {a, b})) == RGPU_ERR_ILLEGAL_ARGUMENT);
  CHECK(status(row(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 1), {a, c, b}, {e}, 0, 1)) == RGPU_ERR_UNSUPPORTED);  // demote beside optional clauses, as the search
  Row r = row(RGPU_OP_TERM, {a});  // (copies: only statuses are read below)
  r.q.n_terms = 2;
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r = row(RGPU_OP_AND, {a, c});
  r.q.n_terms = 3;                                                                                  // one past terms[]
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r.q.n_terms = 2;
  r.q.first_term = -1;
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r.q.first_term = 1;
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r.q.first_term = 0;
  r.q.n_terms = RGPU_MAX_QUERY_TERMS + 1;
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r = row(RGPU_OP_OR, {a, c});
  r.q.n_must_not = 1 << 16;
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r = row(RGPU_OP_OR, {a, c});
  r.q.n_terms = 0;                                                                                  // an OR of nothing
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r = row(RGPU_OP_OR, {a, term(700, -1)});
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  r = row(RGPU_OP_DISMAX, {a, c});
  const float inf = 1.0f / 0.0f;
  std::memcpy(&r.q.n_must_not, &inf, 4);
  CHECK(r.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
  const float tie = 0.3f;                                                                           // a tie-breaker is not a count of clauses
  std::memcpy(&r.q.n_must_not, &tie, 4);
  CHECK(r.plan().status == RGPU_OK && r.plan().kind == COUNT_WINDOWS && r.plan().negative.empty());
  // 64 clauses fit, 65 do not
  std::vector<rgpu_query_term> many;
  for (int i = 0; i < 64; ++i) many.push_back(term(1000 + 16 * i, 2));
  CountRowPlan P = row(RGPU_OP_OR_MSM(64), many).plan();
  CHECK(P.status == RGPU_OK && P.kind == COUNT_WINDOWS && P.need == 64 && P.positive.size() == 64);
  many.pop_back();
  CHECK(row(RGPU_OP_OR_MSM(64), many).plan().kind == COUNT_ZERO);
  CHECK(row(RGPU_OP_OR, many, {a, b}).plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
}

static void test_items() {
  CHECK(count_windows(0, 2048) == 0 && count_windows(1, 2048) == 1 && count_windows(2048, 2048) == 1 && count_windows(2049, 2048) == 2);
  CHECK(count_windows(2147483647, 2048) == 1048576);
  CHECK(count_window_items(4133, 2048, 1) == 3 && count_window_items(4133, 2048, 2) == 2 && count_window_items(4133, 2048, 3) == 1);
  CHECK(count_windows_per_item(4133, 2048, 10, 8192, 0) == 1 && count_windows_per_item(4133, 2048, 10, 8192, 2) == 2 && count_windows_per_item(4133, 2048, 10, 8192, 1000) == 3);
  CHECK(count_windows_per_item(10000000, 2048, 1024, 8192, 0) == 611);   // 4883 windows over 8 items per row
  CHECK(count_windows_per_item(10000000, 2048, 100000, 8192, 0) == 4883 && count_windows_per_item(1, 2048, 1, 8192, 0) == 1);
  for (int32_t max_doc : {1, 2047, 2048, 2049, 4133, 10000000})
    for (int32_t per : {1, 2, 7, 5000}) {
      const int32_t p = count_windows_per_item(max_doc, 2048, 1, 8192, per);
      CHECK(p >= 1 && count_window_items(max_doc, 2048, p) * p >= count_windows(max_doc, 2048) && (count_window_items(max_doc, 2048, p) - 1) * p < count_windows(max_doc, 2048));
    }
}

int main() {
  test_kinds();
  test_refusals();
  test_items();
  std::printf("count_plan_test OK\n");
  return 0;
}
