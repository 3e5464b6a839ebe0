// csrc/host/docset_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_docset_cpu.py): the last
// word of a caller's bit set, which clauses of a collected query exist in the leaf, dead conjunctions, distinct terms and the cost
// order, the (row, term, items) jobs of the list kernel, the refusals, and the mirror's grouping of a mixed batch by key.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rucene_amd/csrc/host/docset_plan.hpp"

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

static void test_words() {
  CHECK(docset_word_count(0) == 0 && docset_word_count(1) == 1 && docset_word_count(64) == 1 && docset_word_count(65) == 2 && docset_word_count(8193) == 129);
  CHECK(docset_word_count(2147483647) == 33554432);
  CHECK(docset_tail_mask(64) == ~0ull && docset_tail_mask(128) == ~0ull && docset_tail_mask(1) == 1ull && docset_tail_mask(63) == (~0ull >> 1) &&
        docset_tail_mask(65) == 1ull);
  for (int32_t max_doc : {1, 63, 64, 65, 127, 128, 129, 8193}) {
    std::vector<uint64_t> w((size_t)docset_word_count(max_doc), ~0ull);  // exactly the words the call may read: ASan watches the end
    const bool whole = max_doc % 64 == 0;
    CHECK(docset_words_valid(w.data(), max_doc) == whole);
    w.back() = docset_tail_mask(max_doc);
    CHECK(docset_words_valid(w.data(), max_doc));
    if (!whole) {
      w.back() |= 1ull << (max_doc & 63);  // the first bit past max_doc
      CHECK(!docset_words_valid(w.data(), max_doc));
      w.back() = 1ull << 63;               // the last bit of the word
      CHECK(!docset_words_valid(w.data(), max_doc));
    }
    w.back() = 1ull << ((max_doc - 1) & 63);  // the last doc alone
    CHECK(docset_words_valid(w.data(), max_doc));
  }
  CHECK(docset_words_valid(nullptr, 0));
}

static void test_query_plans() {
  // terms[]: 0 a(df 300)  1 b(df 5)  2 c(df 40)  3 absent  4 b again  5 d(df 1)  6 c again
  std::vector<rgpu_query_term> t = {term(100, 300), term(200, 5), term(300, 40), term(0, 0), term(200, 5), term(400, 1), term(300, 40)};
  const int64_t n = (int64_t)t.size();
  {  // TERM
    DocsetQueryPlan P = plan_docset_query(query(RGPU_OP_TERM, 1, 0, 0), t.data(), n);
    CHECK(P.status == RGPU_OK && !P.dead && !P.conjunction && P.positive.size() == 1 && P.positive[0] == &t[0].state && P.negative.empty());
    P = plan_docset_query(query(RGPU_OP_TERM, 1, 3, 0), t.data(), n);
    CHECK(P.status == RGPU_OK && P.dead);
    P = plan_docset_query(query(RGPU_OP_TERM, 1, 0, 2), t.data(), n);  // a -b -c
    CHECK(P.status == RGPU_OK && P.positive.size() == 1 && P.negative.size() == 2);
  }
  {  // AND: stable cost order, distinct terms, absent clause, +x -x
    DocsetQueryPlan P = plan_docset_query(query(RGPU_OP_AND, 3, 0, 0), t.data(), n);  // a b c
    CHECK(P.status == RGPU_OK && P.conjunction && P.positive.size() == 3);
    CHECK(P.positive[0] == &t[1].state && P.positive[1] == &t[2].state && P.positive[2] == &t[0].state);
    P = plan_docset_query(query(RGPU_OP_AND, 4, 0, 0), t.data(), n);  // a b c <absent>
    CHECK(P.status == RGPU_OK && P.dead);
    P = plan_docset_query(query(RGPU_OP_AND, 2, 1, 1), t.data(), n);  // b c -<absent>: the MUST_NOT clause drops out
    CHECK(P.status == RGPU_OK && P.conjunction && P.positive.size() == 2 && P.negative.empty());
    P = plan_docset_query(query(RGPU_OP_AND, 2, 4, 1), t.data(), n);  // b d -c
    CHECK(P.status == RGPU_OK && P.conjunction && P.positive[0] == &t[5].state && P.negative.size() == 1 && P.negative[0] == &t[6].state);
    std::vector<rgpu_query_term> r = {term(200, 5), term(200, 5), term(300, 40), term(300, 40)};
    P = plan_docset_query(query(RGPU_OP_AND, 2, 0, 0), r.data(), 4);  // b b: one distinct term, united bit by bit
    CHECK(P.status == RGPU_OK && !P.conjunction && P.positive.size() == 1);
    P = plan_docset_query(query(RGPU_OP_AND, 3, 0, 1), r.data(), 4);  // b b c -c
    CHECK(P.status == RGPU_OK && P.dead);
  }
  {  // OR: absent clauses drop out; nothing left: dead; MUST_NOT only: dead; many clauses
    DocsetQueryPlan P = plan_docset_query(query(RGPU_OP_OR, 5, 0, 0), t.data(), n);  // a b c <absent> b
    CHECK(P.status == RGPU_OK && !P.dead && !P.conjunction && P.positive.size() == 3);
    CHECK(P.positive[0] == &t[0].state && P.positive[1] == &t[1].state && P.positive[2] == &t[2].state);
    P = plan_docset_query(query(RGPU_OP_OR, 1, 3, 0), t.data(), n);
    CHECK(P.status == RGPU_OK && P.dead);
    P = plan_docset_query(query(RGPU_OP_OR, 0, 0, 2), t.data(), n);
    CHECK(P.status == RGPU_OK && P.dead);
    P = plan_docset_query(query(RGPU_OP_OR_MSM(1), 2, 0, 1), t.data(), n);  // a b -c
    CHECK(P.status == RGPU_OK && P.positive.size() == 2 && P.negative.size() == 1);
    P = plan_docset_query(query(RGPU_OP_OR, 1, 6, 0), t.data(), n);  // the last clause of terms[]
    CHECK(P.status == RGPU_OK && P.positive.size() == 1);
    std::vector<rgpu_query_term> many;
    for (int i = 0; i < RGPU_MAX_QUERY_TERMS; ++i) many.push_back(term(1000 + 10 * i, 3 + i));
    P = plan_docset_query(query(RGPU_OP_OR, 16, 0, 0), many.data(), (int64_t)many.size());
    CHECK(P.status == RGPU_OK && P.positive.size() == 16);
    P = plan_docset_query(query(RGPU_OP_OR, RGPU_MAX_QUERY_TERMS - 2, 0, 2), many.data(), (int64_t)many.size());
    CHECK(P.status == RGPU_OK && P.positive.size() == (size_t)RGPU_MAX_QUERY_TERMS - 2 && P.negative.size() == 2);
  }
  {  // the refusals
    CHECK(plan_docset_query(query(RGPU_OP_DISMAX, 2, 0, 0), t.data(), n).status == RGPU_ERR_UNSUPPORTED);
    CHECK(plan_docset_query(query(RGPU_OP_OR_MSM(2), 3, 0, 0), t.data(), n).status == RGPU_ERR_UNSUPPORTED);
    CHECK(plan_docset_query(query(RGPU_OP_TERM, 1, 0, RGPU_NOT_WITH_DEMOTE(0, 1)), t.data(), n).status == RGPU_ERR_UNSUPPORTED);
    CHECK(plan_docset_query(query(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 1), 2, 0, 0), t.data(), n).status == RGPU_ERR_UNSUPPORTED);
    CHECK(plan_docset_query(query(RGPU_OP_WITH_SHOULD(RGPU_OP_TERM, 2) | RGPU_OP_SHOULD_REQUIRED, 1, 0, 0), t.data(), n).status == RGPU_ERR_UNSUPPORTED);
    CHECK(plan_docset_query(query(RGPU_OP_WITH_SHOULD(RGPU_OP_AND, 2) | RGPU_OP_NESTED_MUST, 1, 0, 0), t.data(), n).status == RGPU_ERR_UNSUPPORTED);
    CHECK(plan_docset_query(query(RGPU_OP_AND | RGPU_OP_NESTED_AT(1), 2, 0, 0), t.data(), n).status == RGPU_ERR_UNSUPPORTED);
    CHECK(plan_docset_query(query(RGPU_OP_TERM, 1, 0, 1 << 16), t.data(), n).status == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(plan_docset_query(query(RGPU_OP_TERM, 2, 0, 0), t.data(), n).status == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(plan_docset_query(query(RGPU_OP_AND, 0, 0, 0), t.data(), n).status == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(plan_docset_query(query(RGPU_OP_AND, 3, 5, 0), t.data(), n).status == RGPU_ERR_ILLEGAL_ARGUMENT);   // runs past terms[]
    CHECK(plan_docset_query(query(RGPU_OP_AND, 2, 5, 1), t.data(), n).status == RGPU_ERR_ILLEGAL_ARGUMENT);   // its MUST_NOT clause does
    CHECK(plan_docset_query(query(RGPU_OP_AND, 1, -1, 0), t.data(), n).status == RGPU_ERR_ILLEGAL_ARGUMENT);
    CHECK(plan_docset_query(query(RGPU_OP_OR, RGPU_MAX_QUERY_TERMS, 0, 1), t.data(), n).status == RGPU_ERR_ILLEGAL_ARGUMENT);
    std::vector<rgpu_query_term> neg = {term(5, -3)};
    CHECK(plan_docset_query(query(RGPU_OP_TERM, 1, 0, 0), neg.data(), 1).status == RGPU_ERR_ILLEGAL_ARGUMENT);
    const DocsetQueryPlan P = plan_docset_query(query(RGPU_OP_DISMAX, 2, 0, 0), t.data(), n);
    CHECK(P.why[0] != 0 && P.positive.empty() && P.negative.empty());
  }
}

static void test_jobs() {
  CHECK(docset_term_items(1, 4) == 1 && docset_term_items(2, 4) == 1 && docset_term_items(127, 4) == 1 && docset_term_items(128, 4) == 1);
  CHECK(docset_term_items(129, 4) == 1 && docset_term_items(512, 4) == 1 && docset_term_items(513, 4) == 1 && docset_term_items(640, 4) == 2);
  CHECK(docset_term_items(2176, 4) == 5 && docset_term_items(2304, 4) == 5 && docset_term_items(2176, 1) == 17 && docset_term_items(2304, 1) == 18);
  // terms[]: a(2176) b(5) c(640) d(1) absent
  std::vector<rgpu_query_term> t = {term(100, 2176), term(200, 5), term(300, 640), term(400, 1), term(0, 0)};
  const int64_t n = (int64_t)t.size();
  std::vector<DocsetQueryPlan> plans;
  plans.push_back(plan_docset_query(query(RGPU_OP_TERM, 1, 0, 1), t.data(), n));  // row 0: a -b
  plans.push_back(plan_docset_query(query(RGPU_OP_AND, 3, 0, 0), t.data(), n));   // row 1: a conjunction: no list jobs
  plans.push_back(plan_docset_query(query(RGPU_OP_TERM, 1, 4, 0), t.data(), n));  // row 2: dead
  plans.push_back(plan_docset_query(query(RGPU_OP_OR, 3, 1, 1), t.data(), n));    // row 3: b c d -<absent>
  plans.push_back(plan_docset_query(query(RGPU_OP_OR, 2, 2, 0), t.data(), n));    // row 4: c d
  const DocsetJobs J = plan_docset_jobs(plans, 4);
  CHECK(J.set.size() == 6 && J.clear.size() == 1);
  CHECK(J.set[0].row == 0 && J.set[0].term == &t[0].state && J.set[0].first_item == 0 && J.set[0].n_items == 5);
  CHECK(J.set[1].row == 3 && J.set[1].term == &t[1].state && J.set[1].first_item == 5 && J.set[1].n_items == 1);
  CHECK(J.set[2].row == 3 && J.set[2].term == &t[2].state && J.set[2].first_item == 6 && J.set[2].n_items == 2);
  CHECK(J.set[3].row == 3 && J.set[3].term == &t[3].state && J.set[3].first_item == 8 && J.set[3].n_items == 1);
  CHECK(J.set[4].row == 4 && J.set[4].first_item == 9 && J.set[5].row == 4 && J.set[5].first_item == 11 && J.set_items == 12);
  CHECK(J.clear[0].row == 0 && J.clear[0].term == &t[1].state && J.clear[0].first_item == 0 && J.clear_items == 1);
  // every item of a launch belongs to exactly one job, in order
  int64_t at = 0;
  for (const DocsetListJob& j : J.set) { CHECK(j.first_item == at && j.n_items >= 1); at += j.n_items; }
  CHECK(at == J.set_items);
  CHECK(plan_docset_jobs({}, 4).set.empty());
}

static void test_groups() {
  const DocsetKey none = docset_key({}, {});
  const DocsetKey a = docset_key({7}, {}), a2 = docset_key({7, 7}, {}), ab = docset_key({9, 7}, {}), ba = docset_key({7, 9}, {});
  const DocsetKey a_x = docset_key({7}, {3}), x_a = docset_key({3}, {7});
  CHECK(none.empty() && !a.empty() && a == a2 && ab == ba && !(a == ab) && !(a_x == x_a) && !(a == a_x));
  // caller rows: 0 none, 1 a, 2 ab, 3 none, 4 a(7,7), 5 a-x, 6 ba, 7 a
  const std::vector<DocsetKey> keys = {none, a, ab, none, a2, a_x, ba, a};
  const std::vector<DocsetGroup> G = group_by_docset_key(keys);
  CHECK(G.size() == 4);
  CHECK(G[0].key.empty() && G[0].rows == std::vector<int32_t>({0, 3}));
  CHECK(G[1].key == a && G[1].rows == std::vector<int32_t>({1, 4, 7}));
  CHECK(G[2].key == ab && G[2].rows == std::vector<int32_t>({2, 6}));
  CHECK(G[3].key == a_x && G[3].rows == std::vector<int32_t>({5}));
  std::vector<int> seen(keys.size(), 0);
  for (const DocsetGroup& g : G) for (size_t i = 0; i < g.rows.size(); ++i) { seen[(size_t)g.rows[i]]++; CHECK(i == 0 || g.rows[i - 1] < g.rows[i]); }
  for (int s : seen) CHECK(s == 1);
  CHECK(group_by_docset_key({}).empty());
}

int main() {
  test_words();
  test_query_plans();
  test_jobs();
  test_groups();
  std::printf("docset_plan_test OK\n");
  return 0;
}
