// csrc/host/phrase_opt_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_phrase_opt_cpu.py):
// validation and every refusal, per-leaf presence, dead queries, the stable cost order of the required side, the clause order of the
// optional side, the run capacities.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rucene_amd/csrc/host/phrase_opt_plan.hpp"

using rgpu_host::PhraseOptArrays;
using rgpu_host::PhraseOptPlan;
using rgpu_host::plan_phrase_opt;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static_assert(sizeof(rgpu_phrase_opt_query) == 64, "rgpu_phrase_opt_query is 64 bytes");

static rgpu_term_state state(int32_t df, int64_t fp) {
  rgpu_term_state s{};
  s.doc_start_fp = fp;
  s.skip_offset = -1;
  s.total_term_freq = df;
  s.doc_freq = df;
  s.singleton_doc_id = df == 1 ? 3 : -1;
  return s;
}

// One query at a time: phrases (required first, then optional) and terms (required, optional, MUST_NOT) in the call's layout, with
// unrelated entries in front so that first_phrase / first_term are not 0.
struct Batch {
  std::vector<rgpu_phrase_query> phrases;
  std::vector<rgpu_phrase_term> phrase_terms;
  std::vector<rgpu_query_term> terms;
  int64_t next_fp = 1000;
  Batch() {
    phrase({7, 7});
    term(5);
  }
  void phrase(std::vector<int32_t> dfs, int32_t slop = 0, std::vector<int64_t> fps = {}) {
    rgpu_phrase_query p{};
    p.n_terms = (int32_t)dfs.size();
    p.first_term = (int32_t)phrase_terms.size();
    p.weight = 1.0f;
    p.slop = slop;
    for (size_t i = 0; i < dfs.size(); ++i) {
      rgpu_phrase_term t{};
      t.state = state(dfs[i], i < fps.size() ? fps[i] : next_fp++);
      t.position = (int32_t)i;
      phrase_terms.push_back(t);
    }
    phrases.push_back(p);
  }
  void term(int32_t df, int64_t fp = -1) {
    rgpu_query_term t{};
    t.state = state(df, fp < 0 ? next_fp++ : fp);
    t.weight = 1.0f;
    terms.push_back(t);
  }
  PhraseOptArrays arrays() const {
    return PhraseOptArrays{phrases.data(), (int32_t)phrases.size(), phrase_terms.data(), (int32_t)phrase_terms.size(), terms.data(), (int32_t)terms.size()};
  }
};

// +"a b"(cost 40) +c(df 20) +d(df 600)  "b c"(cost 60) e(df 9) f(absent)  -n(df 3) -m(absent)
static Batch full(rgpu_phrase_opt_query* q) {
  Batch b;
  *q = rgpu_phrase_opt_query{};
  q->first_phrase = (int32_t)b.phrases.size();
  q->first_term = (int32_t)b.terms.size();
  b.phrase({40, 129}, 0, {11, 12});
  b.phrase({129, 60}, 0, {12, 13});
  b.term(20, 14);
  b.term(600, 15);
  b.term(9, 16);
  b.term(0, 17);
  b.term(3, 18);
  b.term(0, 19);
  q->n_req_phrases = 1;
  q->n_opt_phrases = 1;
  q->n_req_terms = 2;
  q->n_opt_terms = 2;
  q->n_must_not = 2;
  q->req_phrase_slot[0] = 1;  // +c +"a b" +d
  q->opt_phrase_slot[0] = 1;  // e "b c" f
  return b;
}

static void test_full_tree() {
  rgpu_phrase_opt_query q;
  Batch b = full(&q);
  PhraseOptPlan P = plan_phrase_opt(q, b.arrays());
  CHECK(P.status == RGPU_OK && !P.dead);
  // must_weights: c(20), "a b"(40), d(600): already in cost order
  CHECK((P.req_order == std::vector<int32_t>{0, ~0, 1}));
  // the distinct required terms, rarest first: c(20), a(40), b(129), d(600)
  CHECK(P.conj.size() == 4 && P.conj[0]->doc_freq == 20 && P.conj[1]->doc_freq == 40 && P.conj[2]->doc_freq == 129 && P.conj[3]->doc_freq == 600);
  CHECK(P.lead_df == 20 && P.plane_slots == 64);
  CHECK(P.must_not.size() == 1 && P.must_not[0]->doc_freq == 3);
  // should_weights: e, "b c", f; f is absent from the leaf
  CHECK((P.opt_order == std::vector<int32_t>{0, ~0}));
  CHECK((P.opt_capacity == std::vector<int32_t>{60}));
  // the cost order follows the leaf's doc freqs: with c at 700 docs the phrase leads, then d, then c
  b.terms[(size_t)q.first_term].state.doc_freq = 700;
  P = plan_phrase_opt(q, b.arrays());
  CHECK((P.req_order == std::vector<int32_t>{~0, 1, 0}) && P.lead_df == 40 && P.conj[0]->doc_freq == 40);
  // equal costs keep the query's order (a stable sort): c at 40 docs stays in front of the phrase
  b.terms[(size_t)q.first_term].state.doc_freq = 40;
  P = plan_phrase_opt(q, b.arrays());
  CHECK((P.req_order == std::vector<int32_t>{0, ~0, 1}));
  q.req_phrase_slot[0] = 0;  // +"a b" +c +d: now the phrase stays in front
  P = plan_phrase_opt(q, b.arrays());
  CHECK((P.req_order == std::vector<int32_t>{~0, 0, 1}));
}

static void test_presence_and_dead() {
  rgpu_phrase_opt_query q;
  Batch b = full(&q);
  // an optional phrase that lacks a term drops out; with the optional term gone too the row is the required scorer's
  b.phrase_terms[(size_t)b.phrases[(size_t)q.first_phrase + 1].first_term + 1].state.doc_freq = 0;
  PhraseOptPlan P = plan_phrase_opt(q, b.arrays());
  CHECK(P.status == RGPU_OK && !P.dead && (P.opt_order == std::vector<int32_t>{0}) && (P.opt_capacity == std::vector<int32_t>{0}));
  b.terms[(size_t)q.first_term + 2].state.doc_freq = 0;
  P = plan_phrase_opt(q, b.arrays());
  CHECK(P.status == RGPU_OK && !P.dead && P.opt_order.empty() && P.lead_df == 20);
  // a required term absent: dead; a required phrase that lacks a term: dead
  Batch c = full(&q);
  c.terms[(size_t)q.first_term + 1].state.doc_freq = 0;
  P = plan_phrase_opt(q, c.arrays());
  CHECK(P.status == RGPU_OK && P.dead && P.conj.empty() && P.req_order.empty());
  Batch d = full(&q);
  d.phrase_terms[(size_t)d.phrases[(size_t)q.first_phrase].first_term].state.doc_freq = 0;
  P = plan_phrase_opt(q, d.arrays());
  CHECK(P.status == RGPU_OK && P.dead);
}

static void test_no_phrase_and_single_clause() {
  // +t u: no phrase at all, null phrase arrays
  Batch b;
  rgpu_phrase_opt_query q{};
  q.first_term = (int32_t)b.terms.size();
  b.term(129);
  b.term(40);
  q.n_req_terms = 1;
  q.n_opt_terms = 1;
  PhraseOptArrays a = b.arrays();
  a.phrases = nullptr;
  a.n_phrases_total = 0;
  a.phrase_terms = nullptr;
  a.n_phrase_terms_total = 0;
  PhraseOptPlan P = plan_phrase_opt(q, a);
  CHECK(P.status == RGPU_OK && !P.dead && (P.req_order == std::vector<int32_t>{0}) && (P.opt_order == std::vector<int32_t>{0}));
  CHECK(P.lead_df == 129 && P.plane_slots == 192 && P.opt_capacity.empty() && P.must_not.empty());
  // the same term required and optional is one distinct term, and served
  b.terms[(size_t)q.first_term + 1] = b.terms[(size_t)q.first_term];
  P = plan_phrase_opt(q, b.arrays());
  CHECK(P.status == RGPU_OK && P.conj.size() == 1 && P.opt_order.size() == 1);
  // a phrase named while the arrays are missing
  q.n_opt_phrases = 1;
  q.n_opt_terms = 0;
  P = plan_phrase_opt(q, a);
  CHECK(P.status == RGPU_ERR_ILLEGAL_ARGUMENT);
}

static void test_refusals() {
  rgpu_phrase_opt_query q;
  Batch b = full(&q);
  auto rc = [&](const rgpu_phrase_opt_query& x) {
    const PhraseOptPlan P = plan_phrase_opt(x, b.arrays());
    CHECK((P.status == RGPU_OK) == (P.why[0] == 0));
    CHECK(P.status == RGPU_OK || (P.conj.empty() && P.req_order.empty() && P.opt_order.empty()));
    return P.status;
  };
  CHECK(rc(q) == RGPU_OK);
  rgpu_phrase_opt_query x = q;
  x.n_req_phrases = 0; x.n_req_terms = 0;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);  // no required clause
  x = q; x.n_opt_phrases = 0; x.n_opt_terms = 0;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);  // no optional clause
  for (int32_t rgpu_phrase_opt_query::*field : {&rgpu_phrase_opt_query::n_req_phrases, &rgpu_phrase_opt_query::n_opt_phrases, &rgpu_phrase_opt_query::n_req_terms,
                                                &rgpu_phrase_opt_query::n_opt_terms, &rgpu_phrase_opt_query::n_must_not}) {
    x = q; x.*field = -1;
    CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);
  }
  x = q; x.n_req_phrases = RGPU_MAX_BOOL_PHRASES + 1;
  CHECK(rc(x) == RGPU_ERR_UNSUPPORTED);
  x = q; x.n_opt_phrases = RGPU_MAX_BOOL_PHRASES + 1;
  CHECK(rc(x) == RGPU_ERR_UNSUPPORTED);
  x = q; x.min_should_match = 256;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);
  x = q; x.min_should_match = -1;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);
  x = q; x.min_should_match = 255;
  CHECK(rc(x) == RGPU_OK);
  x = q; x.req_phrase_slot[0] = 3;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);
  x = q; x.opt_phrase_slot[0] = -1;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);
  x = q; x.first_phrase = (int32_t)b.phrases.size() - 1;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);  // the phrase range ends outside phrases[]
  x = q; x.first_phrase = -1;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);
  x = q; x.first_term = (int32_t)b.terms.size() - 5;
  CHECK(rc(x) == RGPU_ERR_ILLEGAL_ARGUMENT);
  x = q; x.n_opt_terms = 9;  // ten optional clauses with the phrase
  CHECK(rc(x) == RGPU_ERR_UNSUPPORTED);
  // nine optional clauses are served
  {
    Batch n;
    rgpu_phrase_opt_query y{};
    y.first_phrase = (int32_t)n.phrases.size();
    y.first_term = (int32_t)n.terms.size();
    n.phrase({40, 129});
    n.term(20);
    for (int i = 0; i < 8; ++i) n.term(10 + i);
    y.n_opt_phrases = 1; y.n_req_terms = 1; y.n_opt_terms = 8;
    y.opt_phrase_slot[0] = 8;
    PhraseOptPlan P = plan_phrase_opt(y, n.arrays());
    CHECK(P.status == RGPU_OK && P.opt_order.size() == 9 && P.opt_order[8] == ~0 && P.opt_order[0] == 0);
  }
  // two phrases on one slot
  {
    Batch n;
    rgpu_phrase_opt_query y{};
    y.first_phrase = (int32_t)n.phrases.size();
    y.first_term = (int32_t)n.terms.size();
    n.phrase({40, 129});
    n.phrase({30, 129});
    n.term(20);
    y.n_opt_phrases = 2; y.n_req_terms = 1;
    y.opt_phrase_slot[0] = 1; y.opt_phrase_slot[1] = 1;
    CHECK(plan_phrase_opt(y, n.arrays()).status == RGPU_ERR_ILLEGAL_ARGUMENT);
    y.opt_phrase_slot[1] = 0;
    const PhraseOptPlan P = plan_phrase_opt(y, n.arrays());
    CHECK(P.status == RGPU_OK && (P.opt_order == std::vector<int32_t>{~1, ~0}) && (P.opt_capacity == std::vector<int32_t>{40, 30}));
  }
  // a sloppy phrase on either side; a phrase of one term; a term range outside phrase_terms[]
  b.phrases[(size_t)q.first_phrase + 1].slop = 1;
  CHECK(rc(q) == RGPU_ERR_UNSUPPORTED);
  b.phrases[(size_t)q.first_phrase + 1].slop = -1;
  CHECK(rc(q) == RGPU_ERR_ILLEGAL_ARGUMENT);
  b.phrases[(size_t)q.first_phrase + 1].slop = 0;
  b.phrases[(size_t)q.first_phrase].slop = 2;
  CHECK(rc(q) == RGPU_ERR_UNSUPPORTED);
  b.phrases[(size_t)q.first_phrase].slop = 0;
  b.phrases[(size_t)q.first_phrase].n_terms = 1;
  CHECK(rc(q) == RGPU_ERR_ILLEGAL_ARGUMENT);
  b.phrases[(size_t)q.first_phrase].n_terms = 2;
  b.phrases[(size_t)q.first_phrase].first_term = (int32_t)b.phrase_terms.size() - 1;
  CHECK(rc(q) == RGPU_ERR_ILLEGAL_ARGUMENT);
}

static void test_distinct_term_limit() {
  // RGPU_MAX_QUERY_TERMS distinct terms are served, one more is refused whole - also when the leaf lacks a required clause
  Batch b;
  rgpu_phrase_opt_query q{};
  q.first_term = (int32_t)b.terms.size();
  for (int i = 0; i < RGPU_MAX_QUERY_TERMS - 1; ++i) b.term(100 + i);
  b.term(50);
  b.term(3);
  q.n_req_terms = RGPU_MAX_QUERY_TERMS - 2;
  q.n_opt_terms = 1;
  q.n_must_not = 1;
  CHECK(plan_phrase_opt(q, b.arrays()).status == RGPU_OK);
  q.n_must_not = 2;
  CHECK(plan_phrase_opt(q, b.arrays()).status == RGPU_ERR_UNSUPPORTED);
  b.terms[(size_t)q.first_term].state.doc_freq = 0;
  CHECK(plan_phrase_opt(q, b.arrays()).status == RGPU_ERR_UNSUPPORTED);
  q.n_must_not = 1;
  const PhraseOptPlan P = plan_phrase_opt(q, b.arrays());
  CHECK(P.status == RGPU_OK && P.dead);
}

int main() {
  test_full_tree();
  test_presence_and_dead();
  test_no_phrase_and_single_clause();
  test_refusals();
  test_distinct_term_limit();
  std::printf("phrase_opt_plan_test OK\n");
  return 0;
}
