// csrc/host/phrase_or_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_phrase_or_cpu.py):
// the clause order, which clauses exist in the leaf, dead queries, the run capacities, the MUST_NOT terms, the limits and refusals.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rucene_amd/csrc/host/phrase_or_plan.hpp"

using rgpu_host::PhraseOrPlan;
using rgpu_host::plan_phrase_or;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static rgpu_term_state term(int64_t fp, int32_t df) {
  rgpu_term_state s{};
  s.doc_start_fp = fp;
  s.skip_offset = -1;
  s.total_term_freq = 2 * (int64_t)df;
  s.doc_freq = df;
  s.singleton_doc_id = df == 1 ? 7 : -1;
  return s;
}

struct Batch {
  std::vector<rgpu_phrase_query> phrases;
  std::vector<rgpu_phrase_term> pterms;
  std::vector<rgpu_query_term> terms;
  rgpu_phrase_or_query q{};
  void phrase(std::vector<rgpu_term_state> ts, int slot, int slop = 0) {
    rgpu_phrase_query p{};
    p.n_terms = (int32_t)ts.size();
    p.first_term = (int32_t)pterms.size();
    p.weight = 1.0f;
    p.slop = slop;
    for (size_t i = 0; i < ts.size(); ++i) {
      rgpu_phrase_term t{};
      t.state = ts[i];
      t.position = (int32_t)i;
      pterms.push_back(t);
    }
    phrases.push_back(p);
    if (q.n_phrases < RGPU_MAX_BOOL_PHRASES) q.phrase_slot[q.n_phrases] = slot;
    q.n_phrases++;
  }
  void should(rgpu_term_state s) { rgpu_query_term t{}; t.state = s; t.weight = 1.0f; terms.insert(terms.begin() + q.n_terms, t); q.n_terms++; }
  void must_not(rgpu_term_state s) { rgpu_query_term t{}; t.state = s; terms.push_back(t); q.n_must_not++; }
  PhraseOrPlan plan() { return plan_phrase_or(q, phrases.data(), pterms.data(), terms.empty() ? nullptr : terms.data()); }
};

int main() {
  const rgpu_term_state a = term(100, 40), b = term(200, 129), c = term(300, 60), r20 = term(400, 20), t40 = term(500, 40), d600 = term(700, 600),
                        absent = term(0, 0), n1 = term(800, 3), n2 = term(900, 5), one = term(1000, 1);
  {  // the clause order is the query's, whatever the costs: P T T, T P T, T T P
    for (int slot = 0; slot < 3; ++slot) {
      Batch B;
      B.phrase({a, b}, slot);
      B.should(d600); B.should(r20);
      PhraseOrPlan P = B.plan();
      CHECK(P.status == RGPU_OK && !P.dead);
      std::vector<int32_t> want{0, 1};
      want.insert(want.begin() + slot, ~0);
      CHECK(P.order == want);
      CHECK((P.capacity == std::vector<int32_t>{40}) && P.must_not.empty() && P.min_should_match == 0);
    }
  }
  {  // capacities: the smallest doc_freq among the phrase's terms; cost 1 and cost 2 need no special case
    Batch B;
    B.phrase({b, c, d600}, 0);
    B.phrase({one, b}, 1);
    B.phrase({term(1100, 2), b}, 2);
    B.phrase({a, b, a}, 3);  // a repeated term
    PhraseOrPlan P = B.plan();
    CHECK(P.status == RGPU_OK && (P.capacity == std::vector<int32_t>{60, 1, 2, 40}) && (P.order == std::vector<int32_t>{~0, ~1, ~2, ~3}));
  }
  {  // clauses the leaf lacks drop out; min_should_match stays; the same phrase twice stays twice
    Batch B;
    B.phrase({a, absent}, 1);
    B.phrase({a, b}, 3);
    B.phrase({a, b}, 4);
    B.should(absent); B.should(r20);
    B.q.min_should_match = 3;
    PhraseOrPlan P = B.plan();  // should_weights: absent, "a absent", r20, "a b", "a b"
    CHECK(P.status == RGPU_OK && !P.dead && (P.order == std::vector<int32_t>{1, ~1, ~2}) && (P.capacity == std::vector<int32_t>{0, 40, 40}));
    CHECK(P.min_should_match == 3);
  }
  {  // dead: every SHOULD clause dropped (MUST_NOT terms do not keep it alive)
    Batch B;
    B.phrase({a, absent}, 0);
    B.should(absent);
    B.must_not(n1);
    PhraseOrPlan P = B.plan();
    CHECK(P.status == RGPU_OK && P.dead && P.order.empty() && P.must_not.empty());
  }
  {  // MUST_NOT terms: absent ones dropped, the others once each
    Batch B;
    B.phrase({a, b}, 0);
    B.must_not(n1); B.must_not(absent); B.must_not(n1); B.must_not(n2);
    PhraseOrPlan P = B.plan();
    CHECK(!P.dead && P.must_not.size() == 2 && P.must_not[0]->doc_start_fp == 800 && P.must_not[1]->doc_start_fp == 900 && (P.order == std::vector<int32_t>{~0}));
  }
  {  // refusals
    Batch B;  // sloppy
    B.phrase({a, b}, 0, 1);
    B.should(t40);
    CHECK(B.plan().status == RGPU_ERR_UNSUPPORTED);
    Batch C;  // slot out of range
    C.phrase({a, b}, 2);
    C.should(t40);
    CHECK(C.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    C.q.phrase_slot[0] = -1;
    CHECK(C.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    Batch D;  // a slot named twice
    D.phrase({a, b}, 0);
    D.phrase({b, c}, 0);
    CHECK(D.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    Batch E;  // five phrases
    for (int i = 0; i < 5; ++i) E.phrase({a, b}, i);
    CHECK(E.plan().status == RGPU_ERR_UNSUPPORTED);
    Batch F;  // none
    F.q.n_phrases = 0;
    CHECK(F.plan().status == RGPU_ERR_UNSUPPORTED);
    Batch G;  // nine SHOULD clauses pass, ten sum in heap order
    G.phrase({a, b}, 8);
    for (int i = 0; i < 8; ++i) G.should(term(2000 + 10 * i, 50 + i));
    CHECK(G.plan().status == RGPU_OK && G.plan().order.size() == 9 && G.plan().order[8] == ~0);
    G.should(term(5000, 9));
    CHECK(G.plan().status == RGPU_ERR_UNSUPPORTED);
    Batch H;  // min_should_match and clause counts
    H.phrase({a, b}, 0);
    H.q.min_should_match = 255;
    CHECK(H.plan().status == RGPU_OK && H.plan().min_should_match == 255);
    H.q.min_should_match = 256;
    CHECK(H.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    H.q.min_should_match = -1;
    CHECK(H.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    H.q.min_should_match = 0;
    H.q.n_must_not = -1;
    CHECK(H.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    Batch I;  // RGPU_MAX_QUERY_TERMS distinct terms pass, one more is refused — with nothing filled
    I.phrase({a, b}, 0);
    for (int i = 0; i < RGPU_MAX_QUERY_TERMS - 2; ++i) I.must_not(term(10000 + 10 * i, 50 + i));
    CHECK(I.plan().status == RGPU_OK && I.plan().must_not.size() == (size_t)RGPU_MAX_QUERY_TERMS - 2);
    I.must_not(n1);
    PhraseOrPlan P = I.plan();
    CHECK(P.status == RGPU_ERR_UNSUPPORTED && P.order.empty() && P.must_not.empty() && P.capacity.empty());
    Batch J;  // clause positions: SHOULD children and MUST_NOT terms share the window kernel's 64 lanes
    J.phrase({a, b}, 0);
    J.should(a); J.should(b);
    for (int i = 0; i < RGPU_MAX_QUERY_TERMS - 3; ++i) J.must_not(term(10000 + 10 * i, 50 + i));
    CHECK(J.plan().status == RGPU_OK);  // 3 + 61 positions, 63 distinct terms
    J.must_not(n1);
    CHECK(J.plan().status == RGPU_ERR_UNSUPPORTED);  // 65 positions of 64 distinct terms
  }
  std::printf("phrase_or_plan_test OK\n");
  return 0;
}
