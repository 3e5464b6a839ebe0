// csrc/host/phrase_bool_plan.hpp as a stand-alone program (built with -fsanitize=address,undefined by tests/test_phrase_bool_cpu.py):
// the reference order, the de-duplication of the candidate conjunction's clauses, the plane layout, dead queries, the limits.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rucene_amd/csrc/host/phrase_bool_plan.hpp"

using rgpu_host::PhraseBoolPlan;
using rgpu_host::plan_phrase_bool;

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
  rgpu_phrase_bool_query q{};
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
  void req(rgpu_term_state s) { rgpu_query_term t{}; t.state = s; t.weight = 1.0f; terms.insert(terms.begin() + q.n_terms, t); q.n_terms++; }
  void must_not(rgpu_term_state s) { rgpu_query_term t{}; t.state = s; terms.push_back(t); q.n_must_not++; }
  PhraseBoolPlan plan() { return plan_phrase_bool(q, phrases.data(), pterms.data(), terms.empty() ? nullptr : terms.data()); }
};

int main() {
  const rgpu_term_state a = term(100, 40), b = term(200, 129), c = term(300, 60), r20 = term(400, 20), t40 = term(500, 40), t129 = term(600, 129),
                        d600 = term(700, 600), absent = term(0, 0), n1 = term(800, 3);
  {  // cost below / equal (phrase earlier) / above: "a b" costs 40
    Batch B;
    B.phrase({a, b}, 1);
    B.req(d600); B.req(r20);
    PhraseBoolPlan P = B.plan();  // must_weights: d600, "a b", r20 -> r20, "a b", d600
    CHECK(P.status == RGPU_OK && !P.dead);
    CHECK((P.order == std::vector<int32_t>{1, ~0, 0}));
    CHECK(P.conj.size() == 4 && P.conj[0]->doc_freq == 20 && P.conj[3]->doc_freq == 600 && P.lead_df == 20 && P.plane_slots == 64);
  }
  {  // equal cost: the stable sort keeps must_weights order
    Batch B;
    B.phrase({a, b}, 0);
    B.req(t40);
    CHECK((B.plan().order == std::vector<int32_t>{~0, 0}));
    Batch C;
    C.phrase({a, b}, 1);
    C.req(t40);
    CHECK((C.plan().order == std::vector<int32_t>{0, ~0}));
    Batch D;  // third of three
    D.phrase({a, b}, 0);
    D.req(r20); D.req(term(900, 1));
    PhraseBoolPlan P = D.plan();
    CHECK((P.order == std::vector<int32_t>{1, 0, ~0}) && P.lead_df == 1 && P.plane_slots == 64);
  }
  {  // shared terms: +"a b" +a and +"a b" +"b c" hand the conjunction every term once
    Batch B;
    B.phrase({a, b}, 0);
    B.req(a);
    PhraseBoolPlan P = B.plan();
    CHECK(P.conj.size() == 2 && (P.order == std::vector<int32_t>{~0, 0}));
    Batch C;
    C.phrase({a, b}, 0);
    C.phrase({b, c}, 1);
    P = C.plan();
    CHECK(P.conj.size() == 3 && (P.order == std::vector<int32_t>{~0, ~1}) && P.lead_df == 40 && P.plane_slots == 64);
    Batch D;  // "a b a"
    D.phrase({a, b, a}, 0);
    D.req(t129);
    P = D.plan();
    CHECK(P.conj.size() == 3 && P.conj[0]->doc_start_fp == 100);
  }
  {  // plane slots: the lead's doc_freq rounded up to 64
    CHECK(rgpu_host::pb_round_up_64(0) == 0 && rgpu_host::pb_round_up_64(1) == 64 && rgpu_host::pb_round_up_64(64) == 64 && rgpu_host::pb_round_up_64(65) == 128);
    Batch B;
    B.phrase({b, t129}, 0);
    B.req(d600);
    CHECK(B.plan().plane_slots == 192);
  }
  {  // dead queries; MUST_NOT terms: absent ones dropped, the others once each
    Batch B;
    B.phrase({a, absent}, 0);
    B.req(d600);
    CHECK(B.plan().dead && B.plan().status == RGPU_OK);
    Batch C;
    C.phrase({a, b}, 0);
    C.req(absent);
    CHECK(C.plan().dead);
    Batch D;
    D.phrase({a, b}, 0);
    D.must_not(n1); D.must_not(absent); D.must_not(n1);
    PhraseBoolPlan P = D.plan();
    CHECK(!P.dead && P.must_not.size() == 1 && (P.order == std::vector<int32_t>{~0}));
  }
  {  // refusals
    Batch B;
    B.phrase({a, b}, 0, 1);
    CHECK(B.plan().status == RGPU_ERR_UNSUPPORTED);
    Batch C;
    C.phrase({a, b}, 2);
    C.req(t40);
    CHECK(C.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    Batch D;
    D.phrase({a, b}, 0);
    D.phrase({b, c}, 0);
    CHECK(D.plan().status == RGPU_ERR_ILLEGAL_ARGUMENT);
    Batch E;
    for (int i = 0; i < 5; ++i) E.phrase({a, b}, i);
    CHECK(E.plan().status == RGPU_ERR_UNSUPPORTED);
    Batch F;
    F.q.n_phrases = 0;
    CHECK(F.plan().status == RGPU_ERR_UNSUPPORTED);
    Batch G;  // RGPU_MAX_QUERY_TERMS distinct terms pass, one more is refused
    G.phrase({a, b}, 0);
    for (int i = 0; i < RGPU_MAX_QUERY_TERMS - 2; ++i) G.req(term(10000 + 10 * i, 50 + i));
    CHECK(G.plan().status == RGPU_OK && G.plan().conj.size() == (size_t)RGPU_MAX_QUERY_TERMS);
    G.must_not(n1);
    CHECK(G.plan().status == RGPU_ERR_UNSUPPORTED && G.plan().conj.empty());
  }
  std::printf("phrase_bool_plan_test OK\n");
  return 0;
}
