// C++ host-side mirror of the slice of Rucene's search API served by the GPU path, header-only over the C ABI
// (include/rucene_gpu.h). The reference is compiled Rust and this image has no Rust toolchain, so the layer a
// Rucene maintainer would write as a Rust shim is provided in C++ with the reference's names,
// argument meaning and error behaviour (paths relative to /root/reference/src/core):
//
//   search/searcher.rs:205-249, 306-363, 487-525, 732-767   IndexSearcher::search + the largest-leaf statistics
//   search/query/term_query.rs:45-95                         TermQuery::new(term, boost), create_weight
//   search/query/boolean_query.rs:40-86                      BooleanQuery::build
//   search/collector/top_docs.rs:97-183                      TopDocsCollector::new(k), top_docs()
//   search/sort_field/collapse_top_docs.rs:22-36             ScoreDoc
//   error.rs:24-91                                           ErrorKind -> rucene::Error{kind}
//
// Terms are named either by bytes — resolved per leaf through its block-tree dictionary (rgpu_terms_*, the
// TermIterator::seek_exact + term_state step of TermWeight::create_scorer, term_query.rs:150-180) — or, for synthetic
// indexes, by an id into a flat table of BlockTermState records.
#pragma once
#include <dirent.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../../include/rucene_gpu.h"
#include "bm25_similarity.hpp"
#include "docset_plan.hpp"

namespace rucene {

struct Error : std::runtime_error {
  int kind;  // rgpu_status == error.rs ErrorKind
  Error(int k, const std::string& m) : std::runtime_error(m), kind(k) {}
};
inline void check(int32_t rc) {
  if (rc < 0) throw Error(rc, rgpu_last_error(nullptr));
}

struct ScoreDoc {
  int32_t doc;
  float score;
};

class TopDocs {
 public:
  TopDocs() = default;
  TopDocs(int64_t total, std::vector<ScoreDoc> docs) : total_(total), docs_(std::move(docs)) {}
  int64_t total_hits() const { return total_; }
  const std::vector<ScoreDoc>& score_docs() const { return docs_; }  // score desc, then doc asc

 private:
  int64_t total_ = 0;
  std::vector<ScoreDoc> docs_;
};

class TopDocsCollector {
 public:
  explicit TopDocsCollector(size_t estimated_hits) : estimated_hits_(estimated_hits) {}
  bool needs_scores() const { return true; }
  size_t estimated_hits() const { return estimated_hits_; }
  TopDocs top_docs() const { return result_; }
  void set_result(TopDocs r) { result_ = std::move(r); }

 private:
  size_t estimated_hits_;
  TopDocs result_;
};

struct Query {
  virtual ~Query() {}
};
struct TermQuery : Query {
  int64_t term = -1;   // id into LeafReader::terms, or -1 when the term is named by bytes
  std::string text;    // Term::bytes
  float boost;
  explicit TermQuery(int64_t t, float b = 1.0f) : term(t), boost(b) {}
  explicit TermQuery(std::string bytes, float b = 1.0f) : text(std::move(bytes)), boost(b) {}
  bool by_text() const { return term < 0; }
  // The indexed field the term lives in; empty = the leaves' primary field (LeafReader::field). Another field must be one of the
  // leaves' extra_fields: GpuIndexSearcher::search / search_many route such trees to rgpu_search_fields_batch, every other path
  // (count, rescoring, cached filters) answers UnsupportedOperation for them.
  std::string field;
  TermQuery in(std::string f) const { TermQuery t(*this); t.field = std::move(f); return t; }
};
// search/query/match_all_query.rs: every doc, ConstantScoreScorer with the weight's default of 0.0. Served by a searcher whose
// required_sets is on: alone, and as the `query` of a FilteredQuery — clauses(MatchAllDocsQuery, {F}, {X}) is "#F -X", which is
// "+*:* #F -X" (boolean_query.rs:76-79 gives a query of MUST_NOT clauses alone the MUST clause).
struct MatchAllDocsQuery : Query {};
struct BooleanQuery : Query {
  std::vector<TermQuery> must_queries, should_queries, must_not_queries;
  int32_t min_should_match = 0;
  // RGPU_OP_SHOULD_REQUIRED: the SHOULD clauses are a should-only BooleanQuery nested under MUST ("+a +(b c)") — set by
  // NestedBooleanQuery::required_disjunction, never by build()
  bool should_required = false;
  // RGPU_OP_NESTED_MUST: the SHOULD slots hold a must-only BooleanQuery nested under MUST ("+a +(+b +c)") — set by
  // NestedBooleanQuery::nested_conjunction
  bool nested_must = false;
  int32_t nested_at = 0;  // RGPU_OP_NESTED_AT: how many of the MUST term clauses stood before the nested clause in the caller's query
  // boolean_query.rs:40-86 restricted to what the GPU path serves: SHOULD-only term trees, or MUST clauses with optional
  // SHOULD clauses beside them (ReqOptScorer, its sequential skipping rule included: see RGPU_OP_WITH_SHOULD), each
  // optionally with MUST_NOT term clauses (ReqNotScorer); a single clause without MUST_NOTs
  // collapses to that clause
  // FILTER clauses are required clauses that score 0 (create_weight with needs_scores = false -> NonScoringSimilarity,
  // boolean_query.rs:106-108, searcher.rs:158-202): they join the MUST clauses with boost 0, which leaves every sum unchanged
  static std::unique_ptr<Query> build(std::vector<TermQuery> musts, std::vector<TermQuery> shoulds, int32_t min_should_match = 0,
                                      std::vector<TermQuery> must_nots = {}, std::vector<TermQuery> filters = {}) {
    const int32_t msm = min_should_match > 0 ? min_should_match : (musts.empty() ? 1 : 0);
    if (musts.empty() && shoulds.empty() && must_nots.empty() && filters.empty())
      throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "boolean query should at least contain one inner query!");
    for (TermQuery& f : filters) f.boost = 0.0f;
    if (must_nots.empty() && musts.size() + shoulds.size() + filters.size() == 1)  // a lone FILTER: ConstantScoreQuery, boost 0
      return std::unique_ptr<Query>(new TermQuery(!filters.empty() ? filters[0] : (musts.empty() ? shoulds[0] : musts[0])));
    musts.insert(musts.end(), filters.begin(), filters.end());
    if (msm > 255) throw Error(RGPU_ERR_UNSUPPORTED, "min_should_match above 255");
    // (beside MUST clauses min_should_match has no effect — ReqOptScorer only advances the optional scorer — and a tree of
    // MUST_NOT clauses only matches nothing: BooleanWeight::create_scorer -> None)
    auto q = std::unique_ptr<BooleanQuery>(new BooleanQuery());
    q->must_queries = std::move(musts);
    q->should_queries = std::move(shoulds);
    q->must_not_queries = std::move(must_nots);
    q->min_should_match = q->must_queries.empty() ? msm : 0;
    return std::unique_ptr<Query>(q.release());
  }
};

// query/disjunction_max_query.rs:43-114: the union of the disjuncts' docs, each scored max + (sum - max) * tie_breaker_multiplier over
// the disjuncts that hold it (DisjunctionMaxScorer, scorer/disjunction_scorer.rs:106-185, 246-286). TermQuery disjuncts only here
// (RGPU_OP_DISMAX); a dismax over other queries is the caller's CPU path.
struct DisjunctionMaxQuery : Query {
  std::vector<TermQuery> disjuncts;
  float tie_breaker_multiplier;
  explicit DisjunctionMaxQuery(std::vector<TermQuery> d, float tie = 0.0f) : disjuncts(std::move(d)), tie_breaker_multiplier(tie) {
    if (disjuncts.empty()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "DisjunctionMaxQuery: sub query should not be empty!");  // ::build, :51-68
  }
  // DisjunctionMaxQuery::build: a lone disjunct IS that query
  static std::unique_ptr<Query> build(std::vector<TermQuery> d, float tie = 0.0f) {
    std::unique_ptr<DisjunctionMaxQuery> q(new DisjunctionMaxQuery(std::move(d), tie));
    if (q->disjuncts.size() == 1) return std::unique_ptr<Query>(new TermQuery(q->disjuncts[0]));
    return std::unique_ptr<Query>(q.release());
  }
  // rgpu_query.n_must_not of an RGPU_OP_DISMAX query: the multiplier's f32 bit pattern
  int32_t tie_bits() const {
    int32_t bits;
    std::memcpy(&bits, &tie_breaker_multiplier, sizeof bits);
    return bits;
  }
  std::vector<TermQuery> extract_terms() const { return disjuncts; }  // :91-97
};

// BooleanQuery over TermQuery and DisjunctionMaxQuery-of-TermQuery clauses whose terms may live in different fields - the multi-field
// query "(title:a | body:a) (title:b | body:b)" every query parser emits (rgpu_search_fields_batch in include/rucene_gpu.h): all
// SHOULD (min_should_match counts groups) or all MUST, with MUST_NOT TermQuery clauses of any field. A BooleanQuery / DisjunctionMaxQuery
// / TermQuery that names a further field is served the same way (GpuIndexSearcher::cross_spec). Ten or more groups or disjuncts are
// UnsupportedOperation when searched: the reference sums those in heap order.
// With GpuIndexSearcher::field_trees = true the trees QueryStringQueryBuilder builds over several fields are served too
// (rgpu_search_fields_tree_batch): a group may be a SUM - a nested should-only BooleanQuery of TermQuery clauses, "(title:w body:w)" -
// and MUST groups may stand beside SHOULD groups (must_should: ReqOptScorer, its sequential rule kept). Off by default: such a query
// is UnsupportedOperation, as these trees have been.
struct MultiFieldQuery : Query {
  struct Group {
    bool dismax = false;
    float tie_breaker_multiplier = 0.0f;
    std::vector<TermQuery> terms;  // one TermQuery, or the disjuncts, or the nested clauses
    bool sum = false;              // a nested should-only BooleanQuery of `terms`
    int32_t min_should_match = 0;  // ... and its min_should_match (0 and 1 are served)
  };
  std::vector<Group> groups;
  bool must = false;  // the groups are MUST clauses (else SHOULD)
  int32_t min_should_match = 0;
  std::vector<TermQuery> must_not_queries;
  std::vector<Group> should_groups;  // must = true: SHOULD groups beside the MUST ones (the optional side of ReqOptScorer)
  static Group sum_of(std::vector<TermQuery> clauses, int32_t min_should_match = 0) {
    if (clauses.empty()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "boolean query should at least contain one inner query!");
    Group g;
    g.sum = true;
    g.min_should_match = min_should_match;
    g.terms = std::move(clauses);
    return g;
  }
  bool is_tree() const {
    if (!should_groups.empty()) return true;
    for (const Group& g : groups) if (g.sum) return true;
    return false;
  }
  static Group term(TermQuery t) { Group g; g.terms.push_back(std::move(t)); return g; }
  static Group dismax(std::vector<TermQuery> disjuncts, float tie) {
    if (disjuncts.empty()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "DisjunctionMaxQuery: sub query should not be empty!");
    Group g;
    g.dismax = true;
    g.tie_breaker_multiplier = tie;
    g.terms = std::move(disjuncts);
    return g;
  }
  static std::unique_ptr<MultiFieldQuery> should(std::vector<Group> groups, int32_t min_should_match = 0, std::vector<TermQuery> must_nots = {}) {
    std::unique_ptr<MultiFieldQuery> q(new MultiFieldQuery());
    q->groups = std::move(groups);
    q->min_should_match = min_should_match;
    q->must_not_queries = std::move(must_nots);
    return q;
  }
  static std::unique_ptr<MultiFieldQuery> all_must(std::vector<Group> groups, std::vector<TermQuery> must_nots = {}) {
    std::unique_ptr<MultiFieldQuery> q = should(std::move(groups), 0, std::move(must_nots));
    q->must = true;
    return q;
  }
  static std::unique_ptr<MultiFieldQuery> must_should(std::vector<Group> musts, std::vector<Group> shoulds, int32_t min_should_match = 0,
                                                      std::vector<TermQuery> must_nots = {}) {
    std::unique_ptr<MultiFieldQuery> q = all_must(std::move(musts), std::move(must_nots));
    q->should_groups = std::move(shoulds);
    q->min_should_match = min_should_match;  // (accepted, without effect: ReqOptScorer only advance()s the optional scorer)
    return q;
  }
};

// query/boosting_query.rs:29-118, scorer/boosting_scorer.rs:40-81: the positive query's docs, counts and scores, a doc's score
// multiplied once by negative_boost where the negative query also holds it; a leaf in which the negative query has no scorer matches
// nothing. Served here (RGPU_NOT_WITH_DEMOTE): a positive that is a TermQuery or a BooleanQuery packing to TERM / AND / OR (with or
// without MUST_NOT clauses), a negative that is a TermQuery or a should-only BooleanQuery with min_should_match <= 1, and
// 0 < negative_boost < 1 (BoostingScorer::new's debug_assert); anything else is UnsupportedOperation when the query is searched — the
// caller's CPU path.
struct BoostingQuery : Query {
  std::shared_ptr<const Query> positive, negative;
  float negative_boost;
  BoostingQuery(std::shared_ptr<const Query> pos, std::shared_ptr<const Query> neg, float boost)
      : positive(std::move(pos)), negative(std::move(neg)), negative_boost(boost) {}
  // the positive query as the GPU path takes it (a TermQuery or a BooleanQuery without optional or nested clauses), else Unsupported
  const Query* served_positive() const {
    if (!(negative_boost > 0.0f && negative_boost < 1.0f)) throw Error(RGPU_ERR_UNSUPPORTED, "a BoostingQuery is served by the GPU path for 0 < negative_boost < 1");
    if (dynamic_cast<const TermQuery*>(positive.get())) return positive.get();
    if (auto* b = dynamic_cast<const BooleanQuery*>(positive.get()))
      if ((b->must_queries.empty() || b->should_queries.empty()) && !b->should_required && !b->nested_must) return b;
    throw Error(RGPU_ERR_UNSUPPORTED, "a BoostingQuery is served by the GPU path when its positive query is a term or a flat TERM / AND / OR boolean query");
  }
  // the negative query as a union of term clauses, else Unsupported
  std::vector<TermQuery> demoting_terms() const {
    if (auto* t = dynamic_cast<const TermQuery*>(negative.get())) return {*t};
    if (auto* b = dynamic_cast<const BooleanQuery*>(negative.get()))
      if (b->must_queries.empty() && b->must_not_queries.empty() && !b->should_queries.empty() && b->min_should_match <= 1) return b->should_queries;
    throw Error(RGPU_ERR_UNSUPPORTED, "a BoostingQuery is served by the GPU path when its negative query is a term or a flat disjunction of terms");
  }
};

// A BooleanQuery whose MUST / SHOULD clauses may themselves be queries (BooleanQuery::build takes Vec<Box<dyn Query>>,
// boolean_query.rs:40-86). The GPU path serves flat trees of term clauses; `flattened()` folds ONE level — a MUST clause that is
// a must-only BooleanQuery, a SHOULD clause that is a should-only one (min_should_match <= 1) — into a flat BooleanQuery, or
// returns null when the tree is not of that shape. The reference does not rewrite such trees: it sums a + (b + c) where the
// flat query sums (a + b) + c — the same docs and hit counts, scores equal within 1e-5 relative (north_star's float
// tolerance), not bit for bit. GpuIndexSearcher folds only when `flatten_nested` is set; everything else goes to `cpu_fallback`
// ("everything else to the CPU path"; the Rust shim: rust/gpu/searcher.rs).
struct NestedBooleanQuery : Query {
  std::vector<std::unique_ptr<Query>> must_queries, should_queries;
  std::vector<TermQuery> must_not_queries;
  int32_t min_should_match = 0;
  // Nested clauses that do NOT score have exact flat forms (same docs, counts and f32 sums as the reference's scorer tree):
  //   * a MUST_NOT clause that is a should-only BooleanQuery of terms, "-(b c)": ReqNotScorer excludes what the nested
  //     DisjunctionSumScorer matches, b or c — the MUST_NOT clauses b, c (boolean_query.rs:236-252 builds one disjunction over the
  //     MUST_NOT scorers with the OUTER min_should_match: equal only while that is <= 1, so msm > 1 is not expanded);
  //   * a FILTER clause that is a must-only BooleanQuery of terms, "#(+b +c)": its weights are created with needs_scores = false
  //     (boolean_query.rs:106-108), every clause scores 0.0 and the conjunction's 0.0 + 0.0 joins the outer sum as one 0.0 — the
  //     FILTER clauses b, c (MUST clauses of boost 0; x + 0.0 == x wherever the cost order puts them).
  std::vector<std::unique_ptr<Query>> must_not_nested, filter_nested;
  // -> MUST_NOT terms (the query's own + the expanded ones) and the zero-boost MUST terms the nested FILTER clauses stand for; false:
  // a nested non-scoring clause of another shape (the tree goes to cpu_fallback)
  bool scoring_clauses_are_terms() const {
    for (const auto* v : {&must_queries, &should_queries})
      for (const auto& q : *v)
        if (!dynamic_cast<const TermQuery*>(q.get())) return false;
    return true;
  }
  // `filter_disjunction` (optional): a FILTER clause that is a should-only BooleanQuery of 1..9 terms, "+a #(b c)" — served by
  // required_disjunction() as the required disjunction of zero-boost clauses; at most one, and only where the caller asks for it
  bool expand_non_scoring(std::vector<TermQuery>* nots, std::vector<TermQuery>* zeros, const BooleanQuery** filter_disjunction = nullptr) const {
    *nots = must_not_queries;
    zeros->clear();
    for (const auto& q : must_not_nested) {
      if (auto* t = dynamic_cast<const TermQuery*>(q.get())) { nots->push_back(*t); continue; }
      auto* b = dynamic_cast<const BooleanQuery*>(q.get());
      if (!b || min_should_match > 1 || !b->must_queries.empty() || !b->must_not_queries.empty() || b->should_queries.empty() || b->min_should_match > 1 ||
          b->should_required || b->nested_must)
        return false;
      nots->insert(nots->end(), b->should_queries.begin(), b->should_queries.end());
    }
    for (const auto& q : filter_nested) {
      std::vector<TermQuery> terms;
      if (auto* t = dynamic_cast<const TermQuery*>(q.get())) terms.push_back(*t);
      else {
        auto* b = dynamic_cast<const BooleanQuery*>(q.get());
        if (!b || !b->must_not_queries.empty() || b->should_required || b->nested_must) return false;
        if (b->must_queries.empty()) {  // should-only: a filter by a disjunction
          if (!filter_disjunction || *filter_disjunction || b->should_queries.empty() || b->should_queries.size() > 9 || b->min_should_match > 1) return false;
          *filter_disjunction = b;
          continue;
        }
        if (!b->should_queries.empty()) return false;
        terms = b->must_queries;
      }
      for (TermQuery& t : terms) { t.boost = 0.0f; zeros->push_back(t); }
    }
    return true;
  }
  std::unique_ptr<Query> flattened() const {
    auto fold = [](const std::vector<std::unique_ptr<Query>>& clauses, bool want_must, std::vector<TermQuery>* out) -> bool {
      for (const auto& q : clauses) {
        if (auto* t = dynamic_cast<const TermQuery*>(q.get())) { out->push_back(*t); continue; }
        auto* b = dynamic_cast<const BooleanQuery*>(q.get());
        if (!b || !b->must_not_queries.empty()) return false;
        if (want_must && !b->must_queries.empty() && b->should_queries.empty()) out->insert(out->end(), b->must_queries.begin(), b->must_queries.end());
        else if (!want_must && b->must_queries.empty() && !b->should_queries.empty() && b->min_should_match <= 1)
          out->insert(out->end(), b->should_queries.begin(), b->should_queries.end());
        else return false;
      }
      return true;
    };
    std::vector<TermQuery> musts, shoulds, nots, zeros;
    if (!expand_non_scoring(&nots, &zeros)) return nullptr;
    if (!fold(must_queries, true, &musts)) return nullptr;
    musts.insert(musts.end(), zeros.begin(), zeros.end());
    if (!musts.empty()) {  // SHOULD clauses beside MUST ones stay as they are: ReqOptScorer's optional side takes term clauses only
      for (const auto& q : should_queries) {
        auto* t = dynamic_cast<const TermQuery*>(q.get());
        if (!t) return nullptr;
        shoulds.push_back(*t);
      }
    } else {
      if (!fold(should_queries, false, &shoulds)) return nullptr;
      if (min_should_match > 1 && shoulds.size() != should_queries.size()) return nullptr;  // it counts the OUTER clauses
    }
    return BooleanQuery::build(std::move(musts), std::move(shoulds), min_should_match, std::move(nots));
  }
  // "(b c) a d" / "a (b c) d": a should-only query whose FIRST or SECOND clause is itself a should-only BooleanQuery of terms -> the
  // flat disjunction with the nested clauses moved to the front, else null. DisjunctionSumScorer sums its children in clause order
  // from 0.0 (SimpleQueue, below ten children: disjunction_scorer.rs:41-45, 211-225), the nested scorer's own sum formed first:
  // (a + (b + c)) + d; the flat [b, c, a, d] forms ((b + c) + a) + d — the same f32: the one add that differs has two operands
  // and commutes. Same docs, counts and score bits: no tolerance, no flag. Fewer than ten clauses in all (the clause-order kernel).
  std::unique_ptr<Query> nested_disjunction_first() const {
    if (!must_queries.empty() || min_should_match > 1) return nullptr;
    std::vector<TermQuery> inner, rest, nots, zeros;
    if (!expand_non_scoring(&nots, &zeros) || !zeros.empty()) return nullptr;  // (a FILTER clause makes it a conjunction)
    for (size_t i = 0; i < should_queries.size(); ++i) {
      if (auto* t = dynamic_cast<const TermQuery*>(should_queries[i].get())) { rest.push_back(*t); continue; }
      auto* b = dynamic_cast<const BooleanQuery*>(should_queries[i].get());
      if (!b || !inner.empty() || i > 1 || !b->must_queries.empty() || !b->must_not_queries.empty() || b->min_should_match > 1 ||
          b->should_queries.empty())
        return nullptr;
      inner = b->should_queries;
    }
    if (inner.empty() || inner.size() + rest.size() >= 10) return nullptr;
    inner.insert(inner.end(), rest.begin(), rest.end());
    return BooleanQuery::build({}, std::move(inner), min_should_match, std::move(nots));
  }
  // "+a +(b c)": MUST term clauses and exactly ONE MUST clause that is a should-only BooleanQuery of 1..9 terms
  // (min_should_match <= 1), no SHOULD clause of its own -> the tree as MUST clauses + required SHOULD clauses
  // (RGPU_OP_WITH_SHOULD(AND, n) | RGPU_OP_SHOULD_REQUIRED), else null. BooleanWeight::create_scorer builds
  // ConjunctionScorer([TermScorer ..., DisjunctionSumScorer]) for it (boolean_query.rs:200-215). Whether the kernel's sum — MUST
  // sum + disjunction sum — is the reference's, bit for bit, depends on the children's costs: the library's per-leaf sort (RGPU_OP_NESTED_AT).
  std::unique_ptr<BooleanQuery> required_disjunction() const {
    if (!should_queries.empty()) return nullptr;
    std::unique_ptr<BooleanQuery> out(new BooleanQuery());
    const BooleanQuery* nested = nullptr;
    for (const auto& q : must_queries) {
      if (auto* t = dynamic_cast<const TermQuery*>(q.get())) { out->must_queries.push_back(*t); continue; }
      auto* b = dynamic_cast<const BooleanQuery*>(q.get());
      if (!b || nested) return nullptr;
      nested = b;
      out->nested_at = static_cast<int32_t>(out->must_queries.size());
    }
    std::vector<TermQuery> zeros;
    const BooleanQuery* by_filter = nullptr;
    if (!expand_non_scoring(&out->must_not_queries, &zeros, &by_filter)) return nullptr;
    if (by_filter) {  // "+a #(b c)": the required disjunction of zero-boost clauses (they score 0.0: needs_scores = false), behind the MUST
      if (nested) return nullptr;  // clauses, where BooleanQuery::create_weight puts the FILTER weights (boolean_query.rs:101-108)
      nested = by_filter;
      out->nested_at = static_cast<int32_t>(out->must_queries.size());
    }
    out->must_queries.insert(out->must_queries.end(), zeros.begin(), zeros.end());  // behind every MUST term: nested_at stands
    if (!nested || out->must_queries.empty() || !nested->must_queries.empty() || !nested->must_not_queries.empty() || nested->should_required ||
        nested->min_should_match > 1 || nested->should_queries.empty() || nested->should_queries.size() > 9)
      return nullptr;
    out->should_queries = nested->should_queries;
    if (by_filter) for (TermQuery& t : out->should_queries) t.boost = 0.0f;
    out->should_required = true;
    return out;
  }
  // "+a +(+b +c)": MUST term clauses and exactly ONE MUST clause that is a must-only BooleanQuery of >= 2 terms, no SHOULD clause of
  // its own -> MUST clauses + the nested clauses in the SHOULD slots with nested_must set (RGPU_OP_WITH_SHOULD(AND, n) |
  // RGPU_OP_NESTED_MUST), else null. The reference sums the nested conjunction first (conjunction_scorer.rs:87-95): bit for bit
  // (the library sorts the children per leaf), where the flat fold (flattened()) is within 1e-5.
  std::unique_ptr<BooleanQuery> nested_conjunction() const {
    if (!should_queries.empty()) return nullptr;
    std::unique_ptr<BooleanQuery> out(new BooleanQuery());
    const BooleanQuery* nested = nullptr;
    for (const auto& q : must_queries) {
      if (auto* t = dynamic_cast<const TermQuery*>(q.get())) { out->must_queries.push_back(*t); continue; }
      auto* b = dynamic_cast<const BooleanQuery*>(q.get());
      if (!b || nested) return nullptr;
      nested = b;
      out->nested_at = static_cast<int32_t>(out->must_queries.size());
    }
    std::vector<TermQuery> zeros;
    if (!expand_non_scoring(&out->must_not_queries, &zeros)) return nullptr;
    out->must_queries.insert(out->must_queries.end(), zeros.begin(), zeros.end());  // behind every MUST term: nested_at stands
    if (!nested || out->must_queries.empty() || !nested->should_queries.empty() || !nested->must_not_queries.empty() || nested->should_required ||
        nested->nested_must || nested->must_queries.size() < 2)
      return nullptr;
    out->should_queries = nested->must_queries;
    out->nested_must = true;
    return out;
  }
};

// PhraseQuery (query/phrase_query.rs:60-130: PhraseQuery::build numbers the terms' positions 0, 1, 2, ...;
// explicit positions leave gaps). Needs a positions field (LeafReader::index_options == 3 with pos_bytes).
struct PhraseQuery : Query {
  std::vector<TermQuery> terms;
  std::vector<int32_t> positions;
  float boost;
  int32_t slop;  // 0: ExactPhraseScorer; > 0: SloppyPhraseScorer (phrase_query.rs:312-331)
  explicit PhraseQuery(std::vector<TermQuery> t, std::vector<int32_t> pos = {}, float b = 1.0f, int32_t slop_ = 0)
      : terms(std::move(t)), positions(std::move(pos)), boost(b), slop(slop_) {
    if (slop < 0) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "Slop must be >= 0");
    if (positions.empty()) for (size_t i = 0; i < terms.size(); ++i) positions.push_back(static_cast<int32_t>(i));
    if (terms.size() < 2 || terms.size() != positions.size())
      throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "a phrase needs two or more terms, one position each (a one-term phrase is a TermQuery)");
  }
};

// SpanTermQuery (query/spans/span_term.rs): the spans [position, position + 1) of one term; served as a clause of a SpanNearQuery.
struct SpanTermQuery : Query {
  TermQuery term;
  explicit SpanTermQuery(TermQuery t) : term(std::move(t)) {}
};
// SpanNearQuery::new (query/spans/span_near.rs:101-124): the clauses within `slop` positions of each other, in the clauses' order when
// in_order. The GPU path serves a top-level query with in_order = true whose clauses are all SpanTermQuery (rgpu_search_span_near_batch):
// NearSpansOrdered + SpanScorer, next_limit applied at every slop (spans are always two-phase). The weight sums the idf of every clause's
// term, a term named twice counted twice (build_sim_weight, span.rs:574-602). Unordered near (NearSpansUnordered, span_near.rs:333-528: the
// order among equal cells is its heap's array order, which the kernels keep) is served through rgpu_search_span_unordered_batch by a
// searcher with GpuIndexSearcher::unordered_spans = true; check_served() keeps refusing it, as it does for every caller that has not
// opted in, and the searcher routes opted-in rows around it (check_shape). Nested span clauses (add_nested), a span query under a
// FilteredQuery or in a rescore request are UnsupportedOperation when the query is searched - the caller's CPU path. No boolean query
// of this mirror can hold one.
struct SpanNearQuery : Query {
  std::vector<SpanTermQuery> clauses;
  int32_t nested = 0;  // clauses that are themselves SpanNearQuerys (add_nested): kept as a count, the query is refused when searched
  int32_t slop;
  bool in_order;
  float boost;
  explicit SpanNearQuery(std::vector<SpanTermQuery> c, int32_t slop_ = 0, bool in_order_ = true, float b = 1.0f)
      : clauses(std::move(c)), slop(slop_), in_order(in_order_), boost(b) {
    if (clauses.size() < 2) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "clauses length must not be smaller than 2!");
  }
  SpanNearQuery& add_nested(const SpanNearQuery&) { ++nested; return *this; }
  void check_served() const {
    if (!in_order) throw Error(RGPU_ERR_UNSUPPORTED, "an unordered SpanNearQuery is not served by the GPU path");
    check_shape();
  }
  void check_shape() const {  // what is refused whatever the order
    if (nested > 0) throw Error(RGPU_ERR_UNSUPPORTED, "a SpanNearQuery with nested span clauses is not served by the GPU path");
    if (clauses.size() > RGPU_MAX_PHRASE_TERMS) throw Error(RGPU_ERR_UNSUPPORTED, "a SpanNearQuery of more than RGPU_MAX_PHRASE_TERMS clauses is not served by the GPU path");
    if (slop < 0) throw Error(RGPU_ERR_UNSUPPORTED, "a SpanNearQuery with a negative slop is not served by the GPU path");
  }
};

// BooleanQuery with exact PhraseQuery clauses among its required clauses: +"a b" +c -d #e (rgpu_search_phrase_bool_batch).
// `required`: BooleanWeight::must_weights — the MUST clauses in query order (must()), then the FILTER clauses (filter(): they
// score 0); a clause is a phrase or a term. Only the shapes the GPU path serves can be written here: no SHOULD clause, no phrase
// under MUST_NOT, no nested BooleanQuery; a sloppy phrase clause or more than RGPU_MAX_BOOL_PHRASES phrases is UnsupportedOperation
// when the query is searched — the caller's CPU path (inside a conjunction the reference's SloppyPhraseScorer matches on its
// approximation and scores a stale sloppy_freq, which is not reproduced).
struct PhraseBooleanQuery : Query {
  struct Required {
    std::shared_ptr<PhraseQuery> phrase;  // null: a term clause
    TermQuery term{int64_t(-1)};
    bool filter = false;
  };
  std::vector<Required> required;
  std::vector<TermQuery> must_not_queries;
  PhraseBooleanQuery& must(PhraseQuery p) { return add(Required{std::make_shared<PhraseQuery>(std::move(p)), TermQuery(int64_t(-1)), false}); }
  PhraseBooleanQuery& must(TermQuery t) { return add(Required{nullptr, std::move(t), false}); }
  PhraseBooleanQuery& filter(PhraseQuery p) { return add(Required{std::make_shared<PhraseQuery>(std::move(p)), TermQuery(int64_t(-1)), true}); }
  PhraseBooleanQuery& filter(TermQuery t) { return add(Required{nullptr, std::move(t), true}); }
  PhraseBooleanQuery& must_not(TermQuery t) { must_not_queries.push_back(std::move(t)); return *this; }
  // refused before any leaf is touched
  void check_served() const {
    int n_phrases = 0;
    for (const Required& r : required) {
      if (!r.phrase) continue;
      ++n_phrases;
      if (r.phrase->slop > 0) throw Error(RGPU_ERR_UNSUPPORTED, "a sloppy phrase inside a boolean query is not served by the GPU path");
    }
    if (n_phrases < 1 || n_phrases > RGPU_MAX_BOOL_PHRASES) throw Error(RGPU_ERR_UNSUPPORTED, "a boolean query over phrases holds 1..RGPU_MAX_BOOL_PHRASES phrases");
  }

 private:
  PhraseBooleanQuery& add(Required r) {  // (FILTER clauses stand behind the MUST clauses in must_weights)
    auto at = required.end();
    if (!r.filter) at = std::find_if(required.begin(), required.end(), [](const Required& x) { return x.filter; });
    required.insert(at, std::move(r));
    return *this;
  }
};

// BooleanQuery whose clauses are all SHOULD / MUST_NOT with exact PhraseQuery clauses among the SHOULD ones: "a b" "c d" e -f
// (rgpu_search_phrase_or_batch). `should`: BooleanWeight::should_weights — the SHOULD clauses in query order, a phrase or a term each:
// ONE DisjunctionSumScorer over those that exist in the leaf (boolean_query.rs:217-234), summed in that order. Only the shapes the GPU
// path serves can be written here (no MUST, no FILTER, no phrase under MUST_NOT, no nested BooleanQuery); a sloppy phrase clause, more
// than RGPU_MAX_BOOL_PHRASES phrases or ten or more SHOULD clauses (the heap-order arm) are UnsupportedOperation when the query is
// searched — the caller's CPU path.
struct PhraseDisjunctionQuery : Query {
  struct Should {
    std::shared_ptr<PhraseQuery> phrase;  // null: a term clause
    TermQuery term{int64_t(-1)};
  };
  std::vector<Should> should_queries;
  std::vector<TermQuery> must_not_queries;
  int32_t min_should_match = 1;  // BooleanQuery::build: 0 becomes 1 when there is no MUST clause
  PhraseDisjunctionQuery& should(PhraseQuery p) { should_queries.push_back(Should{std::make_shared<PhraseQuery>(std::move(p)), TermQuery(int64_t(-1))}); return *this; }
  PhraseDisjunctionQuery& should(TermQuery t) { should_queries.push_back(Should{nullptr, std::move(t)}); return *this; }
  PhraseDisjunctionQuery& must_not(TermQuery t) { must_not_queries.push_back(std::move(t)); return *this; }
  PhraseDisjunctionQuery& min_should(int32_t n) { min_should_match = n > 0 ? n : 1; return *this; }
  // refused before any leaf is touched
  void check_served() const {
    int n_phrases = 0;
    for (const Should& c : should_queries) {
      if (!c.phrase) continue;
      ++n_phrases;
      if (c.phrase->slop > 0) throw Error(RGPU_ERR_UNSUPPORTED, "a sloppy phrase inside a boolean query is not served by the GPU path");
    }
    if (n_phrases < 1 || n_phrases > RGPU_MAX_BOOL_PHRASES) throw Error(RGPU_ERR_UNSUPPORTED, "a disjunction over phrases holds 1..RGPU_MAX_BOOL_PHRASES phrases");
    if (should_queries.size() > 9) throw Error(RGPU_ERR_UNSUPPORTED, "ten or more SHOULD clauses with a phrase among them sum in heap order");
    if (min_should_match > 255) throw Error(RGPU_ERR_UNSUPPORTED, "min_should_match above 255");
  }
};

// BooleanQuery of required (MUST / FILTER) AND optional (SHOULD) clauses with exact PhraseQuery clauses on either side: +a +b "a b",
// +"a b" c, +"a b" +c "b c" d -n #f (rgpu_search_phrase_opt_batch): ReqOptScorer(must, DisjunctionSumScorer(should)), its sequential
// rule kept. `required`: BooleanWeight::must_weights — the MUST clauses in query order, then the FILTER clauses (they score 0);
// `should_queries`: should_weights, the SHOULD clauses in query order; a clause is a phrase or a term. Served only by a searcher
// with GpuIndexSearcher::optional_phrases = true (off by default: UnsupportedOperation, as such trees have been). Only the shapes
// the call can express can be written here (no nested BooleanQuery, no phrase under MUST_NOT); a sloppy phrase clause, more than
// RGPU_MAX_BOOL_PHRASES phrases on a side, ten or more SHOULD clauses or a side without a clause are UnsupportedOperation when the query
// is searched — the caller's CPU path. min_should_match is carried and without effect (ReqOptScorer only advances the optional scorer).
struct PhraseOptionalQuery : Query {
  struct Clause {
    std::shared_ptr<PhraseQuery> phrase;  // null: a term clause
    TermQuery term{int64_t(-1)};
    bool filter = false;
  };
  std::vector<Clause> required;
  std::vector<Clause> should_queries;
  std::vector<TermQuery> must_not_queries;
  int32_t min_should_match = 0;
  PhraseOptionalQuery& must(PhraseQuery p) { return add(Clause{std::make_shared<PhraseQuery>(std::move(p)), TermQuery(int64_t(-1)), false}); }
  PhraseOptionalQuery& must(TermQuery t) { return add(Clause{nullptr, std::move(t), false}); }
  PhraseOptionalQuery& filter(PhraseQuery p) { return add(Clause{std::make_shared<PhraseQuery>(std::move(p)), TermQuery(int64_t(-1)), true}); }
  PhraseOptionalQuery& filter(TermQuery t) { return add(Clause{nullptr, std::move(t), true}); }
  PhraseOptionalQuery& should(PhraseQuery p) { should_queries.push_back(Clause{std::make_shared<PhraseQuery>(std::move(p)), TermQuery(int64_t(-1)), false}); return *this; }
  PhraseOptionalQuery& should(TermQuery t) { should_queries.push_back(Clause{nullptr, std::move(t), false}); return *this; }
  PhraseOptionalQuery& must_not(TermQuery t) { must_not_queries.push_back(std::move(t)); return *this; }
  PhraseOptionalQuery& min_should(int32_t n) { min_should_match = n; return *this; }
  // refused before any leaf is touched
  void check_served() const {
    if (required.empty() || should_queries.empty()) throw Error(RGPU_ERR_UNSUPPORTED, "a MUST + SHOULD tree has a required and an optional clause");
    for (const std::vector<Clause>* side : {&required, &should_queries}) {
      int n_phrases = 0;
      for (const Clause& c : *side) {
        if (!c.phrase) continue;
        ++n_phrases;
        if (c.phrase->slop > 0) throw Error(RGPU_ERR_UNSUPPORTED, "a sloppy phrase inside a boolean query is not served by the GPU path");
      }
      if (n_phrases > RGPU_MAX_BOOL_PHRASES) throw Error(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_BOOL_PHRASES phrases on one side of a boolean query");
    }
    if (should_queries.size() > 9) throw Error(RGPU_ERR_UNSUPPORTED, "ten or more SHOULD clauses sum in heap order");
    if (min_should_match < 0 || min_should_match > 255) throw Error(RGPU_ERR_UNSUPPORTED, "min_should_match outside 0..255");
  }

 private:
  PhraseOptionalQuery& add(Clause c) {  // (FILTER clauses stand behind the MUST clauses in must_weights)
    auto at = required.end();
    if (!c.filter) at = std::find_if(required.begin(), required.end(), [](const Clause& x) { return x.filter; });
    required.insert(at, std::move(c));
    return *this;
  }
};

// RescoreRequest (search/scorer/rescorer.rs:67-116): how a second query's score is folded into the first pass's
// A filter that is not a term, as the query cache holds it (search/cache/query_cache.rs:301-372): a handle to one doc set per leaf,
// owned by the GpuIndexSearcher that made it (cache_filter / filter_from_docs / filter_from_bits) until drop_filter or its end.
struct CachedFilter {
  uint64_t id = 0;
};
// `query` restricted to the docs every one of `filters` holds and none of `excludes` holds (rgpu_search_batch_masked). Two spellings:
//   FilteredQuery::filter_query(Q, {F ...})          FilterQuery(Q, F) (query/filter_query.rs:155-233): Q needs a scorer of its own, no more
//   FilteredQuery::clauses(Q, {F ...}, {X ...})      the BooleanQuery "Q's clauses, #F, -X": the rows are the reference's when Q brings a
//                                                    MUST or FILTER clause of its own ("b c #F" is ReqOptScorer(F, b | c) there and matches
//                                                    ALL of F) and, for -X, min_should_match <= 1 (boolean_query.rs:235-251)
// Anything else — a phrase underneath included — is UnsupportedOperation, i.e. cpu_fallback. `query` is not owned.
// GpuIndexSearcher::filtered_phrases = true (off by default) serves EXACT phrases underneath through the masked phrase calls
// (rgpu_search_phrase_batch_masked, _phrase_bool_batch_masked, _phrase_or_batch_masked): a PhraseQuery or PhraseBooleanQuery under either
// spelling, a PhraseDisjunctionQuery under filter_query or under clauses(Q, {}, {X ...}) with min_should_match <= 1. Still refused with it
// on: any sloppy phrase (its next_limit counts deleted docs, not docs outside a filter), clauses(PhraseDisjunctionQuery, {F ...}) — "a b"
// c #F, the doc set is the only required clause —, -X beside min_should_match >= 2, what the phrase queries' own check_served refuses.
struct FilteredQuery : Query {
  const Query* query = nullptr;
  std::vector<CachedFilter> filters, excludes;
  bool as_filter_query = false;
  static FilteredQuery filter_query(const Query& q, std::vector<CachedFilter> f) {
    FilteredQuery out;
    out.query = &q;
    out.filters = std::move(f);
    out.as_filter_query = true;
    return out;
  }
  static FilteredQuery clauses(const Query& q, std::vector<CachedFilter> f, std::vector<CachedFilter> x = {}) {
    FilteredQuery out;
    out.query = &q;
    out.filters = std::move(f);
    out.excludes = std::move(x);
    return out;
  }
  // -> the doc sets are the query's ONLY required clauses (GpuIndexSearcher::required_sets: rgpu_search_batch_required_set collects
  // every doc of them, the query's SHOULD clauses score): clauses(should-only BooleanQuery, {F ...}, {X ...}) — "b c #F -X" — and
  // MatchAllDocsQuery under either spelling — a lone "#F", "-X". With required_sets on clauses(should-only, {}, {X}) is served too,
  // masked: "b c -X" gets no MatchAllDocsQuery, it is ReqNotScorer over the disjunction. Refused there: an exclusion beside
  // min_should_match >= 2, a SHOULD clause of boost <= 0, MUST_NOT term clauses beside the sets (the Python mirror folds those into an
  // excluded set; this mirror does not).
  bool check_served(bool filtered_phrases = false, bool required_sets = false) const;  // (below PhraseBooleanQuery / PhraseDisjunctionQuery's definitions)
};
inline bool FilteredQuery::check_served(bool filtered_phrases, bool required_sets) const {
  if (query && dynamic_cast<const MatchAllDocsQuery*>(query)) {
    if (filters.empty() && excludes.empty()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "a filtered query takes a query and at least one cached filter");
    if (!required_sets) throw Error(RGPU_ERR_UNSUPPORTED, "a doc set as the only required clause is not served by the GPU path (the reference matches all of it)");
    return true;
  }
  if (!query || (filters.empty() && excludes.empty()) || (as_filter_query && (filters.empty() || !excludes.empty())))
    throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "a filtered query takes a query and at least one cached filter");
  const PhraseQuery* phrase = dynamic_cast<const PhraseQuery*>(query);
  const PhraseBooleanQuery* phrase_bool = dynamic_cast<const PhraseBooleanQuery*>(query);
  const PhraseDisjunctionQuery* phrase_or = dynamic_cast<const PhraseDisjunctionQuery*>(query);
  if (phrase || phrase_bool || phrase_or) {
    if (!filtered_phrases || (phrase && phrase->slop > 0)) throw Error(RGPU_ERR_UNSUPPORTED, "a filtered phrase is not served by the GPU path");
    if (phrase_bool) phrase_bool->check_served();
    if (phrase_or) {
      phrase_or->check_served();
      if (as_filter_query) return false;
      if (!filters.empty()) throw Error(RGPU_ERR_UNSUPPORTED, "a doc set as the only required clause is not served by the GPU path (the reference matches all of it)");
      if (phrase_or->min_should_match > 1) throw Error(RGPU_ERR_UNSUPPORTED, "a MUST_NOT doc set beside min_should_match >= 2 is not served by the GPU path");
    }
    return false;
  }
  if (dynamic_cast<const SpanNearQuery*>(query) || dynamic_cast<const SpanTermQuery*>(query))
    throw Error(RGPU_ERR_UNSUPPORTED, "a filtered span query is not served by the GPU path");
  if (dynamic_cast<const FilteredQuery*>(query) || dynamic_cast<const NestedBooleanQuery*>(query))
    throw Error(RGPU_ERR_UNSUPPORTED, "a filtered query over a nested or another filtered query is not served by the GPU path");
  if (as_filter_query) return false;
  if (const BooleanQuery* b = dynamic_cast<const BooleanQuery*>(query)) {
    if (b->must_queries.empty()) {
      if (!required_sets) throw Error(RGPU_ERR_UNSUPPORTED, "a doc set as the only required clause is not served by the GPU path (the reference matches all of it)");
      if (!excludes.empty() && b->min_should_match > 1) throw Error(RGPU_ERR_UNSUPPORTED, "a MUST_NOT doc set beside min_should_match >= 2 is not served by the GPU path");
      if (filters.empty()) return false;  // "b c -X": the masked disjunction
      if (!b->must_not_queries.empty()) throw Error(RGPU_ERR_UNSUPPORTED, "MUST_NOT term clauses beside a doc set as the only required clause are not folded into the set by this mirror");
      if (b->should_required || b->nested_must) throw Error(RGPU_ERR_UNSUPPORTED, "beside a doc set as the only required clause the SHOULD clauses are term queries");
      for (const TermQuery& t : b->should_queries)
        if (!(t.boost > 0.0f)) throw Error(RGPU_ERR_UNSUPPORTED, "beside a doc set as the only required clause a SHOULD clause has a boost > 0");
      return true;
    }
    if (!excludes.empty() && b->min_should_match > 1) throw Error(RGPU_ERR_UNSUPPORTED, "a MUST_NOT doc set beside min_should_match >= 2 is not served by the GPU path");
  }
  return false;
}

// search/query/point_range_query.rs: the docs holding a point of `field` with lower <= value <= upper, both ends inclusive, in unsigned
// byte order of the sortable bytes. ONE dimension (4 or 8 bytes per bound). It does not score — ConstantScoreScorer(0.0) under MUST and
// FILTER alike, PointRangeWeight::new :482 — so it is served as a doc set: GpuIndexSearcher::range_filter builds the CachedFilter on
// the GPU from attached points and range_clauses spells "Q's clauses, +/#ranges, -ranges" as a FilteredQuery. Alone, under SHOULD, as
// the only required clause or beside a phrase (unless filtered_phrases is on, and the phrase exact) it is UnsupportedOperation
// (cpu_fallback), as the same shapes with a CachedFilter are.
struct PointRangeQuery : Query {
  std::string field;
  std::vector<uint8_t> lower, upper;
  int32_t num_dims;   // more than one: UnsupportedOperation at range_filter (what it matches depends on the BKD cell layout)
  PointRangeQuery(std::string f, std::vector<uint8_t> lo, std::vector<uint8_t> hi, int32_t dims = 1)
      : field(std::move(f)), lower(std::move(lo)), upper(std::move(hi)), num_dims(dims) {
    if (num_dims < 1 || lower.size() % static_cast<size_t>(num_dims) != 0)   // PointRangeQuery::new :384-390
      throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "lowerPoint is not a fixed multiple of numDims");
    if (lower.size() != upper.size() || lower.empty())   // :391-397
      throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "lowerPoint and upperPoint have different lengths");
  }
};
// encode_dimension of the four one-dimensional point types (core/util/numeric.rs:163-218): the sign bit flipped, big-endian; floats
// through sortable_float_bits / sortable_double_bits first (bits ^ ((bits >> 31) & 0x7fffffff), arithmetic shift)
struct IntPoint {
  static std::vector<uint8_t> encode(int32_t v) {
    const uint32_t u = static_cast<uint32_t>(v) ^ 0x80000000u;
    return {static_cast<uint8_t>(u >> 24), static_cast<uint8_t>(u >> 16), static_cast<uint8_t>(u >> 8), static_cast<uint8_t>(u)};
  }
  static PointRangeQuery new_range_query(std::string field, int32_t lo, int32_t hi) { return PointRangeQuery(std::move(field), encode(lo), encode(hi)); }
  static PointRangeQuery new_exact_query(std::string field, int32_t v) { return new_range_query(std::move(field), v, v); }
};
struct LongPoint {
  static std::vector<uint8_t> encode(int64_t v) {
    const uint64_t u = static_cast<uint64_t>(v) ^ 0x8000000000000000ull;
    std::vector<uint8_t> out(8);
    for (int i = 0; i < 8; ++i) out[static_cast<size_t>(i)] = static_cast<uint8_t>(u >> (56 - 8 * i));
    return out;
  }
  static PointRangeQuery new_range_query(std::string field, int64_t lo, int64_t hi) { return PointRangeQuery(std::move(field), encode(lo), encode(hi)); }
  static PointRangeQuery new_exact_query(std::string field, int64_t v) { return new_range_query(std::move(field), v, v); }
};
struct FloatPoint {
  static std::vector<uint8_t> encode(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    const uint32_t sortable = bits ^ ((bits & 0x80000000u) ? 0x7fffffffu : 0u);
    return IntPoint::encode(static_cast<int32_t>(sortable));
  }
  static PointRangeQuery new_range_query(std::string field, float lo, float hi) { return PointRangeQuery(std::move(field), encode(lo), encode(hi)); }
  static PointRangeQuery new_exact_query(std::string field, float v) { return new_range_query(std::move(field), v, v); }
};
struct DoublePoint {
  static std::vector<uint8_t> encode(double v) {
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    const uint64_t sortable = bits ^ ((bits & 0x8000000000000000ull) ? 0x7fffffffffffffffull : 0ull);
    return LongPoint::encode(static_cast<int64_t>(sortable));
  }
  static PointRangeQuery new_range_query(std::string field, double lo, double hi) { return PointRangeQuery(std::move(field), encode(lo), encode(hi)); }
  static PointRangeQuery new_exact_query(std::string field, double v) { return new_range_query(std::move(field), v, v); }
};
// one leaf's points of a field for GpuIndexSearcher::attach_points: n_points (doc, value) pairs, values n_points * bytes_per_dim
// sortable bytes; absent() for a leaf without the field
struct LeafPoints {
  const int32_t* docs = nullptr;
  const uint8_t* values = nullptr;
  int64_t n_points = -1;   // -1: the leaf does not hold the field
  static LeafPoints absent() { return LeafPoints(); }
  static LeafPoints of(const int32_t* d, const uint8_t* v, int64_t n) { LeafPoints p; p.docs = d; p.values = v; p.n_points = n; return p; }
};

struct RescoreRequest {
  const Query* query = nullptr;  // TermQuery, an all-MUST / all-SHOULD BooleanQuery, or a PhraseQuery (sloppy: no repeated term)
  float query_weight = 1.0f, rescore_weight = 1.0f;
  rgpu_rescore_mode mode = RGPU_RESCORE_TOTAL;
  int32_t window_size = 0;  // 0: the whole row
};

// One segment: postings file, norms, live docs, FieldReader statistics, and the terms: a block-tree dictionary
// (rgpu_terms_open over the segment's .tim/.tip) and/or a flat term table.
// A further indexed field of a leaf's segment (LeafReader::extra_fields): its postings live in the leaf's one .doc file
struct ExtraField {
  std::string name;
  int32_t field_number = 0;
  int32_t index_options = 2;  // as for rgpu_segment_attach_field, RGPU_FIELD_STORES_PAYLOADS included
  const uint8_t* norms = nullptr;  // null: the field omits norms
  int64_t doc_count = 0, sum_total_term_freq = 0, sum_doc_freq = -1;
  const rgpu_term_state* terms = nullptr;  // a flat table indexed by term id, or ...
  int64_t n_terms = 0;
  const rgpu_terms* dictionary = nullptr;  // ... the segment's block-tree dictionary, asked under field_number (not owned)
  int32_t slot = -1;                       // rgpu_segment_attach_field's, filled by the searcher
  bool term_state(const TermQuery& q, rgpu_term_state* out) const {
    if (q.by_text()) {
      if (!dictionary) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "this field has no term dictionary: query it by term id");
      const int64_t offs[2] = {0, static_cast<int64_t>(q.text.size())};
      uint8_t found = 0;
      check(rgpu_terms_lookup(dictionary, field_number, reinterpret_cast<const uint8_t*>(q.text.data()), offs, 1, out, &found));
      return found != 0;
    }
    if (q.term >= n_terms || terms[q.term].doc_freq <= 0) return false;
    *out = terms[q.term];
    return true;
  }
};

struct LeafReader {
  std::string field = "body";  // the primary field's name: a TermQuery without a field, or with this one, means it
  std::vector<ExtraField> extra_fields;  // the segment's further indexed fields a query may name (TermQuery::field)
  const ExtraField* extra(const std::string& name) const {
    for (const ExtraField& x : extra_fields) if (x.name == name) return &x;
    return nullptr;
  }
  int32_t index_options = 2;  // doc::IndexOptions ordinal of the searched field: 1 Docs, 2 DocsAndFreqs
  const uint8_t* doc_bytes = nullptr;
  size_t doc_len = 0;
  const uint8_t* norms = nullptr;
  const uint64_t* live_docs = nullptr;
  int32_t max_doc = 0, doc_base = 0;
  int64_t doc_count = 0, sum_total_term_freq = 0, sum_doc_freq = -1;
  const rgpu_term_state* terms = nullptr;
  int64_t n_terms = 0;
  const rgpu_terms* dictionary = nullptr;  // not owned
  int32_t field_number = 0;
  // a positions field (index_options == 3): the .pos file and, for a flat term table, each term's position pointers
  const uint8_t* pos_bytes = nullptr;
  size_t pos_len = 0;
  const rgpu_term_positions* term_positions = nullptr;
  rgpu_segment* segment = nullptr;  // filled by the searcher
  // TermIterator::seek_exact + term_state(); false when the term is absent from this leaf
  bool term_state(const TermQuery& q, rgpu_term_state* out) const {
    if (q.by_text()) {
      if (!dictionary) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "this leaf has no term dictionary: query it by term id");
      const int64_t offs[2] = {0, static_cast<int64_t>(q.text.size())};
      uint8_t found = 0;
      check(rgpu_terms_lookup(dictionary, field_number, reinterpret_cast<const uint8_t*>(q.text.data()), offs, 1, out, &found));
      return found != 0;
    }
    if (q.term >= n_terms || terms[q.term].doc_freq <= 0) return false;
    *out = terms[q.term];
    return true;
  }
  // the same plus the position-stream pointers of BlockTermState (lucene50_decode_term, posting_reader.rs:264-306)
  bool positions_state(const TermQuery& q, rgpu_term_state* out, rgpu_term_positions* pos) const {
    if (q.by_text()) {
      if (!dictionary) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "this leaf has no term dictionary: query it by term id");
      const int64_t offs[2] = {0, static_cast<int64_t>(q.text.size())};
      uint8_t found = 0;
      check(rgpu_terms_lookup_positions(dictionary, field_number, reinterpret_cast<const uint8_t*>(q.text.data()), offs, 1, out, pos, &found));
      return found != 0;
    }
    if (!term_state(q, out) || !term_positions) return false;
    *pos = term_positions[q.term];
    return true;
  }
};

// StandardDirectoryReader::open for the slice this path needs (index/reader/directory_reader.rs:90-140, segment_reader.rs):
// the newest commit point segments_N names the segments; per segment .si gives max_doc, .fnm the field's number, then
// _Lucene50_0.{doc,tim,tip}, .nvm/.nvd and _<delgen>.liv — taken out of .cfs for a compound segment. Owns every buffer the
// LeafReaders point into; hand `leaves()` to a GpuIndexSearcher and keep this object alive as long as that searcher.
class IndexDirectory {
 public:
  static std::unique_ptr<IndexDirectory> open(const std::string& path, const std::string& field) {
    std::unique_ptr<IndexDirectory> dir(new IndexDirectory());
    int64_t gen = -1;
    {  // find_segment_file: the highest generation present
      DIR* d = opendir(path.c_str());
      if (!d) throw Error(RGPU_ERR_IO, "cannot list " + path);
      while (dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name.compare(0, 9, "segments_") == 0 && name.size() > 9) gen = std::max<int64_t>(gen, (int64_t)std::stoll(name.substr(9), nullptr, 36));
      }
      closedir(d);
    }
    if (gen < 0) throw Error(RGPU_ERR_IO, "no segments_N file found in " + path);
    const std::vector<uint8_t> commit_bytes = slurp(path + "/segments_" + base36((uint64_t)gen));
    int32_t n = rgpu_commit_from_segments_file(commit_bytes.data(), commit_bytes.size(), gen, nullptr, 0);
    check(n);
    std::vector<rgpu_commit_segment> commit((size_t)n);
    check(rgpu_commit_from_segments_file(commit_bytes.data(), commit_bytes.size(), gen, commit.data(), n));
    int32_t doc_base = 0;
    for (const rgpu_commit_segment& seg : commit) {
      dir->segments_.emplace_back(new Segment());
      Segment& s = *dir->segments_.back();
      const std::string name = seg.name, stem = path + "/" + name;
      const std::vector<uint8_t> si = slurp(stem + ".si");
      rgpu_segment_info info;
      check(rgpu_segment_info_from_lucene62(si.data(), si.size(), seg.id, &info));
      if (seg.del_count > info.max_doc) throw Error(RGPU_ERR_CORRUPT_INDEX, "invalid deletion count");
      std::vector<uint8_t> cfs;
      std::vector<rgpu_compound_entry> entries;
      if (info.is_compound_file) {
        cfs = slurp(stem + ".cfs");
        const std::vector<uint8_t> cfe = slurp(stem + ".cfe");
        int32_t ne = rgpu_compound_entries_from_lucene50(cfe.data(), cfe.size(), cfs.data(), cfs.size(), seg.id, nullptr, 0);
        check(ne);
        entries.resize((size_t)ne);
        check(rgpu_compound_entries_from_lucene50(cfe.data(), cfe.size(), cfs.data(), cfs.size(), seg.id, entries.data(), ne));
      }
      auto part = [&](const std::string& suffix) -> std::vector<uint8_t> {
        if (!info.is_compound_file) return slurp(stem + suffix);
        for (const rgpu_compound_entry& e : entries)
          if (suffix == e.id) return std::vector<uint8_t>(cfs.begin() + e.offset, cfs.begin() + e.offset + e.length);
        throw Error(RGPU_ERR_IO, name + suffix + " is not in the compound file");
      };
      const std::vector<uint8_t> fnm = seg.field_infos_gen > 0 ? slurp(stem + "_" + base36((uint64_t)seg.field_infos_gen) + ".fnm") : part(".fnm");
      size_t names_len = 0;
      int32_t nf = rgpu_field_infos_from_lucene60(fnm.data(), fnm.size(), nullptr, 0, nullptr, 0, &names_len);
      check(nf);
      std::vector<rgpu_field_info> infos((size_t)nf);
      std::vector<char> names(names_len + 1);
      check(rgpu_field_infos_from_lucene60(fnm.data(), fnm.size(), infos.data(), nf, names.data(), names_len, &names_len));
      int32_t field_number = -1, index_options = 0;
      std::vector<rgpu_field_info> indexed;
      const char* p = names.data();
      for (int32_t i = 0; i < nf; ++i, p += std::strlen(p) + 1) {
        if (infos[(size_t)i].index_options != 0) indexed.push_back(infos[(size_t)i]);
        if (field == p) { field_number = infos[(size_t)i].number; index_options = infos[(size_t)i].index_options; }
      }
      if (field_number < 0) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "no field named " + field + " in segment " + name);
      if (index_options != 1 && index_options != 2)
        throw Error(RGPU_ERR_UNSUPPORTED, "the searched field must be indexed with IndexOptions::Docs or ::DocsAndFreqs");
      s.doc = part("_Lucene50_0.doc");
      const std::vector<uint8_t> tim = part("_Lucene50_0.tim"), tip = part("_Lucene50_0.tip"), nvm = part(".nvm"), nvd = part(".nvd");
      check(rgpu_terms_open(tim.data(), tim.size(), tip.data(), tip.size(), indexed.data(), (int32_t)indexed.size(), info.max_doc, &s.terms));
      s.norms.resize((size_t)info.max_doc);
      check(rgpu_norms_from_lucene53(nvm.data(), nvm.size(), nvd.data(), nvd.size(), field_number, info.max_doc, s.norms.data()));
      if (seg.del_gen >= 0 && seg.del_count > 0) {
        const std::vector<uint8_t> liv = slurp(stem + "_" + base36((uint64_t)seg.del_gen) + ".liv");
        s.live.resize((size_t)((info.max_doc + 63) / 64));
        check(rgpu_live_docs_from_lucene50(liv.data(), liv.size(), info.max_doc, seg.del_count, s.live.data()));
      }
      rgpu_field_stats stats;
      check(rgpu_terms_field_stats(s.terms, field_number, &stats));
      LeafReader leaf;
      leaf.doc_bytes = s.doc.data();
      leaf.doc_len = s.doc.size();
      leaf.norms = s.norms.data();
      leaf.live_docs = s.live.empty() ? nullptr : s.live.data();
      leaf.max_doc = info.max_doc;
      leaf.doc_base = doc_base;
      leaf.doc_count = stats.doc_count;
      leaf.sum_total_term_freq = stats.sum_total_term_freq;
      leaf.sum_doc_freq = stats.sum_doc_freq;
      leaf.dictionary = s.terms;
      leaf.field_number = field_number;
      leaf.index_options = index_options;
      dir->leaves_.push_back(leaf);
      doc_base += info.max_doc;
    }
    return dir;
  }
  const std::vector<LeafReader>& leaves() const { return leaves_; }

 private:
  struct Segment {
    std::vector<uint8_t> doc, norms;
    std::vector<uint64_t> live;
    rgpu_terms* terms = nullptr;
    ~Segment() { rgpu_terms_close(terms); }
  };
  std::vector<std::unique_ptr<Segment>> segments_;
  std::vector<LeafReader> leaves_;

  static std::vector<uint8_t> slurp(const std::string& file) {
    std::ifstream f(file, std::ios::binary);
    if (!f) throw Error(RGPU_ERR_IO, "cannot open " + file);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  }
  static std::string base36(uint64_t v) {  // util/numeric.rs:148-160
    std::string r;
    do { r.insert(r.begin(), "0123456789abcdefghijklmnopqrstuvwxyz"[v % 36]); v /= 36; } while (v);
    return r;
  }
};

class GpuIndexSearcher {
 public:
  // DefaultIndexSearcher::new(reader, next_limit) (searcher.rs:291-296): approximations a two-phase scorer (a sloppy phrase)
  // may spend on a leaf without a collected doc before the leaf is abandoned; 0 = the reference's default of 500 000, -1 = none
  int32_t next_limit = 0;
  // `config`: the library's knobs (rgpu_config: byte budgets for the doc bitmaps and the prepared-term store, enqueue-only
  // disjunction batches, work partitioning ...); null = the defaults. abi_version is filled in here.
  GpuIndexSearcher(std::vector<LeafReader> leaves, const BM25Similarity& sim = BM25Similarity(), int device = 0,
                   const rgpu_config* config = nullptr)
      : leaves_(std::move(leaves)), sim_(sim) {
    rgpu_config cfg{};
    if (config) cfg = *config;
    cfg.abi_version = RGPU_ABI_VERSION;
    check(rgpu_init(device, &cfg, &ctx_));
    for (auto& l : leaves_) {
      check(rgpu_segment_upload_field(ctx_, l.doc_bytes, l.doc_len, l.norms, l.max_doc, l.doc_base, l.live_docs, l.index_options, &l.segment));
      if (l.pos_bytes) check(rgpu_segment_attach_positions(l.segment, l.pos_bytes, l.pos_len));
      for (ExtraField& x : l.extra_fields) check(rgpu_segment_attach_field(l.segment, x.norms, x.index_options, &x.slot));  // slots 1.. in the order given
    }
    // searcher.rs:306-363: the first leaf with the largest max_doc provides the collection statistics
    for (size_t i = 1; i < leaves_.size(); ++i)
      if (leaves_[i].max_doc > leaves_[stats_leaf_].max_doc) stats_leaf_ = i;
    const LeafReader& s = leaves_[stats_leaf_];
    stats_.doc_base = s.doc_base;
    stats_.max_doc = max_doc();
    stats_.doc_count = s.doc_count;
    stats_.sum_total_term_freq = s.sum_total_term_freq;
    stats_.sum_doc_freq = s.sum_doc_freq;
  }
  ~GpuIndexSearcher() {
    for (rgpu_planner* p : planners_) rgpu_planner_destroy(p);
    for (auto& m : masks_) for (rgpu_docset* d : m.second) rgpu_docset_free(d);   // doc sets go before their segments
    for (auto& f : filters_) for (rgpu_docset* d : f.second) rgpu_docset_free(d);
    for (auto& p : points_) for (rgpu_points* h : p.second.per_leaf) rgpu_points_free(h);   // points too
    for (auto& l : leaves_) rgpu_segment_free(l.segment);
    rgpu_shutdown(ctx_);
  }
  GpuIndexSearcher(const GpuIndexSearcher&) = delete;
  GpuIndexSearcher& operator=(const GpuIndexSearcher&) = delete;

  int64_t max_doc() const {
    int64_t n = 0;
    for (auto& l : leaves_) n += l.max_doc;
    return n;
  }
  // searcher.rs:732-767: doc_freq of the term in the statistics leaf only
  TermStatistics term_statistics(const TermQuery& term) const {
    TermStatistics ts;
    rgpu_term_state st;
    const bool have = leaves_[stats_leaf_].term_state(term, &st);
    ts.doc_freq = have ? st.doc_freq : 0;
    ts.total_term_freq = have ? st.total_term_freq : 0;
    return ts;
  }
  const CollectionStatistics& collection_statistics() const { return stats_; }

  // Trees the GPU path does not serve: fold one level of nesting (same docs, scores within 1e-5 — NestedBooleanQuery), and / or
  // hand the query to the host's CPU searcher — where rust/gpu/searcher.rs calls DefaultIndexSearcher::search
  bool flatten_nested = false;
  // FilteredQuery over EXACT phrases (PhraseQuery, PhraseBooleanQuery, PhraseDisjunctionQuery) goes through the masked phrase calls
  // instead of being UnsupportedOperation (FilteredQuery's comment says what stays refused)
  bool filtered_phrases = false;
  // Doc sets as the ONLY required clauses — "b c #F", a lone "#F", "-X", MatchAllDocsQuery — go through
  // rgpu_search_batch_required_set (every doc of live AND sets is collected, the docs no SHOULD clause holds at score 0) instead of
  // being UnsupportedOperation; "b c -X" is then searched masked (FilteredQuery::check_served says what stays refused)
  bool required_sets = false;
  // A top-level SpanNearQuery(in_order = false) over SpanTermQuery clauses goes through rgpu_search_span_unordered_batch
  // (NearSpansUnordered, the heap's array order kept) instead of being UnsupportedOperation. Refused either way: nested span clauses,
  // a span query under a FilteredQuery or in a rescore request.
  bool unordered_spans = false;
  // A PhraseOptionalQuery - MUST / FILTER + SHOULD clauses with exact phrases on either side: +a +b "a b", +"a b" c - goes through
  // rgpu_search_phrase_opt_batch (ReqOptScorer over the phrase scorers, its sequential rule kept) instead of being
  // UnsupportedOperation. Refused either way: what PhraseOptionalQuery::check_served refuses, and such a row under a FilteredQuery
  // (the call has no masked form).
  bool optional_phrases = false;
  // serve MultiFieldQuery trees with SUM groups and with SHOULD groups beside MUST groups through rgpu_search_fields_tree_batch (off by
  // default: such rows are UnsupportedOperation, as they have been); rows rgpu_search_fields_batch can express keep going there.
  // What it costs: every must_should query then takes ReqOptScorer's rule, where ONE wavefront walks the query's hits in doc order -
  // about 7 ns per posting of the cheapest MUST group, tens of milliseconds for a `+word` that millions of docs hold (1024 such
  // trees over 10 M docs: 1.3 s against 24 ms without the rule). rgpu_config.req_opt_rule = -1 adds the
  // optional sums everywhere instead, in one pass (same docs and counts, scores >= the reference's).
  bool field_trees = false;
  std::function<void(const Query&, TopDocsCollector&)> cpu_fallback;

  // ---- cached filters: doc sets in HBM as FILTER / MUST_NOT masks (include/rucene_gpu.h rgpu_docset_*) ---------------------------
  // LRUQueryCache::do_cache on the GPU: per leaf the docs `query` matches, live docs NOT applied (query_cache.rs:335-342). A TermQuery
  // or a flat BooleanQuery that packs to TERM / AND / OR with min_should_match <= 1 (MUST_NOT term clauses allowed); anything else is
  // UnsupportedOperation from the library.
  CachedFilter cache_filter(const Query& query) {
    std::vector<rgpu_docset*> sets(leaves_.size(), nullptr);
    try {
      for (size_t li = 0; li < leaves_.size(); ++li) {
        std::vector<rgpu_query> qs;
        std::vector<rgpu_query_term> ts;
        plan({&query}, li, &qs, &ts);
        check(rgpu_docset_collect_batch(leaves_[li].segment, qs.data(), 1, ts.data(), static_cast<int32_t>(ts.size()), &sets[li]));
      }
    } catch (...) {
      for (rgpu_docset* d : sets) rgpu_docset_free(d);
      throw;
    }
    return keep(std::move(sets));
  }
  // GLOBAL doc ids in any order, repeats allowed, split by the leaves' doc bases
  CachedFilter filter_from_docs(const std::vector<int64_t>& global_docs) {
    std::vector<std::vector<int32_t>> per_leaf(leaves_.size());
    for (int64_t d : global_docs) {
      size_t li = 0;
      while (li < leaves_.size() && !(d >= leaves_[li].doc_base && d < static_cast<int64_t>(leaves_[li].doc_base) + leaves_[li].max_doc)) ++li;
      if (li == leaves_.size()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "a doc id outside every leaf");
      per_leaf[li].push_back(static_cast<int32_t>(d - leaves_[li].doc_base));
    }
    std::vector<rgpu_docset*> sets(leaves_.size(), nullptr);
    try {
      for (size_t li = 0; li < leaves_.size(); ++li)
        check(rgpu_docset_from_docs(leaves_[li].segment, per_leaf[li].data(), static_cast<int64_t>(per_leaf[li].size()), &sets[li]));
    } catch (...) {
      for (rgpu_docset* d : sets) rgpu_docset_free(d);
      throw;
    }
    return keep(std::move(sets));
  }
  // FixedBitSet words, ceil(max_doc / 64) per leaf (what a cached BitDocIdSet holds)
  CachedFilter filter_from_bits(const std::vector<const uint64_t*>& per_leaf_words) {
    if (per_leaf_words.size() != leaves_.size()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "a cached filter holds one bit set per leaf");
    std::vector<rgpu_docset*> sets(leaves_.size(), nullptr);
    try {
      for (size_t li = 0; li < leaves_.size(); ++li) check(rgpu_docset_from_words(leaves_[li].segment, per_leaf_words[li], &sets[li]));
    } catch (...) {
      for (rgpu_docset* d : sets) rgpu_docset_free(d);
      throw;
    }
    return keep(std::move(sets));
  }
  // MatchAllDocsQuery as a required clause: every doc of every leaf (rgpu_docset_combine of no operands), made once
  CachedFilter every_doc() {
    if (every_doc_.id != 0 && filters_.count(every_doc_.id)) return every_doc_;
    std::vector<rgpu_docset*> sets(leaves_.size(), nullptr);
    try {
      for (size_t li = 0; li < leaves_.size(); ++li) check(rgpu_docset_combine(leaves_[li].segment, nullptr, 0, nullptr, 0, &sets[li]));
    } catch (...) {
      for (rgpu_docset* d : sets) rgpu_docset_free(d);
      throw;
    }
    return every_doc_ = keep(std::move(sets));
  }
  int64_t filter_cardinality(CachedFilter f) const {
    int64_t n = 0;
    for (rgpu_docset* d : sets_of(f)) {
      int64_t c = 0;
      check(rgpu_docset_cardinality(d, &c));
      n += c;
    }
    return n;
  }
  // frees the filter's doc sets and every memoised combination that names it
  void drop_filter(CachedFilter f) {
    for (auto it = masks_.begin(); it != masks_.end();) {
      const bool names = std::count(it->first.first.begin(), it->first.first.end(), f.id) || std::count(it->first.second.begin(), it->first.second.end(), f.id);
      if (names) { for (rgpu_docset* d : it->second) rgpu_docset_free(d); it = masks_.erase(it); }
      else ++it;
    }
    auto at = filters_.find(f.id);
    if (at == filters_.end()) return;
    for (rgpu_docset* d : at->second) rgpu_docset_free(d);
    filters_.erase(at);
  }

  // ---- point ranges: numeric range filters built as doc sets (include/rucene_gpu.h rgpu_points_*) -----------------------------------
  // The one-dimensional points of `field`, one LeafPoints per leaf (absent(): the leaf lacks the field — the reference has no scorer
  // there: nothing matches under MUST / FILTER, nothing is excluded under MUST_NOT). IndexDirectory attaches nothing: no .dim reader.
  void attach_points(const std::string& field, int32_t bytes_per_dim, const std::vector<LeafPoints>& per_leaf) {
    if (per_leaf.size() != leaves_.size()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "points are attached per leaf");
    FieldPoints fp;
    fp.bytes_per_dim = bytes_per_dim;
    fp.per_leaf.assign(leaves_.size(), nullptr);
    try {
      for (size_t li = 0; li < leaves_.size(); ++li)
        if (per_leaf[li].n_points >= 0)
          check(rgpu_points_attach(leaves_[li].segment, bytes_per_dim, per_leaf[li].docs, per_leaf[li].values, per_leaf[li].n_points, &fp.per_leaf[li]));
    } catch (...) {
      for (rgpu_points* h : fp.per_leaf) rgpu_points_free(h);
      throw;
    }
    auto old = points_.find(field);
    if (old != points_.end()) {
      for (auto it = range_filters_.begin(); it != range_filters_.end();) {
        if (std::get<0>(it->first) == field) { drop_filter(it->second); it = range_filters_.erase(it); }
        else ++it;
      }
      for (rgpu_points* h : old->second.per_leaf) rgpu_points_free(h);
      points_.erase(old);
    }
    points_[field] = std::move(fp);
  }
  // The memo of range_filter is not bounded here: every distinct range leaves ceil(max_doc / 64) * 8 bytes per leaf in HBM until
  // drop_range_filters() (or drop_filter of one) — a caller whose ranges move with every query calls it between batches.
  void drop_range_filters() {
    for (auto& kv : range_filters_) drop_filter(kv.second);
    range_filters_.clear();
  }
  // PointRangeQuery -> CachedFilter, built on the GPU (rgpu_docset_from_point_ranges), memoised per (field, lower, upper). A field never
  // attached: UnsupportedOperation; bounds whose length is not the field's: IllegalArgument (point_range_query.rs:510-522).
  // path: rgpu_docset_from_point_ranges' (0 = the library chooses).
  CachedFilter range_filter(const PointRangeQuery& q, int32_t path = 0) {
    if (q.num_dims != 1) throw Error(RGPU_ERR_UNSUPPORTED, "a multi-dimensional point range is not served by the GPU path");
    auto at = points_.find(q.field);
    if (at == points_.end()) throw Error(RGPU_ERR_UNSUPPORTED, "no points are attached for field " + q.field + ": the range stays on the CPU path");
    const FieldPoints& fp = at->second;
    if (static_cast<int32_t>(q.lower.size()) != fp.bytes_per_dim)
      throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "field " + q.field + " was indexed with another bytesPerDim than this query has");
    const auto key = std::make_tuple(q.field, q.lower, q.upper);
    auto have = range_filters_.find(key);
    if (have != range_filters_.end()) return have->second;
    rgpu_point_range r;
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.lower, q.lower.data(), q.lower.size());
    std::memcpy(r.upper, q.upper.data(), q.upper.size());
    std::vector<rgpu_docset*> sets(leaves_.size(), nullptr);
    try {
      for (size_t li = 0; li < leaves_.size(); ++li) {
        if (fp.per_leaf[li]) check(rgpu_docset_from_point_ranges(fp.per_leaf[li], &r, 1, path, &sets[li]));
        else check(rgpu_docset_from_docs(leaves_[li].segment, nullptr, 0, &sets[li]));   // no such field in this leaf: the empty set
      }
    } catch (...) {
      for (rgpu_docset* d : sets) rgpu_docset_free(d);
      throw;
    }
    const CachedFilter f = keep(std::move(sets));
    range_filters_[key] = f;
    return f;
  }
  // "Q's clauses, +range / #range for every `required`, -range for every `must_not`": a range under MUST and one under FILTER both
  // add + 0.0 to the sum, so both are filters; FilteredQuery::check_served applies the unchanged rules (Q brings a MUST or FILTER
  // clause of its own, ...). The two differ in ONE place, BooleanQuery::build's default: "+range #a b" has min_should_match 0 (a MUST
  // clause stands), "#range #a b" has 1. Q is built without the ranges, so build it with the min_should_match the whole query has —
  // here that takes no care: beside required clauses the SHOULD side is ReqOptScorer's optional scorer, and a disjunction with
  // min_should_match 0 and 1 matches the same docs (BooleanQuery::build above stores 0 whenever a MUST or FILTER clause stands).
  FilteredQuery range_clauses(const Query& q, const std::vector<const PointRangeQuery*>& required, const std::vector<const PointRangeQuery*>& must_not = {}) {
    std::vector<CachedFilter> f, x;
    for (const PointRangeQuery* r : required) f.push_back(range_filter(*r));
    for (const PointRangeQuery* r : must_not) x.push_back(range_filter(*r));
    return FilteredQuery::clauses(q, std::move(f), std::move(x));
  }

  // IndexSearcher::search(query, collector) for a TopDocsCollector
  void search(const Query& query, TopDocsCollector& collector) {
    try {
      std::unique_ptr<Query> folded;
      const Query* q = &query;
      if (dynamic_cast<const NestedBooleanQuery*>(&query)) refuse_other_fields(query);  // (before a fold hides where its clauses stood)
      if (auto* nested = dynamic_cast<const NestedBooleanQuery*>(&query)) {
        std::unique_ptr<BooleanQuery> req = nested->required_disjunction();
        // (the library sorts a conjunction's children by cost per leaf and adds a nested child's sum where ConjunctionScorer::score
        // adds it — RGPU_OP_NESTED_AT breaks ties like the stable sort: the reference's f32 sums whatever the costs)
        if ((folded = nested->nested_disjunction_first())) {}  // exact as a flat disjunction in another clause order
        else if (req) folded = std::move(req);
        else if ((req = nested->nested_conjunction())) folded = std::move(req);
        else if (flatten_nested || nested->scoring_clauses_are_terms()) folded = nested->flattened();  // (only non-scoring clauses nested: exact)  // (what is left — two nested clauses, a disjunction from the third SHOULD clause on — within 1e-5)
        if (!folded) throw Error(RGPU_ERR_UNSUPPORTED, "nested boolean clauses are not served by the GPU path");
        q = folded.get();
      }
      std::vector<const Query*> one{q};
      std::vector<TopDocs> r = search_many(one, collector.estimated_hits());
      collector.set_result(std::move(r[0]));
    } catch (const Error& e) {
      if (e.kind != RGPU_ERR_UNSUPPORTED || !cpu_fallback) throw;  // ErrorKind::UnsupportedOperation -> the CPU path
      cpu_fallback(query, collector);
    }
  }

  // the batched form the hardware wants: one launch set per leaf for many queries
  // (PhraseQuery rows go through rgpu_search_phrase_batch, PhraseBooleanQuery rows through rgpu_search_phrase_bool_batch,
  // PhraseDisjunctionQuery rows through rgpu_search_phrase_or_batch, the rest through rgpu_search_batch: one call per kind and leaf,
  // rows keep their order)
  // FilteredQuery rows are grouped by their combination of doc sets (host/docset_plan.hpp: caller order kept inside a group) and searched
  // masked, one rgpu_search_batch_masked per group and leaf; every other row goes the way it went.
  std::vector<TopDocs> search_many(const std::vector<const Query*>& queries, size_t k) {
    {  // rows that name a further field of the leaves go to rgpu_search_fields_batch; a batch without one goes where it went.
       // That call serves k <= 128: a batch that holds such a row is UnsupportedOperation as a whole for k > 128, its primary-field
       // rows included (they are served up to k = 1024 in a batch of their own) - refused before any leaf is touched
      std::vector<size_t> cross_rows, rest_rows;
      for (size_t i = 0; i < queries.size(); ++i) (names_other_field(*queries[i]) ? cross_rows : rest_rows).push_back(i);
      if (!cross_rows.empty()) {
        std::vector<MultiFieldQuery> specs;
        for (size_t i : cross_rows) specs.push_back(cross_spec(*queries[i]));  // refused before any leaf is touched
        if (k > 128) throw Error(RGPU_ERR_UNSUPPORTED, "a cross-field query is served for k <= 128");
        std::vector<TopDocs> out(queries.size());
        if (!rest_rows.empty()) {
          std::vector<const Query*> rest;
          for (size_t i : rest_rows) rest.push_back(queries[i]);
          std::vector<TopDocs> got = search_many(rest, k);
          for (size_t i = 0; i < rest_rows.size(); ++i) out[rest_rows[i]] = std::move(got[i]);
        }
        std::vector<MultiFieldQuery> flat, trees;
        std::vector<size_t> flat_rows, tree_rows;
        for (size_t i = 0; i < specs.size(); ++i) {
          (specs[i].is_tree() ? trees : flat).push_back(specs[i]);
          (specs[i].is_tree() ? tree_rows : flat_rows).push_back(cross_rows[i]);
        }
        if (!flat.empty()) {
          std::vector<TopDocs> got = search_fields(flat, k);
          for (size_t i = 0; i < flat_rows.size(); ++i) out[flat_rows[i]] = std::move(got[i]);
        }
        if (!trees.empty()) {
          std::vector<TopDocs> got = search_fields_tree(trees, k);
          for (size_t i = 0; i < tree_rows.size(); ++i) out[tree_rows[i]] = std::move(got[i]);
        }
        return out;
      }
    }
    for (const Query* q : queries)
      if (dynamic_cast<const PointRangeQuery*>(q)) throw Error(RGPU_ERR_UNSUPPORTED, "a lone point range is not served by the GPU path (the reference matches all of it)");
    for (const Query* q : queries) {  // refused before any leaf is touched
      if (const SpanNearQuery* near = dynamic_cast<const SpanNearQuery*>(q)) check_span(*near);
      if (dynamic_cast<const SpanTermQuery*>(q)) throw Error(RGPU_ERR_UNSUPPORTED, "a span query is served by the GPU path as a top-level SpanNearQuery only");
    }
    for (const Query* q : queries)
      if (dynamic_cast<const FilteredQuery*>(q) || dynamic_cast<const MatchAllDocsQuery*>(q)) return search_filtered(queries, k);
    std::vector<size_t> phrase_rows, bool_rows, or_rows, opt_rows, span_rows, plain_rows;
    for (const Query* q : queries)  // refused before any leaf is touched
      if (const PhraseOptionalQuery* po = dynamic_cast<const PhraseOptionalQuery*>(q)) {
        if (!optional_phrases) throw Error(RGPU_ERR_UNSUPPORTED, "SHOULD clauses beside a required clause of a boolean query over phrases are not served by the GPU path (optional_phrases)");
        po->check_served();
      }
    for (size_t i = 0; i < queries.size(); ++i) {
      if (dynamic_cast<const PhraseOptionalQuery*>(queries[i])) opt_rows.push_back(i);
      else if (dynamic_cast<const SpanNearQuery*>(queries[i])) span_rows.push_back(i);
      else if (dynamic_cast<const PhraseQuery*>(queries[i])) phrase_rows.push_back(i);
      else if (dynamic_cast<const PhraseBooleanQuery*>(queries[i])) bool_rows.push_back(i);
      else if (dynamic_cast<const PhraseDisjunctionQuery*>(queries[i])) or_rows.push_back(i);
      else plain_rows.push_back(i);
    }
    if (!phrase_rows.empty() || !bool_rows.empty() || !or_rows.empty() || !opt_rows.empty() || !span_rows.empty()) {
      std::vector<TopDocs> out(queries.size());
      auto place = [&](const std::vector<size_t>& rows, std::vector<TopDocs> got) { for (size_t i = 0; i < rows.size(); ++i) out[rows[i]] = std::move(got[i]); };
      std::vector<const PhraseBooleanQuery*> bools;
      for (size_t i : bool_rows) { bools.push_back(static_cast<const PhraseBooleanQuery*>(queries[i])); bools.back()->check_served(); }
      std::vector<const PhraseDisjunctionQuery*> ors;
      for (size_t i : or_rows) { ors.push_back(static_cast<const PhraseDisjunctionQuery*>(queries[i])); ors.back()->check_served(); }
      if (!plain_rows.empty()) {
        std::vector<const Query*> plain;
        for (size_t i : plain_rows) plain.push_back(queries[i]);
        place(plain_rows, search_many(plain, k));
      }
      if (!phrase_rows.empty()) {
        std::vector<const PhraseQuery*> phrases;
        for (size_t i : phrase_rows) phrases.push_back(static_cast<const PhraseQuery*>(queries[i]));
        place(phrase_rows, search_phrases(phrases, k));
      }
      if (!bools.empty()) place(bool_rows, search_phrase_bools(bools, k));
      if (!ors.empty()) place(or_rows, search_phrase_ors(ors, k));
      if (!opt_rows.empty()) {
        std::vector<const PhraseOptionalQuery*> opts;
        for (size_t i : opt_rows) opts.push_back(static_cast<const PhraseOptionalQuery*>(queries[i]));
        place(opt_rows, search_phrase_opts(opts, k));
      }
      if (!span_rows.empty()) {  // ordered rows: rgpu_search_span_near_batch; unordered ones (unordered_spans): rgpu_search_span_unordered_batch
        for (const bool in_order : {true, false}) {
          std::vector<size_t> rows;
          std::vector<const SpanNearQuery*> nears;
          for (size_t i : span_rows)
            if (static_cast<const SpanNearQuery*>(queries[i])->in_order == in_order) { rows.push_back(i); nears.push_back(static_cast<const SpanNearQuery*>(queries[i])); }
          if (!rows.empty()) place(rows, search_span_nears(nears, k, in_order));
        }
      }
      return out;
    }
    const int32_t nq = static_cast<int32_t>(queries.size());
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      std::vector<rgpu_query> qs;
      std::vector<rgpu_query_term> ts;
      plan(queries, li, &qs, &ts);
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      check(rgpu_search_batch(leaves_[li].segment, qs.data(), nq, ts.data(), static_cast<int32_t>(ts.size()), static_cast<int32_t>(k),
                              leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  // ---- IndexSearcher::count (search/searcher.rs:632-654): hit counts without scoring ---------------------------------------------
  // where count() hands what the GPU path refuses (UnsupportedOperation: phrases, spans, nested trees, doc-set clauses); empty: rethrow
  std::function<int64_t(const Query&)> cpu_count_fallback;

  // MatchAllDocsQuery: num_docs from the leaves' live docs, no GPU call (searcher.rs:636-638); a TermQuery on leaves without deletions:
  // the sum of doc_freq, no GPU call (:640-648); anything else through count_many.
  int64_t count(const Query& query) {
    if (dynamic_cast<const MatchAllDocsQuery*>(&query)) {
      int64_t n = 0;
      for (const LeafReader& leaf : leaves_) n += leaf_num_docs(leaf);
      return n;
    }
    bool deletions = false;
    for (const LeafReader& leaf : leaves_) deletions = deletions || leaf.live_docs != nullptr;
    if (const TermQuery* t = dynamic_cast<const TermQuery*>(&query); t && !deletions && primary(*t)) {
      int64_t n = 0;
      rgpu_term_state st;
      for (const LeafReader& leaf : leaves_) if (leaf.term_state(*t, &st)) n += st.doc_freq;
      return n;
    }
    try {
      return count_many({&query})[0];
    } catch (const Error& e) {
      if (e.kind != RGPU_ERR_UNSUPPORTED || !cpu_count_fallback) throw;  // ErrorKind::UnsupportedOperation -> the CPU path
      return cpu_count_fallback(query);
    }
  }

  // the live docs each query matches, summed over the leaves: one rgpu_count_batch per leaf, nothing scored. Term, boolean, dismax and
  // boosting queries; anything else (phrases, spans, FilteredQuery / doc-set rows, nested trees) is UnsupportedOperation.
  std::vector<int64_t> count_many(const std::vector<const Query*>& queries) {
    for (const Query* q : queries)  // refused before any leaf is touched
      if (!dynamic_cast<const TermQuery*>(q) && !dynamic_cast<const BooleanQuery*>(q) && !dynamic_cast<const DisjunctionMaxQuery*>(q) && !dynamic_cast<const BoostingQuery*>(q))
        throw Error(RGPU_ERR_UNSUPPORTED, "a count is served by the GPU path for term, boolean, dismax and boosting queries");
    const int32_t nq = static_cast<int32_t>(queries.size());
    std::vector<int64_t> counts(queries.size(), 0), leaf_counts(queries.size(), 0);
    if (nq == 0) return counts;
    for (size_t li = 0; li < leaves_.size(); ++li) {
      std::vector<rgpu_query> qs;
      std::vector<rgpu_query_term> ts;
      plan(queries, li, &qs, &ts);
      check(rgpu_count_batch(leaves_[li].segment, nullptr, qs.data(), nq, ts.data(), static_cast<int32_t>(ts.size()), leaf_counts.data()));
      for (size_t i = 0; i < counts.size(); ++i) counts[i] += leaf_counts[i];
    }
    return counts;
  }

  // IndexSearcher::search(PhraseQuery, TopDocsCollector(k)) for a batch of exact phrases. PhraseQuery::create_weight
  // (phrase_query.rs:136-186): ONE BM25 weight from the statistics of all the phrase's terms.
  // `masks` (one doc set per leaf, or null): the search restricted to them — rgpu_search_phrase_batch_masked; exact phrases only.
  std::vector<TopDocs> search_phrases(const std::vector<const PhraseQuery*>& queries, size_t k, const std::vector<rgpu_docset*>* masks = nullptr) {
    for (const auto* q : queries) refuse_other_fields(*q);  // (these paths read the primary field's postings, idf and sim table)
    const int32_t nq = static_cast<int32_t>(queries.size());
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      const LeafReader& leaf = leaves_[li];
      if (!leaf.pos_bytes) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase search needs a positions field (LeafReader::pos_bytes)");
      std::vector<rgpu_phrase_query> qs;
      std::vector<rgpu_phrase_term> ts;
      pack_phrases(queries, leaf, &qs, &ts);
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      if (masks)
        check(rgpu_search_phrase_batch_masked(leaf.segment, (*masks)[li], qs.data(), nq, ts.data(), static_cast<int32_t>(ts.size()), static_cast<int32_t>(k),
                                              leaf_hits[li].data(), leaf_totals[li].data()));
      else
        check(rgpu_search_phrase_batch(leaf.segment, qs.data(), nq, ts.data(), static_cast<int32_t>(ts.size()), static_cast<int32_t>(k),
                                       leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  // a SpanNearQuery row: unordered near passes only on a searcher that opted in (unordered_spans), and then around
  // SpanNearQuery::check_served, which keeps refusing it
  void check_span(const SpanNearQuery& near) const {
    if (!near.in_order && unordered_spans) near.check_shape(); else near.check_served();
  }

  // IndexSearcher::search(SpanNearQuery, TopDocsCollector(k)) for a batch of near queries over SpanTermQuery clauses, all ordered
  // (rgpu_search_span_near_batch per leaf) or all unordered (rgpu_search_span_unordered_batch per leaf; unordered_spans). The rows are
  // packed as phrases either way (clause i at position i, `slop` the allowed slop) and merged over the leaves with their doc bases.
  std::vector<TopDocs> search_span_nears(const std::vector<const SpanNearQuery*>& queries, size_t k, bool in_order = true) {
    for (const auto* q : queries) refuse_other_fields(*q);  // (these paths read the primary field's postings, idf and sim table)
    const int32_t nq = static_cast<int32_t>(queries.size());
    std::vector<PhraseQuery> as_phrases;
    std::vector<const PhraseQuery*> rows;
    for (const SpanNearQuery* q : queries) {
      if (q->in_order != in_order) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "search_span_nears: a batch is all ordered or all unordered");
      check_span(*q);
      std::vector<TermQuery> terms;
      for (const SpanTermQuery& c : q->clauses) terms.push_back(c.term);
      as_phrases.emplace_back(std::move(terms), std::vector<int32_t>{}, q->boost, q->slop);
    }
    for (const PhraseQuery& p : as_phrases) rows.push_back(&p);
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      const LeafReader& leaf = leaves_[li];
      if (!leaf.pos_bytes) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "span search needs a positions field (LeafReader::pos_bytes)");
      std::vector<rgpu_phrase_query> qs;
      std::vector<rgpu_phrase_term> ts;
      pack_phrases(rows, leaf, &qs, &ts);
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      if (in_order)
        check(rgpu_search_span_near_batch(leaf.segment, qs.data(), nq, ts.data(), static_cast<int32_t>(ts.size()), 1, static_cast<int32_t>(k),
                                          leaf_hits[li].data(), leaf_totals[li].data()));
      else
        check(rgpu_search_span_unordered_batch(leaf.segment, qs.data(), nq, ts.data(), static_cast<int32_t>(ts.size()), static_cast<int32_t>(k),
                                               leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  // IndexSearcher::search(BooleanQuery over phrases and terms, TopDocsCollector(k)) for a batch: rgpu_search_phrase_bool_batch per leaf.
  // A FILTER clause rides with weight 0 (needs_scores = false); phrase_slot[i] = the phrase's index in `required`.
  // `masks` as for search_phrases: rgpu_search_phrase_bool_batch_masked.
  std::vector<TopDocs> search_phrase_bools(const std::vector<const PhraseBooleanQuery*>& queries, size_t k, const std::vector<rgpu_docset*>* masks = nullptr) {
    for (const auto* q : queries) refuse_other_fields(*q);  // (these paths read the primary field's postings, idf and sim table)
    const int32_t nq = static_cast<int32_t>(queries.size());
    for (const PhraseBooleanQuery* q : queries) q->check_served();
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      const LeafReader& leaf = leaves_[li];
      if (!leaf.pos_bytes) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase search needs a positions field (LeafReader::pos_bytes)");
      std::vector<rgpu_phrase_bool_query> qs;
      std::vector<const PhraseQuery*> phrases;
      std::vector<bool> filtered;
      std::vector<rgpu_query_term> ts;
      auto term_clause = [&](const TermQuery& c, bool scoring) {
        rgpu_query_term qt{};
        if (!leaf.term_state(c, &qt.state)) { qt.state = rgpu_term_state{}; qt.state.skip_offset = -1; qt.state.singleton_doc_id = -1; }
        auto w = weight_of(c);
        qt.weight = scoring ? w.first : 0.0f;
        qt.sim_table = w.second;
        ts.push_back(qt);
      };
      for (const PhraseBooleanQuery* q : queries) {
        rgpu_phrase_bool_query bq{};
        bq.first_phrase = static_cast<int32_t>(phrases.size());
        bq.first_term = static_cast<int32_t>(ts.size());
        for (size_t s = 0; s < q->required.size(); ++s) {
          const PhraseBooleanQuery::Required& r = q->required[s];
          if (r.phrase) {
            bq.phrase_slot[bq.n_phrases++] = static_cast<int32_t>(s);
            phrases.push_back(r.phrase.get());
            filtered.push_back(r.filter);
          } else {
            term_clause(r.term, !r.filter);
            bq.n_terms++;
          }
        }
        for (const TermQuery& c : q->must_not_queries) term_clause(c, false);
        bq.n_must_not = static_cast<int32_t>(q->must_not_queries.size());
        qs.push_back(bq);
      }
      std::vector<rgpu_phrase_query> ps;
      std::vector<rgpu_phrase_term> pts;
      pack_phrases(phrases, leaf, &ps, &pts);
      for (size_t i = 0; i < ps.size(); ++i) { if (filtered[i]) ps[i].weight = 0.0f; ps[i].next_limit = 0; }
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      if (masks)
        check(rgpu_search_phrase_bool_batch_masked(leaf.segment, (*masks)[li], qs.data(), nq, ps.data(), static_cast<int32_t>(ps.size()), pts.data(),
                                                   static_cast<int32_t>(pts.size()), ts.empty() ? nullptr : ts.data(), static_cast<int32_t>(ts.size()),
                                                   static_cast<int32_t>(k), leaf_hits[li].data(), leaf_totals[li].data()));
      else
        check(rgpu_search_phrase_bool_batch(leaf.segment, qs.data(), nq, ps.data(), static_cast<int32_t>(ps.size()), pts.data(), static_cast<int32_t>(pts.size()),
                                            ts.empty() ? nullptr : ts.data(), static_cast<int32_t>(ts.size()), static_cast<int32_t>(k),
                                            leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  // IndexSearcher::search(BooleanQuery of SHOULD phrases and terms, TopDocsCollector(k)) for a batch: rgpu_search_phrase_or_batch per
  // leaf. phrase_slot[i] = the phrase's index in `should_queries`.
  // `masks` as for search_phrases: rgpu_search_phrase_or_batch_masked.
  std::vector<TopDocs> search_phrase_ors(const std::vector<const PhraseDisjunctionQuery*>& queries, size_t k, const std::vector<rgpu_docset*>* masks = nullptr) {
    for (const auto* q : queries) refuse_other_fields(*q);  // (these paths read the primary field's postings, idf and sim table)
    const int32_t nq = static_cast<int32_t>(queries.size());
    for (const PhraseDisjunctionQuery* q : queries) q->check_served();
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      const LeafReader& leaf = leaves_[li];
      if (!leaf.pos_bytes) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase search needs a positions field (LeafReader::pos_bytes)");
      std::vector<rgpu_phrase_or_query> qs;
      std::vector<const PhraseQuery*> phrases;
      std::vector<rgpu_query_term> ts;
      auto term_clause = [&](const TermQuery& c) {
        rgpu_query_term qt{};
        if (!leaf.term_state(c, &qt.state)) { qt.state = rgpu_term_state{}; qt.state.skip_offset = -1; qt.state.singleton_doc_id = -1; }
        auto w = weight_of(c);
        qt.weight = w.first;
        qt.sim_table = w.second;
        ts.push_back(qt);
      };
      for (const PhraseDisjunctionQuery* q : queries) {
        rgpu_phrase_or_query oq{};
        oq.first_phrase = static_cast<int32_t>(phrases.size());
        oq.first_term = static_cast<int32_t>(ts.size());
        oq.min_should_match = q->min_should_match;
        for (size_t s = 0; s < q->should_queries.size(); ++s) {
          const PhraseDisjunctionQuery::Should& c = q->should_queries[s];
          if (c.phrase) {
            oq.phrase_slot[oq.n_phrases++] = static_cast<int32_t>(s);
            phrases.push_back(c.phrase.get());
          } else {
            term_clause(c.term);
            oq.n_terms++;
          }
        }
        for (const TermQuery& c : q->must_not_queries) term_clause(c);
        oq.n_must_not = static_cast<int32_t>(q->must_not_queries.size());
        qs.push_back(oq);
      }
      std::vector<rgpu_phrase_query> ps;
      std::vector<rgpu_phrase_term> pts;
      pack_phrases(phrases, leaf, &ps, &pts);
      for (rgpu_phrase_query& p : ps) p.next_limit = 0;
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      if (masks)
        check(rgpu_search_phrase_or_batch_masked(leaf.segment, (*masks)[li], qs.data(), nq, ps.data(), static_cast<int32_t>(ps.size()), pts.data(),
                                                 static_cast<int32_t>(pts.size()), ts.empty() ? nullptr : ts.data(), static_cast<int32_t>(ts.size()),
                                                 static_cast<int32_t>(k), leaf_hits[li].data(), leaf_totals[li].data()));
      else
        check(rgpu_search_phrase_or_batch(leaf.segment, qs.data(), nq, ps.data(), static_cast<int32_t>(ps.size()), pts.data(), static_cast<int32_t>(pts.size()),
                                          ts.empty() ? nullptr : ts.data(), static_cast<int32_t>(ts.size()), static_cast<int32_t>(k),
                                          leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  // IndexSearcher::search(BooleanQuery of required and optional clauses over phrases and terms, TopDocsCollector(k)) for a batch:
  // rgpu_search_phrase_opt_batch per leaf (optional_phrases). A FILTER clause rides with weight 0; req_phrase_slot[i] / opt_phrase_slot[i]
  // = the phrase's index in `required` / `should_queries`; the phrases stand required first, then optional, the terms required,
  // optional, MUST_NOT. A leaf without positions is served while no query of the batch names a phrase.
  std::vector<TopDocs> search_phrase_opts(const std::vector<const PhraseOptionalQuery*>& queries, size_t k) {
    if (!optional_phrases) throw Error(RGPU_ERR_UNSUPPORTED, "a MUST + SHOULD tree over phrases is not served by the GPU path (optional_phrases)");
    for (const auto* q : queries) refuse_other_fields(*q);  // (these paths read the primary field's postings, idf and sim table)
    const int32_t nq = static_cast<int32_t>(queries.size());
    for (const PhraseOptionalQuery* q : queries) q->check_served();
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      const LeafReader& leaf = leaves_[li];
      std::vector<rgpu_phrase_opt_query> qs;
      std::vector<const PhraseQuery*> phrases;
      std::vector<bool> filtered;
      std::vector<rgpu_query_term> ts;
      auto term_clause = [&](const TermQuery& c, bool scoring) {
        rgpu_query_term qt{};
        if (!leaf.term_state(c, &qt.state)) { qt.state = rgpu_term_state{}; qt.state.skip_offset = -1; qt.state.singleton_doc_id = -1; }
        auto w = weight_of(c);
        qt.weight = scoring ? w.first : 0.0f;
        qt.sim_table = w.second;
        ts.push_back(qt);
      };
      for (const PhraseOptionalQuery* q : queries) {
        rgpu_phrase_opt_query oq{};
        oq.first_phrase = static_cast<int32_t>(phrases.size());
        oq.first_term = static_cast<int32_t>(ts.size());
        oq.min_should_match = q->min_should_match;
        for (size_t s = 0; s < q->required.size(); ++s) {
          const PhraseOptionalQuery::Clause& c = q->required[s];
          if (c.phrase) {
            oq.req_phrase_slot[oq.n_req_phrases++] = static_cast<int32_t>(s);
            phrases.push_back(c.phrase.get());
            filtered.push_back(c.filter);
          } else {
            term_clause(c.term, !c.filter);
            oq.n_req_terms++;
          }
        }
        for (size_t s = 0; s < q->should_queries.size(); ++s) {
          const PhraseOptionalQuery::Clause& c = q->should_queries[s];
          if (c.phrase) {
            oq.opt_phrase_slot[oq.n_opt_phrases++] = static_cast<int32_t>(s);
            phrases.push_back(c.phrase.get());
            filtered.push_back(false);
          } else {
            term_clause(c.term, true);
            oq.n_opt_terms++;
          }
        }
        for (const TermQuery& c : q->must_not_queries) term_clause(c, false);
        oq.n_must_not = static_cast<int32_t>(q->must_not_queries.size());
        qs.push_back(oq);
      }
      if (!phrases.empty() && !leaf.pos_bytes) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase search needs a positions field (LeafReader::pos_bytes)");
      std::vector<rgpu_phrase_query> ps;
      std::vector<rgpu_phrase_term> pts;
      if (!phrases.empty()) pack_phrases(phrases, leaf, &ps, &pts);
      for (size_t i = 0; i < ps.size(); ++i) { if (filtered[i]) ps[i].weight = 0.0f; ps[i].next_limit = 0; }
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      check(rgpu_search_phrase_opt_batch(leaf.segment, qs.data(), nq, ps.empty() ? nullptr : ps.data(), static_cast<int32_t>(ps.size()),
                                         pts.empty() ? nullptr : pts.data(), static_cast<int32_t>(pts.size()), ts.empty() ? nullptr : ts.data(),
                                         static_cast<int32_t>(ts.size()), static_cast<int32_t>(k), leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  // QueryRescorer::rescore (search/scorer/rescorer.rs:118-226) for a batch: row i of `first_pass` is re-ranked by
  // requests[i]. One device call per kind of query and leaf; the last leaf's sorts the windows and re-weights the tails.
  std::vector<TopDocs> rescore(const std::vector<TopDocs>& first_pass, const std::vector<RescoreRequest>& requests, size_t k) {
    const int32_t nq = static_cast<int32_t>(first_pass.size());
    if (requests.size() != first_pass.size()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "one rescore request per row");
    std::vector<rgpu_hit> rows(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
    std::vector<rgpu_rescore_request> reqs;
    for (int32_t q = 0; q < nq; ++q) {
      const std::vector<ScoreDoc>& docs = first_pass[static_cast<size_t>(q)].score_docs();
      for (size_t i = 0; i < docs.size() && i < k; ++i) rows[static_cast<size_t>(q) * k + i] = rgpu_hit{docs[i].doc, docs[i].score};
      const RescoreRequest& r = requests[static_cast<size_t>(q)];
      reqs.push_back(rgpu_rescore_request{r.query_weight, r.rescore_weight, static_cast<int32_t>(r.mode),
                                          r.window_size > 0 ? r.window_size : static_cast<int32_t>(k)});
    }
    // rows by kind: PhraseQuery rows go through rgpu_rescore_phrase_batch, the others through rgpu_rescore_batch (a row's result
    // does not depend on the other rows, so the two sub-batches are rescored apart and scattered back)
    std::vector<size_t> plain, phrase;
    std::vector<const PhraseQuery*> phrases;
    for (size_t q = 0; q < requests.size(); ++q) {
      if (!requests[q].query) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "a rescore request needs a query");
      refuse_other_fields(*requests[q].query);
      if (dynamic_cast<const SpanNearQuery*>(requests[q].query) || dynamic_cast<const SpanTermQuery*>(requests[q].query))
        throw Error(RGPU_ERR_UNSUPPORTED, "rescoring with a span query is not served by the GPU path");
      if (const PhraseQuery* pq = dynamic_cast<const PhraseQuery*>(requests[q].query)) {
        // refused before any leaf is touched (a leaf that lacks the term would serve the row, the next one not)
        for (size_t i = 1; pq->slop > 0 && i < pq->terms.size(); ++i)
          for (size_t j = 0; j < i; ++j)
            if (pq->terms[i].term == pq->terms[j].term && pq->terms[i].text == pq->terms[j].text)
              throw Error(RGPU_ERR_UNSUPPORTED, "phrase rescoring: a sloppy phrase that names a term twice is not served");
        phrase.push_back(q);
        phrases.push_back(pq);
      }
      else plain.push_back(q);
    }
    auto gather = [&](const std::vector<size_t>& which, std::vector<rgpu_hit>* sub, std::vector<rgpu_rescore_request>* sub_reqs) {
      for (size_t q : which) {
        sub->insert(sub->end(), rows.begin() + static_cast<std::ptrdiff_t>(q * k), rows.begin() + static_cast<std::ptrdiff_t>((q + 1) * k));
        sub_reqs->push_back(reqs[q]);
      }
    };
    auto scatter = [&](const std::vector<size_t>& which, const std::vector<rgpu_hit>& sub) {
      for (size_t i = 0; i < which.size(); ++i)
        std::copy(sub.begin() + static_cast<std::ptrdiff_t>(i * k), sub.begin() + static_cast<std::ptrdiff_t>((i + 1) * k),
                  rows.begin() + static_cast<std::ptrdiff_t>(which[i] * k));
    };
    if (!plain.empty()) {
      std::vector<rgpu_hit> sub;
      std::vector<rgpu_rescore_request> sub_reqs;
      gather(plain, &sub, &sub_reqs);
      for (size_t li = 0; li < leaves_.size(); ++li) {
        std::vector<rgpu_query> qs;
        std::vector<rgpu_query_term> ts;
        for (size_t q : plain) pack(*requests[q].query, leaves_[li], &qs, &ts);
        check(rgpu_rescore_batch(leaves_[li].segment, qs.data(), static_cast<int32_t>(plain.size()), ts.data(), static_cast<int32_t>(ts.size()),
                                 sub_reqs.data(), static_cast<int32_t>(k), sub.data(), li + 1 == leaves_.size() ? 1 : 0));
      }
      scatter(plain, sub);
    }
    if (!phrase.empty()) {
      std::vector<rgpu_hit> sub;
      std::vector<rgpu_rescore_request> sub_reqs;
      gather(phrase, &sub, &sub_reqs);
      for (size_t li = 0; li < leaves_.size(); ++li) {
        if (!leaves_[li].pos_bytes) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase rescoring needs a positions field (LeafReader::pos_bytes)");
        std::vector<rgpu_phrase_query> qs;
        std::vector<rgpu_phrase_term> ts;
        pack_phrases(phrases, leaves_[li], &qs, &ts);
        check(rgpu_rescore_phrase_batch(leaves_[li].segment, qs.data(), static_cast<int32_t>(phrase.size()), ts.data(), static_cast<int32_t>(ts.size()),
                                        sub_reqs.data(), static_cast<int32_t>(k), sub.data(), li + 1 == leaves_.size() ? 1 : 0));
      }
      scatter(phrase, sub);
    }
    std::vector<TopDocs> out;
    for (int32_t q = 0; q < nq; ++q) {
      std::vector<ScoreDoc> docs;
      for (size_t i = 0; i < k; ++i) {
        const rgpu_hit& h = rows[static_cast<size_t>(q) * k + i];
        if (h.doc >= 0) docs.push_back(ScoreDoc{h.doc, h.score});
      }
      out.emplace_back(first_pass[static_cast<size_t>(q)].total_hits(), std::move(docs));
    }
    return out;
  }

 private:
  // PhraseQuery objects -> the rgpu_phrase_query[] / rgpu_phrase_term[] of one leaf (rgpu_search_phrase_batch, rgpu_rescore_phrase_batch)
  void pack_phrases(const std::vector<const PhraseQuery*>& queries, const LeafReader& leaf, std::vector<rgpu_phrase_query>* qs_out,
                    std::vector<rgpu_phrase_term>* ts_out) {
    std::vector<rgpu_phrase_query>& qs = *qs_out;
    std::vector<rgpu_phrase_term>& ts = *ts_out;
    for (const PhraseQuery* q : queries) {
      std::vector<TermStatistics> stats;
      for (const TermQuery& t : q->terms) stats.push_back(term_statistics(t));
      const BM25SimWeight w = sim_.compute_weight(stats_, stats.data(), static_cast<int32_t>(stats.size()), q->boost);
      if (sim_table_ < 0) check(sim_table_ = rgpu_sim_table_upload(ctx_, w.cache.data(), w.k1));
      qs.push_back(rgpu_phrase_query{static_cast<int32_t>(q->terms.size()), static_cast<int32_t>(ts.size()), w.weight, sim_table_, q->slop, next_limit});
      for (size_t i = 0; i < q->terms.size(); ++i) {
        rgpu_phrase_term pt{};
        if (!leaf.positions_state(q->terms[i], &pt.state, &pt.positions)) { pt.state = rgpu_term_state{}; pt.state.skip_offset = -1; pt.state.singleton_doc_id = -1; }
        pt.position = q->positions[i];
        ts.push_back(pt);
      }
    }
  }

  CachedFilter keep(std::vector<rgpu_docset*> sets) {
    CachedFilter f;
    f.id = ++next_filter_id_;
    filters_[f.id] = std::move(sets);
    return f;
  }
  const std::vector<rgpu_docset*>& sets_of(CachedFilter f) const {
    auto at = filters_.find(f.id);
    if (at == filters_.end()) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "a cached filter belongs to the searcher that made it (and is gone after drop_filter)");
    return at->second;
  }
  // one doc set per leaf for a combination of filters and excludes: a single filter is its own mask; anything else is combined once per
  // combination and leaf (rgpu_docset_combine) and kept
  const std::vector<rgpu_docset*>& masks_of(const rgpu_host::DocsetKey& key) {
    if (key.filters.size() == 1 && key.excludes.empty()) return sets_of(CachedFilter{key.filters[0]});
    const auto mk = std::make_pair(key.filters, key.excludes);
    auto at = masks_.find(mk);
    if (at != masks_.end()) return at->second;
    std::vector<rgpu_docset*> made(leaves_.size(), nullptr);
    try {
      for (size_t li = 0; li < leaves_.size(); ++li) {
        std::vector<rgpu_docset*> all, none;
        for (uint64_t id : key.filters) all.push_back(sets_of(CachedFilter{id})[li]);
        for (uint64_t id : key.excludes) none.push_back(sets_of(CachedFilter{id})[li]);
        check(rgpu_docset_combine(leaves_[li].segment, all.data(), static_cast<int32_t>(all.size()), none.data(), static_cast<int32_t>(none.size()), &made[li]));
      }
    } catch (...) {
      for (rgpu_docset* d : made) rgpu_docset_free(d);
      throw;
    }
    return masks_.emplace(mk, std::move(made)).first->second;
  }
  std::vector<TopDocs> search_filtered(const std::vector<const Query*>& queries, size_t k) {
    std::vector<rgpu_host::DocsetKey> keys(queries.size());
    std::vector<const Query*> inner(queries.size());
    std::vector<char> required(queries.size(), 0);   // the doc sets are the row's only required clauses (required_sets)
    for (size_t i = 0; i < queries.size(); ++i) {   // refused before any leaf is touched
      inner[i] = queries[i];
      if (const FilteredQuery* f = dynamic_cast<const FilteredQuery*>(queries[i])) {
        required[i] = f->check_served(filtered_phrases, required_sets) ? 1 : 0;
        std::vector<uint64_t> fs, xs;
        for (CachedFilter c : f->filters) { sets_of(c); fs.push_back(c.id); }
        for (CachedFilter c : f->excludes) { sets_of(c); xs.push_back(c.id); }
        if (required[i] && fs.empty()) fs.push_back(every_doc().id);   // "-X" is "+*:* -X"
        keys[i] = rgpu_host::docset_key(std::move(fs), std::move(xs));
        inner[i] = f->query;
      } else if (dynamic_cast<const MatchAllDocsQuery*>(queries[i])) {
        if (!required_sets) throw Error(RGPU_ERR_UNSUPPORTED, "MatchAllDocsQuery is not served by the GPU path (required_sets)");
        required[i] = 1;
        keys[i] = rgpu_host::docset_key({every_doc().id}, {});
      }
    }
    std::vector<TopDocs> out(queries.size());
    // rows whose only required clauses are the sets: groups, and calls, of their own
    std::vector<rgpu_host::DocsetKey> required_keys;
    std::vector<size_t> required_at;
    for (size_t i = 0; i < queries.size(); ++i)
      if (required[i]) { required_keys.push_back(keys[i]); required_at.push_back(i); }
    for (const rgpu_host::DocsetGroup& grp : rgpu_host::group_by_docset_key(required_keys)) {
      std::vector<const BooleanQuery*> part;   // null: no optional side (MatchAllDocsQuery)
      for (int32_t r : grp.rows) part.push_back(dynamic_cast<const BooleanQuery*>(inner[required_at[static_cast<size_t>(r)]]));
      std::vector<TopDocs> got = search_required_sets(part, masks_of(grp.key), k);
      for (size_t i = 0; i < grp.rows.size(); ++i) out[required_at[static_cast<size_t>(grp.rows[i])]] = std::move(got[i]);
    }
    std::vector<rgpu_host::DocsetKey> other_keys;
    std::vector<size_t> other_at;
    for (size_t i = 0; i < queries.size(); ++i)
      if (!required[i]) { other_keys.push_back(keys[i]); other_at.push_back(i); }
    for (const rgpu_host::DocsetGroup& grp0 : rgpu_host::group_by_docset_key(other_keys)) {
      rgpu_host::DocsetGroup grp = grp0;
      for (int32_t& r : grp.rows) r = static_cast<int32_t>(other_at[static_cast<size_t>(r)]);   // rows of the caller's batch again
      std::vector<const Query*> part;
      for (int32_t r : grp.rows) part.push_back(inner[static_cast<size_t>(r)]);
      std::vector<TopDocs> got;
      if (grp.key.empty()) {
        got = search_many(part, k);
      } else {
        const std::vector<rgpu_docset*>& masks = masks_of(grp.key);
        // (filtered_phrases: the group's phrase rows, by kind, through the masked phrase calls; the other rows as they went)
        std::vector<size_t> plain_at, phrase_at, bool_at, or_at;
        for (size_t i = 0; i < part.size(); ++i) {
          if (dynamic_cast<const PhraseQuery*>(part[i])) phrase_at.push_back(i);
          else if (dynamic_cast<const PhraseBooleanQuery*>(part[i])) bool_at.push_back(i);
          else if (dynamic_cast<const PhraseDisjunctionQuery*>(part[i])) or_at.push_back(i);
          else plain_at.push_back(i);
        }
        got.resize(part.size());
        auto place = [&](const std::vector<size_t>& at, std::vector<TopDocs> rows) { for (size_t i = 0; i < at.size(); ++i) got[at[i]] = std::move(rows[i]); };
        if (!plain_at.empty()) {
          std::vector<const Query*> plain;
          for (size_t i : plain_at) plain.push_back(part[i]);
          const int32_t nq = static_cast<int32_t>(plain.size());
          std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
          std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
          for (size_t li = 0; li < leaves_.size(); ++li) {
            std::vector<rgpu_query> qs;
            std::vector<rgpu_query_term> ts;
            plan(plain, li, &qs, &ts);
            leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
            leaf_totals[li].assign(static_cast<size_t>(nq), 0);
            check(rgpu_search_batch_masked(leaves_[li].segment, masks[li], qs.data(), nq, ts.data(), static_cast<int32_t>(ts.size()), static_cast<int32_t>(k),
                                           leaf_hits[li].data(), leaf_totals[li].data()));
          }
          place(plain_at, merge_leaves(leaf_hits, leaf_totals, nq, k));
        }
        if (!phrase_at.empty()) {
          std::vector<const PhraseQuery*> rows;
          for (size_t i : phrase_at) rows.push_back(static_cast<const PhraseQuery*>(part[i]));
          place(phrase_at, search_phrases(rows, k, &masks));
        }
        if (!bool_at.empty()) {
          std::vector<const PhraseBooleanQuery*> rows;
          for (size_t i : bool_at) rows.push_back(static_cast<const PhraseBooleanQuery*>(part[i]));
          place(bool_at, search_phrase_bools(rows, k, &masks));
        }
        if (!or_at.empty()) {
          std::vector<const PhraseDisjunctionQuery*> rows;
          for (size_t i : or_at) rows.push_back(static_cast<const PhraseDisjunctionQuery*>(part[i]));
          place(or_at, search_phrase_ors(rows, k, &masks));
        }
      }
      for (size_t i = 0; i < grp.rows.size(); ++i) out[static_cast<size_t>(grp.rows[i])] = std::move(got[i]);
    }
    return out;
  }

  // Rows whose only required clauses are the doc sets behind `masks` (rgpu_search_batch_required_set): the rows' SHOULD sides as
  // OR queries, {OR, no clause} for a row without one (null). Zero-score rows of earlier leaves carry lower global ids: merge_leaves'
  // order is the reference's.
  std::vector<TopDocs> search_required_sets(const std::vector<const BooleanQuery*>& rows, const std::vector<rgpu_docset*>& masks, size_t k) {
    const int32_t nq = static_cast<int32_t>(rows.size());
    std::vector<const Query*> scored;
    for (const BooleanQuery* b : rows) if (b) scored.push_back(b);
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      std::vector<rgpu_query> some, qs(rows.size(), rgpu_query{RGPU_OP_OR, 0, 0, 0});
      std::vector<rgpu_query_term> ts;
      if (!scored.empty()) plan(scored, li, &some, &ts);
      size_t at = 0;
      for (size_t i = 0; i < rows.size(); ++i) if (rows[i]) qs[i] = some[at++];
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      check(rgpu_search_batch_required_set(leaves_[li].segment, masks[li], qs.data(), nq, ts.empty() ? nullptr : ts.data(), static_cast<int32_t>(ts.size()),
                                           static_cast<int32_t>(k), leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  // TopDocsCollector::finish_parallel (top_docs.rs:157-172) over a handful of leaves: canonical order
  std::vector<TopDocs> merge_leaves(const std::vector<std::vector<rgpu_hit>>& leaf_hits, const std::vector<std::vector<int64_t>>& leaf_totals,
                                    int32_t nq, size_t k) const {
    std::vector<TopDocs> out;
    for (int32_t q = 0; q < nq; ++q) {
      std::vector<ScoreDoc> all;
      int64_t total = 0;
      for (size_t li = 0; li < leaves_.size(); ++li) {
        total += leaf_totals[li][static_cast<size_t>(q)];
        for (size_t i = 0; i < k; ++i) {
          const rgpu_hit& h = leaf_hits[li][static_cast<size_t>(q) * k + i];
          if (h.doc >= 0) all.push_back(ScoreDoc{h.doc, h.score});
        }
      }
      std::stable_sort(all.begin(), all.end(), [](const ScoreDoc& a, const ScoreDoc& b) {
        return a.score > b.score || (a.score == b.score && a.doc < b.doc);
      });
      if (all.size() > k) all.resize(k);
      out.emplace_back(total, std::move(all));
    }
    return out;
  }

  // ---- cross-field queries (rgpu_search_fields_batch) -----------------------------------------------------------------------------
  bool primary(const TermQuery& t) const { return t.field.empty() || t.field == leaves_[0].field; }
  bool any_other_field(const std::vector<TermQuery>& ts) const {
    for (const TermQuery& t : ts) if (!primary(t)) return true;
    return false;
  }
  // does some TermQuery of the tree name a field other than the leaves' primary one?
  bool names_other_field(const Query& q) const {
    if (dynamic_cast<const MultiFieldQuery*>(&q)) return true;  // (served by the cross-field call whatever its fields)
    if (auto* t = dynamic_cast<const TermQuery*>(&q)) return !primary(*t);
    if (auto* b = dynamic_cast<const BooleanQuery*>(&q)) return any_other_field(b->must_queries) || any_other_field(b->should_queries) || any_other_field(b->must_not_queries);
    if (auto* d = dynamic_cast<const DisjunctionMaxQuery*>(&q)) return any_other_field(d->disjuncts);
    if (auto* bo = dynamic_cast<const BoostingQuery*>(&q)) return (bo->served_positive() && names_other_field(*bo->served_positive())) || any_other_field(bo->demoting_terms());
    // every other type that holds TermQuery members: none of them is served across fields (cross_spec refuses them), and none may
    // answer for the primary field's postings under another field's name
    if (auto* p = dynamic_cast<const PhraseQuery*>(&q)) return any_other_field(p->terms);
    if (auto* st = dynamic_cast<const SpanTermQuery*>(&q)) return !primary(st->term);
    if (auto* sn = dynamic_cast<const SpanNearQuery*>(&q)) {
      for (const SpanTermQuery& c : sn->clauses) if (!primary(c.term)) return true;
      return false;
    }
    if (auto* pb = dynamic_cast<const PhraseBooleanQuery*>(&q)) {
      for (const PhraseBooleanQuery::Required& r : pb->required)
        if (r.phrase ? any_other_field(r.phrase->terms) : !primary(r.term)) return true;
      return any_other_field(pb->must_not_queries);
    }
    if (auto* pd = dynamic_cast<const PhraseDisjunctionQuery*>(&q)) {
      for (const PhraseDisjunctionQuery::Should& c : pd->should_queries)
        if (c.phrase ? any_other_field(c.phrase->terms) : !primary(c.term)) return true;
      return any_other_field(pd->must_not_queries);
    }
    if (auto* po = dynamic_cast<const PhraseOptionalQuery*>(&q)) {
      for (const auto* side : {&po->required, &po->should_queries})
        for (const PhraseOptionalQuery::Clause& c : *side)
          if (c.phrase ? any_other_field(c.phrase->terms) : !primary(c.term)) return true;
      return any_other_field(po->must_not_queries);
    }
    if (auto* fq = dynamic_cast<const FilteredQuery*>(&q)) return fq->query && names_other_field(*fq->query);
    if (auto* nb = dynamic_cast<const NestedBooleanQuery*>(&q)) {
      for (const auto* list : {&nb->must_queries, &nb->should_queries, &nb->must_not_nested, &nb->filter_nested})
        for (const std::unique_ptr<Query>& c : *list) if (c && names_other_field(*c)) return true;
      return any_other_field(nb->must_not_queries);
    }
    return false;
  }
  // every path but search / search_many reads the primary field alone: such a tree is the caller's CPU path there
  void refuse_other_fields(const Query& q) const {
    if (names_other_field(q)) throw Error(RGPU_ERR_UNSUPPORTED, "a query that names a further field is served by search / search_many only");
  }
  // a flat tree over TermQuery / DisjunctionMaxQuery clauses as the call's groups; what the call cannot express is UnsupportedOperation
  MultiFieldQuery cross_spec(const Query& q) const {
    MultiFieldQuery m;
    if (auto* mf = dynamic_cast<const MultiFieldQuery*>(&q)) m = *mf;
    else if (auto* t = dynamic_cast<const TermQuery*>(&q)) m.groups.push_back(MultiFieldQuery::term(*t));
    else if (auto* d = dynamic_cast<const DisjunctionMaxQuery*>(&q)) m.groups.push_back(MultiFieldQuery::dismax(d->disjuncts, d->tie_breaker_multiplier));
    else if (auto* b = dynamic_cast<const BooleanQuery*>(&q)) {
      if (b->should_required || b->nested_must) throw Error(RGPU_ERR_UNSUPPORTED, "nested boolean clauses are not served across fields by the GPU path");
      if (!b->must_queries.empty() && !b->should_queries.empty())
        throw Error(RGPU_ERR_UNSUPPORTED, "MUST and SHOULD clauses in one cross-field query (ReqOptScorer) are not served by the GPU path");
      m.must = !b->must_queries.empty();
      for (const TermQuery& t : m.must ? b->must_queries : b->should_queries) m.groups.push_back(MultiFieldQuery::term(t));
      m.min_should_match = m.must ? 0 : b->min_should_match;
      m.must_not_queries = b->must_not_queries;
    } else {
      throw Error(RGPU_ERR_UNSUPPORTED, "query type not served across fields by the GPU path");
    }
    if (m.is_tree() && !field_trees)
      throw Error(RGPU_ERR_UNSUPPORTED, "nested should-only groups and MUST beside SHOULD groups are not served across fields by the GPU path (field_trees)");
    if (!m.should_groups.empty() && !m.must) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "should_groups stand beside MUST groups");
    if (m.groups.empty()) throw Error(RGPU_ERR_UNSUPPORTED, "a query of MUST_NOT clauses alone is not served across fields by the GPU path");
    if (m.should_groups.size() > static_cast<size_t>(RGPU_MAX_FIELD_GROUPS)) throw Error(RGPU_ERR_UNSUPPORTED, "ten or more clauses are summed in heap order by the reference");
    if (m.groups.size() > static_cast<size_t>(RGPU_MAX_FIELD_GROUPS)) throw Error(RGPU_ERR_UNSUPPORTED, "ten or more clauses are summed in heap order by the reference");
    if (!m.must && m.min_should_match >= 2 && !m.must_not_queries.empty())
      throw Error(RGPU_ERR_UNSUPPORTED, "MUST_NOT clauses beside min_should_match >= 2 are not served across fields by the GPU path");
    auto known = [&](const TermQuery& t) {
      if (primary(t)) return;
      for (const LeafReader& l : leaves_) if (!l.extra(t.field)) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "no field '" + t.field + "' among the leaves' extra_fields");
    };
    for (const auto* side : {&m.groups, &m.should_groups})
      for (const MultiFieldQuery::Group& g : *side) {
        if (g.terms.size() > static_cast<size_t>(RGPU_MAX_GROUP_DISJUNCTS)) throw Error(RGPU_ERR_UNSUPPORTED, "ten or more disjuncts are summed in heap order by the reference");
        if (g.dismax && !std::isfinite(g.tie_breaker_multiplier)) throw Error(RGPU_ERR_ILLEGAL_ARGUMENT, "tie_breaker_multiplier is not finite");
        if (g.sum && g.min_should_match >= 2) throw Error(RGPU_ERR_UNSUPPORTED, "a nested min_should_match >= 2 is not served across fields by the GPU path");
        for (const TermQuery& t : g.terms) known(t);
      }
    for (const TermQuery& t : m.must_not_queries) known(t);
    return m;
  }
  // (weight, sim table) of a clause from ITS field's statistics in the statistics leaf (searcher.rs:306-363, 732-767): one cache per field
  std::pair<float, int32_t> field_weight_of(const TermQuery& tq) {
    if (primary(tq)) return weight_of(tq);
    const ExtraField& x = *leaves_[stats_leaf_].extra(tq.field);
    rgpu_term_state st;
    TermStatistics ts;
    const bool have = x.term_state(tq, &st);
    ts.doc_freq = have ? st.doc_freq : 0;
    ts.total_term_freq = have ? st.total_term_freq : 0;
    CollectionStatistics cs = stats_;
    cs.doc_count = x.doc_count;
    cs.sum_total_term_freq = x.sum_total_term_freq;
    cs.sum_doc_freq = x.sum_doc_freq;
    const BM25SimWeight w = sim_.compute_weight(cs, &ts, 1, tq.boost);
    auto at = field_sim_tables_.find(tq.field);
    if (at == field_sim_tables_.end()) {
      int32_t table = -1;
      check(table = rgpu_sim_table_upload(ctx_, w.cache.data(), w.k1));
      at = field_sim_tables_.emplace(tq.field, table).first;
    }
    return {w.weight, at->second};
  }
  std::vector<TopDocs> search_fields(const std::vector<MultiFieldQuery>& specs, size_t k) {
    if (k > 128) throw Error(RGPU_ERR_UNSUPPORTED, "a cross-field query is served for k <= 128");
    const int32_t nq = static_cast<int32_t>(specs.size());
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      const LeafReader& leaf = leaves_[li];
      std::vector<rgpu_fields_query> qs;
      std::vector<rgpu_field_group> gs;
      std::vector<rgpu_field_clause> cs;
      auto clause = [&](const TermQuery& t, bool scored) {
        rgpu_field_clause c{};
        const ExtraField* x = primary(t) ? nullptr : leaf.extra(t.field);
        const bool have = x ? x->term_state(t, &c.state) : leaf.term_state(t, &c.state);
        if (!have) { c.state = rgpu_term_state{}; c.state.skip_offset = -1; c.state.singleton_doc_id = -1; }
        if (scored) { auto w = field_weight_of(t); c.weight = w.first; c.sim_table = w.second; }
        c.field = x ? x->slot : 0;
        cs.push_back(c);
      };
      for (const MultiFieldQuery& m : specs) {
        rgpu_fields_query fq{};
        fq.occur = m.must ? RGPU_OCCUR_MUST : RGPU_OCCUR_SHOULD;
        fq.first_group = static_cast<int32_t>(gs.size());
        fq.n_groups = static_cast<int32_t>(m.groups.size());
        fq.min_should_match = m.must ? 0 : m.min_should_match;
        for (const MultiFieldQuery::Group& g : m.groups) {
          rgpu_field_group fg{};
          fg.first_term = static_cast<int32_t>(cs.size());
          fg.n_terms = static_cast<int32_t>(g.terms.size());
          fg.kind = g.dismax ? RGPU_GROUP_DISMAX : RGPU_GROUP_TERM;
          std::memcpy(&fg.tie_bits, &g.tie_breaker_multiplier, sizeof fg.tie_bits);
          for (const TermQuery& t : g.terms) clause(t, true);
          gs.push_back(fg);
        }
        fq.first_must_not = static_cast<int32_t>(cs.size());
        fq.n_must_not = static_cast<int32_t>(m.must_not_queries.size());
        for (const TermQuery& t : m.must_not_queries) clause(t, false);
        qs.push_back(fq);
      }
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      check(rgpu_search_fields_batch(leaf.segment, qs.data(), nq, gs.data(), static_cast<int32_t>(gs.size()), cs.data(), static_cast<int32_t>(cs.size()),
                                     static_cast<int32_t>(k), leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }
  // field_trees: the rows with SUM groups or SHOULD groups beside MUST groups, through rgpu_search_fields_tree_batch per leaf
  std::vector<TopDocs> search_fields_tree(const std::vector<MultiFieldQuery>& specs, size_t k) {
    if (k > 128) throw Error(RGPU_ERR_UNSUPPORTED, "a cross-field query is served for k <= 128");
    const int32_t nq = static_cast<int32_t>(specs.size());
    std::vector<std::vector<rgpu_hit>> leaf_hits(leaves_.size());
    std::vector<std::vector<int64_t>> leaf_totals(leaves_.size());
    for (size_t li = 0; li < leaves_.size(); ++li) {
      const LeafReader& leaf = leaves_[li];
      std::vector<rgpu_fields_tree_query> qs;
      std::vector<rgpu_field_tree_group> gs;
      std::vector<rgpu_field_clause> cs;
      auto clause = [&](const TermQuery& t, bool scored) {
        rgpu_field_clause c{};
        const ExtraField* x = primary(t) ? nullptr : leaf.extra(t.field);
        const bool have = x ? x->term_state(t, &c.state) : leaf.term_state(t, &c.state);
        if (!have) { c.state = rgpu_term_state{}; c.state.skip_offset = -1; c.state.singleton_doc_id = -1; }
        if (scored) { auto w = field_weight_of(t); c.weight = w.first; c.sim_table = w.second; }
        c.field = x ? x->slot : 0;
        cs.push_back(c);
      };
      for (const MultiFieldQuery& m : specs) {
        rgpu_fields_tree_query fq{};
        fq.first_group = static_cast<int32_t>(gs.size());
        fq.n_must = m.must ? static_cast<int32_t>(m.groups.size()) : 0;
        fq.n_should = static_cast<int32_t>(m.must ? m.should_groups.size() : m.groups.size());
        fq.min_should_match = m.min_should_match;
        for (const auto* side : {&m.groups, &m.should_groups})
          for (const MultiFieldQuery::Group& g : *side) {
            rgpu_field_tree_group fg{};
            fg.first_term = static_cast<int32_t>(cs.size());
            fg.n_terms = static_cast<int32_t>(g.terms.size());
            fg.kind = g.sum ? RGPU_GROUP_SUM : g.dismax ? RGPU_GROUP_DISMAX : RGPU_GROUP_TERM;
            fg.min_should_match = g.sum ? g.min_should_match : 0;
            std::memcpy(&fg.tie_bits, &g.tie_breaker_multiplier, sizeof fg.tie_bits);
            for (const TermQuery& t : g.terms) clause(t, true);
            gs.push_back(fg);
          }
        fq.first_must_not = static_cast<int32_t>(cs.size());
        fq.n_must_not = static_cast<int32_t>(m.must_not_queries.size());
        for (const TermQuery& t : m.must_not_queries) clause(t, false);
        qs.push_back(fq);
      }
      leaf_hits[li].assign(static_cast<size_t>(nq) * k, rgpu_hit{-1, 0.f});
      leaf_totals[li].assign(static_cast<size_t>(nq), 0);
      check(rgpu_search_fields_tree_batch(leaf.segment, qs.data(), nq, gs.data(), static_cast<int32_t>(gs.size()), cs.data(), static_cast<int32_t>(cs.size()),
                                          static_cast<int32_t>(k), leaf_hits[li].data(), leaf_totals[li].data()));
    }
    return merge_leaves(leaf_hits, leaf_totals, nq, k);
  }

  std::pair<float, int32_t> weight_of(const TermQuery& tq) {
    // TermQuery::create_weight (term_query.rs:58-95) -> BM25Similarity::compute_weight
    const TermStatistics ts = term_statistics(tq);
    const BM25SimWeight w = sim_.compute_weight(stats_, &ts, 1, tq.boost);
    if (sim_table_ < 0) check(sim_table_ = rgpu_sim_table_upload(ctx_, w.cache.data(), w.k1));  // one field -> one cache
    return {w.weight, sim_table_};
  }
  // The whole batch at once: the query objects are flattened to op / clause-count / term arrays and handed to the native
  // batch planner (rgpu_plan_batch_*: term resolution in this leaf and in the statistics leaf, BM25 weights, the sim table)
  // — one call per leaf instead of one dictionary lookup and one f64 log per clause. A batch that mixes id-named and
  // byte-named terms (or names terms the leaf cannot resolve that way) goes clause by clause through pack().
  void plan(const std::vector<const Query*>& queries, size_t li, std::vector<rgpu_query>* qs, std::vector<rgpu_query_term>* ts) {
    for (const Query* q : queries) refuse_other_fields(*q);  // (search_many has routed those rows away; every other caller refuses them)
    const LeafReader& leaf = leaves_[li];
    std::vector<int32_t> ops, n_terms, n_not;
    std::vector<int64_t> ids, offs{0};
    std::vector<uint8_t> bytes;
    std::vector<float> boosts;
    bool any_id = false, any_text = false, any_boost = false;
    auto clause = [&](const TermQuery& c) {
      if (c.by_text()) { any_text = true; bytes.insert(bytes.end(), c.text.begin(), c.text.end()); }
      else { any_id = true; }
      ids.push_back(c.term);
      offs.push_back(static_cast<int64_t>(bytes.size()));
      boosts.push_back(c.boost);
      any_boost = any_boost || c.boost != 1.0f;
    };
    for (const Query* q0 : queries) {
      // (a BoostingQuery is planned as its positive query, the demoting clauses as further MUST_NOT clauses; the count's second byte
      // and the boost are written below)
      const BoostingQuery* bo = dynamic_cast<const BoostingQuery*>(q0);
      const Query* q = bo ? bo->served_positive() : q0;
      if (auto* t = dynamic_cast<const TermQuery*>(q)) {
        ops.push_back(RGPU_OP_TERM); n_terms.push_back(1); n_not.push_back(0);
        clause(*t);
      } else if (auto* b = dynamic_cast<const BooleanQuery*>(q)) {
        const bool conj = !b->must_queries.empty();
        ops.push_back(conj ? (RGPU_OP_WITH_SHOULD(RGPU_OP_AND, b->should_queries.size()) | (b->should_required ? RGPU_OP_SHOULD_REQUIRED : 0) | (b->nested_must ? RGPU_OP_NESTED_MUST : 0) | RGPU_OP_NESTED_AT(b->nested_at))
                           : (b->min_should_match > 1 ? RGPU_OP_OR_MSM(b->min_should_match) : (int32_t)RGPU_OP_OR));
        n_terms.push_back(static_cast<int32_t>(conj ? b->must_queries.size() : b->should_queries.size()));
        n_not.push_back(static_cast<int32_t>(b->must_not_queries.size()));
        for (const TermQuery& c : (conj ? b->must_queries : b->should_queries)) clause(c);
        if (conj) for (const TermQuery& c : b->should_queries) clause(c);
        for (const TermQuery& c : b->must_not_queries) clause(c);
      } else if (auto* d = dynamic_cast<const DisjunctionMaxQuery*>(q)) {
        // (the planner resolves and weighs the disjuncts as an OR query's clauses; op and tie-breaker are written below)
        ops.push_back(RGPU_OP_OR); n_terms.push_back(static_cast<int32_t>(d->disjuncts.size())); n_not.push_back(0);
        for (const TermQuery& c : d->disjuncts) clause(c);
      } else {
        throw Error(RGPU_ERR_UNSUPPORTED, "query type not served by the GPU path");
      }
      if (bo) {
        const std::vector<TermQuery> dem = bo->demoting_terms();
        if (n_terms.back() + ((ops.back() >> 16) & 0xff) + n_not.back() + static_cast<int32_t>(dem.size()) > RGPU_MAX_QUERY_TERMS)
          throw Error(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_QUERY_TERMS clauses in one query");
        n_not.back() += static_cast<int32_t>(dem.size());
        for (const TermQuery& c : dem) clause(c);
      }
    }
    const LeafReader& sl = leaves_[stats_leaf_];
    const bool native = (any_id != any_text) && (any_text ? (leaf.dictionary && sl.dictionary) : (leaf.terms && sl.terms));
    if (!native) {
      for (const Query* q : queries) pack(*q, leaf, qs, ts);
      return;
    }
    if (planners_.size() < 2 * leaves_.size()) planners_.resize(2 * leaves_.size(), nullptr);
    const size_t pi = 2 * li + (any_text ? 1 : 0);  // a leaf may be queried by id and by bytes: one planner each
    if (!planners_[pi]) {
      rgpu_plan_stats ps{stats_.max_doc, stats_.doc_count, stats_.sum_total_term_freq, sim_.k1(), sim_.b()};
      if (sim_table_ < 0) {  // one field -> one norm cache, shared with the clause-by-clause path
        const TermStatistics none;
        check(sim_table_ = rgpu_sim_table_upload(ctx_, sim_.compute_weight(stats_, &none, 1, 1.0f).cache.data(), sim_.k1()));
      }
      if (any_text) check(rgpu_planner_create(nullptr, &ps, leaf.dictionary, &sl == &leaf ? nullptr : sl.dictionary, leaf.field_number, &planners_[pi]));
      else check(rgpu_planner_create_flat(nullptr, &ps, leaf.terms, leaf.n_terms, &sl == &leaf ? nullptr : sl.terms, &sl == &leaf ? 0 : sl.n_terms, &planners_[pi]));
      check(rgpu_planner_set_sim_table(planners_[pi], sim_table_));
    }
    qs->resize(queries.size());
    ts->resize(std::max<size_t>(1, ids.size()));
    const int64_t cap = static_cast<int64_t>(ids.size());
    if (any_text)
      check(rgpu_plan_batch_bytes(planners_[pi], static_cast<int32_t>(queries.size()), ops.data(), n_terms.data(), n_not.data(), bytes.data(), offs.data(),
                                  any_boost ? boosts.data() : nullptr, qs->data(), ts->data(), cap));
    else
      check(rgpu_plan_batch_ids(planners_[pi], static_cast<int32_t>(queries.size()), ops.data(), n_terms.data(), n_not.data(), ids.data(),
                                any_boost ? boosts.data() : nullptr, qs->data(), ts->data(), cap));
    ts->resize(ids.size());
    // the second half of a dismax query's packing (the first: the RGPU_OP_OR entry pushed above): the planner knows no op 3, so it
    // resolved and weighed the disjuncts as SHOULD clauses — and rewrote a one-clause query to RGPU_OP_TERM; op and the tie-breaker's
    // bits are written over its records here. pack() writes the same two fields directly.
    for (size_t i = 0; i < queries.size(); ++i)
      if (auto* d = dynamic_cast<const DisjunctionMaxQuery*>(queries[i])) { (*qs)[i].op = RGPU_OP_DISMAX; (*qs)[i].n_must_not = d->tie_bits(); }
    // a BoostingQuery's second half: the last n_demote of the clauses planned as MUST_NOT are the demoting ones
    for (size_t i = 0; i < queries.size(); ++i)
      if (auto* bo = dynamic_cast<const BoostingQuery*>(queries[i])) demote_fields(*bo, &(*qs)[i], ts);
  }
  // RGPU_NOT_WITH_DEMOTE: the demoting clauses' count moves to the second byte of n_must_not, their weight is negative_boost, their
  // table is never read
  static void demote_fields(const BoostingQuery& bo, rgpu_query* rq, std::vector<rgpu_query_term>* ts) {
    const int32_t n_dem = static_cast<int32_t>(bo.demoting_terms().size()), n_not = rq->n_must_not - n_dem;
    rq->n_must_not = RGPU_NOT_WITH_DEMOTE(n_not, n_dem);
    for (int32_t i = 0; i < n_dem; ++i) {
      rgpu_query_term& t = (*ts)[static_cast<size_t>(rq->first_term + rq->n_terms + n_not + i)];
      t.weight = bo.negative_boost;
      t.sim_table = 0;
    }
  }
  void pack(const Query& q0, const LeafReader& leaf, std::vector<rgpu_query>* qs, std::vector<rgpu_query_term>* ts) {
    refuse_other_fields(q0);
    const BoostingQuery* bo = dynamic_cast<const BoostingQuery*>(&q0);
    const Query& q = bo ? *bo->served_positive() : q0;
    const std::vector<TermQuery>* clauses = nullptr;
    const std::vector<TermQuery>* opts = nullptr;  // SHOULD clauses beside MUST ones
    const std::vector<TermQuery>* nots = nullptr;
    std::vector<TermQuery> single;
    int32_t op = RGPU_OP_TERM;
    if (auto* t = dynamic_cast<const TermQuery*>(&q)) {
      single.push_back(*t);
      clauses = &single;
    } else if (auto* b = dynamic_cast<const BooleanQuery*>(&q)) {
      op = b->must_queries.empty() ? (b->min_should_match > 1 ? RGPU_OP_OR_MSM(b->min_should_match) : (int32_t)RGPU_OP_OR)
                                   : (RGPU_OP_WITH_SHOULD(RGPU_OP_AND, b->should_queries.size()) | (b->should_required ? RGPU_OP_SHOULD_REQUIRED : 0) | (b->nested_must ? RGPU_OP_NESTED_MUST : 0) | RGPU_OP_NESTED_AT(b->nested_at));
      clauses = b->must_queries.empty() ? &b->should_queries : &b->must_queries;
      if (!b->must_queries.empty()) opts = &b->should_queries;
      nots = &b->must_not_queries;
    } else if (auto* d = dynamic_cast<const DisjunctionMaxQuery*>(&q)) {
      op = RGPU_OP_DISMAX;
      clauses = &d->disjuncts;
    } else {
      throw Error(RGPU_ERR_UNSUPPORTED, "query type not served by the GPU path");
    }
    std::vector<TermQuery> all(*clauses);  // clause order: MUST / scored, optional SHOULD, MUST_NOT
    if (opts) all.insert(all.end(), opts->begin(), opts->end());
    if (nots) all.insert(all.end(), nots->begin(), nots->end());
    rgpu_query rq{op, static_cast<int32_t>(clauses->size()), static_cast<int32_t>(ts->size()),
                  static_cast<int32_t>(nots ? nots->size() : 0)};
    if (bo) {  // the demoting clauses behind the MUST_NOT ones (counted as such until demote_fields splits the field)
      const std::vector<TermQuery> dem = bo->demoting_terms();
      all.insert(all.end(), dem.begin(), dem.end());
      rq.n_must_not += static_cast<int32_t>(dem.size());
      if (all.size() > static_cast<size_t>(RGPU_MAX_QUERY_TERMS)) throw Error(RGPU_ERR_UNSUPPORTED, "more than RGPU_MAX_QUERY_TERMS clauses in one query");
    }
    if (auto* d = dynamic_cast<const DisjunctionMaxQuery*>(&q)) rq.n_must_not = d->tie_bits();  // RGPU_OP_DISMAX: the tie-breaker's bits
    for (const TermQuery& c : all) {
      rgpu_query_term qt{};
      if (!leaf.term_state(c, &qt.state)) { qt.state = rgpu_term_state{}; qt.state.skip_offset = -1; qt.state.singleton_doc_id = -1; }
      auto w = weight_of(c);
      qt.weight = w.first;
      qt.sim_table = w.second;
      ts->push_back(qt);
    }
    if (bo) demote_fields(*bo, &rq, ts);
    qs->push_back(rq);
  }

  static int64_t leaf_num_docs(const LeafReader& leaf) {
    if (!leaf.live_docs) return leaf.max_doc;
    int64_t n = 0;
    for (int32_t d = 0; d < leaf.max_doc; ++d) n += static_cast<int64_t>((leaf.live_docs[d >> 6] >> (d & 63)) & 1u);
    return n;
  }

  std::vector<LeafReader> leaves_;
  BM25Similarity sim_;
  rgpu_ctx* ctx_ = nullptr;
  size_t stats_leaf_ = 0;
  CollectionStatistics stats_;
  int32_t sim_table_ = -1;
  std::map<std::string, int32_t> field_sim_tables_;  // a further field's norm cache: one table per field
  std::vector<rgpu_planner*> planners_;  // per leaf and naming scheme (2 * leaf + by-bytes), created on first use
  std::map<uint64_t, std::vector<rgpu_docset*>> filters_;  // CachedFilter::id -> one doc set per leaf
  struct FieldPoints {
    int32_t bytes_per_dim = 0;
    std::vector<rgpu_points*> per_leaf;  // null: the leaf lacks the field
  };
  std::map<std::string, FieldPoints> points_;
  std::map<std::tuple<std::string, std::vector<uint8_t>, std::vector<uint8_t>>, CachedFilter> range_filters_;  // the memo of range_filter
  std::map<std::pair<std::vector<uint64_t>, std::vector<uint64_t>>, std::vector<rgpu_docset*>> masks_;  // (filters, excludes) -> combined sets per leaf
  uint64_t next_filter_id_ = 0;
  CachedFilter every_doc_;
};

}  // namespace rucene
