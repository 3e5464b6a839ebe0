// The batch planner (host/batch_planner.hpp, included here as the single file did: mid-file). struct rgpu_planner, planner_sim_table,
// plan_checked, plan_uniform. Entry points: rgpu_planner_create_flat, rgpu_planner_create, rgpu_planner_destroy, rgpu_planner_sim_table,
// rgpu_planner_set_sim_table, rgpu_plan_batch_ids, rgpu_plan_batch_bytes, rgpu_plan_uniform_ids, rgpu_plan_uniform_bytes.
// Uses: rgpu_api.hip itself (rgpu_ctx, fail, rgpu_sim_table_upload), host_formats.hpp (rgpu_terms, BM25Similarity).
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- batch planner (host) -----------------------------------------------------------------------------------------------
#include "../host/batch_planner.hpp"
struct rgpu_planner {
  std::unique_ptr<rucene::BatchPlanner> p;
};
static int32_t planner_sim_table(rgpu_ctx* c, const rgpu_plan_stats* ps, int32_t* table_out) {
  if (!ps) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  if (!(ps->k1 >= 0.0f) || !(ps->b >= 0.0f && ps->b <= 1.0f)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "illegal k1 / b value");  // BM25Similarity::new
  if (!c) { *table_out = -1; return RGPU_OK; }  // the host uploads the field's norm cache itself: rgpu_planner_set_sim_table
  rucene::CollectionStatistics cs;
  cs.max_doc = ps->max_doc;
  cs.doc_count = ps->doc_count;
  cs.sum_total_term_freq = ps->sum_total_term_freq;
  rucene::TermStatistics ts;
  const rucene::BM25SimWeight w = rucene::BM25Similarity(ps->k1, ps->b).compute_weight(cs, &ts, 1, 1.0f);  // the cache depends on the collection alone
  const int32_t t = rgpu_sim_table_upload(c, w.cache.data(), ps->k1);
  if (t < 0) return t;
  *table_out = t;
  return RGPU_OK;
}

extern "C" int32_t rgpu_planner_create_flat(rgpu_ctx* c, const rgpu_plan_stats* ps, const rgpu_term_state* leaf_states, int64_t n_leaf,
                                            const rgpu_term_state* stats_states_or_null, int64_t n_stats, rgpu_planner** out) {
  if (!out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "out is null");
  *out = nullptr;
  if (n_leaf < 0 || (n_leaf > 0 && !leaf_states) || n_stats < 0 || (n_stats > 0 && !stats_states_or_null)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad term tables");
  int32_t table = -1;
  const int32_t rc = planner_sim_table(c, ps, &table);
  if (rc != RGPU_OK) return rc;
  try {
    auto h = std::make_unique<rgpu_planner>();
    h->p.reset(new rucene::BatchPlanner(*ps, table, leaf_states, n_leaf, stats_states_or_null, n_stats));
    *out = h.release();
  } catch (const std::bad_alloc&) { return fail(RGPU_ERR_RUNTIME, "out of host memory"); }
  return RGPU_OK;
}

extern "C" int32_t rgpu_planner_create(rgpu_ctx* c, const rgpu_plan_stats* ps, const rgpu_terms* leaf_terms, const rgpu_terms* stats_terms_or_null,
                                       int32_t field_number, rgpu_planner** out) {
  if (!out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "out is null");
  *out = nullptr;
  if (!leaf_terms) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "leaf_terms is null");
  if (!leaf_terms->dict->field_stats(field_number)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "no such indexed field in this segment");
  int32_t table = -1;
  const int32_t rc = planner_sim_table(c, ps, &table);
  if (rc != RGPU_OK) return rc;
  auto h = std::make_unique<rgpu_planner>();
  h->p.reset(new rucene::BatchPlanner(*ps, table, leaf_terms->dict.get(), stats_terms_or_null ? stats_terms_or_null->dict.get() : nullptr, field_number));
  *out = h.release();
  return RGPU_OK;
}

extern "C" void rgpu_planner_destroy(rgpu_planner* p) { delete p; }
extern "C" int32_t rgpu_planner_sim_table(const rgpu_planner* p) { return p ? p->p->sim_table() : RGPU_ERR_ILLEGAL_ARGUMENT; }
extern "C" int32_t rgpu_planner_set_sim_table(rgpu_planner* p, int32_t sim_table) {
  if (!p || sim_table < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  p->p->set_sim_table(sim_table);
  return RGPU_OK;
}

static int32_t plan_checked(rgpu_planner* p, int32_t n_queries, const int32_t* ops, const int32_t* n_terms, const int32_t* n_must_not,
                            const int64_t* ids, const uint8_t* bytes, const int64_t* offsets, const float* boosts, rgpu_query* queries_out,
                            rgpu_query_term* terms_out, int64_t terms_cap) {
  if (!p || n_queries <= 0 || !ops || !n_terms || !queries_out || !terms_out || terms_cap < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  std::string why;
  const int rc = p->p->plan(n_queries, ops, n_terms, n_must_not, ids, bytes, offsets, boosts, queries_out, terms_out, terms_cap, &why);
  return rc == RGPU_OK ? RGPU_OK : fail(rc, why);
}

extern "C" int32_t rgpu_plan_batch_ids(rgpu_planner* p, int32_t n_queries, const int32_t* ops, const int32_t* n_terms, const int32_t* n_must_not_or_null,
                                       const int64_t* term_ids, const float* boosts_or_null, rgpu_query* queries_out, rgpu_query_term* terms_out,
                                       int64_t terms_cap) {
  if (!term_ids) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "term_ids is null");
  return plan_checked(p, n_queries, ops, n_terms, n_must_not_or_null, term_ids, nullptr, nullptr, boosts_or_null, queries_out, terms_out, terms_cap);
}

extern "C" int32_t rgpu_plan_batch_bytes(rgpu_planner* p, int32_t n_queries, const int32_t* ops, const int32_t* n_terms, const int32_t* n_must_not_or_null,
                                         const uint8_t* term_bytes, const int64_t* term_offsets, const float* boosts_or_null, rgpu_query* queries_out,
                                         rgpu_query_term* terms_out, int64_t terms_cap) {
  if (!term_offsets) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "term_offsets is null");
  static const uint8_t kEmpty = 0;
  return plan_checked(p, n_queries, ops, n_terms, n_must_not_or_null, nullptr, term_bytes ? term_bytes : &kEmpty, term_offsets, boosts_or_null, queries_out,
                      terms_out, terms_cap);
}

// every query the same shape: `op` (RGPU_OP_TERM / AND / OR, OR optionally RGPU_OP_OR_MSM) over n_clauses terms, boost 1
static int32_t plan_uniform(rgpu_planner* p, int32_t op, int32_t n_queries, int32_t n_clauses, const int64_t* ids, const uint8_t* bytes,
                            const int64_t* offsets, rgpu_query* queries_out, rgpu_query_term* terms_out) {
  if (n_queries <= 0 || n_clauses <= 0 || n_clauses > RGPU_MAX_QUERY_TERMS) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad batch shape");
  if ((op >> 16) != 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a uniform batch has no optional clauses");
  thread_local std::vector<int32_t> ops, counts;
  ops.assign((size_t)n_queries, op);
  counts.assign((size_t)n_queries, n_clauses);
  return plan_checked(p, n_queries, ops.data(), counts.data(), nullptr, ids, bytes, offsets, nullptr, queries_out, terms_out,
                      (int64_t)n_queries * n_clauses);
}
extern "C" int32_t rgpu_plan_uniform_ids(rgpu_planner* p, int32_t op, int32_t n_queries, int32_t n_clauses, const int64_t* term_ids,
                                         rgpu_query* queries_out, rgpu_query_term* terms_out) {
  if (!term_ids) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "term_ids is null");
  return plan_uniform(p, op, n_queries, n_clauses, term_ids, nullptr, nullptr, queries_out, terms_out);
}
extern "C" int32_t rgpu_plan_uniform_bytes(rgpu_planner* p, int32_t op, int32_t n_queries, int32_t n_clauses, const uint8_t* term_bytes,
                                           const int64_t* term_offsets, rgpu_query* queries_out, rgpu_query_term* terms_out) {
  if (!term_offsets) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "term_offsets is null");
  static const uint8_t kEmpty = 0;
  return plan_uniform(p, op, n_queries, n_clauses, nullptr, term_bytes ? term_bytes : &kEmpty, term_offsets, queries_out, terms_out);
}

