// Cross-field query-string trees: sum groups, MUST + SHOULD. search_fields_tree_locked.
// Entry point: rgpu_search_fields_tree_batch.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, make_dev_term, Stager / Staged, launch_merge), fields.hpp (FieldScope,
// prepare_field_terms_locked), rows.hpp (api_rows_read_back), kernels/search_fields_tree.hpp, kernels/search_and.hpp (SeqRec,
// k_req_opt_scan), host/fields_tree_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.
#include "../kernels/search_fields_tree.hpp"
#include "../host/fields_tree_plan.hpp"

static_assert(sizeof(FieldsTreeGroupDev) == sizeof(rgpu_host::FieldsTreePlanGroup) && sizeof(FieldsTreeQueryDev) == sizeof(rgpu_host::FieldsTreePlanQuery),
              "kernels/search_fields_tree.hpp mirrors host/fields_tree_plan.hpp");
static_assert(FIELDS_TREE_MODE_SINGLE == rgpu_host::FIELDS_TREE_SINGLE && FIELDS_TREE_MODE_ADD == rgpu_host::FIELDS_TREE_ADD &&
              FIELDS_TREE_MODE_RULE == rgpu_host::FIELDS_TREE_RULE && FIELDS_TREE_KIND_SUM == RGPU_GROUP_SUM && FIELDS_TREE_KIND_DISMAX == RGPU_GROUP_DISMAX,
              "kernels/search_fields_tree.hpp follows host/fields_tree_plan.hpp and include/rucene_gpu.h");
static_assert(fields_tree_lds_bytes(FIELDS_TREE_WINDOW_DOCS) <= OR_LDS_MAX / 2 && FIELDS_TREE_WINDOW_DOCS % 256 == 0,
              "two workgroups of k_fields_tree_windows per CU; the scan steps 256 docs");
static_assert(sizeof(SeqRec) == 2 * sizeof(ScoredPosting), "SeqRec records are laid over the run scratch");
// 4 GiB of 16-byte records per pass of rgpu_search_fields_tree_batch. k_req_opt_scan walks a query's records with ONE wavefront, so a
// pass takes as long as its longest query: fewer passes are faster (section 4.6), more records pin more of the context's run buffer
constexpr int64_t FIELDS_TREE_RECORDS_PER_PASS = (int64_t)1 << 28;

// A term belongs to exactly one field: one doc_start_fp (of a term of doc_freq >= 2; singletons live in the dictionary) named under two
// fields, or under another field than the one it was prepared under, is refused over the WHOLE batch before anything is prepared -
// whatever the number of passes the batch is then served in.
static int32_t fields_tree_check_fields(rgpu_segment* seg, const rgpu_host::FieldsTreePlan& P, const rgpu_field_clause* clauses) {
  std::map<int64_t, int32_t> field_of_fp;
  for (int32_t at : P.clause_of) {
    const rgpu_field_clause& cl = clauses[at];
    if (cl.state.doc_freq < 2) continue;
    const auto it = field_of_fp.emplace(cl.state.doc_start_fp, cl.field);
    if (!it.second && it.first->second != cl.field) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "one doc_start_fp is named under two fields of the segment");
    const TermInfo* info = seg->prepared.find(cl.state.doc_start_fp);
    if (info && info->field != (uint8_t)cl.field) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a term's doc_start_fp was prepared under another field of the segment");
  }
  return RGPU_OK;
}

// rgpu_search_fields_tree_batch behind its argument checks (ctx mutex held, device set, the batch validated and checked by
// fields_tree_check_fields).
// THE TWIN of search_fields_locked (fields.hpp): the run de-duplication, the per-field preparation, the k_score_terms launches, the
// staging and the read-back are that function's text (fields.hpp stays the code it is, so nothing could be shared through it). A
// fix to either belongs in both until the stage in front of the window kernel is factored out of the two.
static int32_t search_fields_tree_locked(rgpu_segment* seg, const rgpu_fields_tree_query* queries, int32_t n_queries, const rgpu_field_tree_group* groups,
                                         const rgpu_field_clause* clauses, int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  rgpu_ctx* c = seg->ctx;
  hipStream_t stream = c->stream;
  const int W = FIELDS_TREE_WINDOW_DOCS;
  const rgpu_host::FieldsTreePlan P =
      rgpu_host::plan_fields_tree(queries, n_queries, groups, clauses, seg->max_doc, W, FIELDS_WAVES, c->cfg.req_opt_rule, c->fields_windows_per_item);
  const size_t nt = P.clause_of.size();
  const int n_fields = 1 + (int)seg->fields.size();
  const int64_t n_records = P.rec_prefix.back();
  const size_t n_rule = P.rule_query.size();
  if (n_records > 0x7fffffffll) return fail(RGPU_ERR_UNSUPPORTED, "the lead groups of the batch hold more than 2^31 postings");

  // ---- one run per DISTINCT clause of the batch (search_fields_locked's rule: a prohibited clause is scored with table 0, only its docs are read)
  std::vector<uint8_t> prohibited(nt, 0);
  for (const rgpu_host::FieldsTreePlanQuery& D : P.queries)
    for (int32_t i = 0; i < D.n_not; ++i) prohibited[(size_t)(D.first_not + i)] = 1;
  using RunKey = std::tuple<int32_t, int64_t, int32_t, int32_t, int64_t, uint32_t, int32_t>;
  std::map<RunKey, int32_t> run_of_key;
  std::vector<int32_t> run_of(nt), first_user;
  for (size_t j = 0; j < nt; ++j) {
    const rgpu_field_clause& cl = clauses[P.clause_of[j]];
    uint32_t wbits = 0;
    if (!prohibited[j]) std::memcpy(&wbits, &cl.weight, 4);
    const bool single = cl.state.doc_freq == 1;
    const RunKey key{cl.field, single ? -1 : cl.state.doc_start_fp, cl.state.doc_freq, single ? cl.state.singleton_doc_id : -1,
                     single ? cl.state.total_term_freq : 0, wbits, prohibited[j] ? 0 : cl.sim_table};
    const auto it = run_of_key.emplace(key, (int32_t)first_user.size());
    if (it.second) first_user.push_back((int32_t)j);
    run_of[j] = it.first->second;
  }
  const size_t nr = first_user.size();
  std::vector<std::vector<int32_t>> of_field((size_t)n_fields);
  for (size_t r = 0; r < nr; ++r) of_field[(size_t)clauses[P.clause_of[(size_t)first_user[r]]].field].push_back(first_user[r]);
  RGPU_TRY(enforce_prepared_budget(seg));
  std::vector<const rgpu_term_state*> ptrs;
  for (int f = 0; f < n_fields; ++f) {
    if (of_field[(size_t)f].empty()) continue;
    ptrs.clear();
    for (int32_t j : of_field[(size_t)f]) ptrs.push_back(&clauses[P.clause_of[(size_t)j]].state);
    RGPU_TRY(prepare_field_terms_locked(seg, f, ptrs.data(), ptrs.size()));
  }
  const int blocks_per_item = 32;
  std::vector<DevTerm> terms_sorted;
  std::vector<int64_t> out_sorted, item_prefix_all;
  std::vector<int32_t> run_len(nt);
  std::vector<int64_t> run_start(nr, 0), run_prefix(nt);
  int64_t run_slots64 = 0;
  struct FieldLaunch { int field; size_t first, n, ip_first; int64_t items, postings; };
  std::vector<FieldLaunch> launches;
  terms_sorted.reserve(nr);
  out_sorted.reserve(nr);
  for (int f = 0; f < n_fields; ++f) {
    if (of_field[(size_t)f].empty()) continue;
    FieldScope scope(seg, f);
    FieldLaunch L{f, terms_sorted.size(), of_field[(size_t)f].size(), item_prefix_all.size(), 0, 0};
    for (int32_t j : of_field[(size_t)f]) {
      const rgpu_field_clause& cl = clauses[P.clause_of[(size_t)j]];
      const TermInfo* info = cl.state.doc_freq >= 2 ? seg->prepared.find(cl.state.doc_start_fp) : nullptr;
      if (info && info->field != (uint8_t)f) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a term's doc_start_fp was prepared under another field of the segment");
      DevTerm t;
      const bool scored = !prohibited[(size_t)j];
      RGPU_TRY(make_dev_term(seg, cl.state, scored ? cl.weight : 0.0f, scored ? cl.sim_table : 0, &t, true, info));
      item_prefix_all.push_back(L.items);
      L.items += t.nblocks == 0 ? 1 : (t.nblocks + blocks_per_item - 1) / blocks_per_item;
      L.postings += t.df;
      terms_sorted.push_back(t);
      out_sorted.push_back(run_slots64);
      run_start[(size_t)run_of[(size_t)j]] = run_slots64;
      run_slots64 += rgpu_host::fields_tree_run_slots(t.df);  // (one run per DISTINCT clause: the prefix is this call's, the capacity the plan's)
    }
    item_prefix_all.push_back(L.items);
    launches.push_back(L);
  }
  int64_t postings = 0;
  for (const FieldLaunch& L : launches) postings += L.postings;
  for (size_t j = 0; j < nt; ++j) {
    run_prefix[j] = run_start[(size_t)run_of[j]];
    run_len[j] = clauses[P.clause_of[j]].state.doc_freq;
  }
  std::vector<int64_t> merge_prefix((size_t)n_queries + 1);
  for (int q = 0; q <= n_queries; ++q) merge_prefix[(size_t)q] = (int64_t)q * P.items_per_query;

  SCRATCH_TAKE(c);
  Stager st(c);
  const auto r_q = st.add<rgpu_host::FieldsTreePlanQuery>((size_t)n_queries);
  const auto r_g = st.add<rgpu_host::FieldsTreePlanGroup>(P.groups.size());
  const auto r_t = st.add<DevTerm>(nr);
  const auto r_os = st.add<int64_t>(nr);
  const auto r_ip = st.add<int64_t>(item_prefix_all.size());
  const auto r_rp = st.add<int64_t>(nt);
  const auto r_rl = st.add<int32_t>(nt);
  const auto r_mp = st.add<int64_t>((size_t)n_queries + 1);
  const auto r_sp = st.add<int64_t>(n_rule + 1);
  const auto r_qm = st.add<int32_t>(n_rule);
  STAGE_SIZED(sg, st);
  sg.put(r_q, P.queries);
  sg.put(r_g, P.groups);
  sg.put(r_t, terms_sorted);
  sg.put(r_os, out_sorted);
  sg.put(r_ip, item_prefix_all);
  sg.put(r_rp, run_prefix);
  sg.put(r_rl, run_len);
  sg.put(r_mp, merge_prefix);
  sg.put(r_sp, P.rec_prefix);
  sg.put(r_qm, P.rule_query);
  RGPU_TRY(sg.upload(stream));
  // the scored runs, and behind them (16-byte aligned: a run slot is 8 bytes) the records of the RULE queries
  const size_t run_slots = (size_t)run_slots64;
  const size_t rec_first_slot = (run_slots + 64 + 1) & ~(size_t)1;
  const size_t all_slots = rec_first_slot + 2 * (size_t)n_records;
  DevVec<ScoredPosting>& runs_buf = all_slots <= RUNS_PER_SLOT_MAX ? c->S->d_runs : c->d_runs;
  HIP_TRY(runs_buf.reserve(all_slots, 0, stream));
  SeqRec* records = reinterpret_cast<SeqRec*>(runs_buf.p + rec_first_slot);
  if (n_records > 0) HIP_TRY(hipMemsetAsync(records, 0xff, (size_t)n_records * sizeof(SeqRec), stream));  // doc = -1: no hit in this slot
  HIP_TRY(c->S->d_tau.reserve((size_t)n_queries, 0, stream));
  HIP_TRY(hipMemsetAsync(c->S->d_tau.p, 0, (size_t)n_queries * 8, stream));
  HIP_TRY(c->S->d_partial_keys.reserve((size_t)P.items * (size_t)k, 0, stream));
  HIP_TRY(c->S->d_partial_counts.reserve((size_t)P.items, 0, stream));
  HIP_TRY(c->host_api_hits.reserve((size_t)n_queries * (size_t)k, 0, stream));
  HIP_TRY(c->host_api_totals.reserve((size_t)n_queries, 0, stream));
  const bool legacy = seg->version < 1;
  const bool wide = k > 64;
  for (const FieldLaunch& L : launches) {  // the TermScorer work, once per field the batch names, with that field's view
    if (L.items == 0) continue;
    FieldScope scope(seg, L.field);
    const SegView sv = seg_view(seg);
    const std::string name = "k_score_terms(field " + std::to_string(L.field) + ")";
    TimedLaunch tl(c, stream, name.c_str(), L.postings);
    const unsigned grid = wg_count((L.items + WG_WAVES - 1) / WG_WAVES);
    const DevTerm* dt = sg.dev(r_t) + L.first;
    const int64_t *dip = sg.dev(r_ip) + L.ip_first, *dos = sg.dev(r_os) + L.first;
    if (legacy)
      RGPU_LAUNCH(k_score_terms<true>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, dt, dip, dos, (int)L.n, L.items, blocks_per_item, runs_buf.p);
    else
      RGPU_LAUNCH(k_score_terms<false>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, dt, dip, dos, (int)L.n, L.items, blocks_per_item, runs_buf.p);
  }
  {
    TimedLaunch tl(c, stream, "k_fields_tree_windows", postings);
    const SegView sv = seg_view(seg);  // (field 0's: the window kernel reads max_doc and the live docs, which the fields share)
    const size_t lds = fields_tree_lds_bytes(W);
    const unsigned grid = (unsigned)(P.items / FIELDS_WAVES);  // exact: items_per_query is a multiple of FIELDS_WAVES
    auto go = [&](auto kern) -> hipError_t {
      const hipError_t e = set_dynamic_lds_once(c, reinterpret_cast<const void*>(kern), lds);
      if (e != hipSuccess) return e;
      RGPU_LAUNCH(kern, dim3(grid), dim3(FIELDS_THREADS), lds, stream, sv, reinterpret_cast<const FieldsTreeQueryDev*>(sg.dev(r_q)),
                  reinterpret_cast<const FieldsTreeGroupDev*>(sg.dev(r_g)), sg.dev(r_rl), sg.dev(r_rp), runs_buf.p, (int)n_queries, (int)P.windows_per_query,
                  (int)P.windows_per_item, (int)P.items_per_query, W, (int)k, c->S->d_partial_keys.p, c->S->d_partial_counts.p, c->S->d_tau.p, records,
                  n_records);
      return hipSuccess;
    };
    HIP_TRY(wide ? go(k_fields_tree_windows<true>) : go(k_fields_tree_windows<false>));
  }
  // SINGLE and ADD queries: the per-item lists are folded (a RULE query's items hold none: its row is written empty here and
  // overwritten below). A batch of RULE queries alone skips the merge.
  if (P.n_single_or_add > 0) {
    if (wide) launch_merge<true>(c, stream, n_queries, k, sg.dev(r_mp), seg->doc_base, c->host_api_hits.p, c->host_api_totals.p);
    else launch_merge<false>(c, stream, n_queries, k, sg.dev(r_mp), seg->doc_base, c->host_api_hits.p, c->host_api_totals.p);
  }
  if (n_rule > 0) {  // ReqOptScorer's rule, the count and the collector over each RULE query's records, in doc order
    TimedLaunch tl(c, stream, "k_req_opt_scan", 0);
    const unsigned grid = wg_count(((int64_t)n_rule + WG_WAVES - 1) / WG_WAVES);
    if (wide)
      RGPU_LAUNCH(k_req_opt_scan<true>, dim3(grid), dim3(WG_THREADS), 0, stream, (const SeqRec*)records, sg.dev(r_sp), (int)n_rule, (int)k, seg->doc_base,
                  sg.dev(r_qm), c->host_api_hits.p, c->host_api_totals.p, 0, 0, (const unsigned long long*)nullptr, (unsigned long long*)nullptr);
    else
      RGPU_LAUNCH(k_req_opt_scan<false>, dim3(grid), dim3(WG_THREADS), 0, stream, (const SeqRec*)records, sg.dev(r_sp), (int)n_rule, (int)k, seg->doc_base,
                  sg.dev(r_qm), c->host_api_hits.p, c->host_api_totals.p, 0, 0, (const unsigned long long*)nullptr, (unsigned long long*)nullptr);
  }
  HIP_TRY(launch_status());
  // the rows travel to staging memory of the call's own first: a failing copy leaves the caller's arrays as they were
  std::vector<HitOut> rows((size_t)n_queries * (size_t)k);
  std::vector<int64_t> totals((size_t)n_queries);
  RGPU_TRY(api_rows_read_back(c, stream, n_queries, k, reinterpret_cast<rgpu_hit*>(rows.data()), totals.data()));
  std::memcpy(hits_out, rows.data(), rows.size() * sizeof(HitOut));
  std::memcpy(total_hits_out, totals.data(), totals.size() * 8);
  return RGPU_OK;
}

extern "C" int32_t rgpu_search_fields_tree_batch(rgpu_segment* seg, const rgpu_fields_tree_query* queries, int32_t n_queries,
                                                 const rgpu_field_tree_group* groups, int32_t n_groups_total, const rgpu_field_clause* clauses,
                                                 int32_t n_clauses_total, int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!seg || !hits_out || !total_hits_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t attached = (1u << (1 + seg->fields.size())) - 1u;
  const char* why = "";
  const int32_t rc = rgpu_host::fields_tree_validate(queries, n_queries, groups, n_groups_total, clauses, n_clauses_total, k, attached, c->n_sim_tables, &why);
  if (rc != RGPU_OK) return fail(rc, why);
  for (int32_t i = 0; i < n_clauses_total; ++i)
    if (clauses[i].state.doc_freq == 1 && (clauses[i].state.singleton_doc_id < 0 || clauses[i].state.singleton_doc_id >= seg->max_doc))
      return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "singleton_doc_id out of range");
  RGPU_TRY(settle_pending(c));
  // The records of the RULE queries are bounded by their lead groups' postings - which a batch of a thousand common words can
  // bring to gigabytes: such a batch is served in runs of consecutive queries of at most `per_pass` records each (a
  // query that holds more on its own is a run of one). Rows do not depend on the split: a query's plan is its own.
  const rgpu_host::FieldsTreePlan whole =
      rgpu_host::plan_fields_tree(queries, n_queries, groups, clauses, seg->max_doc, FIELDS_TREE_WINDOW_DOCS, FIELDS_WAVES, c->cfg.req_opt_rule, 0);
  int64_t per_pass = FIELDS_TREE_RECORDS_PER_PASS;  // (RGPU_FIELDS_TREE_RECORDS_PER_PASS in the environment, read per call: tests)
  if (const char* e = std::getenv("RGPU_FIELDS_TREE_RECORDS_PER_PASS")) per_pass = std::max<int64_t>(1, std::atoll(e));
  RGPU_TRY(fields_tree_check_fields(seg, whole, clauses));
  if (whole.rec_prefix.back() <= per_pass)
    return search_fields_tree_locked(seg, queries, n_queries, groups, clauses, k, hits_out, total_hits_out);
  std::vector<int64_t> recs_of((size_t)n_queries, 0);
  for (size_t i = 0; i < whole.rule_query.size(); ++i) recs_of[(size_t)whole.rule_query[i]] = whole.rec_prefix[i + 1] - whole.rec_prefix[i];
  std::vector<rgpu_hit> rows((size_t)n_queries * (size_t)k);  // (a failing pass leaves the caller's arrays as they were)
  std::vector<int64_t> totals((size_t)n_queries);
  for (int32_t q0 = 0; q0 < n_queries;) {
    int32_t q1 = q0 + 1;
    int64_t recs = recs_of[(size_t)q0];
    while (q1 < n_queries && recs + recs_of[(size_t)q1] <= per_pass) recs += recs_of[(size_t)q1++];
    RGPU_TRY(search_fields_tree_locked(seg, queries + q0, q1 - q0, groups, clauses, k, rows.data() + (size_t)q0 * (size_t)k, totals.data() + q0));
    q0 = q1;
  }
  std::memcpy(hits_out, rows.data(), rows.size() * sizeof(rgpu_hit));
  std::memcpy(total_hits_out, totals.data(), totals.size() * 8);
  return RGPU_OK;
}
