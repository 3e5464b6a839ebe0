// Further fields of a segment and the cross-field search. FieldScope, field_norms_upload, prepare_field_terms_locked, search_fields_locked.
// Entry points: rgpu_segment_attach_field, rgpu_segment_prepare_field_terms, rgpu_segment_get_field_info, rgpu_search_fields_batch.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, the prepare path, make_dev_term, Stager / Staged, launch_merge),
// rows.hpp (api_rows_read_back), kernels/search_fields.hpp, host/fields_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

static_assert(sizeof(FieldsGroupDev) == sizeof(rgpu_host::FieldsPlanGroup) && sizeof(FieldsQueryDev) == sizeof(rgpu_host::FieldsPlanQuery),
              "kernels/search_fields.hpp mirrors host/fields_plan.hpp");
static_assert(FIELDS_MAX_CLAUSES == RGPU_MAX_FIELDS_QUERY_CLAUSES && rgpu_host::FIELDS_RUN_PAD == OR_RUN_PAD, "kernels/search_fields.hpp follows include/rucene_gpu.h");
static_assert(fields_lds_bytes(FIELDS_WINDOW_DOCS) <= OR_LDS_MAX / 3 && FIELDS_WINDOW_DOCS % 256 == 0, "three workgroups of k_fields_windows per CU; the scan steps 256 docs");

// The segment describes field `field` for as long as this lives (ctx->mu held): seg_view() and the prepare path then work for that
// field — the "field view". Field 0: nothing to do.
struct FieldScope {
  rgpu_segment* s;
  rgpu_segment::Field saved;
  bool swapped;
  FieldScope(rgpu_segment* seg, int field) : s(seg), swapped(field > 0) {
    if (!swapped) return;
    saved = take();
    put(s->fields[(size_t)field - 1]);
    s->cur_field = field;
  }
  ~FieldScope() {
    if (!swapped) return;
    put(saved);
    s->cur_field = 0;
  }
  FieldScope(const FieldScope&) = delete;
  FieldScope& operator=(const FieldScope&) = delete;

 private:
  rgpu_segment::Field take() const {
    rgpu_segment::Field f;
    f.d_norms = s->d_norms; f.d_rank_to_norm = s->d_rank_to_norm; f.n_norm_ranks = s->n_norm_ranks; f.index_options = s->index_options0;
    f.has_freqs = s->has_freqs; f.has_positions = s->has_positions; f.has_offsets = s->has_offsets; f.has_payloads = s->has_payloads;
    f.skip_vals = s->skip_vals;
    return f;
  }
  void put(const rgpu_segment::Field& f) {
    s->d_norms = f.d_norms; s->d_rank_to_norm = f.d_rank_to_norm; s->n_norm_ranks = f.n_norm_ranks; s->index_options0 = f.index_options;
    s->has_freqs = f.has_freqs; s->has_positions = f.has_positions; s->has_offsets = f.has_offsets; s->has_payloads = f.has_payloads;
    s->skip_vals = f.skip_vals;
  }
};

// A field's norm bytes into HBM by rgpu_segment_upload_field's rule: ranks + rank_to_norm when at most 64 distinct bytes occur
// (and the context does not ask for raw norms), the bytes themselves otherwise. Synchronous.
static int32_t field_norms_upload(rgpu_ctx* c, const uint8_t* norms, int32_t max_doc, rgpu_segment::Field* f) {
  HIP_TRY(hipMalloc(&f->d_norms, (size_t)max_doc + 64));
  size_t hist[256] = {0};
  for (int32_t d = 0; d < max_doc; ++d) hist[norms[d]]++;
  uint8_t rank_of[256] = {0}, rank_to_norm[64] = {0};
  int used = 0;
  for (int b = 0; b < 256; ++b) if (hist[b]) { if (used < 64) { rank_of[b] = (uint8_t)used; rank_to_norm[used] = (uint8_t)b; } ++used; }
  if (used <= 64 && !c->cfg.raw_norms) {
    std::vector<uint8_t> ranks((size_t)max_doc);
    for (int32_t d = 0; d < max_doc; ++d) ranks[(size_t)d] = rank_of[norms[d]];
    HIP_TRY(hipMalloc(&f->d_rank_to_norm, 64));
    HIP_TRY(hipMemcpy(f->d_norms, ranks.data(), (size_t)max_doc, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(f->d_rank_to_norm, rank_to_norm, 64, hipMemcpyHostToDevice));
    f->n_norm_ranks = used;
  } else {
    HIP_TRY(hipMemcpy(f->d_norms, norms, (size_t)max_doc, hipMemcpyHostToDevice));
  }
  return RGPU_OK;
}

extern "C" int32_t rgpu_segment_attach_field(rgpu_segment* seg, const uint8_t* norms, int32_t index_options, int32_t* field_out) {
  if (!seg || !field_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  const int32_t given = index_options;
  const bool payloads = (index_options & RGPU_FIELD_STORES_PAYLOADS) != 0;
  index_options &= ~RGPU_FIELD_STORES_PAYLOADS;
  if (index_options < 1 || index_options > 4)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "index_options must be 1 (Docs), 2 (DocsAndFreqs), 3 (DocsAndFreqsAndPositions) or 4 (...AndOffsets), "
                                           "optionally | RGPU_FIELD_STORES_PAYLOADS");
  if (payloads && index_options < 3) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a field that stores payloads is indexed with positions (index_options >= 3)");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (seg->fields.size() + 1 >= (size_t)RGPU_MAX_FIELDS) return fail(RGPU_ERR_UNSUPPORTED, "a segment holds at most RGPU_MAX_FIELDS fields");
  rgpu_segment::Field f;
  f.index_options = given;
  f.has_freqs = index_options >= 2;
  f.has_positions = index_options >= 3;
  f.has_offsets = index_options >= 4;
  f.has_payloads = payloads;
  f.skip_vals = !f.has_positions ? 2 : payloads ? 6 : f.has_offsets ? 5 : 4;  // skip_writer.rs:261-289
  if (norms && seg->max_doc > 0) {
    const int32_t rc = field_norms_upload(c, norms, seg->max_doc, &f);
    if (rc != RGPU_OK) {
      if (f.d_norms) (void)hipFree(f.d_norms);
      if (f.d_rank_to_norm) (void)hipFree(f.d_rank_to_norm);
      return rc;
    }
  }
  seg->fields.push_back(f);
  seg->any_positions = seg->any_positions || f.has_positions;
  *field_out = (int32_t)seg->fields.size();
  return RGPU_OK;
}

extern "C" int32_t rgpu_segment_get_field_info(rgpu_segment* seg, int32_t field, rgpu_segment_field_info* out) {
  if (!seg || !out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> g(seg->ctx->mu);
  if (field < 0 || (size_t)field > seg->fields.size()) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a field slot that is not attached");
  std::memset(out, 0, sizeof *out);
  // (read where the values are kept: the segment's own members for field 0, the slot's record otherwise - nothing is swapped)
  const uint8_t* norms = field == 0 ? seg->d_norms : seg->fields[(size_t)field - 1].d_norms;
  const int32_t ranks = field == 0 ? seg->n_norm_ranks : seg->fields[(size_t)field - 1].n_norm_ranks;
  out->norms_bytes = norms ? (int64_t)seg->max_doc : 0;
  out->norm_mode = !norms ? 0 : ranks > 0 ? 1 : 2;
  out->n_norm_ranks = ranks;
  out->index_options = field == 0 ? seg->index_options0 : seg->fields[(size_t)field - 1].index_options;
  out->skip_values = field == 0 ? seg->skip_vals : seg->fields[(size_t)field - 1].skip_vals;
  return RGPU_OK;
}

// Stages A and B for `sts` as terms of `field`, without the budget check (prepare_terms_locked's, which drops the WHOLE store: a call
// that prepares under several fields asks it once, before the first of them)
static int32_t prepare_field_terms_locked(rgpu_segment* seg, int field, const rgpu_term_state* const* sts, size_t n) {
  FieldScope scope(seg, field);
  int32_t rc = prepare_terms_attempt(seg, sts, n, false, nullptr);
  if (rc == -101) rc = prepare_terms_attempt(seg, sts, n, true, nullptr);
  if (rc == -101) rc = fail(RGPU_ERR_CORRUPT_INDEX, "corrupt block framing in .doc (prepare.hpp check #12)");
  if (rc == RGPU_OK) rc = prepare_norms_locked(seg, sts, n);
  return rc;
}

extern "C" int32_t rgpu_segment_prepare_field_terms(rgpu_segment* seg, int32_t field, const rgpu_term_state* terms, int64_t n_terms) {
  if (!seg || (!terms && n_terms > 0) || n_terms < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  std::lock_guard<std::mutex> g(seg->ctx->mu);
  HIP_TRY(hipSetDevice(seg->ctx->device));
  if (field < 0 || (size_t)field > seg->fields.size()) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a field slot that is not attached");
  std::vector<const rgpu_term_state*> ptrs((size_t)n_terms);
  for (int64_t i = 0; i < n_terms; ++i) ptrs[(size_t)i] = &terms[i];
  RGPU_TRY(enforce_prepared_budget(seg));
  return prepare_field_terms_locked(seg, field, ptrs.data(), ptrs.size());
}

// rgpu_search_fields_batch behind its argument checks (ctx mutex held, device set, the batch validated)
static int32_t search_fields_locked(rgpu_segment* seg, const rgpu_fields_query* queries, int32_t n_queries, const rgpu_field_group* groups,
                                    const rgpu_field_clause* clauses, int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  rgpu_ctx* c = seg->ctx;
  hipStream_t stream = c->stream;
  const int W = FIELDS_WINDOW_DOCS;
  const rgpu_host::FieldsPlan P = rgpu_host::plan_fields(queries, n_queries, groups, clauses, seg->max_doc, W, FIELDS_WAVES, c->fields_windows_per_item);
  const size_t nt = P.clause_of.size();
  const int n_fields = 1 + (int)seg->fields.size();

  // ---- one run per DISTINCT clause of the batch: a thousand multi-field queries name the same few (field, term, weight) over and
  // over, and a run is the same whoever reads it. A prohibited clause's weight and sim_table are unused by contract: its run is
  // scored with table 0 (one exists: the batch has a scored clause and passed fields_validate) and only its docs are read.
  std::vector<uint8_t> prohibited(nt, 0);
  for (const rgpu_host::FieldsPlanQuery& D : P.queries)
    for (int32_t i = 0; i < D.n_not; ++i) prohibited[(size_t)(D.first_not + i)] = 1;
  // field, doc_start_fp (a singleton has none of its own), doc_freq, singleton doc and freq, weight bits, table
  using RunKey = std::tuple<int32_t, int64_t, int32_t, int32_t, int64_t, uint32_t, int32_t>;
  std::map<RunKey, int32_t> run_of_key;
  std::vector<int32_t> run_of(nt), first_user;  // flat clause -> its run; run -> the first flat clause that names it
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
  // A term belongs to exactly one field. A batch that names one doc_start_fp under two fields, or under another field than the one
  // it was prepared under, is refused HERE, before anything is prepared: filed under the first field's slot, the term would make every
  // later, correct call fail until the store is dropped.
  {
    std::map<int64_t, int32_t> field_of_fp;
    for (size_t r = 0; r < nr; ++r) {
      const rgpu_field_clause& cl = clauses[P.clause_of[(size_t)first_user[r]]];
      if (cl.state.doc_freq < 2) continue;  // (singletons live in the dictionary: nothing of theirs is filed)
      const auto it = field_of_fp.emplace(cl.state.doc_start_fp, cl.field);
      if (!it.second && it.first->second != cl.field) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "one doc_start_fp is named under two fields of the segment");
      const TermInfo* info = seg->prepared.find(cl.state.doc_start_fp);
      if (info && info->field != (uint8_t)cl.field) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a term's doc_start_fp was prepared under another field of the segment");
    }
  }
  // ---- the runs by field: preparation under each field's view, then the descriptors (the store may move while it grows)
  std::vector<std::vector<int32_t>> of_field((size_t)n_fields);  // runs (by their first flat clause), per field
  for (size_t r = 0; r < nr; ++r) of_field[(size_t)clauses[P.clause_of[(size_t)first_user[r]]].field].push_back(first_user[r]);
  RGPU_TRY(enforce_prepared_budget(seg));
  std::vector<const rgpu_term_state*> ptrs;
  for (int f = 0; f < n_fields; ++f) {
    if (of_field[(size_t)f].empty()) continue;
    ptrs.clear();
    for (int32_t j : of_field[(size_t)f]) ptrs.push_back(&clauses[P.clause_of[(size_t)j]].state);
    RGPU_TRY(prepare_field_terms_locked(seg, f, ptrs.data(), ptrs.size()));
  }
  // k_score_terms' plan per field: its clauses' descriptors, their items (clause, chunk of blocks) and where each one's run starts
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
      run_slots64 += (int64_t)t.df + OR_RUN_PAD;
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
  const auto r_q = st.add<rgpu_host::FieldsPlanQuery>((size_t)n_queries);
  const auto r_g = st.add<rgpu_host::FieldsPlanGroup>(P.groups.size());
  const auto r_t = st.add<DevTerm>(nr);
  const auto r_os = st.add<int64_t>(nr);
  const auto r_ip = st.add<int64_t>(item_prefix_all.size());
  const auto r_rp = st.add<int64_t>(nt);
  const auto r_rl = st.add<int32_t>(nt);
  const auto r_mp = st.add<int64_t>((size_t)n_queries + 1);
  STAGE_SIZED(sg, st);
  sg.put(r_q, P.queries);
  sg.put(r_g, P.groups);
  sg.put(r_t, terms_sorted);
  sg.put(r_os, out_sorted);
  sg.put(r_ip, item_prefix_all);
  sg.put(r_rp, run_prefix);
  sg.put(r_rl, run_len);
  sg.put(r_mp, merge_prefix);
  RGPU_TRY(sg.upload(stream));
  // the scored runs: the slot's own buffer, or - runs that would pin gigabytes in every slot - the context's (search_or_group's rule;
  // this call ends synchronised either way)
  const size_t run_slots = (size_t)run_slots64;
  DevVec<ScoredPosting>& runs_buf = run_slots + 64 <= RUNS_PER_SLOT_MAX ? c->S->d_runs : c->d_runs;
  HIP_TRY(runs_buf.reserve(run_slots + 64, 0, stream));
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
    TimedLaunch tl(c, stream, "k_fields_windows", postings);
    const SegView sv = seg_view(seg);  // (field 0's: the window kernel reads max_doc and the live docs, which the fields share)
    const size_t lds = fields_lds_bytes(W);
    const unsigned grid = (unsigned)(P.items / FIELDS_WAVES);  // exact: items_per_query is a multiple of FIELDS_WAVES
    auto go = [&](auto kern) -> hipError_t {
      const hipError_t e = set_dynamic_lds_once(c, reinterpret_cast<const void*>(kern), lds);
      if (e != hipSuccess) return e;
      RGPU_LAUNCH(kern, dim3(grid), dim3(FIELDS_THREADS), lds, stream, sv, reinterpret_cast<const FieldsQueryDev*>(sg.dev(r_q)),
                  reinterpret_cast<const FieldsGroupDev*>(sg.dev(r_g)), sg.dev(r_rl), sg.dev(r_rp), runs_buf.p, (int)n_queries, (int)P.windows_per_query,
                  (int)P.windows_per_item, (int)P.items_per_query, W, (int)k, c->S->d_partial_keys.p, c->S->d_partial_counts.p, c->S->d_tau.p);
      return hipSuccess;
    };
    HIP_TRY(wide ? go(k_fields_windows<true>) : go(k_fields_windows<false>));
  }
  if (wide) launch_merge<true>(c, stream, n_queries, k, sg.dev(r_mp), seg->doc_base, c->host_api_hits.p, c->host_api_totals.p);
  else launch_merge<false>(c, stream, n_queries, k, sg.dev(r_mp), seg->doc_base, c->host_api_hits.p, c->host_api_totals.p);
  HIP_TRY(launch_status());
  // the rows travel to staging memory of the call's own first: a failing copy leaves the caller's arrays as they were
  std::vector<HitOut> rows((size_t)n_queries * (size_t)k);
  std::vector<int64_t> totals((size_t)n_queries);
  RGPU_TRY(api_rows_read_back(c, stream, n_queries, k, reinterpret_cast<rgpu_hit*>(rows.data()), totals.data()));
  std::memcpy(hits_out, rows.data(), rows.size() * sizeof(HitOut));
  std::memcpy(total_hits_out, totals.data(), totals.size() * 8);
  return RGPU_OK;
}

extern "C" int32_t rgpu_search_fields_batch(rgpu_segment* seg, const rgpu_fields_query* queries, int32_t n_queries, const rgpu_field_group* groups,
                                            int32_t n_groups_total, const rgpu_field_clause* clauses, int32_t n_clauses_total, int32_t k,
                                            rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!seg || !hits_out || !total_hits_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t attached = (1u << (1 + seg->fields.size())) - 1u;
  const char* why = "";
  const int32_t rc = rgpu_host::fields_validate(queries, n_queries, groups, n_groups_total, clauses, n_clauses_total, k, attached, c->n_sim_tables, &why);
  if (rc != RGPU_OK) return fail(rc, why);
  for (int32_t i = 0; i < n_clauses_total; ++i)  // (of every clause, named by a query or not: like rgpu_search_batch's term array)
    if (clauses[i].state.doc_freq == 1 && (clauses[i].state.singleton_doc_id < 0 || clauses[i].state.singleton_doc_id >= seg->max_doc))
      return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "singleton_doc_id out of range");
  RGPU_TRY(settle_pending(c));
  return search_fields_locked(seg, queries, n_queries, groups, clauses, k, hits_out, total_hits_out);
}
