// QueryRescorer: the first pass's top window scored again by a second query: TERM / AND / OR, or a phrase. rescore_params_of, launch_rescore_sort.
// Entry points: rgpu_rescore_batch, rgpu_rescore_phrase_batch.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, SCRATCH_TAKE,
// Stager / STAGE_SIZED, seg_view, prepare_terms_locked, make_dev_term), candidates.hpp (phrase_match_setup), phrase_stages.hpp (PhraseMatchStage /
// phrase_match_stage, same_term, check_phrase_query, check_phrase_terms, phrase_is_dead, emit_phrase, phrase_match_verdict).
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- QueryRescorer ------------------------------------------------------------------------------------------------------------
static_assert(sizeof(RescoreParams) == sizeof(rgpu_rescore_request), "RescoreParams mirrors rgpu_rescore_request");
// a row's request, as the kernels read it: the window is cut to the row and to what one pass sorts
static int32_t rescore_params_of(const rgpu_rescore_request& r, int32_t k, RescoreParams* out) {
  if (r.mode < RGPU_RESCORE_AVG || r.mode > RGPU_RESCORE_MULTIPLY || r.window_size < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad rescore request");
  *out = RescoreParams{r.query_weight, r.rescore_weight, r.mode, std::min(std::min(r.window_size, k), RGPU_PASS_K)};
  return RGPU_OK;
}
// `finish`: every row's window back into score order
static void launch_rescore_sort(rgpu_ctx* c, hipStream_t stream, RescoreParams* d_r, int32_t n_queries, int32_t k) {
  TimedLaunch tl(c, stream, "k_rescore_sort", 0);
  RGPU_LAUNCH(k_rescore_sort, dim3(wg_count((n_queries + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, d_r, (int)n_queries, (int)k, c->host_api_hits.p);
}
extern "C" int32_t rgpu_rescore_batch(rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries, const rgpu_query_term* terms,
                                      int32_t n_terms_total, const rgpu_rescore_request* requests, int32_t k, rgpu_hit* hits_inout,
                                      int32_t finish) {
  if (!seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !requests || !hits_inout)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_PASS_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "rescoring: k must be in 1..128");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  std::vector<const rgpu_term_state*> ptrs;
  std::vector<RescoreParams> rp((size_t)n_queries);
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_query& Q = queries[q];
    const int qop = Q.op & 0xff;
    if (qop < RGPU_OP_TERM || qop > RGPU_OP_OR || (Q.op >> 8) > 1 || Q.n_must_not != 0)  // (MUST_NOT or demoting clauses: any bit of the field)
      return fail(RGPU_ERR_UNSUPPORTED, "rescore queries are TERM, all-MUST or all-SHOULD term queries");
    if (Q.n_terms < 1 || Q.n_terms > RGPU_MAX_QUERY_TERMS || (qop == RGPU_OP_TERM && Q.n_terms != 1)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad clause count");
    if (Q.first_term < 0 || (int64_t)Q.first_term + Q.n_terms > (int64_t)n_terms_total) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "clause range outside terms[]");
    RGPU_TRY(rescore_params_of(requests[q], k, &rp[(size_t)q]));
    for (int i = 0; i < Q.n_terms; ++i) {
      const rgpu_query_term& t = terms[Q.first_term + i];
      if (t.sim_table < 0 || t.sim_table >= c->n_sim_tables) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "unknown sim_table handle");
      if (t.state.doc_freq > 0) ptrs.push_back(&t.state);
    }
  }
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size()));
  std::vector<DevQuery> dq((size_t)n_queries);
  std::vector<DevTerm> dt;
  std::vector<DevTerm> mine;
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_query& Q = queries[q];
    const int qop = Q.op & 0xff;
    mine.clear();
    bool dead = false;
    for (int i = 0; i < Q.n_terms; ++i) {
      const rgpu_query_term& t = terms[Q.first_term + i];
      if (t.state.doc_freq <= 0) { if (qop != RGPU_OP_OR) dead = true; continue; }  // create_scorer -> None: the query matches nothing here
      DevTerm d;
      RGPU_TRY(make_dev_term(seg, t.state, t.weight, t.sim_table, &d));
      mine.push_back(d);
    }
    if (dead) mine.clear();
    if (qop == RGPU_OP_AND) std::stable_sort(mine.begin(), mine.end(), [](const DevTerm& a, const DevTerm& b) { return a.df < b.df; });
    dq[(size_t)q] = DevQuery{qop, (int32_t)mine.size(), (int32_t)dt.size(), 0};
    for (auto& m : mine) dt.push_back(m);
  }
  SCRATCH_TAKE(c);
  Stager st(c);
  const auto r_q = st.add<DevQuery>((size_t)n_queries);
  const auto r_t = st.add<DevTerm>(std::max<size_t>(1, dt.size()));
  const auto r_r = st.add<RescoreParams>((size_t)n_queries);
  STAGE_SIZED(sg, st);
  sg.put(r_q, dq);
  sg.put(r_t, dt);
  sg.put(r_r, rp);
  RGPU_TRY(sg.upload(stream));
  const size_t n_hits = (size_t)n_queries * (size_t)k;
  HIP_TRY(c->host_api_hits.reserve(n_hits, 0, stream));
  HIP_TRY(hipMemcpyAsync(c->host_api_hits.p, hits_inout, n_hits * sizeof(HitOut), hipMemcpyHostToDevice, stream));
  const DevQuery* d_q = sg.dev(r_q);
  const DevTerm* d_t = sg.dev(r_t);
  RescoreParams* d_r = sg.dev(r_r);
  {
    TimedLaunch tl(c, stream, "k_rescore", 0);
    const unsigned grid = wg_count((n_hits + WG_WAVES - 1) / WG_WAVES);
    if (seg->version < 1) RGPU_LAUNCH(k_rescore<true>, dim3(grid), dim3(WG_THREADS), 0, stream, seg_view(seg), d_q, d_t, d_r, (int)n_queries, (int)k, c->host_api_hits.p, finish ? 1 : 0);
    else RGPU_LAUNCH(k_rescore<false>, dim3(grid), dim3(WG_THREADS), 0, stream, seg_view(seg), d_q, d_t, d_r, (int)n_queries, (int)k, c->host_api_hits.p, finish ? 1 : 0);
  }
  if (finish) launch_rescore_sort(c, stream, d_r, n_queries, k);
  HIP_TRY(launch_status());
  HIP_TRY(hipMemcpyAsync(hits_inout, c->host_api_hits.p, n_hits * sizeof(HitOut), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RGPU_OK;
}

// QueryRescorer whose second query is a PhraseQuery: the window's hits are the candidate slots of the phrase match stage.
extern "C" int32_t rgpu_rescore_phrase_batch(rgpu_segment* seg, const rgpu_phrase_query* queries, int32_t n_queries,
                                             const rgpu_phrase_term* terms, int32_t n_terms_total, const rgpu_rescore_request* requests,
                                             int32_t k, rgpu_hit* hits_inout, int32_t finish) {
  if (!seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !requests || !hits_inout)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "phrase rescoring: k must be in 1..RGPU_MAX_K");
  if (!seg->has_positions || !seg->d_pos) return fail(RGPU_ERR_ILLEGAL_STATE, "phrase rescoring needs a positions field with its .pos file attached");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  // ---- validate (every refusal comes before hits_inout is touched)
  std::vector<const rgpu_term_state*> ptrs;
  std::vector<RescoreParams> rp((size_t)n_queries);
  for (int32_t q = 0; q < n_queries; ++q) {
    RGPU_TRY(check_phrase_query(c, queries[q], n_terms_total, false));
    RGPU_TRY(rescore_params_of(requests[q], k, &rp[(size_t)q]));
    RGPU_TRY(check_phrase_terms(seg, queries[q], terms, &ptrs));
  }
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_phrase_query& Q = queries[q];
    // SloppyPhraseScorer finds its repetition groups on the first doc it evaluates in the leaf (init_first_time,
    // phrase_scorer.rs:807-820): in a rescoring that is a conjunction match at or behind the first window hit, not a hit.
    // (A row with a term absent from the leaf is served whatever its terms — create_scorer -> None, nothing matches — and
    // emit_phrase fills same_as for live rows only: absent terms all look alike.)
    if (Q.slop > 0 && !phrase_is_dead(Q, terms))
      for (int i = 1; i < Q.n_terms; ++i)
        for (int j = 0; j < i; ++j)
          if (same_term(terms[Q.first_term + j].state, terms[Q.first_term + i].state))
            return fail(RGPU_ERR_UNSUPPORTED, "phrase rescoring: a sloppy phrase that names a term twice is not served");
  }
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size()));
  // ---- plan: row q owns the candidate slots [q * S, q * S + S)
  const int S = (int)rgpu_host::pb_round_up_64(k);
  const int64_t slots = (int64_t)n_queries * S;
  std::vector<DevQuery> dq((size_t)n_queries);
  std::vector<DevTerm> dt;
  std::vector<PosTerm> pt;
  std::vector<int64_t> emit_prefix((size_t)n_queries + 1);
  std::vector<unsigned long long> emit_count((size_t)n_queries);
  std::vector<int32_t> slops((size_t)n_queries, 0);
  bool any_sloppy = false, any_exact = false;
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_phrase_query& Q = queries[q];
    emit_prefix[(size_t)q] = (int64_t)q * S;
    emit_count[(size_t)q] = (unsigned long long)rp[(size_t)q].window;
    dq[(size_t)q] = DevQuery{RGPU_OP_AND, 0, (int32_t)dt.size(), 0};
    bool dead = false;  // (no hit of the row matches in this leaf)
    RGPU_TRY(emit_phrase(seg, Q, terms, &dt, &pt, &dead));  // (same_as != query_ord: exact phrases only here, "a b a")
    if (dead) continue;
    slops[(size_t)q] = Q.slop;
    (Q.slop > 0 ? any_sloppy : any_exact) = true;
    dq[(size_t)q].n_terms = Q.n_terms;
  }
  emit_prefix[(size_t)n_queries] = slots;
  SCRATCH_TAKE(c);
  Stager st(c);
  const auto r_q = st.add<DevQuery>((size_t)n_queries);
  const auto r_t = st.add<DevTerm>(std::max<size_t>(1, dt.size()));
  const auto r_pt = st.add<PosTerm>(std::max<size_t>(1, pt.size()));
  const auto r_ep = st.add<int64_t>((size_t)n_queries + 1);
  const auto r_ec = st.add<unsigned long long>((size_t)n_queries);
  const auto r_sl = st.add<int32_t>((size_t)n_queries);
  const auto r_gr = st.add<SloppyGroups>((size_t)n_queries);
  const auto r_r = st.add<RescoreParams>((size_t)n_queries);
  STAGE_SIZED(sg, st);
  sg.put(r_q, dq);
  sg.put(r_t, dt);
  sg.put(r_pt, pt);
  sg.put(r_ep, emit_prefix);
  sg.put(r_ec, emit_count);
  sg.put(r_sl, slops);
  sg.fill(r_gr, 0xff);  // "no repetition group": k_sloppy_match reads the region
  sg.put(r_r, rp);
  RGPU_TRY(sg.upload(stream));
  const size_t n_hits = (size_t)n_queries * (size_t)k;
  HIP_TRY(c->host_api_hits.reserve(n_hits, 0, stream));
  HIP_TRY(hipMemcpyAsync(c->host_api_hits.p, hits_inout, n_hits * sizeof(HitOut), hipMemcpyHostToDevice, stream));
  int64_t redo_cap = 0;
  // (zero_keys: k_rescore_phrase_combine reads the slots behind a row's window, and a batch of absent-term rows launches no match kernel)
  RGPU_TRY(phrase_match_setup(c, stream, slots, true, &redo_cap));
  HIP_TRY(c->phrase_count.reserve((size_t)n_queries, 0, stream));
  HIP_TRY(hipMemcpyAsync(c->phrase_count.p, sg.dev(r_ec), (size_t)n_queries * 8, hipMemcpyDeviceToDevice, stream));
  const DevQuery* d_q = sg.dev(r_q);
  const DevTerm* d_t = sg.dev(r_t);
  RescoreParams* d_r = sg.dev(r_r);
  const SegView sv = seg_view(seg);
  {
    TimedLaunch tl(c, stream, "k_rescore_phrase_candidates", 0);
    const unsigned grid = wg_count((slots + WG_WAVES - 1) / WG_WAVES);
    if (seg->version < 1) RGPU_LAUNCH(k_rescore_phrase_candidates<true>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, d_q, d_t, d_r, (int)n_queries, (int)k, S, c->host_api_hits.p, c->phrase_docs.p);
    else RGPU_LAUNCH(k_rescore_phrase_candidates<false>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, d_q, d_t, d_r, (int)n_queries, (int)k, S, c->host_api_hits.p, c->phrase_docs.p);
  }
  RGPU_TRY(phrase_match_stage(seg, stream, PhraseMatchStage{d_q, d_t, sg.dev(r_pt), sg.dev(r_ep), sg.dev(r_sl), sg.dev(r_gr), n_queries, slots, redo_cap, any_exact,
                                                            any_sloppy, false, false, nullptr, nullptr, nullptr, 0}));
  {
    TimedLaunch tl(c, stream, "k_rescore_phrase_combine", 0);
    RGPU_LAUNCH(k_rescore_phrase_combine, dim3(wg_count((n_hits + 255) / 256)), dim3(256), 0, stream, sv, d_r, (int)n_queries, (int)k, S, c->phrase_keys.p, c->host_api_hits.p, finish ? 1 : 0);
  }
  if (finish) launch_rescore_sort(c, stream, d_r, n_queries, k);
  HIP_TRY(launch_status());
  // (a refusal here too leaves hits_inout as it came)
  RGPU_TRY(phrase_match_verdict(c, stream, "a hit doc holds one of an exact phrase's terms more than 1024 times (a sloppy phrase's terms: more than 2048 times in all)",
                               "internal: a candidate doc was not found again"));
  HIP_TRY(hipMemcpyAsync(hits_inout, c->host_api_hits.p, n_hits * sizeof(HitOut), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RGPU_OK;
}

