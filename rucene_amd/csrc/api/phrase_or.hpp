// BooleanQuery of SHOULD / MUST_NOT clauses with exact PhraseQuery clauses among the SHOULD ones: "a b" "c d" e -f.
// search_phrase_or_batch_impl. Entry points: rgpu_search_phrase_or_batch, rgpu_search_phrase_or_batch_masked.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, SCRATCH_TAKE,
// Stager / STAGE_SIZED, prepare_terms_locked, make_dev_term, ensure_and_bitmaps_locked, clause_bitmap_table, and_item_blocks, Group, OrPhraseRuns,
// search_or_group), rows.hpp (RowColumns, api_rows_default, api_rows_read_back), candidates.hpp (lead_items, lead_slots, AndEmitStage,
// and_emit_stage), docsets.hpp (rgpu_docset, docset_check), masked.hpp (PhraseMask, masked_stage_name), phrase_stages.hpp (PhraseMatchStage /
// phrase_match_stage, emit_phrase, phrase_match_verdict), phrase_search.hpp (PhraseClauseArrays, check_phrases_query),
// kernels/search_phrase_or.hpp, host/phrase_or_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- BooleanQuery of SHOULD / MUST_NOT clauses with exact PhraseQuery clauses among the SHOULD ones: "a b" "c d" e -f -------------
// (include/rucene_gpu.h rgpu_search_phrase_or_batch; the plan: host/phrase_or_plan.hpp; the run-building kernels:
// kernels/search_phrase_or.hpp.) Launch sequence, all on the call's stream:
//   1. and_emit_stage (with phrase_match_setup among its memsets in front of the launch: keys zeroed, the redo list sized, d_err
//      zeroed): k_search_and in emit mode, one "virtual query" per (query, phrase that exists in the leaf) -> that phrase's
//      candidate docs (the conjunction of its terms, as rgpu_search_phrase_batch finds them);
//   2. phrase_match_stage over the virtual queries — exact kernels only: one make_key(BM25(phrase freq, norm), doc) or 0 per slot.
//      Once per call; its verdict (phrase_match_verdict: a doc that holds a phrase term more than 1024 times ...) is looked at
//      before anything else runs;
//   3. api_rows_default, then search_or_group over a Group of op OR: clauses in query order, a pseudo DevTerm (df = capacity) at every phrase position,
//      MUST_NOT terms behind them (DevQuery::pad), min_should_match in op bits 8... Its hook fills the phrase clauses' runs between
//      k_score_terms and k_or_windows: k_phrase_run_fill, _count, _scan, _scatter, _sort;
//   4. k > RGPU_PASS_K: step 3 once per pass of 128 hits, as search_impl runs its passes (rgpu_ctx::Pass, ceiling slots). The keys of
//      step 2 stay in c->phrase_keys; what the run-building kernels read besides lives in buffers of the context's, not in the scratch
//      slot that staged steps 1-2 (four passes later that slot is somebody else's).
static int32_t search_phrase_or_batch_impl(rgpu_segment* seg, rgpu_docset* set, const rgpu_phrase_or_query* queries, int32_t n_queries,
                                           const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                           const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                           const rgpu_query_term* terms, int32_t n_terms_total,
                                           int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!seg || !queries || n_queries <= 0 || !phrases || n_phrases_total <= 0 || !phrase_terms || n_phrase_terms_total <= 0 || n_terms_total < 0 ||
      (n_terms_total > 0 && !terms) || !hits_out || !total_hits_out)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (set) RGPU_TRY(docset_check(seg, set));
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "disjunction over phrases: k must be in 1..RGPU_MAX_K");
  if (!seg->has_positions || !seg->d_pos) return fail(RGPU_ERR_ILLEGAL_STATE, "a disjunction over phrases needs a positions field with its .pos file attached");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  // ---- validate, plan
  const size_t nq = (size_t)n_queries;
  std::vector<const rgpu_term_state*> ptrs;
  std::vector<rgpu_host::PhraseOrPlan> plans(nq);
  std::vector<int32_t> first_virtual(nq + 1, 0);  // virtual query (query q, phrase j) = first_virtual[q] + j
  const PhraseClauseArrays arrays{phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total};
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_phrase_or_query& Q = queries[q];
    RGPU_TRY(check_phrases_query(seg, Q, "a disjunction over phrases", arrays, &ptrs));
    plans[(size_t)q] = rgpu_host::plan_phrase_or(Q, phrases, phrase_terms, terms);
    if (plans[(size_t)q].status != RGPU_OK) return fail(plans[(size_t)q].status, plans[(size_t)q].why);
    first_virtual[(size_t)q + 1] = first_virtual[(size_t)q] + Q.n_phrases;
  }
  PhraseMask masked;  // (installed for the whole call: every pass of k > RGPU_PASS_K runs under it)
  RGPU_TRY(masked.install(seg, set));
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size()));
  // the candidate conjunctions answer a dense clause from its doc bitmap, as a phrase search's do
  int64_t bitmap_df = INT64_MAX;
  {
    std::vector<const rgpu_term_state*> clauses;
    std::vector<int32_t> clause_sim;
    clauses.reserve(ptrs.size());  // (every clause of a conjunction is a live term: ptrs holds them all)
    clause_sim.reserve(ptrs.size());
    for (int32_t q = 0; q < n_queries; ++q) {
      const rgpu_host::PhraseOrPlan& P = plans[(size_t)q];
      if (P.dead) continue;
      for (int j = 0; j < queries[q].n_phrases; ++j) {
        if (P.capacity[(size_t)j] <= 0) continue;
        const rgpu_phrase_query& ph = phrases[queries[q].first_phrase + j];
        for (int i = 0; i < ph.n_terms; ++i) { clauses.push_back(&phrase_terms[ph.first_term + i].state); clause_sim.push_back(ph.sim_table); }
      }
    }
    RGPU_TRY(ensure_and_bitmaps_locked(seg, clauses, clause_sim, &bitmap_df));
  }
  // ---- the match stage's arrays (one virtual query per phrase) and the disjunction's Group
  const size_t nv = (size_t)first_virtual[nq];
  std::vector<DevQuery> vq(nv, DevQuery{RGPU_OP_AND, 0, 0, 0});
  std::vector<DevTerm> pdt;
  std::vector<PosTerm> ppt;
  std::vector<int64_t> item_prefix(nv + 1), emit_prefix(nv + 1);
  std::vector<PhraseRunDev> prd(nv, PhraseRunDev{0, 0});
  int64_t lead_blocks = 0;
  for (const rgpu_host::PhraseOrPlan& P : plans) if (!P.dead) for (int32_t cap : P.capacity) lead_blocks += cap / 128;
  const int blocks_per_item = and_item_blocks(c, lead_blocks);
  Group G0;
  G0.op = RGPU_OP_OR;
  OrPhraseRuns hook;
  int64_t items = 0, slots = 0;
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_phrase_or_query& Q = queries[q];
    const rgpu_host::PhraseOrPlan& P = plans[(size_t)q];
    for (int j = 0; j < Q.n_phrases; ++j) {
      const size_t v = (size_t)first_virtual[(size_t)q] + (size_t)j;
      item_prefix[v] = items;
      emit_prefix[v] = slots;
      vq[v].first_term = (int32_t)pdt.size();
      if (P.dead || P.capacity[(size_t)j] <= 0) continue;
      const rgpu_phrase_query& ph = phrases[Q.first_phrase + j];
      bool dead = false;
      RGPU_TRY(emit_phrase(seg, ph, phrase_terms, &pdt, &ppt, &dead));  // (dead: the plan has said so already)
      if (dead) continue;
      vq[v].n_terms = ph.n_terms;
      const DevTerm& lead = pdt[(size_t)vq[v].first_term];
      if (lead.df != P.capacity[(size_t)j]) return fail(RGPU_ERR_ILLEGAL_STATE, "internal: a phrase's lead term is not its rarest");
      items += lead_items(lead, blocks_per_item);
      slots += lead_slots(lead);
    }
    // DisjunctionSumScorer's children in query order, pseudo terms at the phrase positions; the MUST_NOT terms behind them
    DevQuery dq{RGPU_OP_OR | (P.min_should_match > 1 ? P.min_should_match << 8 : 0), 0, (int32_t)G0.terms.size(), 0};
    if (!P.dead) {
      for (int32_t o : P.order) {
        DevTerm t;
        if (o >= 0) {
          const rgpu_query_term& qt = terms[Q.first_term + o];
          RGPU_TRY(make_dev_term(seg, qt.state, qt.weight, qt.sim_table, &t));
        } else {
          std::memset(&t, 0, sizeof t);
          t.df = P.capacity[(size_t)~o];
          t.singleton_doc = -1;
          t.sim_table = phrases[Q.first_phrase + ~o].sim_table;  // (never read: the clause has no k_score_terms item and is never dense)
          prd[(size_t)first_virtual[(size_t)q] + (size_t)~o] = PhraseRunDev{(int32_t)G0.terms.size(), t.df};
        }
        G0.terms.push_back(t);
        hook.pseudo.push_back(o < 0 ? 1 : 0);
        G0.postings += t.df;
      }
      for (const rgpu_term_state* st : P.must_not) {
        DevTerm t;
        RGPU_TRY(make_dev_term(seg, *st, 0.0f, 0, &t));  // needs_scores = false: weight and table are never read
        G0.terms.push_back(t);
        hook.pseudo.push_back(0);
        G0.postings += t.df;
      }
      dq.n_terms = (int32_t)P.order.size();
      dq.pad = (int32_t)P.must_not.size();
    }
    G0.queries.push_back(dq);
    G0.qmap.push_back(q);
  }
  item_prefix[nv] = items;
  emit_prefix[nv] = slots;
  const int n_buckets = (int)(((int64_t)seg->max_doc + PHRASE_OR_BUCKET - 1) / PHRASE_OR_BUCKET);
  const size_t n_cells = nv * (size_t)std::max(1, n_buckets);
  if (items > 0) {
    // ---- 1. + 2.: candidates and keys, once per call
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_vq = st.add<DevQuery>(nv);
    const auto r_pdt = st.add<DevTerm>(pdt.size());
    const auto r_ppt = st.add<PosTerm>(ppt.size());
    const auto r_ip = st.add<int64_t>(nv + 1), r_ep = st.add<int64_t>(nv + 1);
    const auto r_sl = st.add<int32_t>(nv);  // slop 0 throughout
    const auto r_gr = st.add<SloppyGroups>(nv);
    const std::vector<TermBitmap> clause_bitmaps = clause_bitmap_table(seg, vq, pdt, bitmap_df);
    const auto r_bm = st.add_if<TermBitmap>(!clause_bitmaps.empty(), clause_bitmaps.size());
    STAGE_SIZED(sg, st);
    sg.put(r_vq, vq);
    sg.put(r_pdt, pdt);
    sg.put(r_ppt, ppt);
    sg.put(r_ip, item_prefix);
    sg.put(r_ep, emit_prefix);
    sg.fill(r_sl, 0);
    sg.fill(r_gr, 0xff);
    sg.put(r_bm, clause_bitmaps);
    RGPU_TRY(sg.upload(stream));
    int64_t redo_cap = 0;
    // (one conjunction per virtual query; the MUST_NOT clauses belong to the disjunction, step 3; nothing is collected here)
    const char* stage_name = masked.on() ? masked_stage_name(c, "k_search_and(masked phrase-or candidates)", "k_search_and(masked phrase-or, marked)")
                                         : "k_search_and(phrase-or candidates)";
    RGPU_TRY(and_emit_stage(seg, stream, AndEmitStage{stage_name, sg.dev(r_vq), sg.dev(r_pdt), sg.dev(r_ip), sg.dev(r_ep),
                                                      clause_bitmaps.empty() ? nullptr : sg.dev(r_bm), (int32_t)nv, nv, items, slots, blocks_per_item,
                                                      std::min<int>(k, 64), false, 0, 0, &redo_cap, true, masked.on() && c->phrase_mask_compact}));
    RGPU_TRY(phrase_match_stage(seg, stream, PhraseMatchStage{sg.dev(r_vq), sg.dev(r_pdt), sg.dev(r_ppt), sg.dev(r_ep), sg.dev(r_sl), sg.dev(r_gr), (int32_t)nv, slots,
                                                              redo_cap, true, false, false, false, nullptr, nullptr, nullptr, 0}));
    HIP_TRY(launch_status());
    // a refused call writes nothing: the match stage's verdict before the disjunction runs (the sync also frees the slot's stage)
    RGPU_TRY(phrase_match_verdict(c, stream, "a doc holds one of an exact phrase's terms more than 1024 times", "internal: a conjunction match was not found again"));
    // what the run-building kernels read in every pass
    HIP_TRY(c->phrase_or_prefix.reserve(nv + 1, 0, stream));
    HIP_TRY(c->phrase_or_runs.reserve(nv, 0, stream));
    HIP_TRY(c->phrase_or_buckets.reserve(2 * n_cells, 0, stream));
    HIP_TRY(hipMemcpyAsync(c->phrase_or_prefix.p, emit_prefix.data(), (nv + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c->phrase_or_runs.p, prd.data(), nv * sizeof(PhraseRunDev), hipMemcpyHostToDevice, stream));
  }
  // ---- 3.: the hook of search_or_group — the phrase clauses' runs (bounds: kernels/search_phrase_or.hpp)
  hook.fill = [&](const int64_t* d_run_prefix, ScoredPosting* runs) -> int32_t {
    if (items <= 0 || n_buckets <= 0) return RGPU_OK;  // (no phrase exists in this leaf: the group holds no pseudo term)
    const PhraseRunDev* d_pr = c->phrase_or_runs.p;
    uint32_t* counts = c->phrase_or_buckets.p;
    uint32_t* offsets = counts + n_cells;
    const int groups_per_clause = (n_buckets + 63) / 64;  // k_phrase_run_sort: one wavefront per (clause, 64 buckets)
    const int64_t groups = slots / 64, sort_items = (int64_t)nv * groups_per_clause;
    const unsigned ggrid = wg_count((groups + WG_WAVES - 1) / WG_WAVES);
    HIP_TRY(hipMemsetAsync(counts, 0, n_cells * sizeof(uint32_t), stream));
    {
      TimedLaunch tl(c, stream, "k_phrase_run_fill", 0);
      RGPU_LAUNCH(k_phrase_run_fill, dim3((unsigned)nv, PHRASE_OR_FILL_SPLIT), dim3(WG_THREADS), 0, stream, d_pr, d_run_prefix, runs);
    }
    {
      TimedLaunch tl(c, stream, "k_phrase_run_count", 0);
      RGPU_LAUNCH(k_phrase_run_place<false>, dim3(ggrid), dim3(WG_THREADS), 0, stream, d_pr, (const int64_t*)c->phrase_or_prefix.p,
                  (const unsigned long long*)c->phrase_count.p, (const uint64_t*)c->phrase_keys.p, (int)nv, groups, seg->max_doc, n_buckets, counts,
                  (const uint32_t*)offsets, d_run_prefix, runs);
    }
    {
      TimedLaunch tl(c, stream, "k_phrase_run_scan", 0);
      RGPU_LAUNCH(k_phrase_run_scan, dim3(wg_count((nv + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, (int)nv, n_buckets, counts, offsets);
    }
    {
      TimedLaunch tl(c, stream, "k_phrase_run_scatter", 0);
      RGPU_LAUNCH(k_phrase_run_place<true>, dim3(ggrid), dim3(WG_THREADS), 0, stream, d_pr, (const int64_t*)c->phrase_or_prefix.p,
                  (const unsigned long long*)c->phrase_count.p, (const uint64_t*)c->phrase_keys.p, (int)nv, groups, seg->max_doc, n_buckets, counts,
                  (const uint32_t*)offsets, d_run_prefix, runs);
    }
    {
      TimedLaunch tl(c, stream, "k_phrase_run_sort", 0);
      RGPU_LAUNCH(k_phrase_run_sort, dim3(wg_count((sort_items + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, d_pr, sort_items, n_buckets,
                  groups_per_clause, (const uint32_t*)counts, (const uint32_t*)offsets, d_run_prefix, runs);
    }
    return RGPU_OK;
  };
  // one pass: defaults for every row (a leaf that holds no clause of any query merges nothing), then the group
  auto one_pass = [&](int32_t k_pass) -> int32_t {
    const RowColumns cols{k_pass, c->pass.stride > 0 ? c->pass.stride : k_pass, c->pass.col0};
    RGPU_TRY(api_rows_default(c, stream, n_queries, k, &cols));
    if (c->pass.ceil_out) HIP_TRY(hipMemsetAsync(c->pass.ceil_out, 0, nq * 8, stream));
    Group G = G0;  // (search_or_group marks dense clauses in the group it is given)
    return search_or_group(seg, G, k_pass, c->host_api_hits.p, c->host_api_totals.p, stream, &hook);
  };
  c->pass = rgpu_ctx::Pass{};
  int32_t rc = RGPU_OK;
  if (k <= RGPU_PASS_K) {
    rc = one_pass(k);
  } else {  // search_impl's passes: pass p collects the best hits strictly below the worst hit of pass p - 1
    rgpu_ctx::CeilSlot& cs = c->ceil_slots[c->ceil_next];
    c->ceil_next = (c->ceil_next + 1) % N_SCRATCH;
    if (cs.busy) { HIP_TRY(hipEventSynchronize(cs.done)); cs.busy = false; }
    HIP_TRY(cs.d.reserve(nq * 2, 0, stream));
    int flip = 0;
    for (int32_t col0 = 0; col0 < k && rc == RGPU_OK; col0 += RGPU_PASS_K, flip ^= 1) {
      c->pass.stride = k;
      c->pass.col0 = col0;
      c->pass.ceil_in = col0 == 0 ? nullptr : cs.d.p + (size_t)(flip ^ 1) * nq;
      c->pass.ceil_out = cs.d.p + (size_t)flip * nq;
      rc = one_pass(std::min<int32_t>(RGPU_PASS_K, k - col0));
    }
    c->pass = rgpu_ctx::Pass{};
  }
  if (rc != RGPU_OK) { (void)hipStreamSynchronize(stream); return rc; }
  HIP_TRY(launch_status());
  return api_rows_read_back(c, stream, n_queries, k, hits_out, total_hits_out);
}
extern "C" int32_t rgpu_search_phrase_or_batch(rgpu_segment* seg, const rgpu_phrase_or_query* queries, int32_t n_queries,
                                               const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                               const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                               const rgpu_query_term* terms, int32_t n_terms_total,
                                               int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  return search_phrase_or_batch_impl(seg, nullptr, queries, n_queries, phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total, k,
                                     hits_out, total_hits_out);
}
extern "C" int32_t rgpu_search_phrase_or_batch_masked(rgpu_segment* seg, rgpu_docset* set, const rgpu_phrase_or_query* queries, int32_t n_queries,
                                                      const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                                      const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                                      const rgpu_query_term* terms, int32_t n_terms_total,
                                                      int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!set) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  return search_phrase_or_batch_impl(seg, set, queries, n_queries, phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total, k,
                                     hits_out, total_hits_out);
}

