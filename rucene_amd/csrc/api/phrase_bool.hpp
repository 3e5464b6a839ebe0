// BooleanQuery with exact PhraseQuery clauses among its required clauses: +"a b" +c -d #e. search_phrase_bool_batch_impl. Entry points:
// rgpu_search_phrase_bool_batch, rgpu_search_phrase_bool_batch_masked.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, SCRATCH_TAKE,
// Stager / STAGE_SIZED, seg_view, prepare_terms_locked, make_dev_term, ensure_and_bitmaps_locked, clause_bitmap_table, and_item_blocks), rows.hpp
// (api_rows_default, api_rows_read_back), candidates.hpp (lead_items, lead_collect_chunks, AndEmitStage, and_emit_stage), docsets.hpp
// (rgpu_docset, docset_check), masked.hpp (PhraseMask, masked_stage_name), phrase_stages.hpp (PhraseMatchStage / phrase_match_stage,
// emit_phrase, phrase_match_verdict, phrase_collect_chunked, PhraseCollectStage / phrase_collect_stage), phrase_search.hpp (PhraseClauseArrays,
// check_phrases_query), kernels/search_phrase_bool.hpp, host/phrase_bool_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- BooleanQuery with exact PhraseQuery clauses among its required clauses: +"a b" +c -d #e ------------------------------------
// (include/rucene_gpu.h rgpu_search_phrase_bool_batch; the plan: host/phrase_bool_plan.hpp; the two kernels of its own:
// kernels/search_phrase_bool.hpp.) Launch sequence, all on the call's stream:
//   1. and_emit_stage (with phrase_match_setup among its memsets in front of the launch: keys zeroed, the redo list sized from the
//      slots of all planes, d_err zeroed): k_search_and in emit mode over every query's DISTINCT required terms -> plane 0's candidate docs (dense
//      clauses from their doc bitmaps: ensure_and_bitmaps_locked, clause_bitmap_table). MUST_NOT terms are removed
//      here, through the HAS_NOT instantiation: the prohibited probe clears a0 / a1 before the emit branch is reached, and
//      DevQuery::pad is what n_req_not is computed from whether the kernel emits or collects;
//   2. k_phrase_bool_fanout (batches with a query of more than one phrase): plane 0's docs and count to the other planes;
//   3. phrase_match_stage over the virtual queries (query, phrase), plane-major — exact kernels only;
//   4. k_phrase_bool_score: the reference-order f32 sum over plane 0's key;
//   5. phrase_collect_stage over plane 0; the verdict (phrase_match_verdict), then api_rows_read_back.
// Unsupported shapes (see the header): sloppy clauses, phrases under SHOULD / MUST_NOT, SHOULD clauses or nested BooleanQuery clauses
// beside a phrase, more than RGPU_MAX_BOOL_PHRASES phrases.
static_assert(PHRASE_BOOL_MAX_PLANES == RGPU_MAX_BOOL_PHRASES, "k_phrase_bool_score keeps one key per plane in registers");
static int32_t search_phrase_bool_batch_impl(rgpu_segment* seg, rgpu_docset* set, const rgpu_phrase_bool_query* queries, int32_t n_queries,
                                             const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                             const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                             const rgpu_query_term* terms, int32_t n_terms_total,
                                             int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!seg || !queries || n_queries <= 0 || !phrases || n_phrases_total <= 0 || !phrase_terms || n_phrase_terms_total <= 0 || n_terms_total < 0 ||
      (n_terms_total > 0 && !terms) || !hits_out || !total_hits_out)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (set) RGPU_TRY(docset_check(seg, set));
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "boolean query over phrases: k must be in 1..RGPU_MAX_K");
  if (!seg->has_positions || !seg->d_pos) return fail(RGPU_ERR_ILLEGAL_STATE, "a boolean query over phrases needs a positions field with its .pos file attached");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  // ---- validate, plan
  const size_t nq = (size_t)n_queries;
  std::vector<const rgpu_term_state*> ptrs;
  std::vector<rgpu_host::PhraseBoolPlan> plans(nq);
  int max_planes = 1;
  bool any_not = false;
  const PhraseClauseArrays arrays{phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total};
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_phrase_bool_query& Q = queries[q];
    RGPU_TRY(check_phrases_query(seg, Q, "a boolean query over phrases", arrays, &ptrs));
    plans[(size_t)q] = rgpu_host::plan_phrase_bool(Q, phrases, phrase_terms, terms);
    const rgpu_host::PhraseBoolPlan& P = plans[(size_t)q];
    if (P.status != RGPU_OK) return fail(P.status, P.why);
    if (!P.dead) { max_planes = std::max(max_planes, (int)Q.n_phrases); any_not = any_not || !P.must_not.empty(); }
  }
  PhraseMask masked;
  RGPU_TRY(masked.install(seg, set));
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size()));
  // the candidate conjunction answers a dense clause from its doc bitmap, as a phrase search's does
  int64_t bitmap_df = INT64_MAX;
  {
    std::vector<const rgpu_term_state*> clauses;
    std::vector<int32_t> clause_sim;
    clauses.reserve(ptrs.size());  // (every clause of a conjunction is a live term: ptrs holds them all)
    clause_sim.reserve(ptrs.size());
    for (int32_t q = 0; q < n_queries; ++q) {
      if (plans[(size_t)q].dead) continue;
      for (const rgpu_term_state* st : plans[(size_t)q].conj) { clauses.push_back(st); clause_sim.push_back(phrases[queries[q].first_phrase].sim_table); }
    }
    RGPU_TRY(ensure_and_bitmaps_locked(seg, clauses, clause_sim, &bitmap_df));
  }
  // ---- the launch's arrays. Virtual queries (query, phrase) are plane-major: v = j * n_queries + q
  const size_t nv = nq * (size_t)max_planes;
  std::vector<DevQuery> cq(nq, DevQuery{RGPU_OP_AND, 0, 0, 0});  // the candidate conjunction: [distinct required terms][MUST_NOT x pad]
  std::vector<DevTerm> cdt;
  std::vector<DevQuery> vq(nv, DevQuery{RGPU_OP_AND, 0, 0, 0});  // the match stage: one phrase each
  std::vector<DevTerm> pdt;
  std::vector<PosTerm> ppt;
  std::vector<PhraseBoolDev> pbd(nq, PhraseBoolDev{0, 0, 0, 0});  // the scoring kernel
  std::vector<int32_t> order;
  std::vector<DevTerm> sdt;
  std::vector<int64_t> item_prefix(nq + 1), emit_prefix(nv + 1), collect_prefix(nq + 1);
  int64_t lead_blocks = 0;
  for (const rgpu_host::PhraseBoolPlan& P : plans) if (!P.dead) lead_blocks += P.lead_df / 128;
  const int blocks_per_item = and_item_blocks(c, lead_blocks);
  int64_t items = 0, collect_items = 0;
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_phrase_bool_query& Q = queries[q];
    const rgpu_host::PhraseBoolPlan& P = plans[(size_t)q];
    item_prefix[(size_t)q] = items;
    collect_prefix[(size_t)q] = collect_items;
    if (P.dead) continue;
    const int32_t conj_sim = phrases[Q.first_phrase].sim_table;  // (an emitting conjunction loads its lead's table and scores nothing)
    cq[(size_t)q] = DevQuery{RGPU_OP_AND, (int32_t)P.conj.size(), (int32_t)cdt.size(), (int32_t)P.must_not.size()};
    for (const rgpu_term_state* st : P.conj) { cdt.emplace_back(); RGPU_TRY(make_dev_term(seg, *st, 0.0f, conj_sim, &cdt.back())); }
    for (const rgpu_term_state* st : P.must_not) { cdt.emplace_back(); RGPU_TRY(make_dev_term(seg, *st, 0.0f, conj_sim, &cdt.back())); }
    const DevTerm& lead = cdt[(size_t)cq[(size_t)q].first_term];
    items += lead_items(lead, blocks_per_item);
    collect_items += lead_collect_chunks(lead);
    for (int j = 0; j < Q.n_phrases; ++j) {
      const size_t v = (size_t)j * nq + (size_t)q;
      vq[v] = DevQuery{RGPU_OP_AND, 0, (int32_t)pdt.size(), 0};
      bool dead = false;
      RGPU_TRY(emit_phrase(seg, phrases[Q.first_phrase + j], phrase_terms, &pdt, &ppt, &dead));  // (dead: the plan has said so already)
      vq[v].n_terms = dead ? 0 : phrases[Q.first_phrase + j].n_terms;
    }
    pbd[(size_t)q] = PhraseBoolDev{Q.n_phrases, (int32_t)order.size(), (int32_t)P.order.size(), 0};
    const int32_t first_clause = (int32_t)sdt.size();
    for (int i = 0; i < Q.n_terms; ++i) {
      const rgpu_query_term& t = terms[Q.first_term + i];
      sdt.emplace_back();
      RGPU_TRY(make_dev_term(seg, t.state, t.weight, t.sim_table, &sdt.back()));
    }
    for (int32_t o : P.order) order.push_back(o < 0 ? o : first_clause + o);
  }
  item_prefix[nq] = items;
  collect_prefix[nq] = collect_items;
  int64_t slots = 0;
  for (int j = 0; j < max_planes; ++j)
    for (size_t q = 0; q < nq; ++q) {
      emit_prefix[(size_t)j * nq + q] = slots;
      if (!plans[q].dead && j < queries[q].n_phrases) slots += plans[q].plane_slots;
    }
  emit_prefix[nv] = slots;
  const int64_t groups0 = emit_prefix[nq] / 64;  // plane 0's 64-slot groups
  RGPU_TRY(api_rows_default(c, stream, n_queries, k));
  if (items > 0) {
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_cq = st.add<DevQuery>(nq), r_vq = st.add<DevQuery>(nv);
    const auto r_cdt = st.add<DevTerm>(cdt.size()), r_pdt = st.add<DevTerm>(pdt.size()), r_sdt = st.add<DevTerm>(std::max<size_t>(1, sdt.size()));
    const auto r_ppt = st.add<PosTerm>(ppt.size());
    const auto r_pb = st.add<PhraseBoolDev>(nq);
    const auto r_or = st.add<int32_t>(order.size());
    const auto r_ip = st.add<int64_t>(nq + 1), r_ep = st.add<int64_t>(nv + 1), r_cp = st.add<int64_t>(nq + 1);
    const auto r_sl = st.add<int32_t>(nv);  // slop 0 throughout
    const auto r_nl = st.add<int32_t>(nq);  // no next_limit: no scorer here is two-phase
    const auto r_ab = st.add<int32_t>(nq);  // nothing is abandoned
    const auto r_gr = st.add<SloppyGroups>(nv);
    const std::vector<TermBitmap> clause_bitmaps = clause_bitmap_table(seg, cq, cdt, bitmap_df);  // (the required clauses: MUST_NOT ones are walked)
    const auto r_bm = st.add_if<TermBitmap>(!clause_bitmaps.empty(), clause_bitmaps.size());
    STAGE_SIZED(sg, st);
    sg.put(r_cq, cq);
    sg.put(r_vq, vq);
    sg.put(r_cdt, cdt);
    sg.put(r_pdt, pdt);
    sg.put(r_sdt, sdt);
    sg.put(r_ppt, ppt);
    sg.put(r_pb, pbd);
    sg.put(r_or, order);
    sg.put(r_ip, item_prefix);
    sg.put(r_ep, emit_prefix);
    sg.put(r_cp, collect_prefix);
    sg.fill(r_sl, 0);
    sg.fill(r_nl, 0xff);
    sg.fill(r_ab, 0);
    sg.fill(r_gr, 0xff);
    sg.put(r_bm, clause_bitmaps);
    RGPU_TRY(sg.upload(stream));
    const int64_t *d_ep = sg.dev(r_ep), *d_cp = sg.dev(r_cp);
    const int32_t *d_sl = sg.dev(r_sl), *d_nl = sg.dev(r_nl);
    const PhraseBoolDev* d_pb = sg.dev(r_pb);
    const bool chunked = phrase_collect_chunked(k, collect_items);
    int64_t redo_cap = 0;  // (sized from the slots of ALL planes: any of them may hand candidates on)
    // (the conjunctions: one per query, plane 0; slots and counts: every plane's - k_phrase_bool_fanout fills the others)
    const char* stage_name = masked.on() ? masked_stage_name(c, "k_search_and(masked phrase-bool candidates)", "k_search_and(masked phrase-bool, marked)")
                                         : "k_search_and(phrase-bool candidates)";
    RGPU_TRY(and_emit_stage(seg, stream, AndEmitStage{stage_name, sg.dev(r_cq), sg.dev(r_cdt), sg.dev(r_ip), d_ep,
                                                      clause_bitmaps.empty() ? nullptr : sg.dev(r_bm), n_queries, nv, items, slots, blocks_per_item, std::min<int>(k, 64),
                                                      any_not, chunked ? (size_t)collect_items * (size_t)k : 0, chunked ? (size_t)collect_items : 0, &redo_cap, true,
                                                      masked.on() && c->phrase_mask_compact}));
    const unsigned ggrid = wg_count((groups0 + WG_WAVES - 1) / WG_WAVES);
    if (groups0 > 0 && max_planes > 1) {
      TimedLaunch tl(c, stream, "k_phrase_bool_fanout", 0);
      RGPU_LAUNCH(k_phrase_bool_fanout, dim3(ggrid), dim3(WG_THREADS), 0, stream, d_pb, d_ep, c->phrase_count.p, c->phrase_docs.p, (int)n_queries, groups0);
    }
    RGPU_TRY(phrase_match_stage(seg, stream, PhraseMatchStage{sg.dev(r_vq), sg.dev(r_pdt), sg.dev(r_ppt), d_ep, d_sl, sg.dev(r_gr), (int32_t)nv, slots, redo_cap, true,
                                                              false, false, false, nullptr, nullptr, nullptr, 0}));
    if (groups0 > 0) {
      const SegView sv = seg_view(seg);
      TimedLaunch tl(c, stream, "k_phrase_bool_score", 0);
      auto go = [&](auto kern) {
        RGPU_LAUNCH(kern, dim3(ggrid), dim3(WG_THREADS), 0, stream, sv, d_pb, (const int32_t*)sg.dev(r_or), (const DevTerm*)sg.dev(r_sdt), d_ep,
                    (const unsigned long long*)c->phrase_count.p, (int)n_queries, groups0, c->phrase_keys.p, c->d_err);
      };
      if (seg->version < 1) go(k_phrase_bool_score<true>); else go(k_phrase_bool_score<false>);
    }
    // (no sloppy clause, no next_limit: no scorer here is two-phase, nothing is abandoned)
    phrase_collect_stage(seg, stream, PhraseCollectStage{d_ep, d_cp, d_sl, d_nl, n_queries, k, collect_items, false, sg.dev(r_ab), nullptr});
    HIP_TRY(launch_status());
    // a refused call writes nothing: the match stage's verdict first, the rows after it
    RGPU_TRY(phrase_match_verdict(c, stream, "a doc holds one of an exact phrase's terms more than 1024 times", "internal: a conjunction match was not found again"));
  }
  return api_rows_read_back(c, stream, n_queries, k, hits_out, total_hits_out);
}
extern "C" int32_t rgpu_search_phrase_bool_batch(rgpu_segment* seg, const rgpu_phrase_bool_query* queries, int32_t n_queries,
                                                 const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                                 const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                                 const rgpu_query_term* terms, int32_t n_terms_total,
                                                 int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  return search_phrase_bool_batch_impl(seg, nullptr, queries, n_queries, phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total, k,
                                       hits_out, total_hits_out);
}
extern "C" int32_t rgpu_search_phrase_bool_batch_masked(rgpu_segment* seg, rgpu_docset* set, const rgpu_phrase_bool_query* queries, int32_t n_queries,
                                                        const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                                        const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                                        const rgpu_query_term* terms, int32_t n_terms_total,
                                                        int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!set) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  return search_phrase_bool_batch_impl(seg, set, queries, n_queries, phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total, k,
                                       hits_out, total_hits_out);
}

