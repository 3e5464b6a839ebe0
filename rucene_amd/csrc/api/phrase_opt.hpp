// BooleanQuery of required (MUST / FILTER) and optional (SHOULD) clauses with exact PhraseQuery clauses on either side: +a +b "a b",
// +"a b" c, +"a b" +c "b c" d -n #f. search_phrase_opt_batch_impl. Entry point: rgpu_search_phrase_opt_batch.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, SCRATCH_TAKE,
// Stager / STAGE_SIZED, rucene::StageLayout, seg_view, prepare_terms_locked, make_dev_term, ensure_and_bitmaps_locked, clause_bitmap_table, and_item_blocks,
// RUNS_PER_SLOT_MAX), rows.hpp (api_rows_default, api_rows_read_back), candidates.hpp (lead_items, AndEmitStage, and_emit_stage),
// phrase_stages.hpp (PhraseMatchStage / phrase_match_stage, check_phrase_query, check_phrase_terms, emit_phrase, phrase_match_verdict),
// kernels/search_phrase_opt.hpp (with search_phrase_bool.hpp and search_phrase_or.hpp), kernels/search_and.hpp (SeqRec, k_req_opt_scan),
// kernels/search_or.hpp (k_score_terms), host/phrase_opt_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- BooleanQuery of required and optional clauses over exact phrases and terms: +a +b "a b", +"a b" c ------------------------------
// (include/rucene_gpu.h rgpu_search_phrase_opt_batch; the plan: host/phrase_opt_plan.hpp; the kernels of its own:
// kernels/search_phrase_opt.hpp.) The phrase-bool stages run over N = n_queries + (optional phrases that exist in the leaf) pseudo
// queries: pseudo query q < n_queries is query q's required side (planes = its required phrases, or one seeded plane when it names
// none), pseudo query n_queries + e is optional phrase e by itself (one plane, its own terms as the conjunction). Launch sequence,
// all on the call's stream and in ONE scratch slot (the runs and the records are live at once: the records stand behind the runs in
// the slot's run buffer, a region of their own):
//   1. and_emit_stage, "k_search_and(phrase-opt candidates)": every pseudo query's candidate docs, MUST_NOT terms removed there;
//   2. k_phrase_bool_fanout (a query with more than one required phrase), phrase_match_stage (exact kernels only),
//      k_phrase_opt_seed (a required side of terms alone), k_phrase_bool_score: plane 0 of every pseudo query holds
//      make_key(required sum | phrase score, doc) or 0 per candidate. The verdict is looked at here, before anything else runs;
//   3. k_phrase_run_fill, _count, _scan, _scatter, _sort over the N pseudo queries: one doc-ascending {doc, score} run each, whatever
//      order the candidates arrived in (capacity: the lead's doc_freq); dead candidates carry no key and never reach a run;
//   4. k_score_terms: one run per optional term clause that exists in the leaf;
//   5. k_req_opt_join: required run x the query's optional runs -> SeqRec{doc, req, opt} at the required entry's index;
//   6. k_req_opt_scan as it stands: the rule (rgpu_config.req_opt_rule = -1: the join has added opt to req, the rule then cannot
//      change a score), the count and the collector. k > RGPU_PASS_K: only this kernel again per pass of 128 hits, over the same records.
static int32_t search_phrase_opt_batch_impl(rgpu_segment* seg, const rgpu_phrase_opt_query* queries, int32_t n_queries,
                                            const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                            const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                            const rgpu_query_term* terms, int32_t n_terms_total,
                                            int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!seg || !queries || n_queries <= 0 || n_phrases_total < 0 || n_phrase_terms_total < 0 || n_terms_total < 0 || (n_phrases_total > 0 && !phrases) ||
      (n_phrase_terms_total > 0 && !phrase_terms) || (n_terms_total > 0 && !terms) || !hits_out || !total_hits_out)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "MUST + SHOULD tree over phrases: k must be in 1..RGPU_MAX_K");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  // ---- validate, plan: every refusal is decided here, before anything is launched
  const size_t nq = (size_t)n_queries;
  std::vector<rgpu_host::PhraseOptPlan> plans(nq);
  const rgpu_host::PhraseOptArrays arrays{phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total};
  bool any_phrase = false;
  for (size_t q = 0; q < nq; ++q) {
    plans[q] = rgpu_host::plan_phrase_opt(queries[q], arrays);
    if (plans[q].status != RGPU_OK) return fail(plans[q].status, plans[q].why);
    any_phrase = any_phrase || queries[q].n_req_phrases + queries[q].n_opt_phrases > 0;
  }
  if (any_phrase && (!seg->has_positions || !seg->d_pos))
    return fail(RGPU_ERR_ILLEGAL_STATE, "a MUST + SHOULD tree over phrases needs a positions field with its .pos file attached");
  std::vector<const rgpu_term_state*> ptrs;
  for (size_t q = 0; q < nq; ++q) {
    const rgpu_phrase_opt_query& Q = queries[q];
    for (int i = 0; i < Q.n_req_phrases + Q.n_opt_phrases; ++i) {
      const rgpu_phrase_query& ph = phrases[Q.first_phrase + i];
      RGPU_TRY(check_phrase_query(c, ph, n_phrase_terms_total, false));
      RGPU_TRY(check_phrase_terms(seg, ph, phrase_terms, &ptrs));
    }
    const int n_scored = Q.n_req_terms + Q.n_opt_terms;
    for (int i = 0; i < n_scored + Q.n_must_not; ++i) {
      const rgpu_query_term& t = terms[Q.first_term + i];
      if (i < n_scored && (t.sim_table < 0 || t.sim_table >= c->n_sim_tables)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "unknown sim_table handle");
      if (t.state.doc_freq > 0) ptrs.push_back(&t.state);
    }
  }
  if (!ptrs.empty()) RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size()));
  // ---- the pseudo queries: [0, nq) the required sides, then one per optional phrase that exists in its (live) query's leaf
  struct OptPhrase { int32_t q, j; };
  std::vector<OptPhrase> optv;
  std::vector<int32_t> first_optv(nq + 1, 0);
  int max_planes = 1;
  bool any_not = false;
  for (size_t q = 0; q < nq; ++q) {
    first_optv[q] = (int32_t)optv.size();
    const rgpu_host::PhraseOptPlan& P = plans[q];
    if (P.dead) continue;
    max_planes = std::max(max_planes, (int)queries[q].n_req_phrases);
    any_not = any_not || !P.must_not.empty();
    for (int j = 0; j < queries[q].n_opt_phrases; ++j) if (P.opt_capacity[(size_t)j] > 0) optv.push_back(OptPhrase{(int32_t)q, j});
  }
  first_optv[nq] = (int32_t)optv.size();
  const size_t N = nq + optv.size();
  const size_t nv = N * (size_t)max_planes;  // virtual queries (pseudo query, plane), plane-major: v = j * N + p
  auto conj_sim_of = [&](const rgpu_phrase_opt_query& Q) { return Q.n_req_phrases > 0 ? phrases[Q.first_phrase].sim_table : terms[Q.first_term].sim_table; };
  // the candidate conjunctions answer a dense clause from its doc bitmap, as a phrase search's do
  int64_t bitmap_df = INT64_MAX;
  {
    std::vector<const rgpu_term_state*> clauses;
    std::vector<int32_t> clause_sim;
    for (size_t q = 0; q < nq; ++q) {
      if (plans[q].dead) continue;
      for (const rgpu_term_state* st : plans[q].conj) { clauses.push_back(st); clause_sim.push_back(conj_sim_of(queries[q])); }
    }
    for (const OptPhrase& e : optv) {
      const rgpu_phrase_query& ph = phrases[queries[e.q].first_phrase + queries[e.q].n_req_phrases + e.j];
      for (int i = 0; i < ph.n_terms; ++i) { clauses.push_back(&phrase_terms[ph.first_term + i].state); clause_sim.push_back(ph.sim_table); }
    }
    RGPU_TRY(ensure_and_bitmaps_locked(seg, clauses, clause_sim, &bitmap_df));
  }
  // ---- the launches' arrays
  std::vector<DevQuery> cq(N, DevQuery{RGPU_OP_AND, 0, 0, 0});   // the candidate conjunctions
  std::vector<DevTerm> cdt;
  std::vector<DevQuery> vq(nv, DevQuery{RGPU_OP_AND, 0, 0, 0});  // the match stage: one phrase each (n_terms 0: nothing to match)
  std::vector<DevTerm> pdt;
  std::vector<PosTerm> ppt;
  std::vector<PhraseBoolDev> pbd(N, PhraseBoolDev{0, 0, 0, 0});  // k_phrase_bool_score
  std::vector<int32_t> order, seeded(N, 0);
  std::vector<DevTerm> sdt;
  std::vector<int64_t> item_prefix(N + 1), emit_prefix(nv + 1), plane_slots(N, 0);
  std::vector<int32_t> capacity(N, 0);  // of each pseudo query's run
  int64_t lead_blocks = 0;
  for (size_t q = 0; q < nq; ++q) if (!plans[q].dead) lead_blocks += plans[q].lead_df / 128;
  for (const OptPhrase& e : optv) lead_blocks += plans[(size_t)e.q].opt_capacity[(size_t)e.j] / 128;
  const int blocks_per_item = and_item_blocks(c, lead_blocks);
  int64_t items = 0;
  bool any_seeded = false;
  for (size_t q = 0; q < nq; ++q) {
    const rgpu_phrase_opt_query& Q = queries[q];
    const rgpu_host::PhraseOptPlan& P = plans[q];
    item_prefix[q] = items;
    if (P.dead) continue;
    const int32_t conj_sim = conj_sim_of(Q);  // (an emitting conjunction loads its lead's table and scores nothing)
    cq[q] = DevQuery{RGPU_OP_AND, (int32_t)P.conj.size(), (int32_t)cdt.size(), (int32_t)P.must_not.size()};
    for (const rgpu_term_state* st : P.conj) { cdt.emplace_back(); RGPU_TRY(make_dev_term(seg, *st, 0.0f, conj_sim, &cdt.back())); }
    for (const rgpu_term_state* st : P.must_not) { cdt.emplace_back(); RGPU_TRY(make_dev_term(seg, *st, 0.0f, conj_sim, &cdt.back())); }
    items += lead_items(cdt[(size_t)cq[q].first_term], blocks_per_item);
    for (int j = 0; j < Q.n_req_phrases; ++j) {
      const size_t v = (size_t)j * N + q;
      vq[v] = DevQuery{RGPU_OP_AND, 0, (int32_t)pdt.size(), 0};
      bool dead = false;
      RGPU_TRY(emit_phrase(seg, phrases[Q.first_phrase + j], phrase_terms, &pdt, &ppt, &dead));  // (dead: the plan has said so already)
      vq[v].n_terms = dead ? 0 : phrases[Q.first_phrase + j].n_terms;
    }
    // a required side of term clauses alone: one plane, seeded by k_phrase_opt_seed (n_planes == 0 stays "dead in this leaf")
    if (Q.n_req_phrases == 0) { seeded[q] = 1; any_seeded = true; }
    pbd[q] = PhraseBoolDev{std::max<int32_t>(1, Q.n_req_phrases), (int32_t)order.size(), (int32_t)P.req_order.size(), 0};
    const int32_t first_clause = (int32_t)sdt.size();
    for (int i = 0; i < Q.n_req_terms; ++i) {
      const rgpu_query_term& t = terms[Q.first_term + i];
      sdt.emplace_back();
      RGPU_TRY(make_dev_term(seg, t.state, t.weight, t.sim_table, &sdt.back()));
    }
    for (int32_t o : P.req_order) order.push_back(o < 0 ? o : first_clause + o);
    plane_slots[q] = P.plane_slots;
    capacity[q] = P.lead_df;
  }
  for (size_t e = 0; e < optv.size(); ++e) {
    const size_t p = nq + e;
    const rgpu_phrase_opt_query& Q = queries[optv[e].q];
    const rgpu_phrase_query& ph = phrases[Q.first_phrase + Q.n_req_phrases + optv[e].j];
    const int32_t cap = plans[(size_t)optv[e].q].opt_capacity[(size_t)optv[e].j];
    item_prefix[p] = items;
    const size_t first = pdt.size();
    bool dead = false;
    RGPU_TRY(emit_phrase(seg, ph, phrase_terms, &pdt, &ppt, &dead));
    if (dead || pdt[first].df != cap) return fail(RGPU_ERR_ILLEGAL_STATE, "internal: a phrase's lead term is not its rarest");
    vq[p] = DevQuery{RGPU_OP_AND, ph.n_terms, (int32_t)first, 0};
    cq[p] = DevQuery{RGPU_OP_AND, ph.n_terms, (int32_t)cdt.size(), 0};  // the phrase's own terms, rarest first, as the phrase-or call hands them on
    for (int i = 0; i < ph.n_terms; ++i) { const DevTerm t = pdt[first + (size_t)i]; cdt.push_back(t); }
    items += lead_items(cdt[(size_t)cq[p].first_term], blocks_per_item);
    pbd[p] = PhraseBoolDev{1, (int32_t)order.size(), 1, 0};
    order.push_back(~0);
    plane_slots[p] = rgpu_host::popt_round_up_64(cap);
    capacity[p] = cap;
  }
  item_prefix[N] = items;
  int64_t slots = 0;
  for (int j = 0; j < max_planes; ++j)
    for (size_t p = 0; p < N; ++p) {
      emit_prefix[(size_t)j * N + p] = slots;
      if (j < pbd[p].n_planes) slots += plane_slots[p];
    }
  emit_prefix[nv] = slots;
  const int64_t groups0 = emit_prefix[N] / 64;  // plane 0's 64-slot groups
  // ---- the runs: [0, N) the pseudo queries' (filled by k_phrase_run_*), then one per optional term clause present (k_score_terms)
  std::vector<DevTerm> tdt;
  std::vector<ReqOptJoinDev> jq(nq, ReqOptJoinDev{0, 0, 0, 0});
  std::vector<int32_t> opt_runs;
  std::vector<int64_t> seq_prefix(nq + 1, 0);
  const int32_t add_all = c->cfg.req_opt_rule < 0 ? 1 : 0;
  for (size_t q = 0; q < nq; ++q) {
    const rgpu_phrase_opt_query& Q = queries[q];
    const rgpu_host::PhraseOptPlan& P = plans[q];
    seq_prefix[q + 1] = seq_prefix[q] + (P.dead ? 0 : rgpu_host::popt_round_up_64(P.lead_df));
    jq[q] = ReqOptJoinDev{(int32_t)q, (int32_t)opt_runs.size(), 0, add_all};
    if (P.dead) continue;
    for (int32_t o : P.opt_order) {
      if (o >= 0) {
        const rgpu_query_term& t = terms[Q.first_term + Q.n_req_terms + o];
        tdt.emplace_back();
        RGPU_TRY(make_dev_term(seg, t.state, t.weight, t.sim_table, &tdt.back()));
        opt_runs.push_back((int32_t)(N + tdt.size() - 1));
      } else {
        int32_t e = first_optv[q];
        while (optv[(size_t)e].j != ~o) ++e;  // (present: its capacity is positive, so the loop above listed it)
        opt_runs.push_back((int32_t)(nq + (size_t)e));
      }
    }
    jq[q].n_opt = (int32_t)P.opt_order.size();
  }
  const size_t T = tdt.size(), n_runs = N + T;
  int term_blocks_per_item = 32;
  std::vector<int64_t> term_item_prefix(T + 1), run_prefix(n_runs + 1);
  std::vector<int32_t> run_len(n_runs, 0);
  int64_t term_items = 0;
  while (true) {  // (search_or_group's item plan)
    term_items = 0;
    for (size_t t = 0; t < T; ++t) {
      term_item_prefix[t] = term_items;
      term_items += tdt[t].nblocks == 0 ? 1 : (tdt[t].nblocks + term_blocks_per_item - 1) / term_blocks_per_item;
    }
    term_item_prefix[T] = term_items;
    if (term_items <= 1048576 || term_blocks_per_item >= (1 << 17)) break;
    term_blocks_per_item *= 2;
  }
  int64_t postings = 0;
  for (size_t r = 0; r < n_runs; ++r) {
    run_len[r] = r < N ? capacity[r] : tdt[r - N].df;
    run_prefix[r] = postings;
    if (run_len[r] > 0) postings += (int64_t)run_len[r] + OR_RUN_PAD;
  }
  run_prefix[n_runs] = postings;
  const int64_t n_records = seq_prefix[nq];
  // the run buffer's two regions (host/stage_layout.hpp: each on a 256-byte boundary): the runs and, behind them, the records -
  // live at once here, so the records are not laid over the run scratch as search_pass lays them
  rucene::StageLayout run_layout;
  const auto r_runs = run_layout.add<ScoredPosting>((size_t)postings + 64);
  const auto r_recs = run_layout.add<SeqRec>((size_t)n_records);
  const size_t run_buf_entries = (run_layout.used + sizeof(ScoredPosting) - 1) / sizeof(ScoredPosting);
  std::vector<PhraseRunDev> prd(N);
  for (size_t p = 0; p < N; ++p) prd[p] = PhraseRunDev{(int32_t)p, capacity[p]};
  const int n_buckets = (int)(((int64_t)seg->max_doc + PHRASE_OR_BUCKET - 1) / PHRASE_OR_BUCKET);
  const size_t n_cells = N * (size_t)std::max(1, n_buckets);

  RGPU_TRY(api_rows_default(c, stream, n_queries, k));
  if (items > 0) {
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_cq = st.add<DevQuery>(N), r_vq = st.add<DevQuery>(nv);
    const auto r_cdt = st.add<DevTerm>(cdt.size()), r_pdt = st.add<DevTerm>(std::max<size_t>(1, pdt.size())), r_sdt = st.add<DevTerm>(std::max<size_t>(1, sdt.size()));
    const auto r_tdt = st.add<DevTerm>(std::max<size_t>(1, T));
    const auto r_ppt = st.add<PosTerm>(std::max<size_t>(1, ppt.size()));
    const auto r_pb = st.add<PhraseBoolDev>(N);
    const auto r_or = st.add<int32_t>(std::max<size_t>(1, order.size())), r_sd = st.add<int32_t>(N);
    const auto r_ip = st.add<int64_t>(N + 1), r_ep = st.add<int64_t>(nv + 1);
    const auto r_sl = st.add<int32_t>(nv);  // slop 0 throughout
    const auto r_gr = st.add<SloppyGroups>(nv);
    const auto r_pr = st.add<PhraseRunDev>(N);
    const auto r_tip = st.add<int64_t>(T + 1), r_rp = st.add<int64_t>(n_runs + 1), r_sp = st.add<int64_t>(nq + 1);
    const auto r_rl = st.add<int32_t>(n_runs), r_orn = st.add<int32_t>(std::max<size_t>(1, opt_runs.size()));
    const auto r_jq = st.add<ReqOptJoinDev>(nq);
    const std::vector<TermBitmap> clause_bitmaps = clause_bitmap_table(seg, cq, cdt, bitmap_df);  // (the required clauses: MUST_NOT ones are walked)
    const auto r_bm = st.add_if<TermBitmap>(!clause_bitmaps.empty(), clause_bitmaps.size());
    STAGE_SIZED(sg, st);
    sg.put(r_cq, cq);
    sg.put(r_vq, vq);
    sg.put(r_cdt, cdt);
    sg.put(r_pdt, pdt);
    sg.put(r_sdt, sdt);
    sg.put(r_tdt, tdt);
    sg.put(r_ppt, ppt);
    sg.put(r_pb, pbd);
    sg.put(r_or, order);
    sg.put(r_sd, seeded);
    sg.put(r_ip, item_prefix);
    sg.put(r_ep, emit_prefix);
    sg.fill(r_sl, 0);
    sg.fill(r_gr, 0xff);
    sg.put(r_pr, prd);
    sg.put(r_tip, term_item_prefix);
    sg.put(r_rp, run_prefix);
    sg.put(r_sp, seq_prefix);
    sg.put(r_rl, run_len);
    sg.put(r_orn, opt_runs);
    sg.put(r_jq, jq);
    sg.put(r_bm, clause_bitmaps);
    RGPU_TRY(sg.upload(stream));
    const int64_t* d_ep = sg.dev(r_ep);
    const PhraseBoolDev* d_pb = sg.dev(r_pb);
    const SegView sv = seg_view(seg);
    // ---- 1.: the candidates of every pseudo query
    int64_t redo_cap = 0;
    RGPU_TRY(and_emit_stage(seg, stream, AndEmitStage{"k_search_and(phrase-opt candidates)", sg.dev(r_cq), sg.dev(r_cdt), sg.dev(r_ip), d_ep,
                                                      clause_bitmaps.empty() ? nullptr : sg.dev(r_bm), (int32_t)N, nv, items, slots, blocks_per_item,
                                                      std::min<int>(k, 64), any_not, 0, 0, &redo_cap, true, false}));
    // ---- 2.: plane 0's keys
    const unsigned ggrid = wg_count((groups0 + WG_WAVES - 1) / WG_WAVES);
    if (groups0 > 0 && max_planes > 1) {
      TimedLaunch tl(c, stream, "k_phrase_bool_fanout", 0);
      RGPU_LAUNCH(k_phrase_bool_fanout, dim3(ggrid), dim3(WG_THREADS), 0, stream, d_pb, d_ep, c->phrase_count.p, c->phrase_docs.p, (int)N, groups0);
    }
    RGPU_TRY(phrase_match_stage(seg, stream, PhraseMatchStage{sg.dev(r_vq), sg.dev(r_pdt), sg.dev(r_ppt), d_ep, sg.dev(r_sl), sg.dev(r_gr), (int32_t)nv, slots, redo_cap,
                                                              !pdt.empty(), false, false, false, nullptr, nullptr, nullptr, 0}));
    if (groups0 > 0 && any_seeded) {
      TimedLaunch tl(c, stream, "k_phrase_opt_seed", 0);
      RGPU_LAUNCH(k_phrase_opt_seed, dim3(ggrid), dim3(WG_THREADS), 0, stream, (const int32_t*)sg.dev(r_sd), d_ep, (const unsigned long long*)c->phrase_count.p,
                  (const int32_t*)c->phrase_docs.p, (int)N, groups0, c->phrase_keys.p);
    }
    if (groups0 > 0) {
      TimedLaunch tl(c, stream, "k_phrase_bool_score", 0);
      auto go = [&](auto kern) {
        RGPU_LAUNCH(kern, dim3(ggrid), dim3(WG_THREADS), 0, stream, sv, d_pb, (const int32_t*)sg.dev(r_or), (const DevTerm*)sg.dev(r_sdt), d_ep,
                    (const unsigned long long*)c->phrase_count.p, (int)N, groups0, c->phrase_keys.p, c->d_err);
      };
      if (seg->version < 1) go(k_phrase_bool_score<true>); else go(k_phrase_bool_score<false>);
    }
    HIP_TRY(launch_status());
    // a refused call writes nothing: the verdict before anything else runs
    RGPU_TRY(phrase_match_verdict(c, stream, "a doc holds one of an exact phrase's terms more than 1024 times", "internal: a conjunction match was not found again"));
    // ---- 3.: the pseudo queries' runs (bounds: kernels/search_phrase_or.hpp)
    const bool own_runs = run_buf_entries <= RUNS_PER_SLOT_MAX;
    DevVec<ScoredPosting>& runs_buf = own_runs ? c->S->d_runs : c->d_runs;
    HIP_TRY(runs_buf.reserve(run_buf_entries, 0, stream));
    ScoredPosting* runs = reinterpret_cast<ScoredPosting*>(reinterpret_cast<uint8_t*>(runs_buf.p) + r_runs.off);
    SeqRec* records = reinterpret_cast<SeqRec*>(reinterpret_cast<uint8_t*>(runs_buf.p) + r_recs.off);
    const int64_t* d_rp = sg.dev(r_rp);
    if (groups0 > 0 && n_buckets > 0) {
      HIP_TRY(c->phrase_or_buckets.reserve(2 * n_cells, 0, stream));
      const PhraseRunDev* d_pr = sg.dev(r_pr);
      uint32_t* counts = c->phrase_or_buckets.p;
      uint32_t* offsets = counts + n_cells;
      const int groups_per_clause = (n_buckets + 63) / 64;  // k_phrase_run_sort: one wavefront per (clause, 64 buckets)
      const int64_t sort_items = (int64_t)N * groups_per_clause;
      HIP_TRY(hipMemsetAsync(counts, 0, n_cells * sizeof(uint32_t), stream));
      {
        TimedLaunch tl(c, stream, "k_phrase_run_fill", 0);
        RGPU_LAUNCH(k_phrase_run_fill, dim3((unsigned)N, PHRASE_OR_FILL_SPLIT), dim3(WG_THREADS), 0, stream, d_pr, d_rp, runs);
      }
      {
        TimedLaunch tl(c, stream, "k_phrase_run_count", 0);
        RGPU_LAUNCH(k_phrase_run_place<false>, dim3(ggrid), dim3(WG_THREADS), 0, stream, d_pr, d_ep, (const unsigned long long*)c->phrase_count.p,
                    (const uint64_t*)c->phrase_keys.p, (int)N, groups0, seg->max_doc, n_buckets, counts, (const uint32_t*)offsets, d_rp, runs);
      }
      {
        TimedLaunch tl(c, stream, "k_phrase_run_scan", 0);
        RGPU_LAUNCH(k_phrase_run_scan, dim3(wg_count((N + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, (int)N, n_buckets, counts, offsets);
      }
      {
        TimedLaunch tl(c, stream, "k_phrase_run_scatter", 0);
        RGPU_LAUNCH(k_phrase_run_place<true>, dim3(ggrid), dim3(WG_THREADS), 0, stream, d_pr, d_ep, (const unsigned long long*)c->phrase_count.p,
                    (const uint64_t*)c->phrase_keys.p, (int)N, groups0, seg->max_doc, n_buckets, counts, (const uint32_t*)offsets, d_rp, runs);
      }
      {
        TimedLaunch tl(c, stream, "k_phrase_run_sort", 0);
        RGPU_LAUNCH(k_phrase_run_sort, dim3(wg_count((sort_items + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, d_pr, sort_items, n_buckets,
                    groups_per_clause, (const uint32_t*)counts, (const uint32_t*)offsets, d_rp, runs);
      }
    }
    // ---- 4.: the optional term clauses' runs (run N + t: out_prefix = run_prefix + N)
    if (term_items > 0) {
      TimedLaunch tl(c, stream, "k_score_terms", 0);
      const unsigned grid = wg_count((term_items + WG_WAVES - 1) / WG_WAVES);
      if (seg->version < 1)
        RGPU_LAUNCH(k_score_terms<true>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_tdt), (const int64_t*)sg.dev(r_tip), d_rp + N, (int)T,
                    term_items, term_blocks_per_item, runs);
      else
        RGPU_LAUNCH(k_score_terms<false>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_tdt), (const int64_t*)sg.dev(r_tip), d_rp + N, (int)T,
                    term_items, term_blocks_per_item, runs);
    }
    // ---- 5.: the records (bounds: kernels/search_phrase_opt.hpp)
    const int64_t* d_sp = sg.dev(r_sp);
    if (n_records > 0) {
      TimedLaunch tl(c, stream, "k_req_opt_join", 0);
      const int64_t jgroups = n_records / 64;
      RGPU_LAUNCH(k_req_opt_join, dim3(wg_count((jgroups + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, (const ReqOptJoinDev*)sg.dev(r_jq),
                  (const int32_t*)sg.dev(r_orn), d_rp, (const int32_t*)sg.dev(r_rl), (const ScoredPosting*)runs, d_sp, (int)n_queries, jgroups, records);
    }
    // ---- 6.: the rule, the count, the collector; deeper pages in passes over the same records
    auto scan = [&](int32_t k_pass, int stride, int col0, const unsigned long long* ceil_in, unsigned long long* ceil_out) {
      TimedLaunch tl(c, stream, "k_req_opt_scan", 0);
      const unsigned grid = wg_count((nq + WG_WAVES - 1) / WG_WAVES);
      if (k_pass > 64)
        RGPU_LAUNCH(k_req_opt_scan<true>, dim3(grid), dim3(WG_THREADS), 0, stream, (const SeqRec*)records, d_sp, (int)n_queries, (int)k_pass, seg->doc_base,
                    (const int32_t*)nullptr, c->host_api_hits.p, c->host_api_totals.p, stride, col0, ceil_in, ceil_out);
      else
        RGPU_LAUNCH(k_req_opt_scan<false>, dim3(grid), dim3(WG_THREADS), 0, stream, (const SeqRec*)records, d_sp, (int)n_queries, (int)k_pass, seg->doc_base,
                    (const int32_t*)nullptr, c->host_api_hits.p, c->host_api_totals.p, stride, col0, ceil_in, ceil_out);
    };
    if (k <= RGPU_PASS_K) {
      scan(k, 0, 0, nullptr, nullptr);
    } else {  // search_impl's passes: pass p collects the best hits strictly below the worst hit of pass p - 1
      rgpu_ctx::CeilSlot& cs = c->ceil_slots[c->ceil_next];
      c->ceil_next = (c->ceil_next + 1) % N_SCRATCH;
      if (cs.busy) { HIP_TRY(hipEventSynchronize(cs.done)); cs.busy = false; }
      HIP_TRY(cs.d.reserve(nq * 2, 0, stream));
      int flip = 0;
      for (int32_t col0 = 0; col0 < k; col0 += RGPU_PASS_K, flip ^= 1)
        scan(std::min<int32_t>(RGPU_PASS_K, k - col0), k, col0, col0 == 0 ? nullptr : cs.d.p + (size_t)(flip ^ 1) * nq, cs.d.p + (size_t)flip * nq);
    }
    HIP_TRY(launch_status());
  }
  return api_rows_read_back(c, stream, n_queries, k, hits_out, total_hits_out);  // (ends synchronised: the slot and the run buffer are free again)
}
extern "C" int32_t rgpu_search_phrase_opt_batch(rgpu_segment* seg, const rgpu_phrase_opt_query* queries, int32_t n_queries,
                                                const rgpu_phrase_query* phrases, int32_t n_phrases_total,
                                                const rgpu_phrase_term* phrase_terms, int32_t n_phrase_terms_total,
                                                const rgpu_query_term* terms, int32_t n_terms_total,
                                                int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  return search_phrase_opt_batch_impl(seg, queries, n_queries, phrases, n_phrases_total, phrase_terms, n_phrase_terms_total, terms, n_terms_total, k,
                                      hits_out, total_hits_out);
}

