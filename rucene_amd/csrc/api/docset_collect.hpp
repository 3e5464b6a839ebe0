// Doc sets collected from queries: every doc a row matches, as one set per row. Entry point: rgpu_docset_collect_batch.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, scratch_mark /
// SCRATCH_TAKE, Stager / STAGE_SIZED, seg_view, validate_state, prepare_terms_locked, make_dev_term, rgpu_sim_table_upload, and_item_blocks),
// candidates.hpp (lead_items, lead_slots, AndEmitStage, and_emit_stage), docsets.hpp (rgpu_docset, docset_new, docset_delete, docset_finish),
// kernels/docset.hpp, host/docset_plan.hpp.
// The function had no banner of its own in the single file: it followed the point ranges.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

extern "C" int32_t rgpu_docset_collect_batch(rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries, const rgpu_query_term* terms,
                                             int32_t n_terms_total, rgpu_docset** out_sets) {
  if (!seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !out_sets) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  for (int32_t q = 0; q < n_queries; ++q) out_sets[q] = nullptr;
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  // ---- plan: refusals come before anything is allocated
  std::vector<rgpu_host::DocsetQueryPlan> plans((size_t)n_queries);
  std::vector<const rgpu_term_state*> ptrs;
  bool any_conj = false;
  for (int32_t q = 0; q < n_queries; ++q) {
    plans[(size_t)q] = rgpu_host::plan_docset_query(queries[q], terms, n_terms_total);
    const rgpu_host::DocsetQueryPlan& P = plans[(size_t)q];
    if (P.status != RGPU_OK) return fail(P.status, P.why);
    for (const std::vector<const rgpu_term_state*>* side : {&P.positive, &P.negative})
      for (const rgpu_term_state* st : *side) {
        RGPU_TRY(validate_state(seg, *st));
        if (st->doc_freq == 1 && (st->singleton_doc_id < 0 || st->singleton_doc_id >= seg->max_doc)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "singleton_doc_id out of range");
        ptrs.push_back(st);
      }
    any_conj = any_conj || P.conjunction;
  }
  if (any_conj && c->n_sim_tables <= 0)
    return fail(RGPU_ERR_ILLEGAL_STATE, "collecting a conjunction runs the search's conjunction kernel: upload a similarity table first (rgpu_sim_table_upload)");
  // (a conjunction's lead is walked with its posting-order norms, as in a search; the list kernel needs the blocks alone)
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size(), any_conj));
  std::vector<rgpu_docset*> sets((size_t)n_queries, nullptr);
  auto drop = [&](int32_t rc) { (void)hipStreamSynchronize(stream); for (rgpu_docset* d : sets) docset_delete(d); return rc; };
  for (int32_t q = 0; q < n_queries; ++q) { const int32_t rc = docset_new(seg, &sets[(size_t)q]); if (rc != RGPU_OK) return drop(rc); }
  std::vector<uint32_t*> rows((size_t)n_queries);
  for (int32_t q = 0; q < n_queries; ++q) rows[(size_t)q] = reinterpret_cast<uint32_t*>(sets[(size_t)q]->d_words);
  const SegView sv = seg_view(seg);
  const bool legacy = seg->version < 1;
  auto lists = [&]() -> int32_t {  // ---- TERM / OR rows: bits set list by list, then the MUST_NOT lists cleared
    const rgpu_host::DocsetJobs J = rgpu_host::plan_docset_jobs(plans, DOCSET_BLOCKS_PER_ITEM);
    if (J.set.empty()) return RGPU_OK;
    std::vector<DevTerm> dt;
    std::vector<DocsetJob> js, jc;
    std::vector<int64_t> ps, pc;
    int64_t postings = 0;
    for (const std::vector<rgpu_host::DocsetListJob>* side : {&J.set, &J.clear})
      for (const rgpu_host::DocsetListJob& j : *side) {
        dt.emplace_back();
        RGPU_TRY(make_dev_term(seg, *j.term, 0.0f, 0, &dt.back(), false));
        // (the plan sized the job from doc_freq; the prepared term must agree, or items would run past its blocks)
        if (rgpu_host::docset_term_items(dt.back().df, DOCSET_BLOCKS_PER_ITEM) != j.n_items || (dt.back().df >= 2 && dt.back().nblocks != dt.back().df / 128))
          return fail(RGPU_ERR_ILLEGAL_STATE, "internal: a prepared term disagrees with its doc_freq");
        (side == &J.set ? js : jc).push_back(DocsetJob{(uint32_t)(dt.size() - 1), (uint32_t)j.row});
        (side == &J.set ? ps : pc).push_back(j.first_item);
        postings += j.term->doc_freq;
      }
    ps.push_back(J.set_items);
    pc.push_back(J.clear_items);
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_t = st.add<DevTerm>(dt.size());
    const auto r_js = st.add<DocsetJob>(js.size()), r_jc = st.add<DocsetJob>(std::max<size_t>(1, jc.size()));
    const auto r_ps = st.add<int64_t>(ps.size()), r_pc = st.add<int64_t>(pc.size());
    const auto r_rows = st.add<uint32_t*>(rows.size());
    STAGE_SIZED(sg, st);
    sg.put(r_t, dt);
    sg.put(r_js, js);
    sg.put(r_jc, jc);
    sg.put(r_ps, ps);
    sg.put(r_pc, pc);
    sg.put(r_rows, rows);
    RGPU_TRY(sg.upload(stream));
    {
      TimedLaunch tl(c, stream, "k_docset_lists", postings);
      const unsigned grid = wg_count(((unsigned long long)J.set_items + DOCSET_WAVES - 1) / DOCSET_WAVES);
      if (legacy) RGPU_LAUNCH((k_docset_lists<true, false>), dim3(grid), dim3(DOCSET_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const DocsetJob*)sg.dev(r_js),
                              (const int64_t*)sg.dev(r_ps), (int)js.size(), J.set_items, (uint32_t* const*)sg.dev(r_rows));
      else RGPU_LAUNCH((k_docset_lists<false, false>), dim3(grid), dim3(DOCSET_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const DocsetJob*)sg.dev(r_js),
                       (const int64_t*)sg.dev(r_ps), (int)js.size(), J.set_items, (uint32_t* const*)sg.dev(r_rows));
    }
    if (!jc.empty()) {
      TimedLaunch tl(c, stream, "k_docset_lists", 0);
      const unsigned grid = wg_count(((unsigned long long)J.clear_items + DOCSET_WAVES - 1) / DOCSET_WAVES);
      if (legacy) RGPU_LAUNCH((k_docset_lists<true, true>), dim3(grid), dim3(DOCSET_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const DocsetJob*)sg.dev(r_jc),
                              (const int64_t*)sg.dev(r_pc), (int)jc.size(), J.clear_items, (uint32_t* const*)sg.dev(r_rows));
      else RGPU_LAUNCH((k_docset_lists<false, true>), dim3(grid), dim3(DOCSET_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const DocsetJob*)sg.dev(r_jc),
                       (const int64_t*)sg.dev(r_pc), (int)jc.size(), J.clear_items, (uint32_t* const*)sg.dev(r_rows));
    }
    HIP_TRY(launch_status());
    HIP_TRY(scratch_mark(c, stream));
    return RGPU_OK;
  };
  auto conjunctions = [&]() -> int32_t {  // ---- AND rows: k_search_and emits the matches (deleted docs included, marked), scattered into bits
    if (!any_conj) return RGPU_OK;
    const size_t nq = (size_t)n_queries;
    std::vector<DevQuery> dq(nq, DevQuery{RGPU_OP_AND, 0, 0, 0});
    std::vector<DevTerm> dt;
    std::vector<int64_t> item_prefix(nq + 1), emit_prefix(nq + 1);
    int64_t lead_blocks = 0;
    for (const rgpu_host::DocsetQueryPlan& P : plans) if (P.conjunction) lead_blocks += P.positive[0]->doc_freq / 128;
    const int blocks_per_item = and_item_blocks(c, lead_blocks);
    int64_t items = 0, slots = 0;
    bool any_not = false;
    for (size_t q = 0; q < nq; ++q) {
      const rgpu_host::DocsetQueryPlan& P = plans[q];
      item_prefix[q] = items;
      emit_prefix[q] = slots;
      dq[q].first_term = (int32_t)dt.size();
      if (!P.conjunction) continue;
      int32_t sim = terms[queries[q].first_term].sim_table;  // (an emitting conjunction loads its lead's table and scores nothing)
      if (sim < 0 || sim >= c->n_sim_tables) sim = 0;
      dq[q] = DevQuery{RGPU_OP_AND, (int32_t)P.positive.size(), (int32_t)dt.size(), (int32_t)P.negative.size()};
      for (const rgpu_term_state* st : P.positive) { dt.emplace_back(); RGPU_TRY(make_dev_term(seg, *st, 0.0f, sim, &dt.back())); }
      for (const rgpu_term_state* st : P.negative) { dt.emplace_back(); RGPU_TRY(make_dev_term(seg, *st, 0.0f, sim, &dt.back())); }
      any_not = any_not || !P.negative.empty();
      const DevTerm& lead = dt[(size_t)dq[q].first_term];
      items += lead_items(lead, blocks_per_item);
      slots += lead_slots(lead);
    }
    item_prefix[nq] = items;
    emit_prefix[nq] = slots;
    if (items == 0) return RGPU_OK;
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_q = st.add<DevQuery>(nq);
    const auto r_t = st.add<DevTerm>(dt.size());
    const auto r_ip = st.add<int64_t>(nq + 1), r_ep = st.add<int64_t>(nq + 1);
    const auto r_rows = st.add<uint32_t*>(rows.size());
    STAGE_SIZED(sg, st);
    sg.put(r_q, dq);
    sg.put(r_t, dt);
    sg.put(r_ip, item_prefix);
    sg.put(r_ep, emit_prefix);
    sg.put(r_rows, rows);
    RGPU_TRY(sg.upload(stream));
    // (no clause bitmaps: every clause is walked; nothing is collected: k_emit 1, the narrowest kind of list)
    RGPU_TRY(and_emit_stage(seg, stream, AndEmitStage{"k_search_and(doc set candidates)", sg.dev(r_q), sg.dev(r_t), sg.dev(r_ip), sg.dev(r_ep), nullptr, n_queries, nq,
                                                      items, slots, blocks_per_item, 1, any_not, 0, 0}));
    if (slots > 0) {
      TimedLaunch tl(c, stream, "k_docset_from_emitted", 0);
      RGPU_LAUNCH(k_docset_from_emitted, dim3(wg_count(((unsigned long long)slots + DOCSET_THREADS - 1) / DOCSET_THREADS)), dim3(DOCSET_THREADS), 0, stream,
                  (const int32_t*)c->phrase_docs.p, (const int64_t*)sg.dev(r_ep), (const unsigned long long*)c->phrase_count.p, (int)n_queries, slots, seg->max_doc,
                  (uint32_t* const*)sg.dev(r_rows));
    }
    HIP_TRY(launch_status());
    HIP_TRY(scratch_mark(c, stream));
    return RGPU_OK;
  };
  int32_t rc = lists();
  if (rc == RGPU_OK) rc = conjunctions();
  for (int32_t q = 0; q < n_queries && rc == RGPU_OK; ++q) rc = docset_finish(sets[(size_t)q], stream);
  if (rc != RGPU_OK) return drop(rc);
  for (int32_t q = 0; q < n_queries; ++q) out_sets[q] = sets[(size_t)q];
  return RGPU_OK;
}

