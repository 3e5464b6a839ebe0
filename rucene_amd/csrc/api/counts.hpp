// Hit counts without scoring (IndexSearcher::count). Entry point: rgpu_count_batch.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, settle_pending,
// scratch_mark / SCRATCH_TAKE, Stager / STAGE_SIZED, seg_view, validate_state, prepare_terms_locked, make_dev_term, rgpu_sim_table_upload, bitmap_of,
// and_item_blocks), candidates.hpp (lead_items, lead_slots, AndEmitStage, and_emit_stage), docsets.hpp (rgpu_docset, docset_check), masked.hpp
// (docset_mask_locked), kernels/count.hpp, host/count_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- hit counts without scoring (include/rucene_gpu.h rgpu_count_batch; the plan: host/count_plan.hpp; the kernels:
// kernels/count.hpp) -----------------------------------------------------------------------------------------------------------------
// IndexSearcher::count (search/searcher.rs:632-654): counts[q] = the docs of `live AND set` row q matches in this leaf. Launch sequence:
//   term preparation as a search (only what is not prepared yet); a memset of the row counters;
//   k_count_lists     when some row is a LIST row
//   k_count_windows   when some row is a WINDOWS row (one launch: the bit or the counter form is a row's own)
//   k_search_and in emit mode (and_emit_stage, "k_search_and(count candidates)") + k_count_emitted   when some row is a CONJ row
//   one copy of the counters back; the call returns synchronised. A batch of ZERO and DOC_FREQ rows alone launches nothing.
extern "C" int32_t rgpu_count_batch(rgpu_segment* seg, rgpu_docset* set_or_null, const rgpu_query* queries, int32_t n_queries,
                                    const rgpu_query_term* terms, int32_t n_terms_total, int64_t* counts_out) {
  if (!seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !counts_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (set_or_null) RGPU_TRY(docset_check(seg, set_or_null));
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  // ---- plan: every refusal comes before anything is launched or written
  rgpu_host::CountMask cm;
  cm.deletions = seg->d_live != nullptr;
  cm.set = set_or_null != nullptr;
  cm.empty_set = set_or_null != nullptr && set_or_null->cardinality == 0;
  const size_t nq = (size_t)n_queries;
  std::vector<rgpu_host::CountRowPlan> plans(nq);
  std::vector<const rgpu_term_state*> ptrs;
  bool any_list = false, any_conj = false, any_windows = false;
  for (size_t q = 0; q < nq; ++q) {
    plans[q] = rgpu_host::plan_count_query(queries[q], terms, n_terms_total, cm);
    const rgpu_host::CountRowPlan& P = plans[q];
    if (P.status != RGPU_OK) return fail(P.status, P.why);
    for (const std::vector<rgpu_host::CountClause>* side : {&P.positive, &P.negative})
      for (const rgpu_host::CountClause& cl : *side) {
        RGPU_TRY(validate_state(seg, *cl.term));
        if (cl.term->doc_freq == 1 && (cl.term->singleton_doc_id < 0 || cl.term->singleton_doc_id >= seg->max_doc)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "singleton_doc_id out of range");
        ptrs.push_back(cl.term);
      }
    any_list = any_list || P.kind == rgpu_host::COUNT_LIST;
    any_conj = any_conj || P.kind == rgpu_host::COUNT_CONJ;
    any_windows = any_windows || P.kind == rgpu_host::COUNT_WINDOWS;
  }
  if (any_conj && c->n_sim_tables <= 0)
    return fail(RGPU_ERR_ILLEGAL_STATE, "counting a conjunction runs the search's conjunction kernel: upload a similarity table first (rgpu_sim_table_upload)");
  if (!any_list && !any_conj && !any_windows) {  // ZERO and DOC_FREQ rows alone: the host knows
    for (size_t q = 0; q < nq; ++q) counts_out[q] = plans[q].kind == rgpu_host::COUNT_DOC_FREQ ? plans[q].doc_freq : 0;
    return RGPU_OK;
  }
  RGPU_TRY(settle_pending(c));  // (a deferred batch's redo reads scratch this call is about to take)
  const uint64_t* mask64 = seg->d_live;
  if (set_or_null) RGPU_TRY(docset_mask_locked(seg, set_or_null, &mask64));
  const uint32_t* mask = reinterpret_cast<const uint32_t*>(mask64);
  // (a conjunction's lead is walked with its posting-order norms, as in a search; the other kernels need the blocks alone)
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size(), any_conj));
  HIP_TRY(c->count_rows.reserve(nq, 0, stream));
  HIP_TRY(hipMemsetAsync(c->count_rows.p, 0, nq * 8, stream));
  unsigned long long* const d_counts = c->count_rows.p;
  const SegView sv = seg_view(seg);
  const bool legacy = seg->version < 1;
  auto dev_term = [&](const rgpu_term_state& st, std::vector<DevTerm>& dt) -> int32_t {
    dt.emplace_back();
    RGPU_TRY(make_dev_term(seg, st, 0.0f, 0, &dt.back(), false));
    // (the items are sized from doc_freq; the prepared term must agree, or a wavefront would run past its blocks)
    if (dt.back().df >= 2 && dt.back().nblocks != dt.back().df / 128) return fail(RGPU_ERR_ILLEGAL_STATE, "internal: a prepared term disagrees with its doc_freq");
    return RGPU_OK;
  };
  auto lists = [&]() -> int32_t {  // ---- LIST rows
    if (!any_list) return RGPU_OK;
    std::vector<DevTerm> dt;
    std::vector<CountJob> jobs;
    std::vector<int64_t> prefix;
    int64_t items = 0, postings = 0;
    for (size_t q = 0; q < nq; ++q) {
      if (plans[q].kind != rgpu_host::COUNT_LIST) continue;
      const rgpu_term_state& st = *plans[q].positive[0].term;
      RGPU_TRY(dev_term(st, dt));
      jobs.push_back(CountJob{(uint32_t)(dt.size() - 1), (uint32_t)q});
      prefix.push_back(items);
      items += rgpu_host::docset_term_items(st.doc_freq, DOCSET_BLOCKS_PER_ITEM);
      postings += st.doc_freq;
    }
    prefix.push_back(items);
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_t = st.add<DevTerm>(dt.size());
    const auto r_j = st.add<CountJob>(jobs.size());
    const auto r_p = st.add<int64_t>(prefix.size());
    STAGE_SIZED(sg, st);
    sg.put(r_t, dt);
    sg.put(r_j, jobs);
    sg.put(r_p, prefix);
    RGPU_TRY(sg.upload(stream));
    {
      TimedLaunch tl(c, stream, "k_count_lists", postings);
      const unsigned grid = wg_count(((unsigned long long)items + COUNT_WAVES - 1) / COUNT_WAVES);
      if (legacy) RGPU_LAUNCH(k_count_lists<true>, dim3(grid), dim3(COUNT_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const CountJob*)sg.dev(r_j),
                              (const int64_t*)sg.dev(r_p), (int)jobs.size(), items, mask, d_counts);
      else RGPU_LAUNCH(k_count_lists<false>, dim3(grid), dim3(COUNT_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const CountJob*)sg.dev(r_j),
                       (const int64_t*)sg.dev(r_p), (int)jobs.size(), items, mask, d_counts);
    }
    HIP_TRY(launch_status());
    HIP_TRY(scratch_mark(c, stream));
    return RGPU_OK;
  };
  auto windows = [&]() -> int32_t {  // ---- WINDOWS rows
    if (!any_windows) return RGPU_OK;
    std::vector<DevTerm> dt;
    std::vector<CountRow> rows;
    std::vector<CountClauseDev> cls;
    int64_t postings = 0;
    for (size_t q = 0; q < nq; ++q) {
      const rgpu_host::CountRowPlan& P = plans[q];
      if (P.kind != rgpu_host::COUNT_WINDOWS) continue;
      rows.push_back(CountRow{(int32_t)cls.size(), (int32_t)P.positive.size(), (int32_t)P.negative.size(), P.need, P.need_not, (int32_t)q});
      for (const std::vector<rgpu_host::CountClause>* side : {&P.positive, &P.negative})
        for (const rgpu_host::CountClause& cl : *side) {
          RGPU_TRY(dev_term(*cl.term, dt));
          // a doc bitmap some search has built already is read in the bit form; this call builds none (that takes a similarity table)
          const TermBitmap bm = P.bit_form() ? bitmap_of(seg, dt.back()) : NO_BITMAP;
          cls.push_back(CountClauseDev{(uint32_t)(dt.size() - 1), (uint32_t)cl.mult, bm.words != nullptr ? bm.memb : nullptr});
          postings += cl.term->doc_freq;
        }
    }
    const int32_t per_item = rgpu_host::count_windows_per_item(seg->max_doc, COUNT_WINDOW_DOCS, (int64_t)rows.size(), 8192, c->count_windows_per_item);
    const int64_t items_per_row = rgpu_host::count_window_items(seg->max_doc, COUNT_WINDOW_DOCS, per_item);
    if (items_per_row <= 0) return RGPU_OK;  // (a segment without docs)
    if (items_per_row > 0x7fffffff) return fail(RGPU_ERR_ILLEGAL_STATE, "internal: window items per row");
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_t = st.add<DevTerm>(dt.size());
    const auto r_r = st.add<CountRow>(rows.size());
    const auto r_c = st.add<CountClauseDev>(cls.size());
    STAGE_SIZED(sg, st);
    sg.put(r_t, dt);
    sg.put(r_r, rows);
    sg.put(r_c, cls);
    RGPU_TRY(sg.upload(stream));
    {
      TimedLaunch tl(c, stream, "k_count_windows", postings);
      const int64_t items = (int64_t)rows.size() * items_per_row;
      const unsigned grid = wg_count(((unsigned long long)items + COUNT_WAVES - 1) / COUNT_WAVES);
      if (legacy) RGPU_LAUNCH(k_count_windows<true>, dim3(grid), dim3(COUNT_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const CountRow*)sg.dev(r_r),
                              (const CountClauseDev*)sg.dev(r_c), (int)rows.size(), (int)items_per_row, (int)per_item, mask, d_counts);
      else RGPU_LAUNCH(k_count_windows<false>, dim3(grid), dim3(COUNT_THREADS), 0, stream, sv, (const DevTerm*)sg.dev(r_t), (const CountRow*)sg.dev(r_r),
                       (const CountClauseDev*)sg.dev(r_c), (int)rows.size(), (int)items_per_row, (int)per_item, mask, d_counts);
    }
    HIP_TRY(launch_status());
    HIP_TRY(scratch_mark(c, stream));
    return RGPU_OK;
  };
  auto conjunctions = [&]() -> int32_t {  // ---- CONJ rows: k_search_and emits the matches (deleted docs marked), counted against the mask
    if (!any_conj) return RGPU_OK;
    std::vector<DevQuery> dq(nq, DevQuery{RGPU_OP_AND, 0, 0, 0});
    std::vector<DevTerm> dt;
    std::vector<int64_t> item_prefix(nq + 1), emit_prefix(nq + 1);
    int64_t lead_blocks = 0;
    for (const rgpu_host::CountRowPlan& P : plans) if (P.kind == rgpu_host::COUNT_CONJ) lead_blocks += P.positive[0].term->doc_freq / 128;
    const int blocks_per_item = and_item_blocks(c, lead_blocks);
    int64_t items = 0, slots = 0;
    bool any_not = false;
    for (size_t q = 0; q < nq; ++q) {
      const rgpu_host::CountRowPlan& P = plans[q];
      item_prefix[q] = items;
      emit_prefix[q] = slots;
      dq[q].first_term = (int32_t)dt.size();
      if (P.kind != rgpu_host::COUNT_CONJ) continue;
      int32_t sim = terms[queries[q].first_term].sim_table;  // (an emitting conjunction loads its lead's table and scores nothing)
      if (sim < 0 || sim >= c->n_sim_tables) sim = 0;
      dq[q] = DevQuery{RGPU_OP_AND, (int32_t)P.positive.size(), (int32_t)dt.size(), (int32_t)P.negative.size()};
      for (const std::vector<rgpu_host::CountClause>* side : {&P.positive, &P.negative})
        for (const rgpu_host::CountClause& cl : *side) { dt.emplace_back(); RGPU_TRY(make_dev_term(seg, *cl.term, 0.0f, sim, &dt.back())); }
      any_not = any_not || !P.negative.empty();
      const DevTerm& lead = dt[(size_t)dq[q].first_term];
      items += lead_items(lead, blocks_per_item);
      slots += lead_slots(lead);
    }
    item_prefix[nq] = items;
    emit_prefix[nq] = slots;
    if (items == 0 || slots == 0) return RGPU_OK;
    SCRATCH_TAKE(c);
    Stager st(c);
    const auto r_q = st.add<DevQuery>(nq);
    const auto r_t = st.add<DevTerm>(dt.size());
    const auto r_ip = st.add<int64_t>(nq + 1), r_ep = st.add<int64_t>(nq + 1);
    STAGE_SIZED(sg, st);
    sg.put(r_q, dq);
    sg.put(r_t, dt);
    sg.put(r_ip, item_prefix);
    sg.put(r_ep, emit_prefix);
    RGPU_TRY(sg.upload(stream));
    // (no clause bitmaps: every clause is walked; nothing is collected: k_emit 1, the narrowest kind of list)
    RGPU_TRY(and_emit_stage(seg, stream, AndEmitStage{"k_search_and(count candidates)", sg.dev(r_q), sg.dev(r_t), sg.dev(r_ip), sg.dev(r_ep), nullptr, n_queries, nq,
                                                      items, slots, blocks_per_item, 1, any_not, 0, 0}));
    {
      TimedLaunch tl(c, stream, "k_count_emitted", 0);
      RGPU_LAUNCH(k_count_emitted, dim3(wg_count(((unsigned long long)slots + COUNT_THREADS - 1) / COUNT_THREADS)), dim3(COUNT_THREADS), 0, stream,
                  (const int32_t*)c->phrase_docs.p, (const int64_t*)sg.dev(r_ep), (const unsigned long long*)c->phrase_count.p, (int)n_queries, slots, seg->max_doc,
                  mask, d_counts);
    }
    HIP_TRY(launch_status());
    HIP_TRY(scratch_mark(c, stream));
    return RGPU_OK;
  };
  std::vector<unsigned long long> got(nq, 0ull);
  auto run = [&]() -> int32_t {
    RGPU_TRY(lists());
    RGPU_TRY(windows());
    RGPU_TRY(conjunctions());
    HIP_TRY(hipMemcpyAsync(got.data(), d_counts, nq * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RGPU_OK;
  };
  const int32_t rc = run();
  if (rc != RGPU_OK) { (void)hipStreamSynchronize(stream); return rc; }
  for (size_t q = 0; q < nq; ++q) {
    const rgpu_host::CountRowPlan& P = plans[q];
    counts_out[q] = P.kind == rgpu_host::COUNT_ZERO ? 0 : P.kind == rgpu_host::COUNT_DOC_FREQ ? P.doc_freq : (int64_t)got[q];
  }
  return RGPU_OK;
}

