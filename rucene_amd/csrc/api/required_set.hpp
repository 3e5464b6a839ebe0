// A doc set as the only required clause of a query: "b c #F", a lone #F, *:*. docset_head_locked, RequiredSetRows, required_set_rows,
// required_set_search_locked. Entry points: rgpu_docset_head, rgpu_search_batch_device_required_set, rgpu_search_batch_required_set,
// rgpu_merge_topk_device.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, settle_pending,
// search_impl), rows.hpp (api_rows_read_back), docsets.hpp (rgpu_docset, docset_head_alloc_bytes, docset_check), masked.hpp (docset_mask_locked,
// MaskScope, docset_mark_in_flight), kernels/docset.hpp.
// Left where the single file had it: rgpu_merge_topk_device, the merge of several leaves' device-side rows, closes this part though it serves
// every enqueue-only call.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- a doc set as the only required clause: "b c #F", a lone #F, *:* (include/rucene_gpu.h rgpu_docset_head,
// rgpu_search_batch_required_set; the kernels: kernels/docset.hpp) -------------------------------------------------------------------
// Launch sequences:
//   head (first use of a set, or a larger n than before)   [k_docset_combine: live AND set, as a masked search] k_docset_chunk_counts,
//                                                          k_docset_head_scan, k_docset_select_head (n > 0 and M not empty)
//   rgpu_search_batch[_device]_required_set                [head] the masked search of the rows that have SHOULD clauses (k_init_hits
//                                                          alone when none has), k_required_set_fill
// The head of M = live AND set for at least n docs: |M| and the first min(n, |M|) docs, kept with the set. Ends synchronised when it
// builds (any stream may read the head afterwards); a head that is replaced waits for the searches in flight that read the old one.
static int32_t docset_head_locked(rgpu_segment* seg, rgpu_docset* set, int32_t n, const uint64_t* mask) {
  if (set->head_n >= 0 && ((int64_t)set->head_n >= (int64_t)n || (int64_t)set->head_n >= set->live_cardinality)) return RGPU_OK;
  rgpu_ctx* c = seg->ctx;
  hipStream_t stream = c->stream;
  const int64_t n_words = (int64_t)set->n_words;
  const int64_t n_chunks = (n_words + DOCSET_HEAD_CHUNK_WORDS - 1) / DOCSET_HEAD_CHUNK_WORDS;
  int32_t* head = nullptr;
  uint8_t* work = nullptr;  // [n_chunks] i64 prefix, i64 total, [n_chunks] i32 counts
  const size_t o_total = (size_t)n_chunks * 8, o_counts = o_total + 8, work_bytes = o_counts + (size_t)n_chunks * 4;
  long long total = 0;
  auto run = [&]() -> int32_t {
    HIP_TRY(hipMalloc(&head, docset_head_alloc_bytes(n)));
    if (n_chunks == 0) return RGPU_OK;
    HIP_TRY(hipMalloc(&work, work_bytes));
    long long* d_prefix = reinterpret_cast<long long*>(work);
    long long* d_total = reinterpret_cast<long long*>(work + o_total);
    int* d_counts = reinterpret_cast<int*>(work + o_counts);
    {
      TimedLaunch tl(c, stream, "k_docset_chunk_counts", 0);
      RGPU_LAUNCH(k_docset_chunk_counts, dim3((unsigned)n_chunks), dim3(DOCSET_THREADS), 0, stream, mask, n_words, d_counts);
    }
    {
      TimedLaunch tl(c, stream, "k_docset_head_scan", 0);
      RGPU_LAUNCH(k_docset_head_scan, dim3(1), dim3(64), 0, stream, (const int*)d_counts, (int)n_chunks, d_prefix, d_total);
    }
    if (n > 0) {  // (a chunk whose prefix is at or past n, an empty M among them, returns at once)
      TimedLaunch tl(c, stream, "k_docset_select_head", 0);
      RGPU_LAUNCH(k_docset_select_head, dim3((unsigned)n_chunks), dim3(DOCSET_THREADS), 0, stream, mask, n_words, (const long long*)d_prefix, (int)n, head);
    }
    HIP_TRY(launch_status());
    HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RGPU_OK;
  };
  const int32_t rc = run();
  if (rc != RGPU_OK) (void)hipStreamSynchronize(stream);
  if (work) (void)hipFree(work);
  if (rc != RGPU_OK) { if (head) (void)hipFree(head); return rc; }
  if (set->d_head) {  // searches enqueued on other streams may still read the old head
    for (hipEvent_t ev : set->in_flight) (void)hipEventSynchronize(ev);
    (void)hipFree(set->d_head);
  }
  set->d_head = head;
  set->head_n = n;
  set->live_cardinality = (int64_t)total;
  return RGPU_OK;
}

extern "C" int32_t rgpu_docset_head(rgpu_segment* seg, rgpu_docset* set, int32_t n, int32_t* docs_out, int32_t* n_out, int64_t* live_cardinality_out) {
  if (!seg || !set || !n_out || !live_cardinality_out || n < 0 || (n > 0 && !docs_out)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (n > RGPU_MAX_K) return fail(RGPU_ERR_UNSUPPORTED, "a doc set's head holds at most RGPU_MAX_K docs");
  RGPU_TRY(docset_check(seg, set));
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t* mask = nullptr;
  RGPU_TRY(docset_mask_locked(seg, set, &mask));
  RGPU_TRY(docset_head_locked(seg, set, n, mask));
  const int32_t m = (int32_t)std::min<int64_t>(n, set->live_cardinality);
  if (m > 0) HIP_TRY(hipMemcpy(docs_out, set->d_head, (size_t)m * 4, hipMemcpyDeviceToHost));
  *n_out = m;
  *live_cardinality_out = set->live_cardinality;
  return RGPU_OK;
}

// The rows rgpu_search_batch_required_set accepts, as the masked search takes them: msm bytes cleared (ReqOptScorer only advance()s
// the optional scorer), a row without an optional side as a TERM query of an absent term (appended to the clauses), which launches
// nothing and leaves the row's defaults. `scored`: rows that have SHOULD clauses.
struct RequiredSetRows {
  std::vector<rgpu_query> queries;
  std::vector<rgpu_query_term> terms;
  int32_t scored = 0;
};
static int32_t required_set_rows(const rgpu_ctx* c, const rgpu_query* queries, int32_t n_queries, const rgpu_query_term* terms, int32_t n_terms_total,
                                 RequiredSetRows* out) {
  out->queries.assign(queries, queries + n_queries);
  bool any_empty = false;
  for (int32_t q = 0; q < n_queries; ++q) {
    rgpu_query& Q = out->queries[(size_t)q];
    const int qop = Q.op & 0xff;
    if (qop < RGPU_OP_TERM || qop > RGPU_OP_DISMAX) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "unknown query op");
    if (qop != RGPU_OP_TERM && qop != RGPU_OP_OR) return fail(RGPU_ERR_UNSUPPORTED, "beside a required doc set: RGPU_OP_TERM or a flat RGPU_OP_OR (the SHOULD clauses)");
    if ((Q.op & ~0xffff) != 0) return fail(RGPU_ERR_UNSUPPORTED, "beside a required doc set: no RGPU_OP_WITH_SHOULD, nested or required-SHOULD flags");
    if (Q.n_must_not != 0) return fail(RGPU_ERR_UNSUPPORTED, "beside a required doc set: no MUST_NOT or demoting clauses (fold MUST_NOT terms into the set)");
    Q.op = qop;  // the msm byte has no effect
    if (Q.n_terms < 0 || Q.n_terms > RGPU_MAX_QUERY_TERMS || (qop == RGPU_OP_TERM && Q.n_terms != 1)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad clause count");
    if (Q.n_terms == 0) { any_empty = true; continue; }
    if (!terms || Q.first_term < 0 || (int64_t)Q.first_term + Q.n_terms > (int64_t)n_terms_total) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "clause range outside terms[]");
    for (int i = 0; i < Q.n_terms; ++i) {
      const float w = terms[Q.first_term + i].weight;
      // a score of 0 in O would tie with the fill: a full row could hide zero-score docs with lower ids
      if (!(std::isfinite(w) && w > 0.0f)) return fail(RGPU_ERR_UNSUPPORTED, "beside a required doc set a SHOULD clause's weight is finite and > 0");
    }
    ++out->scored;
  }
  if (out->scored > 0 && any_empty) {
    if (c->n_sim_tables <= 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "unknown sim_table handle");
    out->terms.assign(terms, terms + n_terms_total);
    rgpu_query_term absent;
    std::memset(&absent, 0, sizeof absent);
    absent.state.skip_offset = -1;
    absent.state.singleton_doc_id = -1;
    out->terms.push_back(absent);
    for (rgpu_query& Q : out->queries)
      if (Q.n_terms == 0) Q = rgpu_query{RGPU_OP_TERM, 1, n_terms_total, 0};
  }
  return RGPU_OK;
}
// mask installed by the caller's scope; rows to device memory, the fill enqueued behind the search on `s`
static int32_t required_set_search_locked(rgpu_segment* seg, rgpu_docset* set, const RequiredSetRows& R, const rgpu_query_term* terms, int32_t n_terms_total,
                                          int32_t k, HitOut* hits_dev, int64_t* totals_dev, hipStream_t s) {
  rgpu_ctx* c = seg->ctx;
  const int32_t n_queries = (int32_t)R.queries.size();
  if (R.scored > 0) {
    const bool own = !R.terms.empty();
    RGPU_TRY(search_impl(seg, R.queries.data(), n_queries, own ? R.terms.data() : terms, own ? (int32_t)R.terms.size() : n_terms_total, k, hits_dev, totals_dev, s));
  } else {
    RGPU_LAUNCH(k_init_hits, dim3(wg_count(((size_t)n_queries * k + 255) / 256)), dim3(256), 0, s, hits_dev, (int64_t)n_queries, (int)k, (int)k, 0);
  }
  {
    TimedLaunch tl(c, s, "k_required_set_fill", 0);
    RGPU_LAUNCH(k_required_set_fill, dim3(wg_count(((unsigned long long)n_queries + REQUIRED_SET_FILL_WAVES - 1) / REQUIRED_SET_FILL_WAVES)),
                dim3(64 * REQUIRED_SET_FILL_WAVES), 0, s, hits_dev, totals_dev, (int)n_queries, (int)k, (const int32_t*)set->d_head,
                (int)std::min<int64_t>(std::min<int64_t>(set->head_n, set->live_cardinality), k), set->live_cardinality, seg->doc_base);
  }
  HIP_TRY(launch_status());
  return RGPU_OK;
}
static_assert(REQUIRED_SET_MAX_HEAD == RGPU_MAX_K && DOCSET_HEAD_CHUNK_WORDS == RGPU_DOCSET_HEAD_CHUNK_WORDS, "kernels/docset.hpp follows include/rucene_gpu.h");

extern "C" int32_t rgpu_search_batch_device_required_set(rgpu_segment* seg, rgpu_docset* set, const rgpu_query* queries, int32_t n_queries,
                                                         const rgpu_query_term* terms, int32_t n_terms_total, int32_t k, void* hits_dev,
                                                         void* totals_dev, void* hip_stream) {
  if (!seg || !set || !queries || n_queries <= 0 || n_terms_total < 0 || !hits_dev || !totals_dev) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  RGPU_TRY(docset_check(seg, set));
  rgpu_ctx* c = seg->ctx;
  RequiredSetRows R;
  RGPU_TRY(required_set_rows(c, queries, n_queries, terms, n_terms_total, &R));
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
  RGPU_TRY(settle_pending(c));
  const uint64_t* mask = nullptr;
  RGPU_TRY(docset_mask_locked(seg, set, &mask));
  RGPU_TRY(docset_head_locked(seg, set, k, mask));
  c->defer_or = false;  // never defers, as a masked call
  int32_t rc;
  {
    MaskScope scope(seg, mask);
    rc = required_set_search_locked(seg, set, R, terms, n_terms_total, k, (HitOut*)hits_dev, (int64_t*)totals_dev, s);
  }
  docset_mark_in_flight(set, s);
  return rc;
}

extern "C" int32_t rgpu_search_batch_required_set(rgpu_segment* seg, rgpu_docset* set, const rgpu_query* queries, int32_t n_queries,
                                                  const rgpu_query_term* terms, int32_t n_terms_total, int32_t k, rgpu_hit* hits_out,
                                                  int64_t* total_hits_out) {
  if (!seg || !set || !queries || n_queries <= 0 || n_terms_total < 0 || !hits_out || !total_hits_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  RGPU_TRY(docset_check(seg, set));
  rgpu_ctx* c = seg->ctx;
  RequiredSetRows R;
  RGPU_TRY(required_set_rows(c, queries, n_queries, terms, n_terms_total, &R));
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  RGPU_TRY(settle_pending(c));
  const uint64_t* mask = nullptr;
  RGPU_TRY(docset_mask_locked(seg, set, &mask));
  RGPU_TRY(docset_head_locked(seg, set, k, mask));
  c->defer_or = false;
  HIP_TRY(c->host_api_hits.reserve((size_t)n_queries * (size_t)k, 0, c->stream));
  HIP_TRY(c->host_api_totals.reserve((size_t)n_queries, 0, c->stream));
  {
    MaskScope scope(seg, mask);
    RGPU_TRY(required_set_search_locked(seg, set, R, terms, n_terms_total, k, c->host_api_hits.p, c->host_api_totals.p, c->stream));
  }
  return api_rows_read_back(c, c->stream, n_queries, k, hits_out, total_hits_out);
}

extern "C" int32_t rgpu_merge_topk_device(rgpu_ctx* c, const void* hits_dev, const void* totals_dev, int32_t n_lists, int32_t n_queries,
                                          int32_t k, void* hits_out_dev, void* totals_out_dev, void* hip_stream) {
  if (!c || !hits_dev || !totals_dev || !hits_out_dev || !totals_out_dev || n_lists <= 0 || n_queries <= 0)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
  {
    TimedLaunch tl(c, s, "k_merge_lists", 0);
    const unsigned grid = wg_count((n_queries + WG_WAVES - 1) / WG_WAVES);
    if (k > 64)
      RGPU_LAUNCH(k_merge_lists<true>, dim3(grid), dim3(WG_THREADS), 0, s, (const HitOut*)hits_dev, (const int64_t*)totals_dev,
                         (int64_t)n_queries * k, (int64_t)n_queries, n_lists, n_queries, k, (HitOut*)hits_out_dev, (int64_t*)totals_out_dev);
    else
      RGPU_LAUNCH(k_merge_lists<false>, dim3(grid), dim3(WG_THREADS), 0, s, (const HitOut*)hits_dev, (const int64_t*)totals_dev,
                         (int64_t)n_queries * k, (int64_t)n_queries, n_lists, n_queries, k, (HitOut*)hits_out_dev, (int64_t*)totals_out_dev);
  }
  HIP_TRY(launch_status());
  return RGPU_OK;  // enqueue only, like rgpu_search_batch_device
}

