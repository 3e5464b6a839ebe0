// Masked search: a doc set as the FILTER / MUST_NOT mask of a call. docset_mask_locked, MaskScope, docset_mark_in_flight; for the masked phrase
// calls PhraseMask, masked_stage_name, refuse_sloppy_masked. Entry points: rgpu_search_batch_device_masked, rgpu_search_batch_masked.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, HIP_TRY / RGPU_TRY, settle_pending, search_impl), rows.hpp (search_batch_host_locked),
// docsets.hpp (rgpu_docset, docset_alloc_bytes, docset_combine_launch, docset_check).
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- masked search -----------------------------------------------------------------------------------------------------------------
// The mask of a masked call: the set itself when the segment has no deletions, else `live AND set`, formed by k_docset_combine the
// first time the set is used and kept (segments are immutable). Ends synchronised when it forms one, so that any stream may read it.
static int32_t docset_mask_locked(rgpu_segment* seg, rgpu_docset* set, const uint64_t** mask_out) {
  if (!seg->d_live) { *mask_out = set->d_words; return RGPU_OK; }
  if (!set->d_mask) {
    rgpu_ctx* c = seg->ctx;
    uint64_t* m = nullptr;
    HIP_TRY(hipMalloc(&m, docset_alloc_bytes(set->n_words)));
    const uint64_t* self[1] = {set->d_words};
    int32_t rc = hipMemsetAsync(m, 0, docset_alloc_bytes(set->n_words), c->stream) == hipSuccess ? RGPU_OK : fail(RGPU_ERR_RUNTIME, "memset of a doc set's mask failed");
    if (rc == RGPU_OK) rc = docset_combine_launch(c, c->stream, set->max_doc, self, 1, nullptr, 0, seg->d_live, m, set->d_count + 1);
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == RGPU_OK) rc = fail(RGPU_ERR_RUNTIME, "forming a doc set's mask failed");
    if (rc != RGPU_OK) { (void)hipFree(m); return rc; }
    set->d_mask = m;
  }
  *mask_out = set->d_mask;
  return RGPU_OK;
}
// installs the mask for the rest of the scope. Before it: closures pending from earlier (unmasked, or differently masked) calls are
// settled — a redo they launch reads the segment's live docs as they were when the batch was enqueued. Inside it nothing is deferred
// (the entry points leave defer_or false), so no closure of a masked call ever runs outside its scope.
struct MaskScope {
  rgpu_segment* seg;
  MaskScope(rgpu_segment* s, const uint64_t* mask) : seg(s) { seg->call_mask = mask; }
  ~MaskScope() { seg->call_mask = nullptr; }
};
// one event per masked call behind its work on `s`: rgpu_docset_free waits for them (events seen finished are recycled here)
static void docset_mark_in_flight(rgpu_docset* set, hipStream_t s) {
  size_t kept = 0;
  hipEvent_t ev = nullptr;
  for (hipEvent_t e : set->in_flight) {
    if (hipEventQuery(e) == hipSuccess) { if (!ev) ev = e; else (void)hipEventDestroy(e); }
    else set->in_flight[kept++] = e;
  }
  (void)hipGetLastError();  // (hipErrorNotReady of the queries is not an error)
  set->in_flight.resize(kept);
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipStreamSynchronize(s); return; }
  if (hipEventRecord(ev, s) == hipSuccess) set->in_flight.push_back(ev);
  else { (void)hipEventDestroy(ev); (void)hipStreamSynchronize(s); }
}

// The masked exact-phrase calls (rgpu_search_phrase_batch_masked, _phrase_bool_batch_masked, _phrase_or_batch_masked): what each does
// under the context's mutex before its first launch - closures pending from earlier calls settled, `live AND set` formed (once, kept)
// and installed for the rest of the call. `set` null: the unmasked call, nothing happens. The caller has refused sloppy phrases
// already: an exact phrase under a mask is the phrase on a leaf whose live docs are the mask, a sloppy one is not (next_limit counts
// deleted docs, not docs outside the filter).
struct PhraseMask {
  rgpu_segment* seg = nullptr;
  rgpu_docset* set = nullptr;
  ~PhraseMask() { if (seg) { seg->call_mask = nullptr; docset_mark_in_flight(set, seg->ctx->stream); } }
  int32_t install(rgpu_segment* s, rgpu_docset* d) {
    if (!d) return RGPU_OK;
    rgpu_ctx* c = s->ctx;
    RGPU_TRY(settle_pending(c));
    const uint64_t* mask = nullptr;
    RGPU_TRY(docset_mask_locked(s, d, &mask));
    c->defer_or = false;  // a masked call never defers
    s->call_mask = mask;
    seg = s;
    set = d;
    return RGPU_OK;
  }
  bool on() const { return seg != nullptr; }
};
// the launch names of the candidate stage under a mask: the compacting instantiation's own, the marking one's own (RGPU_PHRASE_MASK_COMPACT=0);
// rgpu_kernel_stat::name holds 47 characters
static const char* masked_stage_name(const rgpu_ctx* c, const char* compact, const char* marked) { return c->phrase_mask_compact ? compact : marked; }
static int32_t refuse_sloppy_masked(const rgpu_phrase_query* phrases, int32_t n) {
  for (int32_t i = 0; i < n; ++i)
    if (phrases[i].slop > 0) return fail(RGPU_ERR_UNSUPPORTED, "a sloppy phrase under a doc set is not served: next_limit counts deleted docs, not docs outside the filter");
  return RGPU_OK;
}

extern "C" int32_t rgpu_search_batch_device_masked(rgpu_segment* seg, rgpu_docset* set, const rgpu_query* queries, int32_t n_queries,
                                                   const rgpu_query_term* terms, int32_t n_terms_total, int32_t k, void* hits_dev,
                                                   void* totals_dev, void* hip_stream) {
  if (!seg || !set || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !hits_dev || !totals_dev)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  RGPU_TRY(docset_check(seg, set));
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
  RGPU_TRY(settle_pending(c));
  const uint64_t* mask = nullptr;
  RGPU_TRY(docset_mask_locked(seg, set, &mask));
  c->defer_or = false;  // a masked call never defers: its redo would run later, outside the scope
  int32_t rc;
  {
    MaskScope scope(seg, mask);
    rc = search_impl(seg, queries, n_queries, terms, n_terms_total, k, (HitOut*)hits_dev, (int64_t*)totals_dev, s);
  }
  docset_mark_in_flight(set, s);
  return rc;
}

extern "C" int32_t rgpu_search_batch_masked(rgpu_segment* seg, rgpu_docset* set, const rgpu_query* queries, int32_t n_queries,
                                            const rgpu_query_term* terms, int32_t n_terms_total, int32_t k, rgpu_hit* hits_out,
                                            int64_t* total_hits_out) {
  if (!seg || !set || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !hits_out || !total_hits_out)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  RGPU_TRY(docset_check(seg, set));
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  RGPU_TRY(settle_pending(c));
  const uint64_t* mask = nullptr;
  RGPU_TRY(docset_mask_locked(seg, set, &mask));
  c->defer_or = false;
  MaskScope scope(seg, mask);
  return search_batch_host_locked(seg, queries, n_queries, terms, n_terms_total, k, hits_out, total_hits_out);
}

