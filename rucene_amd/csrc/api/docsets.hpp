// Doc sets: cached filters, one bit per doc of a leaf. rgpu_docset, docset_head_alloc_bytes / docset_alloc_bytes, docset_new / _delete /
// _combine_launch / _finish / _check. Entry points: rgpu_docset_from_words, rgpu_docset_from_docs, rgpu_docset_combine,
// rgpu_docset_cardinality, rgpu_docset_bytes, rgpu_docset_words, rgpu_docset_free.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count),
// kernels/docset.hpp, host/docset_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- doc sets: cached filters as FILTER / MUST_NOT masks (include/rucene_gpu.h rgpu_docset_*; the plan: host/docset_plan.hpp; the
// kernels: kernels/docset.hpp) -----------------------------------------------------------------------------------------------------
// Every constructor ends synchronised on the context's stream, so a finished set can be read from any stream without an event. A
// masked search installs `live AND set` as the segment's live docs for the duration of the call (MaskScope, under ctx->mu): the
// kernels take SegView by value, and every host decision asks live_words(). Launch sequences:
//   from_words        copy, k_docset_combine (the count)
//   from_docs         copy, k_docset_from_docs, k_docset_combine (the count)
//   collect_batch     term preparation as a search; k_docset_lists<set>, k_docset_lists<clear> for TERM / OR rows; k_search_and in
//                     emit mode (MUST_NOT clauses through its HAS_NOT instantiation) and k_docset_from_emitted for AND rows; one
//                     k_docset_combine per row (the count)
//   combine           k_docset_combine, once per DOCSET_MAX_OPERANDS operands of a side
//   masked search     first use of a set on a segment with deletions: k_docset_combine (live AND set), kept; then the search
struct rgpu_docset {
  rgpu_ctx* ctx = nullptr;
  uint64_t seg_uid = 0;
  int32_t max_doc = 0;
  size_t n_words = 0;
  uint64_t* d_words = nullptr;           // n_words u64 (the allocation is never empty)
  uint64_t* d_mask = nullptr;            // live AND set: formed by the first masked search when the segment has deletions
  unsigned long long* d_count = nullptr; // [0]: cardinality (k_docset_combine), [1]: ids out of range (k_docset_from_docs) / a count nobody reads; 4 words
  int64_t cardinality = 0;
  // the head of `live AND set` (rgpu_docset_head, rgpu_search_batch_required_set): its first min(head_n, live_cardinality) docs,
  // built for the largest n asked for so far; sets and live docs are immutable, so nothing ever invalidates it
  int32_t* d_head = nullptr;
  int32_t head_n = -1;                   // -1: never built
  int64_t live_cardinality = 0;          // |live AND set|, known once a head is built
  std::vector<hipEvent_t> in_flight;     // one per masked search enqueued and not yet seen finished
};

static size_t docset_head_alloc_bytes(int32_t n) { return std::max<size_t>(256, (size_t)std::max<int32_t>(n, 0) * 4); }
static size_t docset_alloc_bytes(size_t n_words) { return std::max<size_t>(16, (n_words * 8 + 15) & ~size_t(15)); }

static int32_t docset_new(rgpu_segment* seg, rgpu_docset** out, bool zeroed = true) {  // !zeroed: every word gets written by its builder
  rgpu_docset* d = new rgpu_docset();
  d->ctx = seg->ctx;
  d->seg_uid = seg->uid;
  d->max_doc = seg->max_doc;
  d->n_words = (size_t)rgpu_host::docset_word_count(seg->max_doc);
  hipError_t e = hipMalloc(&d->d_words, docset_alloc_bytes(d->n_words));
  if (e == hipSuccess) e = hipMalloc(&d->d_count, 32);
  // (!zeroed: the builder writes the n_words words; the padding of an odd count is zeroed all the same — no byte of a set is ever undefined)
  if (e == hipSuccess) {
    const size_t from = zeroed ? 0 : d->n_words * 8, bytes = docset_alloc_bytes(d->n_words);
    if (from < bytes) e = hipMemsetAsync(reinterpret_cast<uint8_t*>(d->d_words) + from, 0, bytes - from, seg->ctx->stream);
  }
  if (e != hipSuccess) {
    if (d->d_words) (void)hipFree(d->d_words);
    if (d->d_count) (void)hipFree(d->d_count);
    delete d;
    return fail(RGPU_ERR_RUNTIME, std::string("doc set allocation: ") + hipGetErrorString(e));
  }
  *out = d;
  return RGPU_OK;
}
static void docset_delete(rgpu_docset* d) {
  if (!d) return;
  for (hipEvent_t ev : d->in_flight) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
  if (d->d_words) (void)hipFree(d->d_words);
  if (d->d_mask) (void)hipFree(d->d_mask);
  if (d->d_head) (void)hipFree(d->d_head);
  if (d->d_count) (void)hipFree(d->d_count);
  delete d;
}

// out = AND all_of, minus every none_of, inside [0, max_doc) [AND live]; *d_count += its cardinality. Enqueue-only.
static int32_t docset_combine_launch(rgpu_ctx* c, hipStream_t stream, int32_t max_doc, const uint64_t* const* all_of, int32_t n_all,
                                     const uint64_t* const* none_of, int32_t n_none, const uint64_t* live, uint64_t* out,
                                     unsigned long long* d_count) {
  HIP_TRY(hipMemsetAsync(d_count, 0, 8, stream));
  const int64_t n_words = rgpu_host::docset_word_count(max_doc);
  if (n_words == 0) return RGPU_OK;
  const unsigned grid = wg_count(((unsigned long long)(n_words + 1) / 2 + DOCSET_THREADS - 1) / DOCSET_THREADS);
  int32_t a = 0, x = 0;
  bool first = true;
  while (first || a < n_all || x < n_none) {  // rounds of DOCSET_MAX_OPERANDS per side; later rounds start from what the earlier ones left
    DocsetCombineArgs args;
    std::memset(&args, 0, sizeof args);
    args.max_doc = max_doc;
    if (!first) args.all_of[args.n_all++] = out;
    while (a < n_all && args.n_all < DOCSET_MAX_OPERANDS) args.all_of[args.n_all++] = all_of[a++];
    while (x < n_none && args.n_none < DOCSET_MAX_OPERANDS) args.none_of[args.n_none++] = none_of[x++];
    const bool last = a >= n_all && x >= n_none;
    args.live = last ? live : nullptr;
    if (!last) HIP_TRY(hipMemsetAsync(d_count, 0, 8, stream));
    TimedLaunch tl(c, stream, "k_docset_combine", 0);
    RGPU_LAUNCH(k_docset_combine, dim3(grid), dim3(DOCSET_THREADS), 0, stream, args, out, last ? d_count : d_count + 1);
    first = false;
  }
  HIP_TRY(launch_status());
  return RGPU_OK;
}
// the bits past max_doc cleared (there are none unless a caller's words had some: refused before), the set counted; ends synchronised
static int32_t docset_finish(rgpu_docset* d, hipStream_t stream) {
  const uint64_t* self[1] = {d->d_words};
  RGPU_TRY(docset_combine_launch(d->ctx, stream, d->max_doc, self, 1, nullptr, 0, nullptr, d->d_words, d->d_count));
  unsigned long long n = 0;
  HIP_TRY(hipMemcpyAsync(&n, d->d_count, 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  d->cardinality = (int64_t)n;
  return RGPU_OK;
}
static int32_t docset_check(const rgpu_segment* seg, const rgpu_docset* set) {
  if (set->seg_uid != seg->uid || set->ctx != seg->ctx) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "the doc set belongs to another segment");
  return RGPU_OK;
}

extern "C" int32_t rgpu_docset_from_words(rgpu_segment* seg, const uint64_t* words, rgpu_docset** out_set) {
  if (!seg || !out_set || (!words && seg->max_doc > 0)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  *out_set = nullptr;
  if (!rgpu_host::docset_words_valid(words, seg->max_doc)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a bit at or past max_doc is set");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  rgpu_docset* d = nullptr;
  RGPU_TRY(docset_new(seg, &d));
  int32_t rc = RGPU_OK;
  if (d->n_words > 0 && hipMemcpyAsync(d->d_words, words, d->n_words * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    rc = fail(RGPU_ERR_RUNTIME, "copy of the doc set's words failed");
  if (rc == RGPU_OK) rc = docset_finish(d, c->stream);
  if (rc != RGPU_OK) { (void)hipStreamSynchronize(c->stream); docset_delete(d); return rc; }
  *out_set = d;
  return RGPU_OK;
}

extern "C" int32_t rgpu_docset_from_docs(rgpu_segment* seg, const int32_t* docs, int64_t n_docs, rgpu_docset** out_set) {
  if (!seg || !out_set || n_docs < 0 || (!docs && n_docs > 0)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  *out_set = nullptr;
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  rgpu_docset* d = nullptr;
  RGPU_TRY(docset_new(seg, &d));
  int32_t* d_docs = nullptr;
  auto run = [&]() -> int32_t {
    if (n_docs > 0) {
      HIP_TRY(hipMalloc(&d_docs, (size_t)n_docs * 4));
      HIP_TRY(hipMemcpyAsync(d_docs, docs, (size_t)n_docs * 4, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemsetAsync(d->d_count + 1, 0, 8, c->stream));
      {
        TimedLaunch tl(c, c->stream, "k_docset_from_docs", n_docs);
        RGPU_LAUNCH(k_docset_from_docs, dim3(wg_count(((unsigned long long)n_docs + DOCSET_THREADS - 1) / DOCSET_THREADS)), dim3(DOCSET_THREADS), 0, c->stream,
                    d_docs, n_docs, seg->max_doc, reinterpret_cast<uint32_t*>(d->d_words), reinterpret_cast<unsigned int*>(d->d_count + 1));
      }
      HIP_TRY(launch_status());
      unsigned int bad = 0;
      HIP_TRY(hipMemcpyAsync(&bad, d->d_count + 1, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (bad != 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a doc id outside [0, max_doc)");
    }
    return docset_finish(d, c->stream);
  };
  const int32_t rc = run();
  if (rc != RGPU_OK) (void)hipStreamSynchronize(c->stream);
  if (d_docs) (void)hipFree(d_docs);
  if (rc != RGPU_OK) { docset_delete(d); return rc; }
  *out_set = d;
  return RGPU_OK;
}

extern "C" int32_t rgpu_docset_combine(rgpu_segment* seg, rgpu_docset* const* all_of, int32_t n_all, rgpu_docset* const* none_of, int32_t n_none,
                                       rgpu_docset** out_set) {
  if (!seg || !out_set || n_all < 0 || n_none < 0 || (n_all > 0 && !all_of) || (n_none > 0 && !none_of)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  *out_set = nullptr;
  std::vector<const uint64_t*> a, x;
  for (int32_t i = 0; i < n_all; ++i) { if (!all_of[i]) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null doc set"); RGPU_TRY(docset_check(seg, all_of[i])); a.push_back(all_of[i]->d_words); }
  for (int32_t i = 0; i < n_none; ++i) { if (!none_of[i]) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null doc set"); RGPU_TRY(docset_check(seg, none_of[i])); x.push_back(none_of[i]->d_words); }
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  rgpu_docset* d = nullptr;
  RGPU_TRY(docset_new(seg, &d));
  int32_t rc = docset_combine_launch(c, c->stream, d->max_doc, a.data(), n_all, x.data(), n_none, nullptr, d->d_words, d->d_count);
  unsigned long long n = 0;
  if (rc == RGPU_OK && (hipMemcpyAsync(&n, d->d_count, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess))
    rc = fail(RGPU_ERR_RUNTIME, "doc set combine failed");
  if (rc != RGPU_OK) { (void)hipStreamSynchronize(c->stream); docset_delete(d); return rc; }
  d->cardinality = (int64_t)n;
  *out_set = d;
  return RGPU_OK;
}

extern "C" int32_t rgpu_docset_cardinality(const rgpu_docset* set, int64_t* n_out) {
  if (!set || !n_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  *n_out = set->cardinality;
  return RGPU_OK;
}
extern "C" int64_t rgpu_docset_bytes(const rgpu_docset* set) {
  if (!set) return 0;
  return (int64_t)docset_alloc_bytes(set->n_words) * (set->d_mask ? 2 : 1) + 32 + (set->d_head ? (int64_t)docset_head_alloc_bytes(set->head_n) : 0);
}
extern "C" int32_t rgpu_docset_words(rgpu_docset* set, uint64_t* words_out) {
  if (!set || (!words_out && set->n_words > 0)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  if (set->n_words == 0) return RGPU_OK;
  std::lock_guard<std::mutex> g(set->ctx->mu);
  HIP_TRY(hipSetDevice(set->ctx->device));
  HIP_TRY(hipMemcpy(words_out, set->d_words, set->n_words * 8, hipMemcpyDeviceToHost));
  return RGPU_OK;
}
extern "C" void rgpu_docset_free(rgpu_docset* set) {
  if (!set) return;
  (void)hipSetDevice(set->ctx->device);
  std::lock_guard<std::mutex> g(set->ctx->mu);  // (a masked call in another thread finishes enqueueing first)
  docset_delete(set);  // waits for every masked search in flight that reads the set
}

