// The device-side rows of a blocking call (c->host_api_hits / c->host_api_totals): their defaults, their way out to the caller's arrays, and
// the blocking search itself. RowColumns, api_rows_default, api_rows_read_back, search_batch_host_locked. Entry point: rgpu_search_batch.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, wg_count, settle_pending, search_impl).
// Left where the single file had it: phrase_redo_cap, the redo queue's size of the phrase match stage, closes this part; its one caller is
// phrase_match_setup (candidates.hpp).
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- the device-side rows of a blocking call: c->host_api_hits ([n_queries][k]) and c->host_api_totals, grow-only ---------------
// Every row's defaults - total 0 and "no hit" in every column: what a query that launches nothing, or a leaf that holds none of
// its clauses, returns. `pass`: one pass of a k > RGPU_PASS_K call, which fills `width` columns from `col0` on of rows `stride`
// wide; null: the whole rows of k columns.
struct RowColumns { int32_t width, stride, col0; };
static int32_t api_rows_default(rgpu_ctx* c, hipStream_t stream, int32_t n_queries, int32_t k, const RowColumns* pass = nullptr) {
  const size_t nq = (size_t)n_queries;
  const RowColumns cols = pass ? *pass : RowColumns{k, k, 0};
  HIP_TRY(c->host_api_hits.reserve(nq * (size_t)k, 0, stream));
  HIP_TRY(c->host_api_totals.reserve(nq, 0, stream));
  HIP_TRY(hipMemsetAsync(c->host_api_totals.p, 0, nq * 8, stream));
  RGPU_LAUNCH(k_init_hits, dim3(wg_count((nq * (size_t)cols.width + 255) / 256)), dim3(256), 0, stream, c->host_api_hits.p, (int64_t)n_queries, (int)cols.width,
              (int)cols.stride, (int)cols.col0);
  return RGPU_OK;
}
// ... and the rows out to the caller's arrays; ends synchronised. `verdict`: also fetch the phrase match stage's verdict
// (c->d_err[0]) in the same round - one synchronise less for a call that is content to have written its rows when it refuses
// (rgpu_search_phrase_batch; include/rucene_gpu.h says per call what a refusal leaves).
static int32_t api_rows_read_back(rgpu_ctx* c, hipStream_t stream, int32_t n_queries, int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out, int* verdict = nullptr) {
  hipError_t e0 = verdict ? hipMemcpyAsync(verdict, c->d_err, sizeof(int), hipMemcpyDeviceToHost, stream) : hipSuccess;
  hipError_t e1 = hipMemcpyAsync(hits_out, c->host_api_hits.p, (size_t)n_queries * (size_t)k * sizeof(HitOut), hipMemcpyDeviceToHost, stream);
  hipError_t e2 = hipMemcpyAsync(total_hits_out, c->host_api_totals.p, (size_t)n_queries * 8, hipMemcpyDeviceToHost, stream);
  hipError_t e3 = hipStreamSynchronize(stream);
  if (e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(RGPU_ERR_RUNTIME, "device to host copy failed");
  return RGPU_OK;
}

// rgpu_search_batch behind its argument checks (ctx mutex held, device set): shared with rgpu_search_batch_masked
static int32_t search_batch_host_locked(rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries, const rgpu_query_term* terms,
                                        int32_t n_terms_total, int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  rgpu_ctx* c = seg->ctx;
  // device-side result rows of the blocking variant live in the context (grow-only): the call ends with a stream
  // sync, so they are free again when it returns
  // IndexSearcher::search is ONE query per call (search/searcher.rs:487-525): a batch of one is a launch-latency exercise — 66 us
  // of wall time around 23 us of kernels (round 6's latency leg), two of its six stream operations being the device-to-host
  // copies of 88 bytes. Rows of up to 256 KiB are therefore written by the kernels straight into pinned host memory
  // (hipHostMalloc: device-visible, coherent) and copied to the caller's arrays by the CPU after the one stream sync.
  const size_t hits_bytes = (size_t)n_queries * (size_t)k * sizeof(HitOut), tot_bytes = (size_t)n_queries * 8;
  if (hits_bytes + tot_bytes <= ((size_t)256 << 10)) {
    HIP_TRY(c->host_api_rows.reserve(hits_bytes + tot_bytes));
    HitOut* p_hits = reinterpret_cast<HitOut*>(c->host_api_rows.p);
    int64_t* p_tot = reinterpret_cast<int64_t*>(c->host_api_rows.p + hits_bytes);
    int32_t rc = search_impl(seg, queries, n_queries, terms, n_terms_total, k, p_hits, p_tot, c->stream);
    if (rc != RGPU_OK) return rc;
    rc = settle_pending(c);  // (nothing is deferred on this path; a closure left by an earlier deferred batch may own the stream's tail)
    if (rc != RGPU_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(hits_out, p_hits, hits_bytes);
    std::memcpy(total_hits_out, p_tot, tot_bytes);
    return RGPU_OK;
  }
  HIP_TRY(c->host_api_hits.reserve((size_t)n_queries * (size_t)k, 0, c->stream));
  HIP_TRY(c->host_api_totals.reserve((size_t)n_queries, 0, c->stream));
  RGPU_TRY(search_impl(seg, queries, n_queries, terms, n_terms_total, k, c->host_api_hits.p, c->host_api_totals.p, c->stream));
  return api_rows_read_back(c, c->stream, n_queries, k, hits_out, total_hits_out);
}

extern "C" int32_t rgpu_search_batch(rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries, const rgpu_query_term* terms,
                                     int32_t n_terms_total, int32_t k, rgpu_hit* hits_out, int64_t* total_hits_out) {
  if (!seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !hits_out || !total_hits_out)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return search_batch_host_locked(seg, queries, n_queries, terms, n_terms_total, k, hits_out, total_hits_out);
}

static int64_t phrase_redo_cap(int64_t slots) {
  // (developer knob: RGPU_PHRASE_REDO_CAP=<n> shrinks the list of left-over candidates, so that a test reaches the pass that runs without it)
  int64_t redo_cap = PHRASE_REDO_LIST_CAP;
  if (const char* e = std::getenv("RGPU_PHRASE_REDO_CAP")) redo_cap = std::max<int64_t>(0, std::min<int64_t>(redo_cap, std::atoll(e)));
  return std::min<int64_t>(slots, redo_cap);
}
