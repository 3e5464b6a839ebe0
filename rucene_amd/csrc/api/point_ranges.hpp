// Point ranges: the points of a numeric field on the device, and range filters over them built as doc sets. rgpu_points, points_delete,
// points_scan_launch. Entry points: rgpu_points_attach, rgpu_points_get_info, rgpu_points_free, rgpu_docset_from_point_ranges.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count),
// docsets.hpp (rgpu_docset, docset_new, docset_delete, docset_combine_launch), kernels/points.hpp, host/points_plan.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- point ranges: numeric range filters built as doc sets (include/rucene_gpu.h rgpu_points_*; the plan: host/points_plan.hpp;
// the kernels: kernels/points.hpp) --------------------------------------------------------------------------------------------------
// Launch sequences of rgpu_docset_from_point_ranges, per range as the plan answers it:
//   nothing        memset of the set (its construction), k_docset_combine (the count)
//   every doc      k_docset_combine with no operands (all ones inside [0, max_doc), counted)
//   scatter        memset, k_docset_from_docs over docs_by_value[i0, i1), k_docset_combine (the count)
//   scan           dense: k_points_scan<K, true> (no memset: every word has one writer); else memset, k_points_scan<K, false>;
//                  ONE launch per POINTS_SCAN_RANGES scanned ranges of the call; k_docset_combine per set (the count)
// and one synchronisation at the end of the call.
struct rgpu_points {
  rgpu_segment* seg = nullptr;
  rgpu_ctx* ctx = nullptr;
  uint64_t seg_uid = 0;
  rgpu_host::PointsColumns cols;    // keys_sorted stays; the other columns are released after the upload
  void* d_keys_by_doc = nullptr;    // u32 / u64 keys in doc order, whole chunks, zero-filled behind n_points
  int32_t* d_docs_by_doc = nullptr; // not dense only; whole chunks
  int32_t* d_docs_by_value = nullptr;
  int64_t hbm_bytes = 0;
};

static void points_delete(rgpu_points* p) {
  if (!p) return;
  if (p->d_keys_by_doc) (void)hipFree(p->d_keys_by_doc);
  if (p->d_docs_by_doc) (void)hipFree(p->d_docs_by_doc);
  if (p->d_docs_by_value) (void)hipFree(p->d_docs_by_value);
  delete p;
}

extern "C" int32_t rgpu_points_attach(rgpu_segment* seg, int32_t bytes_per_dim, const int32_t* docs, const uint8_t* values, int64_t n_points,
                                      rgpu_points** out_points) {
  if (!seg || !out_points) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  *out_points = nullptr;
  if (bytes_per_dim != 4 && bytes_per_dim != 8) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "points: one dimension of 4 or 8 bytes");
  if (n_points < 0 || n_points >= ((int64_t)1 << 31) || (n_points > 0 && (!docs || !values))) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));   // (before anything is allocated: an early return owns nothing)
  rgpu_points* p = new rgpu_points();
  if (rgpu_host::points_build(seg->max_doc, bytes_per_dim, docs, values, n_points, p->cols) != RGPU_OK) {
    delete p;
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "points: a doc id outside [0, max_doc)");
  }
  p->seg = seg;
  p->ctx = seg->ctx;
  p->seg_uid = seg->uid;
  rgpu_host::PointsColumns& C = p->cols;
  const size_t padded = (size_t)rgpu_host::points_padded_count(n_points, seg->max_doc, bytes_per_dim, C.dense);
  const size_t n = (size_t)n_points;
  auto run = [&]() -> int32_t {
    HIP_TRY(hipMalloc(&p->d_keys_by_doc, padded * (size_t)bytes_per_dim));
    HIP_TRY(hipMemsetAsync(p->d_keys_by_doc, 0, padded * (size_t)bytes_per_dim, c->stream));
    p->hbm_bytes += (int64_t)(padded * (size_t)bytes_per_dim);
    std::vector<uint32_t> k32;
    if (bytes_per_dim == 4) {
      k32.resize(n);
      for (size_t i = 0; i < n; ++i) k32[i] = (uint32_t)C.keys_by_doc[i];
    }
    if (n > 0) HIP_TRY(hipMemcpyAsync(p->d_keys_by_doc, bytes_per_dim == 4 ? (const void*)k32.data() : (const void*)C.keys_by_doc.data(), n * (size_t)bytes_per_dim,
                                      hipMemcpyHostToDevice, c->stream));
    if (!C.dense) {
      HIP_TRY(hipMalloc(&p->d_docs_by_doc, padded * 4));
      HIP_TRY(hipMemsetAsync(p->d_docs_by_doc, 0, padded * 4, c->stream));
      if (n > 0) HIP_TRY(hipMemcpyAsync(p->d_docs_by_doc, C.docs_by_doc.data(), n * 4, hipMemcpyHostToDevice, c->stream));
      p->hbm_bytes += (int64_t)(padded * 4);
    }
    HIP_TRY(hipMalloc(&p->d_docs_by_value, std::max<size_t>(n, 1) * 4));
    if (n > 0) HIP_TRY(hipMemcpyAsync(p->d_docs_by_value, C.docs_by_value.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    p->hbm_bytes += (int64_t)(std::max<size_t>(n, 1) * 4);
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the host vectors the copies read go away below)
    return RGPU_OK;
  };
  const int32_t rc = run();
  if (rc != RGPU_OK) { (void)hipStreamSynchronize(c->stream); points_delete(p); return rc; }
  std::vector<uint64_t>().swap(C.keys_by_doc);
  std::vector<int32_t>().swap(C.docs_by_doc);
  std::vector<int32_t>().swap(C.docs_by_value);
  *out_points = p;
  return RGPU_OK;
}

extern "C" int32_t rgpu_points_get_info(const rgpu_points* points, rgpu_points_info* out) {
  if (!points || !out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof *out);
  out->n_points = points->cols.n_points;
  out->doc_count = points->cols.doc_count;
  out->hbm_bytes = points->hbm_bytes;
  out->bytes_per_dim = points->cols.bytes_per_dim;
  out->dense = points->cols.dense ? 1 : 0;
  if (points->cols.n_points > 0) {
    rgpu_host::points_key_bytes(points->cols.min_key, points->cols.bytes_per_dim, out->min_value);
    rgpu_host::points_key_bytes(points->cols.max_key, points->cols.bytes_per_dim, out->max_value);
  }
  return RGPU_OK;
}

extern "C" void rgpu_points_free(rgpu_points* points) {
  if (!points) return;
  (void)hipSetDevice(points->ctx->device);
  std::lock_guard<std::mutex> g(points->ctx->mu);  // a build in another thread ends synchronised under this lock
  points_delete(points);
}

template <typename K, bool DENSE>
static int32_t points_scan_launch(rgpu_points* p, const std::vector<rgpu_host::PointsRangePlan>& plans, const std::vector<int32_t>& pass,
                                  const std::vector<rgpu_docset*>& sets, hipStream_t stream) {
  PointsScanArgs<K> a;
  std::memset(&a, 0, sizeof a);
  a.n_ranges = (int32_t)pass.size();
  a.max_doc = p->cols.max_doc;
  a.n_points = p->cols.n_points;
  for (size_t i = 0; i < pass.size(); ++i) {
    const rgpu_host::PointsRangePlan& P = plans[(size_t)pass[i]];
    a.lower[i] = (K)P.lower;
    a.span[i] = (K)(P.upper - P.lower);
    a.rows[i] = reinterpret_cast<uint32_t*>(sets[(size_t)pass[i]]->d_words);
  }
  constexpr int64_t chunk = 64 * (16 / (int64_t)sizeof(K));
  const int64_t padded = rgpu_host::points_padded_count(p->cols.n_points, p->cols.max_doc, (int32_t)sizeof(K), DENSE);
  const int64_t n_chunks = padded / chunk;
  const unsigned grid = (unsigned)std::min<int64_t>(POINTS_SCAN_MAX_BLOCKS, (n_chunks + DOCSET_WAVES - 1) / DOCSET_WAVES);
  {
    TimedLaunch tl(p->ctx, stream, "k_points_scan", p->cols.n_points);
    RGPU_LAUNCH((k_points_scan<K, DENSE>), dim3(grid), dim3(DOCSET_THREADS), 0, stream, static_cast<const K*>(p->d_keys_by_doc), p->d_docs_by_doc, a);
  }
  HIP_TRY(launch_status());
  return RGPU_OK;
}

extern "C" int32_t rgpu_docset_from_point_ranges(rgpu_points* points, const rgpu_point_range* ranges, int32_t n_ranges, int32_t path,
                                                 rgpu_docset** out_sets) {
  if (!points || !ranges || n_ranges <= 0 || !out_sets || path < 0 || path > 2) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  for (int32_t r = 0; r < n_ranges; ++r) out_sets[r] = nullptr;
  rgpu_ctx* c = points->ctx;
  rgpu_segment* seg = points->seg;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  const rgpu_host::PointsColumns& C = points->cols;
  const std::vector<rgpu_host::PointsRangePlan> plans = rgpu_host::plan_point_ranges(C, ranges, n_ranges, path);
  const std::vector<std::vector<int32_t>> passes = rgpu_host::points_scan_passes(plans);
  std::vector<rgpu_docset*> sets((size_t)n_ranges, nullptr);
  std::vector<unsigned long long> counts((size_t)n_ranges, 0ull);
  auto run = [&]() -> int32_t {
    for (int32_t r = 0; r < n_ranges; ++r) {
      const rgpu_host::PointsAnswer ans = plans[(size_t)r].answer;
      const bool written_whole = ans == rgpu_host::POINTS_EVERY_DOC || (ans == rgpu_host::POINTS_SCAN && C.dense);
      RGPU_TRY(docset_new(seg, &sets[(size_t)r], !written_whole));
    }
    for (int32_t r = 0; r < n_ranges; ++r) {
      const rgpu_host::PointsRangePlan& P = plans[(size_t)r];
      if (P.answer != rgpu_host::POINTS_SCATTER) continue;
      rgpu_docset* d = sets[(size_t)r];
      const int64_t m = P.i1 - P.i0;
      HIP_TRY(hipMemsetAsync(d->d_count + 1, 0, 8, stream));
      {
        TimedLaunch tl(c, stream, "k_docset_from_docs", m);
        RGPU_LAUNCH(k_docset_from_docs, dim3(wg_count(((unsigned long long)m + DOCSET_THREADS - 1) / DOCSET_THREADS)), dim3(DOCSET_THREADS), 0, stream,
                    points->d_docs_by_value + P.i0, m, seg->max_doc, reinterpret_cast<uint32_t*>(d->d_words), reinterpret_cast<unsigned int*>(d->d_count + 1));
      }
      HIP_TRY(launch_status());
    }
    for (const std::vector<int32_t>& pass : passes) {
      if (C.bytes_per_dim == 4) RGPU_TRY(C.dense ? (points_scan_launch<uint32_t, true>(points, plans, pass, sets, stream)) : (points_scan_launch<uint32_t, false>(points, plans, pass, sets, stream)));
      else RGPU_TRY(C.dense ? (points_scan_launch<uint64_t, true>(points, plans, pass, sets, stream)) : (points_scan_launch<uint64_t, false>(points, plans, pass, sets, stream)));
    }
    // the count of every set (an every-doc set is formed by the same launch); one synchronisation for the call
    for (int32_t r = 0; r < n_ranges; ++r) {
      rgpu_docset* d = sets[(size_t)r];
      const uint64_t* self[1] = {d->d_words};
      const bool all = plans[(size_t)r].answer == rgpu_host::POINTS_EVERY_DOC;
      RGPU_TRY(docset_combine_launch(c, stream, d->max_doc, self, all ? 0 : 1, nullptr, 0, nullptr, d->d_words, d->d_count));
      HIP_TRY(hipMemcpyAsync(&counts[(size_t)r], d->d_count, 8, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return RGPU_OK;
  };
  const int32_t rc = run();
  if (rc != RGPU_OK) {
    (void)hipStreamSynchronize(stream);
    for (rgpu_docset* d : sets) docset_delete(d);
    return rc;
  }
  for (int32_t r = 0; r < n_ranges; ++r) { sets[(size_t)r]->cardinality = (int64_t)counts[(size_t)r]; out_sets[r] = sets[(size_t)r]; }
  return RGPU_OK;
}

