// Positions of a segment: the .pos and .pay files attached, and position lists decoded for a caller. pos_term_of, decode_positions_impl.
// Entry points: rgpu_segment_attach_positions, rgpu_segment_attach_payloads, rgpu_decode_positions_device, rgpu_decode_positions.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, SCRATCH_TAKE,
// Stager / STAGE_SIZED, seg_view, prepare_terms_locked, make_dev_term), host/doc_format.hpp.
// Its banner "exact phrases" headed all the phrase code of the single file: the stages are in phrase_stages.hpp, the calls in phrase_search.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- exact phrases -----------------------------------------------------------------------------------------------------------
extern "C" int32_t rgpu_segment_attach_positions(rgpu_segment* seg, const uint8_t* pos_file, size_t pos_len) {
  if (!seg || !pos_file) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (!seg->has_positions) return fail(RGPU_ERR_ILLEGAL_STATE, "the segment was not uploaded as a positions field (index_options >= 3)");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<uint8_t> head(128);
  const size_t head_n = std::min(seg->doc_len, head.size());
  HIP_TRY(hipMemcpy(head.data(), seg->d_doc, head_n, hipMemcpyDeviceToHost));  // the .doc header: id + suffix to compare with
  int64_t start = 0;
  std::string why;
  const int rc = rucene::parse_pos_file(pos_file, pos_len, head.data(), seg->version, &start, &why);
  if (rc != 0) return fail(rc, why);
  if (seg->d_pos) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(seg->d_pos); seg->d_pos = nullptr; }
  const size_t pad = 8192;  // speculative row / VInt-block loads may run past the last position byte
  HIP_TRY(hipMalloc(&seg->d_pos, pos_len + pad));
  HIP_TRY(hipMemcpy(seg->d_pos, pos_file, pos_len, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(seg->d_pos + pos_len, 0, pad));
  seg->pos_len = pos_len;
  return RGPU_OK;
}

// Lucene50PostingsReader::open's third file (posting_reader.rs:131-156). Nothing on this path reads payload bytes or offsets
// (phrase scorers ask for positions only and get the iterator that walks past them, :189-212), so the file is checked — header,
// version, segment id / suffix, footer — as open() checks it, and not kept.
extern "C" int32_t rgpu_segment_attach_payloads(rgpu_segment* seg, const uint8_t* pay_file, size_t pay_len) {
  if (!seg || !pay_file) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (!seg->has_offsets && !seg->has_payloads)
    return fail(RGPU_ERR_ILLEGAL_STATE, "the segment's field stores neither payloads nor offsets (index_options 4 / RGPU_FIELD_STORES_PAYLOADS)");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<uint8_t> head(128);
  const size_t head_n = std::min(seg->doc_len, head.size());
  HIP_TRY(hipMemcpy(head.data(), seg->d_doc, head_n, hipMemcpyDeviceToHost));
  int64_t start = 0;
  std::string why;
  const int rc = rucene::parse_pay_file(pay_file, pay_len, head.data(), seg->version, &start, &why);
  if (rc != 0) return fail(rc, why);
  seg->pay_checked = true;
  return RGPU_OK;
}

// BlockPostingIterator::{next, next_position} to exhaustion for every given term (kernels/decode_positions.hpp): ends synchronised
// where a term's positions lie in .pos (a phrase's planner adds phrase_pos / query_ord / same_as: emit_phrase)
static PosTerm pos_term_of(const rgpu_term_state& st, const rgpu_term_positions& pos) {
  PosTerm p{};
  p.pos_start_fp = (uint64_t)pos.pos_start_fp;
  p.total_term_freq = st.total_term_freq;
  // posting_reader.rs:1195-1203: fewer than 128 positions -> all VInts; exactly 128 -> one packed block, no trailing one
  p.last_pos_block_fp = st.total_term_freq < 128 ? pos.pos_start_fp : (st.total_term_freq == 128 ? -1 : pos.pos_start_fp + pos.last_pos_block_offset);
  return p;
}

static int32_t decode_positions_impl(rgpu_segment* seg, const rgpu_term_state* terms, const rgpu_term_positions* positions, int64_t n_terms,
                                     int32_t* positions_dev, hipStream_t stream) {
  rgpu_ctx* c = seg->ctx;
  if (!seg->has_positions || !seg->d_pos) return fail(RGPU_ERR_ILLEGAL_STATE, "a positions decode needs a positions field with its .pos file attached");
  std::vector<const rgpu_term_state*> ptrs;
  int64_t expect = 0;
  for (int64_t i = 0; i < n_terms; ++i) {
    const rgpu_term_state& st = terms[i];
    if (st.doc_freq < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "negative doc_freq");
    if (st.doc_freq == 0) continue;
    if (st.total_term_freq < st.doc_freq) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "total_term_freq below doc_freq");
    if (positions[i].pos_start_fp < 0 || (size_t)positions[i].pos_start_fp >= seg->pos_len) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "pos_start_fp outside the .pos file");
    expect += st.total_term_freq;
    ptrs.push_back(&st);
  }
  if (expect == 0) return RGPU_OK;
  if (expect > 0xfffffff0ll) return fail(RGPU_ERR_UNSUPPORTED, "one call decodes at most 2^32 positions: split the term list");
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size(), false));  // stage A: directory (with dir_pos), block store, tails
  std::vector<DevTerm> dt;
  std::vector<PosTerm> pt;
  std::vector<int64_t> item_prefix;
  int64_t items = 0;
  for (int64_t i = 0; i < n_terms; ++i) {
    const rgpu_term_state& st = terms[i];
    if (st.doc_freq == 0) continue;
    DevTerm d;
    RGPU_TRY(make_dev_term(seg, st, 0.f, 0, &d, false));
    dt.push_back(d);
    pt.push_back(pos_term_of(st, positions[i]));
    item_prefix.push_back(items);
    items += (int64_t)d.nblocks + ((d.df == 1 || d.tail_n > 0) ? 1 : 0);
  }
  item_prefix.push_back(items);
  const int nt = (int)dt.size();
  SCRATCH_TAKE(c);
  Stager st(c);
  const auto r_t = st.add<DevTerm>(dt.size());
  const auto r_pt = st.add<PosTerm>(pt.size());
  const auto r_ip = st.add<int64_t>(item_prefix.size());
  STAGE_SIZED(sg, st);
  sg.put(r_t, dt);
  sg.put(r_pt, pt);
  sg.put(r_ip, item_prefix);
  RGPU_TRY(sg.upload(stream));
  const int64_t n_tiles = (items + SCAN_TILE - 1) / SCAN_TILE;
  HIP_TRY(c->pos_counts.reserve((size_t)items + 64, 0, stream));
  HIP_TRY(c->pos_tiles.reserve((size_t)n_tiles + 8, 0, stream));
  HIP_TRY(hipMemsetAsync(c->d_err, 0, 4 * sizeof(int), stream));
  const DevTerm* d_t = sg.dev(r_t);
  const PosTerm* d_pt = sg.dev(r_pt);
  const int64_t* d_ip = sg.dev(r_ip);
  unsigned long long* d_tiles = c->pos_tiles.p + 8;
  unsigned long long* d_total = c->pos_tiles.p + 1;
  const SegView sv = seg_view(seg);
  const bool legacy = seg->version < 1;
  const unsigned grid = wg_count((items + WG_WAVES - 1) / WG_WAVES);
  {
    TimedLaunch tl(c, stream, "k_pos_counts", expect);
    if (legacy) RGPU_LAUNCH(k_pos_counts<true>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, d_t, d_ip, nt, items, c->pos_counts.p);
    else RGPU_LAUNCH(k_pos_counts<false>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, d_t, d_ip, nt, items, c->pos_counts.p);
  }
  {
    TimedLaunch tl(c, stream, "k_scan_rows", 0);
    RGPU_LAUNCH(k_scan_reduce, dim3((unsigned)n_tiles), dim3(PREP_THREADS), 0, stream, c->pos_counts.p, items, d_tiles);
    RGPU_LAUNCH(k_scan_tiles, dim3(1), dim3(PREP_THREADS), 0, stream, d_tiles, n_tiles, (unsigned long long)expect, d_total, c->d_err);
    RGPU_LAUNCH(k_scan_down, dim3((unsigned)n_tiles), dim3(PREP_THREADS), 0, stream, c->pos_counts.p, items, d_tiles);
  }
  {
    TimedLaunch tl(c, stream, "k_decode_positions", expect);
    if (legacy)
      RGPU_LAUNCH(k_decode_positions<true>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, d_t, d_pt, d_ip, nt, items, c->pos_counts.p,
                         (int64_t)seg->pos_len, positions_dev, c->d_err);
    else
      RGPU_LAUNCH(k_decode_positions<false>, dim3(grid), dim3(WG_THREADS), 0, stream, sv, d_t, d_pt, d_ip, nt, items, c->pos_counts.p,
                         (int64_t)seg->pos_len, positions_dev, c->d_err);
  }
  int err4[4] = {0, 0, 0, 0};
  unsigned long long total = 0;
  HIP_TRY(hipMemcpyAsync(err4, c->d_err, 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(launch_status());
  if (err4[0] != 0 || total != (unsigned long long)expect)
    return fail(RGPU_ERR_CORRUPT_INDEX, total != (unsigned long long)expect ? "the postings' freqs do not add up to total_term_freq" : "corrupt position data in .pos");
  return RGPU_OK;
}

extern "C" int32_t rgpu_decode_positions_device(rgpu_segment* seg, const rgpu_term_state* terms, const rgpu_term_positions* positions, int64_t n_terms,
                                                void* positions_dev, void* hip_stream) {
  if (!seg || !terms || !positions || n_terms <= 0 || !positions_dev) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  std::lock_guard<std::mutex> g(seg->ctx->mu);
  HIP_TRY(hipSetDevice(seg->ctx->device));
  return decode_positions_impl(seg, terms, positions, n_terms, (int32_t*)positions_dev, hip_stream ? (hipStream_t)hip_stream : seg->ctx->stream);
}

extern "C" int32_t rgpu_decode_positions(rgpu_segment* seg, const rgpu_term_state* terms, const rgpu_term_positions* positions, int64_t n_terms,
                                         int32_t* positions_out) {
  if (!seg || !terms || !positions || n_terms <= 0 || !positions_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  int64_t total = 0;
  for (int64_t i = 0; i < n_terms; ++i) if (terms[i].doc_freq > 0) total += std::max<int64_t>(0, terms[i].total_term_freq);
  if (total == 0) return RGPU_OK;
  int32_t* d_pos = nullptr;
  HIP_TRY(hipMalloc(&d_pos, (size_t)total * 4));
  int32_t rc = decode_positions_impl(seg, terms, positions, n_terms, d_pos, c->stream);
  if (rc == RGPU_OK && hipMemcpy(positions_out, d_pos, (size_t)total * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(RGPU_ERR_RUNTIME, "device to host copy failed");
  (void)hipFree(d_pos);
  return rc;
}

