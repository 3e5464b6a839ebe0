// The tail. Entry points: rgpu_bm25_encode_norm, and what only a variant build has: rgpu_debug_counters under -DRGPU_ORX_TIME,
// -DRGPU_LZ_TIME, -DRGPU_AND_TIME or -DRGPU_EXP_COUNT, rgpu_debug_trace under -DRGPU_TERM_TRACE or -DRGPU_AND_TRACE.
// Uses: the counters and traces the kernels of kernels/*.hpp keep in those builds; BM25Similarity (included by host_formats.hpp).
// Wart: rgpu_bm25_encode_norm stands here, behind the fused call, and not beside the other rgpu_bm25_* of host_formats.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

extern "C" uint8_t rgpu_bm25_encode_norm(float boost, int32_t field_length) {
  return rucene::BM25Similarity::encode_norm_value(boost, field_length);
}

#ifdef RGPU_ORX_TIME
extern "C" int32_t rgpu_debug_counters(unsigned long long* out8, int32_t reset) {  // k_or_wide wave-cycles per phase (search_or_wide.hpp)
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_orx_dbg), 64) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_orx_dbg), z, 64) != hipSuccess) return -1;
  }
  return 0;
}
#endif
#ifdef RGPU_LZ_TIME
extern "C" int32_t rgpu_debug_counters(unsigned long long* out8, int32_t reset) {  // k_or_lazy wave-cycles per phase (search_or_lazy.hpp)
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_lz_dbg), 64) != hipSuccess) return -1;
  unsigned long long more[8];
  if (hipMemcpyFromSymbol(more, HIP_SYMBOL(g_lz_dbg), 64, 64) != hipSuccess) return -1;
  std::fprintf(stderr, "[lz steps] lazy-only test on in %llu of %llu steps; a doc in enough lists in %llu; bound iterations %llu; mean need %.2f, need_hi %.2f\n", more[0], more[3],
               more[1], more[2], more[0] ? (double)more[4] / (double)more[0] : 0.0, more[0] ? (double)more[5] / (double)more[0] : 0.0);
  if (reset) {
    unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_lz_dbg), z, 128) != hipSuccess) return -1;
  }
  return 0;
}
#endif
#ifdef RGPU_AND_TIME
extern "C" int32_t rgpu_debug_counters(unsigned long long* out8, int32_t reset) {  // k_search_and wave-cycles per phase (search_and.hpp)
  unsigned long long all[16];
  if (hipMemcpyFromSymbol(all, HIP_SYMBOL(g_and_time), 128) != hipSuccess) return -1;
  std::memcpy(out8, all, 64);
  std::fprintf(stderr, "[and time] cycles: set-up %llu, first probe %llu, loop(queued) %llu, loop(block by block) %llu, epilogue %llu | items %llu, pops %llu, block vectors %llu, "
               "queued survivors %llu, walked decodes: after a pop %llu, block by block %llu\n", all[0], all[1], all[2], all[3], all[4], all[5], all[6], all[7], all[8], all[9], all[10]);
  if (reset) {
    unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_and_time), z, 128) != hipSuccess) return -1;
  }
  return 0;
}
#endif
#ifdef RGPU_TERM_TRACE
extern "C" int32_t rgpu_debug_trace(void* out, int32_t n) {  // the most recent k_search_term launch's item timeline
  if (n > TERM_TRACE_CAP) n = TERM_TRACE_CAP;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_term_trace), (size_t)n * sizeof(TermTraceRec)) == hipSuccess ? n : -1;
}
#endif
#ifdef RGPU_AND_TRACE
// the most recent k_search_and launch's item timeline: n records of {t0, t1 (100 MHz wall clock), q, chunk, lead blocks, survivors popped}
extern "C" int32_t rgpu_debug_trace(void* out, int32_t n) {
  if (n > AND_TRACE_CAP) n = AND_TRACE_CAP;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_and_trace), (size_t)n * sizeof(AndTraceRec)) == hipSuccess ? n : -1;
}
#endif
#ifdef RGPU_EXP_COUNT
extern "C" int32_t rgpu_debug_counters(unsigned long long* out8, int32_t reset) {  // [0..3] TERM, [4..7] AND
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_term_dbg), 32) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out8 + 4, HIP_SYMBOL(g_and_dbg), 32) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[4] = {0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_term_dbg), z, 32) != hipSuccess || hipMemcpyToSymbol(HIP_SYMBOL(g_and_dbg), z, 32) != hipSuccess) return -1;
  }
  return 0;
}
#endif
