// The candidate stage the phrase, doc-set and count calls share: k_search_and in emit mode fills an array of candidate slots per query.
// phrase_match_setup, lead_items / lead_slots / lead_collect_chunks, AndEmitStage, and_emit_stage. No entry point of its own.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, wg_count, seg_view, and_xcd_chunk, and_grid),
// rows.hpp (phrase_redo_cap).
// Left where the single file had it: phrase_match_setup stands ahead of the stage it serves. Its banner's "phrase_match_stage (below, with
// the exact phrases)" now means phrase_stages.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- the set-up of phrase_match_stage (below, with the exact phrases), in front of the launch that fills the slots - and_emit_stage
// runs it among its own memsets, a rescoring by itself - and whether or not the stage will have a slot to look at:
// the callers read d_err afterwards.
// `zero_keys`: zero c->phrase_keys. The match kernels write a key (or 0) to every slot below a query's count and to none above it:
// a 64-candidate group past a query's count is never written. rgpu_rescore_phrase_batch needs the zeroes: k_rescore_phrase_combine
// reads a row's slots by position, a 64-candidate kernel leaves the slots behind a row's window unwritten, and a batch of
// absent-term rows launches no match kernel at all. rgpu_search_phrase_bool_batch and _phrase_or_batch ask for them too:
// k_phrase_bool_score and k_phrase_run_place walk the slots by 64-slot group (both also look at the count; the zeroes are kept as
// the second line they have been). rgpu_search_phrase_batch does without the memset: its collectors read emit_count[q] slots of
// query q and nothing behind them.
static int32_t phrase_match_setup(rgpu_ctx* c, hipStream_t stream, int64_t slots, bool zero_keys, int64_t* redo_cap) {
  HIP_TRY(c->phrase_docs.reserve((size_t)slots + 64, 0, stream));
  HIP_TRY(c->phrase_keys.reserve((size_t)slots + 64, 0, stream));
  *redo_cap = phrase_redo_cap(slots);
  HIP_TRY(c->phrase_redo.reserve((size_t)*redo_cap + 64, 0, stream));
  if (zero_keys) HIP_TRY(hipMemsetAsync(c->phrase_keys.p, 0, (size_t)slots * 8, stream));
  HIP_TRY(hipMemsetAsync(c->d_err, 0, 4 * sizeof(int), stream));  // [0]: error code, [2]: slots on the redo list, [3]: "a candidate needs the wide lists"
  return RGPU_OK;
}

// ---- the candidate stage: k_search_and in emit mode ------------------------------------------------------------------------------
// A conjunction that collects nothing: the docs that hold every required clause of (virtual) query q (and none of its MUST_NOT
// clauses, DevQuery::pad) go to c->phrase_docs from slot emit_prefix[q] on, their number to c->phrase_count[q]. What reads the
// slots afterwards is the caller's business: phrase_match_stage (rgpu_search_phrase_batch, _phrase_bool_batch, _phrase_or_batch)
// or k_docset_from_emitted (rgpu_docset_collect_batch).
// A query's share of the launch, from the conjunction's lead (its first, rarest, clause): work items of `blocks_per_item` lead
// blocks ...
static inline int64_t lead_items(const DevTerm& lead, int blocks_per_item) { return lead.nblocks == 0 ? 1 : (lead.nblocks + blocks_per_item - 1) / blocks_per_item; }
// ... candidate slots: the lead's doc_freq bounds the matches; whole groups of 64 (the 64 slots of a k_phrase_match_lanes wavefront
// belong to one query) ...
static inline int64_t lead_slots(const DevTerm& lead) { return rgpu_host::pb_round_up_64((int64_t)lead.df); }
// ... and items of the chunked collector (k_phrase_collect_items)
static inline int64_t lead_collect_chunks(const DevTerm& lead) { return ((int64_t)lead.df + PHRASE_COLLECT_CHUNK - 1) / PHRASE_COLLECT_CHUNK; }
struct AndEmitStage {
  const char* name;  // of the launch in the kernel statistics
  const DevQuery* d_q;
  const DevTerm* d_t;
  const int64_t* d_ip;     // items in front of each query's
  const int64_t* d_ep;     // slots in front of each query's
  const TermBitmap* d_bm;  // clause_bitmap_table, or null
  int32_t n_queries;       // the conjunctions (virtual queries where a query runs several)
  // entries of c->phrase_count to reserve and zero: n_queries, or more where later stages count slots of their own behind the
  // conjunctions' (rgpu_search_phrase_bool_batch: one plane per phrase, k_phrase_bool_fanout fills planes 1..)
  size_t n_counts;
  int64_t items, slots;
  int blocks_per_item;
  int k_emit;    // width of the (empty) top-k lists the kernel keeps all the same: the narrowest kind the caller's k allows
  bool any_not;  // some query has MUST_NOT clauses: the HAS_NOT instantiation
  // least sizes of c->S->d_partial_keys / d_partial_counts: the kernel's own lists need items * k_emit and items; the chunked phrase
  // collector reuses both buffers behind it and needs them larger (0: no such need)
  size_t partial_keys, partial_counts;
  // phrase_match_stage comes behind (the phrase callers): the stage runs phrase_match_setup, zeroing the keys or not, between its
  // memset of the counts and those of the thresholds, and hands the set-up's *redo_cap on. Every memset of the call then stands in
  // front of the conjunction, the large one (the keys) second as it always has: with the set-up called by the callers in front of
  // this stage - the same memsets, the keys first - rgpu_search_phrase_bool_batch took 0.05 - 0.07 ms of 2.15 longer per call, none
  // of it inside a kernel (the phrase-bool launch sequence).
  int64_t* redo_cap = nullptr;
  bool zero_keys = false;
  // the masked exact-phrase calls (seg's live docs are `live AND set`): the LIVE_ONLY instantiation - a candidate that is not live is
  // dropped, not marked; the slots behind the survivors stay unwritten, as the slots behind any query's count do
  bool live_only = false;
};
static int32_t and_emit_stage(rgpu_segment* seg, hipStream_t stream, const AndEmitStage& a) {
  rgpu_ctx* c = seg->ctx;
  const size_t nq = (size_t)a.n_queries;
  HIP_TRY(c->phrase_docs.reserve((size_t)a.slots + 64, 0, stream));  // (phrase_match_setup reserves it too: a doc-set call runs no set-up, a rescoring not this stage)
  HIP_TRY(c->phrase_count.reserve(a.n_counts, 0, stream));
  HIP_TRY(c->S->d_partial_keys.reserve(std::max((size_t)a.items * (size_t)a.k_emit, a.partial_keys), 0, stream));
  HIP_TRY(c->S->d_partial_counts.reserve(std::max((size_t)a.items, a.partial_counts), 0, stream));
  HIP_TRY(c->S->d_tau.reserve(nq, 0, stream));  // (thresholds and counted words: per conjunction)
  HIP_TRY(c->S->d_touched.reserve(nq * 2, 0, stream));
  HIP_TRY(hipMemsetAsync(c->phrase_count.p, 0, a.n_counts * 8, stream));
  if (a.redo_cap) RGPU_TRY(phrase_match_setup(c, stream, a.slots, a.zero_keys, a.redo_cap));
  HIP_TRY(hipMemsetAsync(c->S->d_tau.p, 0, nq * 8, stream));
  HIP_TRY(hipMemsetAsync(c->S->d_touched.p, 0, nq * 16, stream));
  TimedLaunch tl(c, stream, a.name, 0);
  const SegView sv = seg_view(seg);
  const int xcd_chunk = and_xcd_chunk(seg);
  const unsigned grid = wg_count(and_grid((a.items + AND_WG_WAVES - 1) / AND_WG_WAVES, xcd_chunk));
  auto go = [&](auto kern) {
    RGPU_LAUNCH(kern, dim3(grid), dim3(AND_WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_ip, (int)a.n_queries, a.items, a.blocks_per_item, a.k_emit,
                c->S->d_partial_keys.p, c->S->d_partial_counts.p, c->S->d_tau.p, c->S->d_touched.p, a.d_ep, c->phrase_count.p, (void*)c->phrase_docs.p,
                (const unsigned long long*)nullptr, (const int32_t*)nullptr, a.d_bm, xcd_chunk);
  };
  const bool legacy = seg->version < 1;
  if (a.live_only) {
    if (a.any_not) { if (legacy) go(k_search_and<true, false, true, false, false, true>); else go(k_search_and<false, false, true, false, false, true>); }
    else { if (legacy) go(k_search_and<true, false, false, false, false, true>); else go(k_search_and<false, false, false, false, false, true>); }
    return RGPU_OK;
  }
  if (a.any_not) { if (legacy) go(k_search_and<true, false, true, false>); else go(k_search_and<false, false, true, false>); }
  else { if (legacy) go(k_search_and<true, false, false, false>); else go(k_search_and<false, false, false, false>); }
  return RGPU_OK;
}

