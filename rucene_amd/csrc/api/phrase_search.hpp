// Phrase and span searches: exact and sloppy PhraseQuery, ordered and unordered SpanNearQuery over term clauses, each also under a doc-set
// mask. check_span_clauses, search_phrase_batch_impl. Entry points: rgpu_search_span_near_batch, rgpu_search_span_unordered_batch,
// rgpu_search_phrase_batch, rgpu_search_phrase_batch_masked.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, launch_status, HIP_TRY / RGPU_TRY, SCRATCH_TAKE, Stager / STAGE_SIZED,
// prepare_terms_locked, ensure_and_bitmaps_locked, clause_bitmap_table, and_item_blocks), rows.hpp (api_rows_default, api_rows_read_back),
// candidates.hpp (lead_items, lead_slots, lead_collect_chunks, AndEmitStage, and_emit_stage), docsets.hpp (rgpu_docset, docset_check),
// masked.hpp (PhraseMask, masked_stage_name, refuse_sloppy_masked), phrase_stages.hpp (PhraseMatchStage / phrase_match_stage,
// check_phrase_query, check_phrase_terms, emit_phrase, phrase_match_status, phrase_collect_chunked, PhraseCollectStage / phrase_collect_stage).
// Left where the single file had them: PhraseClauseArrays and check_phrases_query open this part, which does not use them; they serve
// phrase_bool.hpp and phrase_or.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- a boolean query over phrases, as rgpu_search_phrase_bool_batch and rgpu_search_phrase_or_batch take one: its own fields, its
// phrases and its term clauses (those the leaf holds go to `ptrs` for the preparation). `noun`: what the caller's messages call it.
struct PhraseClauseArrays {
  const rgpu_phrase_query* phrases;
  int32_t n_phrases_total;
  const rgpu_phrase_term* phrase_terms;
  int32_t n_phrase_terms_total;
  const rgpu_query_term* terms;
  int32_t n_terms_total;
};
template <typename BoolQuery>
static int32_t check_phrases_query(const rgpu_segment* seg, const BoolQuery& Q, const char* noun, const PhraseClauseArrays& a, std::vector<const rgpu_term_state*>* ptrs) {
  const rgpu_ctx* c = seg->ctx;
  if (Q.n_phrases < 1 || Q.n_phrases > RGPU_MAX_BOOL_PHRASES) return fail(RGPU_ERR_UNSUPPORTED, std::string(noun) + " holds 1..RGPU_MAX_BOOL_PHRASES phrases");
  if (Q.first_phrase < 0 || (int64_t)Q.first_phrase + Q.n_phrases > (int64_t)a.n_phrases_total) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "phrase range outside phrases[]");
  if (Q.n_terms < 0 || Q.n_must_not < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "negative clause count");
  if (Q.n_terms + (int64_t)Q.n_must_not > 0 && (Q.first_term < 0 || (int64_t)Q.first_term + Q.n_terms + Q.n_must_not > (int64_t)a.n_terms_total))
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "clause range outside terms[]");
  for (int i = 0; i < Q.n_phrases; ++i) {
    const rgpu_phrase_query& P = a.phrases[Q.first_phrase + i];
    RGPU_TRY(check_phrase_query(c, P, a.n_phrase_terms_total, false));
    RGPU_TRY(check_phrase_terms(seg, P, a.phrase_terms, ptrs));
  }
  for (int64_t i = 0; i < (int64_t)Q.n_terms + Q.n_must_not; ++i) {
    const rgpu_query_term& t = a.terms[Q.first_term + i];
    if (i < Q.n_terms && (t.sim_table < 0 || t.sim_table >= c->n_sim_tables)) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "unknown sim_table handle");
    if (t.state.doc_freq > 0) ptrs->push_back(&t.state);
  }
  return RGPU_OK;
}

// rgpu_search_span_near_batch: clause i of a span-near query is rgpu_phrase_term i with position = i, reserved = 0
static int32_t check_span_clauses(const rgpu_phrase_query& Q, const rgpu_phrase_term* terms) {
  for (int i = 0; i < Q.n_terms; ++i) {
    const rgpu_phrase_term& t = terms[Q.first_term + i];
    if (t.position != i) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "span near: rgpu_phrase_term.position must be the clause's index");
    if (t.reserved != 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "span near: rgpu_phrase_term.reserved must be 0");
  }
  return RGPU_OK;
}

static int32_t search_phrase_batch_impl(rgpu_segment* seg, rgpu_docset* set, const rgpu_phrase_query* queries, int32_t n_queries,
                                        const rgpu_phrase_term* terms, int32_t n_terms_total, int32_t k, rgpu_hit* hits_out,
                                        int64_t* total_hits_out, bool span = false, bool unordered = false) {
  // unordered (with span): rgpu_search_span_unordered_batch - the same plan, checks and collectors; the match stage runs
  // NearSpansUnordered's kernels (kernels/search_span_unordered.hpp).
  // span: rgpu_search_span_near_batch - the queries are ordered SpanNearQuerys over SpanTermQuery clauses. The plan, the candidate
  // stage and the collectors are the phrases'; the match stage runs the span kernels, and the collectors are handed a marker in
  // place of the slops: SpanScorer is two-phase whatever the slop (span.rs:1033-1091), so next_limit applies at slop 0 too.
  if (!seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !hits_out || !total_hits_out)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (set) { RGPU_TRY(docset_check(seg, set)); RGPU_TRY(refuse_sloppy_masked(queries, n_queries)); }
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "phrase search: k must be in 1..RGPU_MAX_K");
  if (!seg->has_positions || !seg->d_pos) return fail(RGPU_ERR_ILLEGAL_STATE, "phrase search needs a positions field with its .pos file attached");
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = c->stream;
  // ---- validate, resolve, plan
  std::vector<const rgpu_term_state*> ptrs;
  for (int32_t q = 0; q < n_queries; ++q) {
    RGPU_TRY(check_phrase_query(c, queries[q], n_terms_total, true));
    RGPU_TRY(check_phrase_terms(seg, queries[q], terms, &ptrs));
    if (span) RGPU_TRY(check_span_clauses(queries[q], terms));
  }
  PhraseMask masked;
  RGPU_TRY(masked.install(seg, set));
  RGPU_TRY(prepare_terms_locked(seg, ptrs.data(), ptrs.size()));
  // the conjunction that finds a phrase's candidates answers a dense clause from its doc bitmap, as a BooleanQuery's does
  int64_t bitmap_df = INT64_MAX;
  {
    std::vector<const rgpu_term_state*> clauses;
    std::vector<int32_t> clause_sim;
    clauses.reserve((size_t)n_terms_total);
    clause_sim.reserve((size_t)n_terms_total);
    for (int32_t q = 0; q < n_queries; ++q)
      for (int i = 0; i < queries[q].n_terms; ++i) { clauses.push_back(&terms[queries[q].first_term + i].state); clause_sim.push_back(queries[q].sim_table); }
    RGPU_TRY(ensure_and_bitmaps_locked(seg, clauses, clause_sim, &bitmap_df));
  }
  std::vector<DevQuery> dq((size_t)n_queries);
  std::vector<DevTerm> dt;
  std::vector<PosTerm> pt;
  std::vector<int64_t> item_prefix((size_t)n_queries + 1), emit_prefix((size_t)n_queries + 1), collect_prefix((size_t)n_queries + 1);
  std::vector<int32_t> slops((size_t)n_queries, 0), limits((size_t)n_queries, -1);
  std::vector<int32_t> two_phase;  // span: what the collectors read in place of the slops - 1 for every live query
  if (span) two_phase.assign((size_t)n_queries, 0);
  bool any_span = false;
  int64_t collect_items = 0;
  bool any_cutoff = false;
  bool any_sloppy = false, any_exact = false;
  bool sloppy_rpts = false;  // some sloppy phrase names a term twice (SloppyPhraseScorer's repetition groups: k_sloppy_groups)
  int64_t phrase_lead_blocks = 0;  // the conjunctions' lead blocks: every phrase's rarest term
  for (int32_t q = 0; q < n_queries; ++q) {
    int64_t least = INT64_MAX;
    for (int i = 0; i < queries[q].n_terms; ++i) least = std::min<int64_t>(least, std::max<int64_t>(0, terms[queries[q].first_term + i].state.doc_freq));
    if (least != INT64_MAX) phrase_lead_blocks += least / 128;
  }
  const int blocks_per_item = and_item_blocks(c, phrase_lead_blocks);
  int64_t items = 0, slots = 0;
  for (int32_t q = 0; q < n_queries; ++q) {
    const rgpu_phrase_query& Q = queries[q];
    item_prefix[(size_t)q] = items;
    emit_prefix[(size_t)q] = slots;
    collect_prefix[(size_t)q] = collect_items;
    dq[(size_t)q] = DevQuery{RGPU_OP_AND, 0, (int32_t)dt.size(), 0};
    bool dead = false;
    RGPU_TRY(emit_phrase(seg, Q, terms, &dt, &pt, &dead));
    if (dead) continue;
    slops[(size_t)q] = Q.slop;
    limits[(size_t)q] = Q.next_limit == 0 ? 500000 /* searcher.rs:47 DEFAULT_DISMATCH_NEXT_LIMIT */
                                          : (Q.next_limit == RGPU_NEXT_LIMIT_ZERO ? 0 /* DefaultIndexSearcher::new(reader, Some(0)) */ : Q.next_limit);
    if (span) {
      // the loaders hand out position - phrase_pos: a span clause's positions are the term's own
      for (size_t i = pt.size() - (size_t)Q.n_terms; i < pt.size(); ++i) pt[i].phrase_pos = 0;
      two_phase[(size_t)q] = 1;
      any_span = true;
    } else {
      (Q.slop > 0 ? any_sloppy : any_exact) = true;
    }
    if (!span && Q.slop > 0) for (size_t i = pt.size() - (size_t)Q.n_terms; i < pt.size(); ++i) sloppy_rpts = sloppy_rpts || pt[i].same_as != pt[i].query_ord;
    dq[(size_t)q].n_terms = Q.n_terms;
    const DevTerm& lead = dt[(size_t)dq[(size_t)q].first_term];
    items += lead_items(lead, blocks_per_item);
    slots += lead_slots(lead);
    collect_items += lead_collect_chunks(lead);
    any_cutoff = any_cutoff || ((span || Q.slop > 0) && limits[(size_t)q] >= 0);
  }
  item_prefix[(size_t)n_queries] = items;
  emit_prefix[(size_t)n_queries] = slots;
  collect_prefix[(size_t)n_queries] = collect_items;
  RGPU_TRY(api_rows_default(c, stream, n_queries, k));
  if (items > 0) {
    SCRATCH_TAKE(c);
    Stager st(c);
    const size_t nq = (size_t)n_queries;
    const auto r_q = st.add<DevQuery>(nq);
    const auto r_t = st.add<DevTerm>(dt.size());
    const auto r_pt = st.add<PosTerm>(pt.size());
    const auto r_ip = st.add<int64_t>(nq + 1), r_ep = st.add<int64_t>(nq + 1);
    const auto r_sl = st.add<int32_t>(nq), r_nl = st.add<int32_t>(nq);
    const auto r_tp = st.add_if<int32_t>(span, nq);
    const auto r_gr = st.add<SloppyGroups>(nq);  // written by k_sloppy_groups
    const auto r_cp = st.add<int64_t>(nq + 1);   // the chunked collector's items
    const auto r_ab = st.add<int32_t>(nq);       // k_phrase_cutoff's flags (zeroed by the copy)
    const auto r_cut = st.add<PhraseCut>(nq);    // ... and what its chunked form reduces into
    const std::vector<TermBitmap> clause_bitmaps = clause_bitmap_table(seg, dq, dt, bitmap_df);
    const auto r_bm = st.add_if<TermBitmap>(!clause_bitmaps.empty(), clause_bitmaps.size());
    STAGE_SIZED(sg, st);
    sg.put(r_q, dq);
    sg.put(r_t, dt);
    sg.put(r_pt, pt);
    sg.put(r_sl, slops);
    sg.put(r_tp, two_phase);
    sg.put(r_nl, limits);
    sg.put(r_ip, item_prefix);
    sg.put(r_ep, emit_prefix);
    sg.put(r_cp, collect_prefix);
    sg.fill(r_ab, 0);
    for (size_t q = 0; q < nq; ++q) sg.host(r_cut)[q] = PhraseCut{0x7fffffff, 0x7fffffff, 0ull};
    // "no repetition group" for every query (grp = -1): k_sloppy_groups only runs when some phrase repeats a term, k_sloppy_match
    // reads the region either way (the copy used to carry whatever the pinned buffer held)
    sg.fill(r_gr, 0xff);
    sg.put(r_bm, clause_bitmaps);
    RGPU_TRY(sg.upload(stream));
    const DevQuery* d_q = sg.dev(r_q);
    const DevTerm* d_t = sg.dev(r_t);
    const int64_t *d_ep = sg.dev(r_ep), *d_cp = sg.dev(r_cp);
    const int32_t *d_sl = sg.dev(r_sl), *d_nl = sg.dev(r_nl);
    PhraseCut* d_cut = sg.dev(r_cut);
    const bool chunked = phrase_collect_chunked(k, collect_items);
    int64_t redo_cap = 0;
    // (k_emit: the conjunction only emits candidates, its (empty) top-k lists are the narrow kind)
    const char* stage_name = masked.on() ? masked_stage_name(c, "k_search_and(masked phrase candidates)", "k_search_and(masked phrase, marked)")
                                         : (span ? "k_search_and(span candidates)" : "k_search_and(phrase candidates)");
    const int32_t* d_collect_sl = span ? sg.dev(r_tp) : d_sl;  // "two-phase" to the collectors: slop > 0, or a span query
    RGPU_TRY(and_emit_stage(seg, stream, AndEmitStage{stage_name, d_q, d_t, sg.dev(r_ip), d_ep, clause_bitmaps.empty() ? nullptr : sg.dev(r_bm),
                                                      n_queries, nq, items, slots, blocks_per_item, std::min<int>(k, 64), false,
                                                      chunked ? (size_t)collect_items * (size_t)k : 0, chunked ? (size_t)collect_items : 0,
                                                      &redo_cap, false /* the collectors read a query's first emit_count slots only */,
                                                      masked.on() && c->phrase_mask_compact}));
    RGPU_TRY(phrase_match_stage(seg, stream, PhraseMatchStage{d_q, d_t, sg.dev(r_pt), d_ep, d_sl, sg.dev(r_gr), n_queries, slots, redo_cap, any_exact, any_sloppy,
                                                              sloppy_rpts, true, d_cut, d_cp, d_nl, collect_items, any_span, span && unordered}));
    phrase_collect_stage(seg, stream, PhraseCollectStage{d_ep, d_cp, d_collect_sl, d_nl, n_queries, k, collect_items, any_cutoff, sg.dev(r_ab), d_cut});
    HIP_TRY(launch_status());
  }
  // the verdict in the same round as the rows (nothing launched: nothing to ask, and d_err may hold another call's)
  int err = 0;
  RGPU_TRY(api_rows_read_back(c, stream, n_queries, k, hits_out, total_hits_out, items > 0 ? &err : nullptr));
  return phrase_match_status(err, span ? (unordered ? "a doc holds the terms of an unordered span query's clauses more than 2048 times in all"
                                                   : "a doc holds the term of a span clause more than 1024 times")
                                       : "a doc holds one of an exact phrase's terms more than 1024 times (a sloppy phrase's terms: more than 2048 times in all)",
                             "internal: a conjunction match was not found again");
}
// (include/rucene_gpu.h rgpu_search_span_near_batch; the match kernels: kernels/search_span.hpp)
extern "C" int32_t rgpu_search_span_near_batch(rgpu_segment* seg, const rgpu_phrase_query* queries, int32_t n_queries,
                                               const rgpu_phrase_term* terms, int32_t n_terms_total, int32_t in_order, int32_t k,
                                               rgpu_hit* hits_out, int64_t* total_hits_out) {
  // NearSpansUnordered is another walk and another call: rgpu_search_span_unordered_batch
  if (in_order == 0) return fail(RGPU_ERR_UNSUPPORTED, "span near: only in_order = true is served (unordered near: rgpu_search_span_unordered_batch)");
  return search_phrase_batch_impl(seg, nullptr, queries, n_queries, terms, n_terms_total, k, hits_out, total_hits_out, true);
}
// (include/rucene_gpu.h rgpu_search_span_unordered_batch; the match kernels: kernels/search_span_unordered.hpp)
extern "C" int32_t rgpu_search_span_unordered_batch(rgpu_segment* seg, const rgpu_phrase_query* queries, int32_t n_queries,
                                                    const rgpu_phrase_term* terms, int32_t n_terms_total, int32_t k, rgpu_hit* hits_out,
                                                    int64_t* total_hits_out) {
  return search_phrase_batch_impl(seg, nullptr, queries, n_queries, terms, n_terms_total, k, hits_out, total_hits_out, true, true);
}
extern "C" int32_t rgpu_search_phrase_batch(rgpu_segment* seg, const rgpu_phrase_query* queries, int32_t n_queries,
                                            const rgpu_phrase_term* terms, int32_t n_terms_total, int32_t k, rgpu_hit* hits_out,
                                            int64_t* total_hits_out) {
  return search_phrase_batch_impl(seg, nullptr, queries, n_queries, terms, n_terms_total, k, hits_out, total_hits_out);
}
extern "C" int32_t rgpu_search_phrase_batch_masked(rgpu_segment* seg, rgpu_docset* set, const rgpu_phrase_query* queries, int32_t n_queries,
                                                   const rgpu_phrase_term* terms, int32_t n_terms_total, int32_t k, rgpu_hit* hits_out,
                                                   int64_t* total_hits_out) {
  if (!set) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  return search_phrase_batch_impl(seg, set, queries, n_queries, terms, n_terms_total, k, hits_out, total_hits_out);
}

