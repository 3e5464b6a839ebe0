// The stages every phrase call shares. PhraseMatchStage / phrase_match_stage: one key per candidate slot; the shared phrase plan (same_term,
// check_phrase_query, check_phrase_terms, phrase_is_dead, emit_phrase) and the verdict (phrase_match_status, phrase_match_verdict);
// phrase_collect_chunked, PhraseCollectStage / phrase_collect_stage: the keys into each row's top k. No entry point of its own.
// Uses: rgpu_api.hip itself (rgpu_ctx, rgpu_segment, fail, HIP_TRY / RGPU_TRY / RGPU_LAUNCH, TimedLaunch, HostClock, wg_count, seg_view,
// make_dev_term, launch_merge), positions.hpp (pos_term_of), kernels/search_phrase.hpp, search_span.hpp and search_span_unordered.hpp. The
// match stage's set-up, phrase_match_setup, is in candidates.hpp, and the size of its redo queue, phrase_redo_cap, in rows.hpp.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- the match stage of a phrase search: one key per candidate slot into c->phrase_keys ------------------------------------------
// The kernels read an array of candidate slots (emit_prefix / emit_count / emit_docs = c->phrase_count / c->phrase_docs) and do not
// care what filled it: and_emit_stage (the conjunction of rgpu_search_phrase_batch, _phrase_bool_batch and _phrase_or_batch) or
// k_rescore_phrase_candidates (the window of rgpu_rescore_phrase_batch). phrase_match_setup has run in front of whatever fills
// the slots (and_emit_stage runs it; a rescoring calls it): it reserves c->phrase_docs, c->phrase_keys and c->phrase_redo (redo_cap slots) and zeroes c->d_err. What
// comes behind the stage: phrase_collect_stage, k_phrase_bool_score, the run-building kernels of a disjunction,
// k_rescore_phrase_combine; the callers read the verdict, d_err[0], afterwards (phrase_match_status).
struct PhraseMatchStage {
  const DevQuery* d_q;
  const DevTerm* d_t;
  const PosTerm* d_pt;
  const int64_t* d_ep;
  const int32_t* d_sl;
  SloppyGroups* d_gr;
  int32_t n_queries;
  int64_t slots;     // a multiple of 64, every query's share too
  int64_t redo_cap;  // phrase_match_setup's
  bool any_exact, any_sloppy;
  bool sloppy_rpts;  // some sloppy phrase names a term twice
  // k_sloppy_groups (a search only: a rescoring refuses sloppy phrases that repeat a term and leaves the groups at "none")
  bool with_groups;
  PhraseCut* d_cut0;
  const int64_t* d_cp0;
  const int32_t* d_nl0;
  int64_t collect_items;
  // rgpu_search_span_near_batch: every live query of the call is an ordered SpanNearQuery (d_sl: its true slops) - the span
  // kernels run instead of the phrase kernels (any_exact and any_sloppy are false then)
  bool any_span = false;
  // rgpu_search_span_unordered_batch: the span queries are unordered (NearSpansUnordered) - kernels/search_span_unordered.hpp runs
  // in place of kernels/search_span.hpp, on the same ladder. No other caller sets it.
  bool unordered_span = false;
};
static int32_t phrase_match_stage(rgpu_segment* seg, hipStream_t stream, const PhraseMatchStage& a) {
  rgpu_ctx* c = seg->ctx;
  if (a.slots == 0 || !(a.any_exact || a.any_sloppy || a.any_span)) return RGPU_OK;  // no slot, or no live phrase to look at one: d_err stays "fine"
  const SegView sv = seg_view(seg);
  const bool legacy = seg->version < 1;
  // One wavefront per candidate slot, first with the small position lists / pools (seven wavefronts per SIMD). A doc that holds
  // a term more often than those hold positions (rare: Rucene clamps freqs to 10) leaves PHRASE_REDO in its slot: one look at
  // the flag, then the wide instantiations over the marked candidates only.
  // (one wavefront per slot: at most PHRASE_LAUNCH_SLOTS slots per launch — a grid of more than 2^32 work-items is cut short)
  auto per_slot = [&](int64_t n, auto launch) {
    for (int64_t s0 = 0; s0 < n; s0 += PHRASE_LAUNCH_SLOTS) {
      const int64_t s1 = std::min(n, s0 + PHRASE_LAUNCH_SLOTS);
      launch(dim3(wg_count((s1 - s0 + WG_WAVES - 1) / WG_WAVES)), s0, s1);
    }
  };
  // (list: null = every slot of the launch; else the listed slots — the ones a 64-candidate kernel handed on)
  auto exact = [&](auto kern, const int64_t* list, int64_t n) {
    per_slot(n, [&](dim3 grid, int64_t s0, int64_t s1) {
      RGPU_LAUNCH(kern, grid, dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl, (int)a.n_queries, s1,
                  (int64_t)seg->pos_len, c->phrase_keys.p, c->d_err, c->d_err + 3, list, s0);
    });
  };
  auto sloppy = [&](auto kern, const int64_t* list, int64_t n) {
    per_slot(n, [&](dim3 grid, int64_t s0, int64_t s1) {
      RGPU_LAUNCH(kern, grid, dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl, a.d_gr, (int)a.n_queries, s1,
                  (int64_t)seg->pos_len, c->phrase_keys.p, c->d_err, c->d_err + 3, list, s0);
    });
  };
  auto sloppy_groups = [&]() {  // the repetition groups of each query's first candidate doc (phrases with a repeated term)
    TimedLaunch tl(c, stream, "k_sloppy_groups", 0);
    if (a.collect_items > 0)  // every sloppy query's smallest live candidate, chunk by chunk
      RGPU_LAUNCH(k_phrase_cutoff_items<2>, dim3(wg_count((a.collect_items + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, a.d_cp0, a.d_ep,
                  c->phrase_count.p, c->phrase_keys.p, (const int32_t*)c->phrase_docs.p, a.d_sl, a.d_nl0, (int)a.n_queries, a.collect_items, a.d_cut0);
    const unsigned ggrid = wg_count((a.n_queries + WG_WAVES - 1) / WG_WAVES);
    auto go = [&](auto kern) {
      RGPU_LAUNCH(kern, dim3(ggrid), dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl,
                  (int)a.n_queries, (int64_t)seg->pos_len, a.d_gr, c->d_err, (const PhraseCut*)a.d_cut0);
    };
    if (legacy) go(k_sloppy_groups<true>); else go(k_sloppy_groups<false>);
  };
  const int64_t* const all_slots = nullptr;
  const int64_t groups = a.slots / 64;
  const dim3 lanes_grid(wg_count((groups + WG_WAVES - 1) / WG_WAVES));
  // ---- first pass. Packed (.doc version 1) segments: 64 candidates per wavefront; what those kernels hand on is listed.
  // Legacy segments (the packed streams of a block are laid out differently): one candidate per wavefront throughout.
  if (a.any_exact) {
    if (legacy) {
      TimedLaunch tl(c, stream, "k_phrase_match", 0);
      exact(k_phrase_match<true, PHRASE_SMALL_CAP, false>, all_slots, a.slots);
    } else {
      TimedLaunch tl(c, stream, "k_phrase_match_lanes", 0);
      RGPU_LAUNCH(k_phrase_match_lanes, lanes_grid, dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl,
                  (int)a.n_queries, groups, (int64_t)seg->pos_len, c->phrase_keys.p, c->d_err + 3, c->phrase_redo.p, (int)a.redo_cap, c->d_err + 2);
    }
  }
  if (a.any_sloppy) {
    if (legacy) {
      if (a.with_groups) sloppy_groups();
      TimedLaunch tl(c, stream, "k_sloppy_match", 0);
      sloppy(k_sloppy_match<true, SLOPPY_SMALL_POOL, false>, all_slots, a.slots);
    } else {
      if (a.sloppy_rpts) sloppy_groups();  // the repetition groups: k_sloppy_rpt_lanes (and what it hands on) needs them
      {
        TimedLaunch tl(c, stream, "k_sloppy_match_lanes", 0);
        RGPU_LAUNCH(k_sloppy_match_lanes, lanes_grid, dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl,
                    (int)a.n_queries, groups, (int64_t)seg->pos_len, c->phrase_keys.p, c->d_err + 3, c->phrase_redo.p, (int)a.redo_cap, c->d_err + 2,
                    a.sloppy_rpts ? 1 : 0);
      }
      if (a.sloppy_rpts) {  // phrases that repeat a term: the scorer's repeats machinery per lane
        TimedLaunch tl(c, stream, "k_sloppy_rpt_lanes", 0);
        RGPU_LAUNCH(k_sloppy_rpt_lanes, lanes_grid, dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl,
                    a.d_gr, (int)a.n_queries, groups, (int64_t)seg->pos_len, c->phrase_keys.p, c->d_err + 3, c->phrase_redo.p, (int)a.redo_cap, c->d_err + 2);
      }
    }
  }
  if (a.any_span && a.unordered_span) {  // unordered span-near queries: the sloppy phrases' ladder (one pool), NearSpansUnordered's walk
    if (legacy) {
      TimedLaunch tl(c, stream, "k_span_unordered", 0);
      exact(k_span_unordered<true, SLOPPY_SMALL_POOL, false>, all_slots, a.slots);
    } else {
      TimedLaunch tl(c, stream, "k_span_unordered_lanes", 0);
      RGPU_LAUNCH(k_span_unordered_lanes, lanes_grid, dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl,
                  (int)a.n_queries, groups, (int64_t)seg->pos_len, c->phrase_keys.p, c->d_err + 3, c->phrase_redo.p, (int)a.redo_cap, c->d_err + 2);
    }
  } else if (a.any_span) {  // ordered span-near queries: as the exact phrases' ladder, with the span walk (kernels/search_span.hpp)
    if (legacy) {
      TimedLaunch tl(c, stream, "k_span_near", 0);
      exact(k_span_near<true, PHRASE_SMALL_CAP, false>, all_slots, a.slots);
    } else {
      TimedLaunch tl(c, stream, "k_span_near_lanes", 0);
      RGPU_LAUNCH(k_span_near_lanes, lanes_grid, dim3(WG_THREADS), 0, stream, sv, a.d_q, a.d_t, a.d_pt, a.d_ep, c->phrase_count.p, c->phrase_docs.p, a.d_sl,
                  (int)a.n_queries, groups, (int64_t)seg->pos_len, c->phrase_keys.p, c->d_err + 3, c->phrase_redo.p, (int)a.redo_cap, c->d_err + 2);
    }
  }
  // ---- which candidates wait for another pass (bits PHRASE_REDO_*): one look per stage that can raise one
  int listed = 0, redo = 0;  // d_err[2]: slots on the list, d_err[3]: the bits
  auto redo_bits = [&]() -> int32_t {
    int two[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(two, c->d_err + 2, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    listed = two[0];
    redo = two[1];
    return RGPU_OK;
  };
  RGPU_TRY(redo_bits());
  // the one-candidate kernels over the listed slots (or, should the list have overflowed, over every slot)
  const bool by_list = !legacy && (int64_t)listed <= a.redo_cap;
  const int64_t* const left = by_list ? (const int64_t*)c->phrase_redo.p : all_slots;
  const int64_t n_left = by_list ? (int64_t)listed : a.slots;
  constexpr int REDO_FROM_LANES = PHRASE_REDO_LANES | PHRASE_REDO_SLOPPY_LANES | PHRASE_REDO_SPAN_LANES | PHRASE_REDO_SPAN_UNORD_LANES;
  if (HostClock::on() && (redo & REDO_FROM_LANES))
    std::fprintf(stderr, "[phrase] %d of %lld candidate slots left for the one-candidate kernels\n", listed, (long long)a.slots);
  if (redo & PHRASE_REDO_LANES) {
    TimedLaunch tl(c, stream, "k_phrase_match(left by the 64-candidate kernel)", 0);
    exact(k_phrase_match<false, PHRASE_SMALL_CAP, true>, left, n_left);
  }
  if (redo & PHRASE_REDO_SLOPPY_LANES) {
    TimedLaunch tl(c, stream, "k_sloppy_match(left by the 64-candidate kernel)", 0);  // (the groups are there: computed in front of the 64-candidate kernels)
    sloppy(k_sloppy_match<false, SLOPPY_SMALL_POOL, true>, left, n_left);
  }
  if (redo & PHRASE_REDO_SPAN_LANES) {
    TimedLaunch tl(c, stream, "k_span_near(left by the 64-candidate kernel)", 0);
    exact(k_span_near<false, PHRASE_SMALL_CAP, true>, left, n_left);
  }
  if (redo & PHRASE_REDO_SPAN_UNORD_LANES) {
    // ("unord": rgpu_kernel_stat.name holds 47 characters)
    TimedLaunch tl(c, stream, "k_span_unord(left by the 64-candidate kernel)", 0);
    exact(k_span_unordered<false, SLOPPY_SMALL_POOL, true>, left, n_left);
  }
  if (redo & REDO_FROM_LANES) RGPU_TRY(redo_bits());
  if (redo & PHRASE_REDO_WIDE) {
    TimedLaunch tl(c, stream, "k_phrase_match(wide lists)", 0);
    if (legacy) exact(k_phrase_match<true, PHRASE_LIST_CAP, true>, left, n_left); else exact(k_phrase_match<false, PHRASE_LIST_CAP, true>, left, n_left);
  }
  if (redo & PHRASE_REDO_SPAN_WIDE) {
    TimedLaunch tl(c, stream, "k_span_near(wide lists)", 0);
    if (legacy) exact(k_span_near<true, PHRASE_LIST_CAP, true>, left, n_left); else exact(k_span_near<false, PHRASE_LIST_CAP, true>, left, n_left);
  }
  if (redo & PHRASE_REDO_SPAN_UNORD_WIDE) {
    TimedLaunch tl(c, stream, "k_span_unordered(wide pool)", 0);
    if (legacy) exact(k_span_unordered<true, SLOPPY_POOL, true>, left, n_left); else exact(k_span_unordered<false, SLOPPY_POOL, true>, left, n_left);
  }
  if (redo & PHRASE_REDO_SLOPPY) {
    TimedLaunch tl(c, stream, "k_sloppy_match(wide pool)", 0);
    if (legacy) sloppy(k_sloppy_match<true, SLOPPY_POOL, true>, left, n_left); else sloppy(k_sloppy_match<false, SLOPPY_POOL, true>, left, n_left);
  }
  return RGPU_OK;
}

// ---- the plan in front of it, shared by the phrase search and the phrase rescoring -----------------------------------------------
// Term equality: how PosTerm::same_as tells repeated terms (repeating_terms, phrase_scorer.rs:909-931)
static bool same_term(const rgpu_term_state& a, const rgpu_term_state& b) {
  return a.doc_start_fp == b.doc_start_fp && a.doc_freq == b.doc_freq && a.singleton_doc_id == b.singleton_doc_id && a.total_term_freq == b.total_term_freq;
}
// a query's own fields (`searching`: next_limit is looked at, a rescoring has no use for it) ...
static int32_t check_phrase_query(const rgpu_ctx* c, const rgpu_phrase_query& Q, int32_t n_terms_total, bool searching) {
  if (Q.n_terms < 2 || Q.n_terms > RGPU_MAX_PHRASE_TERMS) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a phrase has 2..RGPU_MAX_PHRASE_TERMS terms");
  if (Q.slop < 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "Slop must be >= 0");  // PhraseQuery::new (phrase_query.rs:77)
  if (searching && Q.next_limit < RGPU_NEXT_LIMIT_ZERO) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "rgpu_phrase_query.next_limit: 0 (the searcher's default), n > 0, -1 (none) or RGPU_NEXT_LIMIT_ZERO");
  if (Q.first_term < 0 || (int64_t)Q.first_term + Q.n_terms > (int64_t)n_terms_total) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "term range outside terms[]");
  if (Q.sim_table < 0 || Q.sim_table >= c->n_sim_tables) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "unknown sim_table handle");
  return RGPU_OK;
}
// ... and its terms: those the leaf holds go to `ptrs` for the preparation, the ones of a row with an absent term too
static int32_t check_phrase_terms(const rgpu_segment* seg, const rgpu_phrase_query& Q, const rgpu_phrase_term* terms, std::vector<const rgpu_term_state*>* ptrs) {
  for (int i = 0; i < Q.n_terms; ++i) {
    const rgpu_phrase_term& t = terms[Q.first_term + i];
    if (t.state.doc_freq <= 0) continue;
    if (t.positions.pos_start_fp < 0 || (size_t)t.positions.pos_start_fp >= seg->pos_len) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "pos_start_fp outside the .pos file");
    if (t.state.total_term_freq < t.state.doc_freq) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "total_term_freq below doc_freq");
    ptrs->push_back(&t.state);
  }
  return RGPU_OK;
}
static bool phrase_is_dead(const rgpu_phrase_query& Q, const rgpu_phrase_term* terms) {  // a term absent from the leaf
  for (int i = 0; i < Q.n_terms; ++i) if (terms[Q.first_term + i].state.doc_freq <= 0) return true;
  return false;
}
// One query's clauses behind `dt` / `pt`, rarest term first: it drives the conjunction (conjunction_scorer.rs:30). *dead: nothing was
// pushed, PhraseWeight::create_scorer -> None (phrase_query.rs:275-283) — no doc of this leaf matches.
static int32_t emit_phrase(const rgpu_segment* seg, const rgpu_phrase_query& Q, const rgpu_phrase_term* terms, std::vector<DevTerm>* dt, std::vector<PosTerm>* pt, bool* dead) {
  *dead = phrase_is_dead(Q, terms);
  if (*dead) return RGPU_OK;
  const rgpu_phrase_term* mine = terms + Q.first_term;
  int order[RGPU_MAX_PHRASE_TERMS];
  for (int i = 0; i < Q.n_terms; ++i) order[i] = i;
  std::stable_sort(order, order + Q.n_terms, [&](int a, int b) { return mine[a].state.doc_freq < mine[b].state.doc_freq; });
  for (int o = 0; o < Q.n_terms; ++o) {
    const int i = order[o];
    dt->emplace_back();
    RGPU_TRY(make_dev_term(seg, mine[i].state, Q.weight, Q.sim_table, &dt->back()));
    PosTerm p = pos_term_of(mine[i].state, mine[i].positions);
    p.phrase_pos = mine[i].position;
    p.query_ord = i;  // PhrasePositions::ord: the sloppy scorer keeps the query's order (phrase_query.rs:324-331 does not sort)
    p.same_as = i;    // ... and tells repeated terms by Term equality
    for (int j = 0; j < i; ++j) if (same_term(mine[j].state, mine[i].state)) { p.same_as = j; break; }
    pt->push_back(p);
  }
  return RGPU_OK;
}
// what the match stage left in d_err[0], in the caller's words
static int32_t phrase_match_status(int err, const char* held_too_often, const char* not_found_again) {
  if (err == 0) return RGPU_OK;
  return fail(err, err == RGPU_ERR_UNSUPPORTED ? held_too_often : (err == RGPU_ERR_ILLEGAL_STATE ? not_found_again : "corrupt position data in .pos"));
}
// ... fetched by itself, synchronised: the calls that look at the verdict before they write anything to the caller's arrays
static int32_t phrase_match_verdict(rgpu_ctx* c, hipStream_t stream, const char* held_too_often, const char* not_found_again) {
  int err = 0;
  HIP_TRY(hipMemcpyAsync(&err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return phrase_match_status(err, held_too_often, not_found_again);
}

// ---- the collectors behind it: every query's best k keys (its candidate slots: and_emit_stage's) into the call's rows --------------
// k <= RGPU_PASS_K: one wavefront per chunk of PHRASE_COLLECT_CHUNK candidates (lead_collect_chunks), k_merge_items folds a query's
// lists; deeper pages (or nothing to chunk): one wavefront per query, in passes. The chunked collector's lists live in
// c->S->d_partial_keys / d_partial_counts: and_emit_stage is asked for collect_items * k and collect_items of them.
static bool phrase_collect_chunked(int32_t k, int64_t collect_items) { return k <= RGPU_PASS_K && collect_items > 0; }
struct PhraseCollectStage {
  const int64_t* d_ep;  // slots in front of each query's
  const int64_t* d_cp;  // chunks in front of each query's
  const int32_t* d_sl;  // slops
  const int32_t* d_nl;  // next_limit per query, -1: none
  int32_t n_queries, k;
  int64_t collect_items;
  // Some sloppy query has a next_limit (the two-phase rule: a query whose first collected doc has more than next_limit candidates
  // in front of it yields nothing): k_phrase_cutoff_items finds, chunk by chunk, the first collected doc and the candidates in
  // front of it into d_cut, k_phrase_cutoff_decide sets the flags. Without: d_ab is all zero (nothing is abandoned), d_cut unused.
  bool any_cutoff;
  int32_t* d_ab;
  PhraseCut* d_cut;
};
static void phrase_collect_stage(rgpu_segment* seg, hipStream_t stream, const PhraseCollectStage& a) {
  rgpu_ctx* c = seg->ctx;
  const bool wide = a.k > 64;  // the wide top-k lists
  if (phrase_collect_chunked(a.k, a.collect_items)) {
    {
      TimedLaunch tl(c, stream, "k_phrase_collect", 0);
      const unsigned grid = wg_count((a.collect_items + WG_WAVES - 1) / WG_WAVES);
      if (a.any_cutoff) {
        RGPU_LAUNCH(k_phrase_cutoff_items<0>, dim3(grid), dim3(WG_THREADS), 0, stream, a.d_cp, a.d_ep, c->phrase_count.p, c->phrase_keys.p,
                    (const int32_t*)c->phrase_docs.p, a.d_sl, a.d_nl, (int)a.n_queries, a.collect_items, a.d_cut);
        RGPU_LAUNCH(k_phrase_cutoff_items<1>, dim3(grid), dim3(WG_THREADS), 0, stream, a.d_cp, a.d_ep, c->phrase_count.p, c->phrase_keys.p,
                    (const int32_t*)c->phrase_docs.p, a.d_sl, a.d_nl, (int)a.n_queries, a.collect_items, a.d_cut);
        RGPU_LAUNCH(k_phrase_cutoff_decide, dim3(wg_count((a.n_queries + 255) / 256)), dim3(256), 0, stream, c->phrase_count.p, a.d_sl, a.d_nl, (int)a.n_queries,
                    a.d_cut, a.d_ab);
      }
      const auto collect_items = wide ? k_phrase_collect_items<true> : k_phrase_collect_items<false>;
      RGPU_LAUNCH(collect_items, dim3(grid), dim3(WG_THREADS), 0, stream, a.d_cp, a.d_ep, c->phrase_count.p, c->phrase_keys.p, (const int32_t*)a.d_ab,
                  (int)a.n_queries, a.collect_items, (int)a.k, c->S->d_partial_keys.p, c->S->d_partial_counts.p);
    }
    if (wide) launch_merge<true>(c, stream, a.n_queries, a.k, a.d_cp, seg->doc_base, c->host_api_hits.p, c->host_api_totals.p);
    else launch_merge<false>(c, stream, a.n_queries, a.k, a.d_cp, seg->doc_base, c->host_api_hits.p, c->host_api_totals.p);
  } else {
    TimedLaunch tl(c, stream, "k_phrase_collect", 0);
    const auto collect = wide ? k_phrase_collect<true> : k_phrase_collect<false>;
    RGPU_LAUNCH(collect, dim3(wg_count((a.n_queries + WG_WAVES - 1) / WG_WAVES)), dim3(WG_THREADS), 0, stream, a.d_ep, c->phrase_count.p, c->phrase_keys.p,
                (const int32_t*)c->phrase_docs.p, a.d_sl, a.d_nl, (int)a.n_queries, (int)a.k, seg->doc_base, c->host_api_hits.p, c->host_api_totals.p);
  }
}

