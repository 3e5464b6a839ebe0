// SpanNearQuery(in_order = true) over SpanTermQuery clauses on the GPU: the match kernels of rgpu_search_span_near_batch.
// Candidates (k_search_and in emit mode), the redo list and the collectors are the phrase path's (search_phrase.hpp); what is
// new is the walk that turns a candidate doc's positions into a span frequency.
//
// The reference (search/query/spans/): NearSpansOrdered (span_near.rs:725-852) takes every position p0 of clause 0 in ascending
// order and runs stretch_to_order (:759-776): clause i >= 1 is advanced to its first start >= end(i - 1) (advance_position,
// span.rs:214-219: it only ever moves forward), match_width sums start(i) - end(i - 1); a clause that runs out of positions ends
// the doc (one_exhausted_in_current_doc: later p0 are not looked at). A span counts iff match_width <= slop. SpanScorer
// (span.rs:489-519) adds compute_slop_factor(width) = 1 / (width + 1) (bm25_similarity.rs:65-67) per span, in the order the spans
// come out, to an f32 that starts at 0.0; the score is BM25(freq, norm). A doc is a hit when it has a span — there is no
// "> f32::EPSILON" rule as the sloppy phrase scorer has one. A SpanTermQuery's span is [position, position + 1), its own width 0
// (span_term.rs:170-200); every clause has its own iterator, so a term may be named by several clauses.
//
// end(i - 1) is non-decreasing in p0 (induction over i: end(0) = p0 + 1 ascends, and the first start >= a larger bound is no
// smaller), so the clause's persistent cursor stands exactly on the lower bound of end(i - 1) in its list, for every p0: the
// lanes kernel keeps cursors, the one-candidate kernel searches lower bounds — the same spans. Exhaustion is monotone for the same
// reason: once a p0's chain runs out of positions, every later p0's does.
//
// PosTerm::phrase_pos is 0 for every clause of a span query (the host sets it), so the loaders hand out plain positions;
// PosTerm::query_ord is the clause's index in the query (device clauses are in cost order for the conjunction).
#pragma once
#include "search_phrase.hpp"

namespace rgpu {

constexpr int PHRASE_REDO_SPAN_LANES = 16;  // bits of *redo: k_span_near at all (left by k_span_near_lanes) ...
constexpr int PHRASE_REDO_SPAN_WIDE = 32;   // ... and k_span_near with PHRASE_LIST_CAP lists
constexpr int32_t SPAN_EXHAUSTED = 0x7fffffff;

// ---- 64 candidates per wavefront ----------------------------------------------------------------------------------------------------
// Each lane runs the ordered walk for its own candidate: clause t's positions in the lane's LDS column t (16-bit cells, clause
// order; SLOPPY_LANE_TERMS x PHRASE_LANE_CAP x 64 cells per wavefront as k_sloppy_match_lanes), the clauses' cursors in registers
// (unrolled over SLOPPY_LANE_TERMS). More clauses, more than PHRASE_LANE_CAP positions of a clause's term in the doc, a position
// above 32767 and whatever lanes_doc_positions hands on go to k_span_near through the list (PHRASE_REDO_SPAN_LANES).
// slops: the TRUE slops (the collectors get a marker array instead: a span query is two-phase at slop 0 too).
__global__ __launch_bounds__(WG_THREADS) void k_span_near_lanes(SegView seg, const DevQuery* __restrict__ queries,
                                                                const DevTerm* __restrict__ terms, const PosTerm* __restrict__ pterms,
                                                                const int64_t* __restrict__ emit_prefix,
                                                                const unsigned long long* __restrict__ emit_count,
                                                                const int32_t* __restrict__ emit_docs, const int32_t* __restrict__ slops, int n_queries,
                                                                int64_t n_groups, int64_t pos_len, uint64_t* __restrict__ keys_out, int* redo,
                                                                int64_t* __restrict__ redo_list, int redo_cap, int* redo_n) {
  constexpr int NT = SLOPPY_LANE_TERMS;
  __shared__ __attribute__((aligned(16))) int32_t areas[WG_WAVES][384];
  __shared__ int16_t lists[WG_WAVES][NT][PHRASE_LANE_CAP * 64];
  const int lane = lane_id();
  const int wave = wave_id();
  const int64_t group = (int64_t)blockIdx.x * WG_WAVES + wave;
  if (group >= n_groups) return;
  const int64_t slot = group * 64 + lane;
  const int q = upper_slot_wave(emit_prefix, n_queries, group * 64, lane);
  const int slop = slops[q];
  const int64_t idx = slot - emit_prefix[q];
  const int64_t cnt = (int64_t)emit_count[q];
  if (idx - lane >= cnt) return;  // nothing in these 64 slots (the collectors read the first emit_count[q] slots only)
  const int32_t doc = idx < cnt ? emit_docs[slot] : -1;
  const bool act = doc >= 0;  // (a deleted doc: an approximation that is never checked, bulk_scorer.rs:100)
  bool again = false;
  const DevQuery Q = queries[q];
  const int n = Q.n_terms;
  bool takes = n >= 2 && n <= NT;
  for (int c = 0; takes && c < n; ++c) {  // (a clause index outside the columns cannot come from the host's plan; it hands the query on)
    const int o = pterms[Q.first_term + c].query_ord;
    if (o < 0 || o >= n) takes = false;
  }
  if (!takes) again = act;
  // ---- every clause's positions in the lane's doc: column = the clause's index in the query
  int32_t fr[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) fr[t] = 0;
  for (int c = 0; takes && c < n; ++c) {
    if (!__ballot(act && !again)) break;
    const DevTerm T = terms[Q.first_term + c];
    const PosTerm P = pterms[Q.first_term + c];
    const int f = lanes_doc_positions<int16_t>(seg, T, P, doc, act, again, pos_len, areas[wave], lists[wave][P.query_ord], lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) fr[t] = t == P.query_ord ? f : fr[t];
  }
  const bool live = act && !again;
  float sfreq = 0.0f;
  bool has_span = false;
  if (live) {
    const int16_t* L = &lists[wave][0][0];
    int32_t cur[NT];  // clause t's cursor: it never moves back within the doc
#pragma unroll
    for (int t = 0; t < NT; ++t) cur[t] = 0;
    bool exhausted = false;
    for (int i0 = 0; i0 < fr[0] && !exhausted; ++i0) {
      int32_t end = (int32_t)L[i0 * 64 + lane] + 1;  // a SpanTermQuery's span: [position, position + 1)
      int32_t width = 0;
#pragma unroll
      for (int t = 1; t < NT; ++t) {
        if (t < n && !exhausted) {  // stretch_to_order (:759-776)
          int k = cur[t];
          int32_t s = 0;
          while (k < fr[t]) {  // advance_position(end(t - 1))
            s = (int32_t)L[(t * PHRASE_LANE_CAP + k) * 64 + lane];
            if (s >= end) break;
            ++k;
          }
          cur[t] = k;
          if (k >= fr[t]) {
            exhausted = true;  // one_exhausted_in_current_doc
          } else {
            width += s - end;
            end = s + 1;
          }
        }
      }
      if (!exhausted && width <= slop) {
        sfreq += 1.0f / ((float)width + 1.0f);  // compute_slop_factor (bm25_similarity.rs:65-67)
        has_span = true;
      }
    }
  }
  uint64_t key = 0ull;
  if (live && has_span) {
    const DevTerm T0 = terms[Q.first_term];
    const float* table = seg.sim_tables + (size_t)T0.sim_table * 257;
    const float k1 = table[256];
    float nrm = k1;
    if (seg.norms != nullptr) {
      const uint32_t nb = seg.norms[doc];
      nrm = table[seg.n_norm_ranks > 0 ? (uint32_t)seg.rank_to_norm[nb] : nb];
    }
    key = make_key(bm25_score(T0.weight * (k1 + 1.0f), sfreq, nrm), doc);
  }
  lanes_finish(again, key, slot, keys_out, redo, PHRASE_REDO_SPAN_LANES, redo_list, redo_cap, redo_n, lane);
}

// ---- one candidate per wavefront ------------------------------------------------------------------------------------------------------
// What the lanes kernel hands on, and every candidate of a legacy (.doc version 0) segment. The wavefront keeps one chain per p0:
// E[i] = end of the chain that starts at clause 0's i-th position (SPAN_EXHAUSTED once it ran out of positions), W[i] = its width
// so far. Clause after clause in QUERY order, the clause's positions go to C and every lane takes the chains i = lane, lane + 64, ..:
// the lower bound of E[i] in C is where the clause's cursor stands for that p0 (see the header comment). The f32 sum is then formed
// over i ascending — the order the spans come out — by every lane alike (LDS broadcasts), and a chain that ran out ends it.
// CAP / REDO_ONLY: as k_phrase_match's — PHRASE_SMALL_CAP lists first; a doc that holds a clause's term more often leaves
// PHRASE_REDO and raises PHRASE_REDO_SPAN_WIDE, the CAP = PHRASE_LIST_CAP instantiation takes it; more than that: -5 in *err.
// Bounds: i < n_a <= CAP indexes E and W, lo < freq <= CAP indexes C; the loader writes at most `cap` entries.
template <bool LEGACY, int CAP, bool REDO_ONLY>
__global__ __launch_bounds__(WG_THREADS) void k_span_near(SegView seg, const DevQuery* __restrict__ queries,
                                                          const DevTerm* __restrict__ terms, const PosTerm* __restrict__ pterms,
                                                          const int64_t* __restrict__ emit_prefix,
                                                          const unsigned long long* __restrict__ emit_count,
                                                          const int32_t* __restrict__ emit_docs, const int32_t* __restrict__ slops, int n_queries,
                                                          int64_t n_slots, int64_t pos_len, uint64_t* __restrict__ keys_out, int* err, int* redo,
                                                          const int64_t* __restrict__ redo_list, int64_t first) {
  // (first / n_slots / redo_list: as k_phrase_match's)
  __shared__ __attribute__((aligned(16))) uint8_t slabs[WG_WAVES][SLAB_BYTES];
  __shared__ int32_t lists_e[WG_WAVES][CAP];
  __shared__ int32_t lists_w[WG_WAVES][CAP];
  __shared__ int32_t lists_c[WG_WAVES][CAP];
  __shared__ float caches[WG_WAVES][256];
  const int lane = lane_id();
  const int wave = wave_id();
  const int64_t work = first + (int64_t)blockIdx.x * WG_WAVES + wave;
  if (work >= n_slots) return;
  const int64_t slot = (REDO_ONLY && redo_list != nullptr) ? redo_list[work] : work;
  if (REDO_ONLY && keys_out[slot] != PHRASE_REDO) return;
  const int q = upper_slot_wave(emit_prefix, n_queries, slot, lane);
  const int slop = slops[q];
  const int64_t idx = slot - emit_prefix[q];
  if ((unsigned long long)idx >= emit_count[q]) {  // the conjunction produced fewer matches than the lead term has docs
    if (lane == 0) keys_out[slot] = 0ull;
    return;
  }
  const int32_t doc = emit_docs[slot];
  if (doc < 0) {  // a deleted doc (marked by the conjunction): an approximation that is never checked (bulk_scorer.rs:100)
    if (lane == 0) keys_out[slot] = 0ull;
    return;
  }
  const DevQuery Q = queries[q];
  const int n = Q.n_terms;
  uint8_t* slab = slabs[wave];
  int32_t* E = lists_e[wave];
  int32_t* W = lists_w[wave];
  int32_t* C = lists_c[wave];
  auto give_up = [&](int code) {
    if (lane == 0) { atomicMin(err, code); keys_out[slot] = 0ull; }
  };
  // lane c: the query-order index of device clause c
  const int32_t my_ord = lane < n ? pterms[Q.first_term + lane].query_ord : -1;
  int n_a = 0;
  for (int o = 0; o < n; ++o) {
    const uint64_t who = __ballot(my_ord == o);
    if (!who) { give_up(-4); return; }  // (cannot come from the host's plan)
    const int c = (int)__builtin_ctzll(who);
    const DevTerm T = terms[Q.first_term + c];
    const PosTerm P = pterms[Q.first_term + c];
    const int freq = phrase_doc_positions<LEGACY>(seg, T, P, doc, pos_len, slab, o == 0 ? E : C, CAP, lane);
    if (freq == -5 && CAP < PHRASE_LIST_CAP) {  // does not fit the small lists: the big instantiation takes this candidate
      if (lane == 0) { keys_out[slot] = PHRASE_REDO; atomicOr(redo, PHRASE_REDO_SPAN_WIDE); }
      return;
    }
    if (freq < 0) { give_up(freq); return; }
    if (o == 0) {
      n_a = freq;
      for (int i = lane; i < n_a; i += 64) { E[i] = E[i] + 1; W[i] = 0; }
    } else {
      for (int i = lane; i < n_a; i += 64) {
        const int32_t e = E[i];
        if (e != SPAN_EXHAUSTED) {
          int lo = 0, hi = freq;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (C[mid] < e) lo = mid + 1; else hi = mid;
          }
          if (lo >= freq) {
            E[i] = SPAN_EXHAUSTED;
          } else {
            const int32_t s = C[lo];
            W[i] += s - e;
            E[i] = s + 1;
          }
        }
      }
    }
    wave_sync();
  }
  float sfreq = 0.0f;
  bool has_span = false;
  for (int i = 0; i < n_a; ++i) {  // (wave-uniform: every lane forms the same sum, in p0 order)
    if (E[i] == SPAN_EXHAUSTED) break;
    const int32_t width = W[i];
    if (width <= slop) {
      sfreq += 1.0f / ((float)width + 1.0f);  // compute_slop_factor (bm25_similarity.rs:65-67)
      has_span = true;
    }
  }
  uint64_t key = 0ull;
  if (has_span) {
    const DevTerm T0 = terms[Q.first_term];
    float k1;
    load_sim_table(seg, T0.sim_table, caches[wave], lane, k1);
    wave_sync();
    const float wk = T0.weight * (k1 + 1.0f);
    const float nrm = seg.norms != nullptr ? caches[wave][seg.norms[doc]] : k1;
    key = make_key(bm25_score(wk, sfreq, nrm), doc);
  }
  if (lane == 0) keys_out[slot] = key;
}

}  // namespace rgpu
