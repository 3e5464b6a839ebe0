// SpanNearQuery(in_order = false) over SpanTermQuery clauses on the GPU: the match kernels of rgpu_search_span_unordered_batch.
// Candidates (k_search_and in emit mode), the redo list and the collectors are the phrase path's (search_phrase.hpp), the position
// loaders are shared with the ordered kernels (search_span.hpp); what is new is NearSpansUnordered's walk.
//
// The reference (search/query/spans/span_near.rs:333-528). One doc that holds every clause's term:
//   set-up   sub_span_cells_to_positions_queue (:393-404): the heap is cleared; cells 0 .. n - 1, in clause order, move to their
//            first position (SpansCell::next_start_position, :581-588: adjust_length, adjust_max) and are pushed
//            (binary_heap.rs:131-135: data.push, sift_up(0, old_len)).
//   at_match (:406-412) end(max cell) - start(heap top) - total_span_length <= slop. A term span is [p, p + 1) (span_term.rs:170-200),
//            so total_span_length is n once every cell stands on a position, and with width() = start(max cell) - start(heap top)
//            (:512-515) a span counts iff width <= slop + n - 1.
//   the loop two_phase_current_doc_matches (:428-447) and next_start_position (:451-486) are one loop cut in two: evaluate
//            at_match; advance the heap's TOP cell through peek_mut (next_start_position, adjust_length, adjust_max); PeekMut's drop
//            runs sift_down(0) = sift_down_range(0, len) (binary_heap.rs:29-35, :167-190); a cell without a further position ends
//            the doc there (:443-445, :475-480) - positions of the other clauses behind it are never looked at.
//   order    SpansCellElement::cmp (:681-696) is reversed: a <= b in the heap's sense is (start_a, end_a) >= (start_b, end_b), and
//            end = start + 1 here, so the start alone decides. sift_up (binary_heap.rs:149-163) stops at element <= parent: the new
//            cell climbs only past a parent with a STRICTLY greater start. sift_down_range takes the right child when
//            left <= right (start_left >= start_right) and stops at element >= child (start_element <= start_child).
//            Among cells at one start the order is therefore the ARRAY's, and with two distinct terms at one position (stacked
//            tokens) which of them moves first changes the spans: the array is kept here operation by operation, never re-derived.
//   max cell adjust_max (:568-577) makes a cell the max cell iff its end is strictly greater than the max cell's. Ends only grow
//            within a doc and only the max cell's start / end are read, so "the max cell" is the running maximum of the starts.
//            max_end_position_cell_idx survives from the previous doc, whose TermSpans stand at -1 / -1 on a fresh doc
//            (span_term.rs:188-196): cell 0's first position (>= 0) beats the -1, or cell 0 is that cell - either way the maximum
//            after set-up is the maximum of the first positions. The previous doc's index is harmless.
//   scoring  SpanScorer::set_freq_current_doc (span.rs:489-519) adds 1 / (width + 1) per span, in f32 from 0.0, in the order the
//            spans come out; the score is BM25(freq, norm); a doc is a hit iff it has a span.
//
// PosTerm::phrase_pos is 0 for every clause (the host sets it); PosTerm::query_ord is the clause's index in the query.
#pragma once
#include "search_span.hpp"

namespace rgpu {

constexpr int PHRASE_REDO_SPAN_UNORD_LANES = 64;  // bits of *redo: k_span_unordered at all (left by k_span_unordered_lanes) ...
constexpr int PHRASE_REDO_SPAN_UNORD_WIDE = 128;  // ... and k_span_unordered with the SLOPPY_POOL pool

// ---- 64 candidates per wavefront ----------------------------------------------------------------------------------------------------
// Each lane runs the walk for its own candidate: clause t's positions in the lane's LDS column t (16-bit cells, as
// k_span_near_lanes: the same 36 864 B per workgroup). The lane's state is four registers and no array, so nothing is indexed
// dynamically and the kernel has no scratch:
//   heap  data[j] = (heap >> 3 j) & 7, j < n <= 6: clause indices, 18 bits
//   curs  clause t's cursor = (curs >> 4 t) & 15 <= PHRASE_LANE_CAP - 1 < 16, 24 bits
//   frs   clause t's freq   = (frs >> 4 t) & 15  <= PHRASE_LANE_CAP < 16
//   mx    the running maximum of the starts
// A cell's current start is read back from the column (start_of). More clauses, more than PHRASE_LANE_CAP positions of a clause's
// term in the doc, a position above 32767 and whatever lanes_doc_positions hands on go to k_span_unordered through the list
// (PHRASE_REDO_SPAN_UNORD_LANES).
// Bounds: a heap index j < n <= SLOPPY_LANE_TERMS; a heap entry is a clause index t < n; a cursor c < freq(t) <= PHRASE_LANE_CAP,
// so the cell (t * PHRASE_LANE_CAP + c) * 64 + lane lies inside the wavefront's lists. The loop advances one cursor per round:
// at most n * PHRASE_LANE_CAP rounds.
static_assert(PHRASE_LANE_CAP < 16 && SLOPPY_LANE_TERMS <= 8, "k_span_unordered_lanes packs cursors in 4 bits and heap entries in 3");
__global__ __launch_bounds__(WG_THREADS) void k_span_unordered_lanes(SegView seg, const DevQuery* __restrict__ queries,
                                                                     const DevTerm* __restrict__ terms, const PosTerm* __restrict__ pterms,
                                                                     const int64_t* __restrict__ emit_prefix,
                                                                     const unsigned long long* __restrict__ emit_count,
                                                                     const int32_t* __restrict__ emit_docs, const int32_t* __restrict__ slops,
                                                                     int n_queries, int64_t n_groups, int64_t pos_len, uint64_t* __restrict__ keys_out,
                                                                     int* redo, int64_t* __restrict__ redo_list, int redo_cap, int* redo_n) {
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
  uint32_t frs = 0;
  for (int c = 0; takes && c < n; ++c) {
    if (!__ballot(act && !again)) break;
    const DevTerm T = terms[Q.first_term + c];
    const PosTerm P = pterms[Q.first_term + c];
    const int f = lanes_doc_positions<int16_t>(seg, T, P, doc, act, again, pos_len, areas[wave], lists[wave][P.query_ord], lane);
    frs |= (uint32_t)(f > 0 && f <= PHRASE_LANE_CAP ? f : 0) << (4 * P.query_ord);
  }
  bool live = act && !again;
  for (int t = 0; t < n && t < NT; ++t) live = live && ((frs >> (4 * t)) & 15u) != 0u;  // (a clause without a position: not from the conjunction)
  float sfreq = 0.0f;
  bool has_span = false;
  if (live) {
    const int16_t* L = &lists[wave][0][0];
    uint32_t heap = 0, curs = 0;
    auto start_of = [&](int t) -> int32_t { return (int32_t)L[(t * PHRASE_LANE_CAP + (int)((curs >> (4 * t)) & 15u)) * 64 + lane]; };
    auto data = [&](int j) -> int { return (int)((heap >> (3 * j)) & 7u); };
    auto put = [&](int j, int t) { heap = (heap & ~(7u << (3 * j))) | ((uint32_t)t << (3 * j)); };
    int32_t mx = 0;
    for (int t = 0; t < n; ++t) {  // set-up: push cell t (data.push, sift_up(0, t))
      const int32_t p = start_of(t);
      mx = t == 0 || p > mx ? p : mx;
      int pos = t;
      while (pos > 0) {
        const int parent = (pos - 1) >> 1;
        const int pe = data(parent);
        if (!(p < start_of(pe))) break;  // element <= parent
        put(pos, pe);
        pos = parent;
      }
      put(pos, t);
    }
    while (true) {
      const int top = data(0);
      const int32_t width = mx - start_of(top);
      if (width - (n - 1) <= slop) {  // at_match
        sfreq += 1.0f / ((float)width + 1.0f);  // compute_slop_factor (bm25_similarity.rs:65-67)
        has_span = true;
      }
      const int c = (int)((curs >> (4 * top)) & 15u) + 1;
      if (c >= (int)((frs >> (4 * top)) & 15u)) break;  // the top cell has no further position: the doc ends here
      curs += 1u << (4 * top);
      const int32_t p = start_of(top);
      mx = p > mx ? p : mx;
      int pos = 0, child = 1;  // PeekMut::drop: sift_down_range(0, n)
      while (child < n) {
        int ce = data(child);
        int32_t cs = start_of(ce);
        if (child + 1 < n) {
          const int re = data(child + 1);
          const int32_t rs = start_of(re);
          if (cs >= rs) { ++child; ce = re; cs = rs; }  // left <= right: the right child
        }
        if (p <= cs) break;  // element >= child
        put(pos, ce);
        pos = child;
        child = 2 * pos + 1;
      }
      put(pos, top);
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
  lanes_finish(again || (act && !live), key, slot, keys_out, redo, PHRASE_REDO_SPAN_UNORD_LANES, redo_list, redo_cap, redo_n, lane);
}

// ---- one candidate per wavefront ------------------------------------------------------------------------------------------------------
// What the lanes kernel hands on, and every candidate of a legacy (.doc version 0) segment; up to SLOPPY_MAX_TERMS = 16 clauses.
// Every clause's positions go in one LDS pool, as k_sloppy_match's. Lane i keeps cell i (query order): s_start (its positions'
// offset in the pool), s_n (their count), s_at (the cursor), s_pos (the current start). Lane j keeps data[j] of the heap. The walk
// is wave-uniform scalar steps over readlane, the way k_sloppy_match walks its queue.
// POOL / REDO_ONLY: as k_sloppy_match's - SLOPPY_SMALL_POOL first; a doc whose clauses hold more positions in all leaves PHRASE_REDO
// and raises PHRASE_REDO_SPAN_UNORD_WIDE, the POOL = SLOPPY_POOL instantiation takes it; more than SLOPPY_POOL positions in all:
// -5 (RGPU_ERR_UNSUPPORTED) in *err, the sloppy phrases' rule.
// Bounds: the loader writes at most POOL - used entries at pool + used, so s_start + s_n <= used <= POOL and every pool offset
// s_start + s_at with s_at < s_n stays below POOL; a cursor moves only while s_at + 1 < s_n; heap indices are < n <= 16 < 64 lanes
// (n is checked against SLOPPY_MAX_TERMS here as well as on the host). One cursor advances per round: at most `used` rounds.
template <bool LEGACY, int POOL, bool REDO_ONLY>
__global__ __launch_bounds__(WG_THREADS) void k_span_unordered(SegView seg, const DevQuery* __restrict__ queries,
                                                               const DevTerm* __restrict__ terms, const PosTerm* __restrict__ pterms,
                                                               const int64_t* __restrict__ emit_prefix,
                                                               const unsigned long long* __restrict__ emit_count,
                                                               const int32_t* __restrict__ emit_docs, const int32_t* __restrict__ slops, int n_queries,
                                                               int64_t n_slots, int64_t pos_len, uint64_t* __restrict__ keys_out, int* err, int* redo,
                                                               const int64_t* __restrict__ redo_list, int64_t first) {
  // (first / n_slots / redo_list: as k_phrase_match's)
  __shared__ __attribute__((aligned(16))) uint8_t slabs[WG_WAVES][SLAB_BYTES];
  __shared__ int32_t pools[WG_WAVES][POOL];
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
  int32_t* pool = pools[wave];
  auto give_up = [&](int code) {
    if (lane == 0) { atomicMin(err, code); keys_out[slot] = 0ull; }
  };
  if (n < 2 || n > SLOPPY_MAX_TERMS) { give_up(-4); return; }  // (cannot come from the host's plan)
  // ---- every clause's positions in this doc; lane i keeps cell i (query order)
  int32_t s_start = 0, s_n = 0;
  int used = 0;
  for (int c = 0; c < n; ++c) {
    const DevTerm T = terms[Q.first_term + c];
    const PosTerm P = pterms[Q.first_term + c];
    const int freq = phrase_doc_positions<LEGACY>(seg, T, P, doc, pos_len, slabs[wave], pool + used, POOL - used, lane);
    if (freq == -5 && POOL < SLOPPY_POOL) {  // does not fit the small pool: the big instantiation takes this candidate
      if (lane == 0) { keys_out[slot] = PHRASE_REDO; atomicOr(redo, PHRASE_REDO_SPAN_UNORD_WIDE); }
      return;
    }
    if (freq < 0) { give_up(freq); return; }
    if (lane == P.query_ord) { s_start = used; s_n = freq; }
    used += freq;
  }
  if (__ballot(lane < n && s_n <= 0)) { give_up(-4); return; }  // a cell without a position (cannot come from the host's plan)
  wave_sync();
  int32_t s_at = 0;
  int32_t s_pos = lane < n ? pool[s_start] : 0;
  // std BinaryHeap<SpansCellElement>: lane j = data[j]
  int32_t heap = 0;
  int32_t mx = 0;
  for (int i = 0; i < n; ++i) {  // set-up: push cell i (data.push, sift_up(0, i))
    const int32_t p = readlane(s_pos, i);
    mx = i == 0 || p > mx ? p : mx;
    int pos = i;
    while (pos > 0) {
      const int parent = (pos - 1) >> 1;
      const int pe = readlane(heap, parent);
      if (!(p < readlane(s_pos, pe))) break;  // element <= parent
      heap = lane == pos ? pe : heap;
      pos = parent;
    }
    heap = lane == pos ? i : heap;
  }
  float sfreq = 0.0f;
  bool has_span = false;
  while (true) {  // (wave-uniform: every lane forms the same sum)
    const int top = readlane(heap, 0);
    const int32_t width = mx - readlane(s_pos, top);
    if (width - (n - 1) <= slop) {  // at_match
      sfreq += 1.0f / ((float)width + 1.0f);  // compute_slop_factor (bm25_similarity.rs:65-67)
      has_span = true;
    }
    const int a = readlane(s_at, top) + 1;
    if (a >= readlane(s_n, top)) break;  // the top cell has no further position: the doc ends here
    const int32_t p = pool[readlane(s_start, top) + a];
    s_at = lane == top ? a : s_at;
    s_pos = lane == top ? p : s_pos;
    mx = p > mx ? p : mx;
    int pos = 0, child = 1;  // PeekMut::drop: sift_down_range(0, n)
    while (child < n) {
      int ce = readlane(heap, child);
      int32_t cs = readlane(s_pos, ce);
      if (child + 1 < n) {
        const int re = readlane(heap, child + 1);
        const int32_t rs = readlane(s_pos, re);
        if (cs >= rs) { ++child; ce = re; cs = rs; }  // left <= right: the right child
      }
      if (p <= cs) break;  // element >= child
      heap = lane == pos ? ce : heap;
      pos = child;
      child = 2 * pos + 1;
    }
    heap = lane == pos ? top : heap;
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
