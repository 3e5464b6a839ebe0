// Cross-field BooleanQuery over TermQuery / DisjunctionMaxQuery groups (rgpu_search_fields_batch), in two stages:
//   1. k_score_terms   (search_or.hpp, as it stands) once per FIELD the batch names, with that field's view of the segment: every
//                      clause, MUST_NOT ones included, becomes a {doc, score} run closed by 64 sentinels — the TermScorer work, with
//                      the norm byte and the sim table of the clause's own field;
//   2. k_fields_windows  one wavefront per (query, range of W-doc windows). Per window: the MUST_NOT runs mark their docs; then the
//                      groups in the query's summation order (clause order under SHOULD — DisjunctionSumScorer over a SimpleQueue,
//                      disjunction_scorer.rs:213-225 —, the leaf's stable cost order under MUST — conjunction_scorer.rs:30, 87-95; the
//                      host has sorted them): each disjunct's run is walked from its cursor into a per-doc group sum and group maximum
//                      (from 0.0f / -inf, disjunct order: disjunction_scorer.rs:246-262), the group is folded into the doc's outer sum
//                      (max + (sum - max) * tie as three f32 operations for a dismax group, the clause's own score for a term group;
//                      the first group on a doc stores 0.0f + g under SHOULD and g under MUST, later ones add) and the doc's group
//                      count goes up by one. The scan offers every doc whose count reaches the query's `need`, that no prohibited
//                      clause holds and that is live, to the wave's top-k (wave.hpp); k_merge_items folds the per-item lists.
// Nothing is decoded in the window kernel (dense clauses inside it, doc bitmaps for MUST and k > 128 are the next steps: DESIGN.md).
#pragma once
#include "search_or.hpp"

namespace rgpu {

struct FieldsGroupDev {  // host/fields_plan.hpp FieldsPlanGroup
  int32_t first_term, n_terms;
  uint32_t tie_bits;
  int32_t kind;  // 0: the one clause's score; 1: max + (sum - max) * tie
};
struct FieldsQueryDev {  // host/fields_plan.hpp FieldsPlanQuery
  int32_t first_group, n_groups, first_not, n_not, need, must;
};

constexpr int FIELDS_WAVES = 8;
constexpr int FIELDS_THREADS = 64 * FIELDS_WAVES;
// Per wavefront and doc of a window: outer sum, group sum, group maximum (f32 each) and one byte — the group count in its low
// nibble (at most 9), FIELDS_IN_GROUP while the current group has touched the doc, FIELDS_EXCLUDED once a prohibited clause holds it.
// 512 docs: 6656 B per wavefront, 53 248 B per workgroup of eight — three workgroups (24 wavefronts, six per SIMD) share a CU's
// 160 KB; 1024 docs would leave one workgroup per CU.
constexpr int FIELDS_WINDOW_DOCS = 512;
constexpr uint32_t FIELDS_IN_GROUP = 0x10u, FIELDS_EXCLUDED = 0x80u, FIELDS_COUNT_MASK = 0x0fu;
constexpr int FIELDS_MAX_CLAUSES = 128;  // RGPU_MAX_FIELDS_QUERY_CLAUSES: two cursors per lane
__host__ __device__ constexpr size_t fields_wave_lds_bytes(int W) { return (size_t)W * 13; }
__host__ __device__ constexpr size_t fields_lds_bytes(int W) { return (size_t)FIELDS_WAVES * fields_wave_lds_bytes(W); }

// A workgroup's wavefronts work on one query (items_per_query is a multiple of FIELDS_WAVES); workgroup b takes query b % n_queries,
// as k_or_windows does, so that a query's later workgroups start from the thresholds its earlier ones published (SharedTau).
template <bool WIDE>
__global__ __launch_bounds__(FIELDS_THREADS) void k_fields_windows(SegView seg, const FieldsQueryDev* __restrict__ queries,
                                                                   const FieldsGroupDev* __restrict__ groups,
                                                                   const int32_t* __restrict__ run_len,
                                                                   const int64_t* __restrict__ run_prefix,
                                                                   const ScoredPosting* __restrict__ runs, int n_queries,
                                                                   int windows_per_query, int windows_per_item, int items_per_query,
                                                                   int W, int k, uint64_t* __restrict__ partial_keys,
                                                                   int32_t* __restrict__ partial_counts,
                                                                   unsigned long long* __restrict__ tau_slots) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  const int wave = wave_id();
  uint8_t* slice = smem + (size_t)wave * fields_wave_lds_bytes(W);
  float* acc = reinterpret_cast<float*>(slice);  // the outer sum: valid where the count is not 0
  float* gsum = acc + W;                         // the current group's sum and maximum: valid where FIELDS_IN_GROUP is set
  float* gmax = gsum + W;
  uint8_t* flag = reinterpret_cast<uint8_t*>(gmax + W);
  const int q = (int)(blockIdx.x % (unsigned)n_queries);
  const int g = (int)(blockIdx.x / (unsigned)n_queries) * FIELDS_WAVES + wave;
  const int64_t item = (int64_t)q * items_per_query + g;
  const FieldsQueryDev Q = queries[q];
  const bool has_live = seg.live != nullptr;

  WaveTopK top;
  uint64_t tau = 0, floor = 0;
  int hits_lane = 0;
  SharedTau shared{tau_slots + q};
  shared.fold(shared.peek(), tau, floor);
  const int win0 = g * windows_per_item;
  const int win1 = Q.n_groups > 0 ? min(windows_per_query, win0 + windows_per_item) : win0;  // a query that is dead in this leaf: nothing
  const int32_t first_doc = win0 * W;

  // ---- cursors: the query's clauses are one flat range [c0, c0 + n_cl) — its groups' disjuncts in summation order, then the MUST_NOT
  // clauses; lane l owns the cursors of clauses l and l + 64 (slot 0 / 1): the absolute index of the first entry with doc >= the
  // item's first window, found by one lane-parallel binary search per slot, and the doc under it (INT_MAX: exhausted)
  const int c0 = Q.n_groups > 0 ? groups[Q.first_group].first_term : Q.first_not;
  const int n_cl = Q.first_not + Q.n_not - c0;
  int64_t at0 = 0, at1 = 0;
  int32_t next0 = 0x7fffffff, next1 = 0x7fffffff;
  if (win0 < win1) {
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
      const int cl = lane + 64 * slot;
      const bool mine = cl < n_cl;
      const int64_t base = mine ? run_prefix[c0 + cl] : 0;
      int lo = 0, hi = mine ? run_len[c0 + cl] : 0;
      while (__ballot(lo < hi)) {
        if (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (runs[base + mid].doc < first_doc) lo = mid + 1; else hi = mid;
        }
      }
      const int64_t at = base + lo;
      const int32_t next = mine ? runs[at].doc : 0x7fffffff;  // (a run ends in sentinels: at most its first one)
      if (slot == 0) { at0 = at; next0 = next; } else { at1 = at; next1 = next; }
    }
  }
  for (int i = lane; i < W / 4; i += 64) reinterpret_cast<uint32_t*>(flag)[i] = 0u;
  wave_sync();

  for (int win = win0; win < win1; ++win) {
    const int32_t w0 = win * W;
    const int32_t w1 = min(seg.max_doc, w0 + W);
    const uint32_t wlen = (uint32_t)(w1 - w0);
    const uint64_t active0 = __ballot(next0 < w1), active1 = __ballot(next1 < w1);  // clauses with a posting in this window
    bool touched_any = false;  // wave-uniform: some flag byte of this window is not 0

    // one clause's postings of this window, from its cursor; MARK: a prohibited clause, GROUP: a disjunct of the current group
    auto walk = [&](int cl, bool prohibited) {
      const int src = cl & 63;
      const bool hi_slot = cl >= 64;
      const int64_t at = (int64_t)readlane64((uint64_t)(hi_slot ? at1 : at0), src);
      int taken = 0;
      int32_t next;
      ScoredPosting e = runs[at + lane];
      while (true) {
        const bool in = e.doc < w1;  // runs are doc-sorted: the in-window entries are a prefix (docs >= w0: the cursor's invariant)
        const int n = __popcll(__ballot(in));
        const uint32_t o = (uint32_t)(e.doc - w0);
        if (in && o < wlen) {  // all docs of one clause are distinct: no two lanes meet in one cell
          const uint32_t f = flag[o];
          if (prohibited) {
            flag[o] = (uint8_t)(f | FIELDS_EXCLUDED);
          } else if (f & FIELDS_IN_GROUP) {
            gsum[o] = gsum[o] + e.score;             // score_sum += sub_score
            gmax[o] = fmaxf(gmax[o], e.score);       // score_max = score_max.max(sub_score)
          } else {
            gsum[o] = 0.0f + e.score;                // from score_sum = 0
            gmax[o] = e.score;                       // from -inf
            flag[o] = (uint8_t)(f | FIELDS_IN_GROUP);
          }
        }
        taken += n;
        if (n < 64) { next = readlane(e.doc, n); break; }
        e = runs[at + taken + lane];  // a stretch longer than 64
      }
      if (lane == src) {
        if (hi_slot) { at1 += taken; next1 = next; } else { at0 += taken; next0 = next; }
      }
      touched_any = true;
      wave_sync();
    };
    auto is_active = [&](int cl) -> bool { return (((cl >= 64 ? active1 : active0) >> (cl & 63)) & 1ull) != 0ull; };

    // ---- ReqNotScorer: the prohibited clauses' docs first
    for (int i = 0; i < Q.n_not; ++i) {
      const int cl = Q.first_not - c0 + i;
      if (is_active(cl)) walk(cl, true);
    }
    // ---- the groups, in summation order
    for (int gi = 0; gi < Q.n_groups; ++gi) {
      const FieldsGroupDev G = groups[Q.first_group + gi];
      bool group_touched = false;
      for (int i = 0; i < G.n_terms; ++i) {
        const int cl = G.first_term - c0 + i;
        if (is_active(cl)) { walk(cl, false); group_touched = true; }
      }
      if (!group_touched) continue;
      // fold the group into the outer sum of the docs it touched: four docs per lane per step
      const float tie = __uint_as_float(G.tie_bits);
      const bool dismax = G.kind != 0;
      for (uint32_t i0 = 0; i0 < wlen; i0 += 256) {
        const uint32_t at = i0 + 4u * (uint32_t)lane;
        uint32_t f4 = *reinterpret_cast<const uint32_t*>(flag + at);
        if (f4 & 0x10101010u) {
          const float4 s4 = *reinterpret_cast<const float4*>(gsum + at);
          const float4 m4 = *reinterpret_cast<const float4*>(gmax + at);
          float4 a4 = *reinterpret_cast<const float4*>(acc + at);
          auto fold = [&](int j, float s, float m, float& a) {
            const uint32_t f = (f4 >> (8 * j)) & 0xffu;
            if (!(f & FIELDS_IN_GROUP)) return;
            float gsc = m;  // a term group: the clause's own score
            if (dismax) {   // three f32 operations (the library is built with -ffp-contract=off)
              const float diff = s - m;
              const float prod = diff * tie;
              gsc = m + prod;
            }
            a = (f & FIELDS_COUNT_MASK) ? a + gsc : (Q.must ? gsc : 0.0f + gsc);
            f4 = (f4 & ~(0xffu << (8 * j))) | ((((f & ~FIELDS_IN_GROUP) + 1u) & 0xffu) << (8 * j));
          };
          fold(0, s4.x, m4.x, a4.x);
          fold(1, s4.y, m4.y, a4.y);
          fold(2, s4.z, m4.z, a4.z);
          fold(3, s4.w, m4.w, a4.w);
          *reinterpret_cast<float4*>(acc + at) = a4;
          *reinterpret_cast<uint32_t*>(flag + at) = f4;
        }
      }
      wave_sync();
    }

    // ---- scan the window: a doc enough groups hold, that no prohibited clause holds and that is live, is one collected hit
    if (touched_any) {
      for (uint32_t i0 = 0; i0 < wlen; i0 += 256) {  // uniform trip count: the offer is a wave-wide operation
        const uint32_t at = i0 + 4u * (uint32_t)lane;
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(flag + at);
        if (__ballot(f4 != 0u)) {
          *reinterpret_cast<uint32_t*>(flag + at) = 0u;
          const float4 v = *reinterpret_cast<const float4*>(acc + at);
          const int32_t d = w0 + (int32_t)at;
          auto hit = [&](int j) -> bool {
            const uint32_t f = (f4 >> (8 * j)) & 0xffu;
            bool h = !(f & FIELDS_EXCLUDED) && (int)(f & FIELDS_COUNT_MASK) >= Q.need;  // (a set byte lies inside the window: d + j < w1)
            if (h && has_live) h = doc_is_live(seg.live, d + j);
            return h;
          };
          const bool h0 = hit(0), h1 = hit(1), h2 = hit(2), h3 = hit(3);
          hits_lane += (int)h0 + (int)h1 + (int)h2 + (int)h3;
          const uint32_t thi = (uint32_t)(tau >> 32);
          const bool c0k = h0 && float_order_bits(v.x) >= thi, c1k = h1 && float_order_bits(v.y) >= thi,
                     c2k = h2 && float_order_bits(v.z) >= thi, c3k = h3 && float_order_bits(v.w) >= thi;
          if (__ballot(c0k || c1k || c2k || c3k)) {
            uint64_t key = c0k ? make_key(v.x, d) : 0ull;
            if (__ballot(key > tau)) topk_offer<WIDE>(top, key, tau, k, lane, floor);
            key = c1k ? make_key(v.y, d + 1) : 0ull;
            if (__ballot(key > tau)) topk_offer<WIDE>(top, key, tau, k, lane, floor);
            key = c2k ? make_key(v.z, d + 2) : 0ull;
            if (__ballot(key > tau)) topk_offer<WIDE>(top, key, tau, k, lane, floor);
            key = c3k ? make_key(v.w, d + 3) : 0ull;
            if (__ballot(key > tau)) topk_offer<WIDE>(top, key, tau, k, lane, floor);
          }
        }
      }
      wave_sync();
    }
  }
  shared.publish<WIDE>(top, k, lane);
  uint64_t* pk = partial_keys + (size_t)item * (size_t)k;
  if (lane < k) pk[lane] = top.a;
  if (WIDE && lane + 64 < k) pk[lane + 64] = top.b;
  const int count = wave_reduce_add(hits_lane);
  if (lane == 0) partial_counts[item] = count;
}

}  // namespace rgpu
