// Cross-field query-string trees (rgpu_search_fields_tree_batch): BooleanQuery over TermQuery / DisjunctionMaxQuery / nested should-only
// BooleanQuery ("SUM") groups under MUST and SHOULD. Stage 1 is k_score_terms (search_or.hpp) once per field, as for
// rgpu_search_fields_batch; stage 2 is k_fields_tree_windows, k_fields_windows (search_fields.hpp, which stays the code it is) with
//   * a SUM group folded as its per-doc sum (the first touch stores 0.0f + s: DisjunctionSumScorer over a SimpleQueue,
//     disjunction_scorer.rs:211-225);
//   * a second per-doc accumulator for required/optional queries: a SHOULD group beside MUST groups is folded into `opt`
//     (0.0f + g first, then added, in clause order) and sets FIELDS_TREE_OPT_HELD; the count nibble counts MUST groups only;
//   * three ways out of the scan, by the query's mode (host/fields_tree_plan.hpp):
//       SINGLE  offer `acc` to the wave's top-k, as k_fields_windows does;
//       ADD     (rgpu_config.req_opt_rule = -1) offer acc + opt, opt = 0.0f where no optional group holds the doc;
//       RULE    one SeqRec{doc, req, opt} per collected hit, in doc order per query; k_req_opt_scan (search_and.hpp, as it stands)
//               then applies ReqOptScorer's doc-to-doc rule and writes the rows.
// Record emission (RULE). Every hit is held by the query's lead group - the required side's cheapest, its first `lead_terms` flat
// clauses -, so the item that covers docs [d0, d1) leaves at most L(d1) - L(d0) records, L(d) = the number of entries with doc < d
// summed over the lead group's runs. L(d0) is the sum of the lower bounds the cursor search finds anyway: the item writes its hits
// compactly from slot rec_base + L(d0), in doc order (a ballot-free prefix over the four docs a lane scans per step). Item regions
// are disjoint and ordered by doc, a query's region is its lead group's doc_freq sum (the host pre-fills it with doc = -1, which
// k_req_opt_scan passes over): deterministic, no atomics, memory bounded by the lead group's postings.
#pragma once
#include "search_and.hpp"
#include "search_fields.hpp"

namespace rgpu {

struct FieldsTreeGroupDev {  // host/fields_tree_plan.hpp FieldsTreePlanGroup
  int32_t first_term, n_terms;
  uint32_t tie_bits;
  int32_t kind;  // 0: the one clause's score; 1: max + (sum - max) * tie; 2: the sum
  int32_t optional, pad;
};
struct FieldsTreeQueryDev {  // host/fields_tree_plan.hpp FieldsTreePlanQuery
  int32_t first_group, n_groups, first_not, n_not, need, must, mode, lead_terms;
  int64_t rec_base;
};
constexpr int FIELDS_TREE_MODE_SINGLE = 0, FIELDS_TREE_MODE_ADD = 1, FIELDS_TREE_MODE_RULE = 2;
constexpr int FIELDS_TREE_KIND_TERM = 0, FIELDS_TREE_KIND_DISMAX = 1, FIELDS_TREE_KIND_SUM = 2;

// Per wavefront and doc of a window: outer sum, group sum, group maximum, optional sum (f32 each) and the flag byte of
// k_fields_windows with one more bit. 512 docs: 8704 B per wavefront, 69 632 B per workgroup of eight - two workgroups (sixteen
// wavefronts, four per SIMD) share a CU's 160 KB. 256 docs would fit four workgroups, but the kernel is bound by the run walks,
// whose per-window cost (two ballots, a cursor hand-off and a 64-entry load per active clause) doubles per doc at half the window,
// and the scan already steps 256 docs: the window stays the one k_fields_windows uses, so that one item geometry serves both calls.
constexpr int FIELDS_TREE_WINDOW_DOCS = 512;
constexpr uint32_t FIELDS_TREE_OPT_HELD = 0x20u;
__host__ __device__ constexpr size_t fields_tree_wave_lds_bytes(int W) { return (size_t)W * 17; }
__host__ __device__ constexpr size_t fields_tree_lds_bytes(int W) { return (size_t)FIELDS_WAVES * fields_tree_wave_lds_bytes(W); }

template <bool WIDE>
__global__ __launch_bounds__(FIELDS_THREADS) void k_fields_tree_windows(SegView seg, const FieldsTreeQueryDev* __restrict__ queries,
                                                                        const FieldsTreeGroupDev* __restrict__ groups,
                                                                        const int32_t* __restrict__ run_len,
                                                                        const int64_t* __restrict__ run_prefix,
                                                                        const ScoredPosting* __restrict__ runs, int n_queries,
                                                                        int windows_per_query, int windows_per_item, int items_per_query,
                                                                        int W, int k, uint64_t* __restrict__ partial_keys,
                                                                        int32_t* __restrict__ partial_counts,
                                                                        unsigned long long* __restrict__ tau_slots,
                                                                        SeqRec* __restrict__ records, int64_t n_records) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  const int wave = wave_id();
  uint8_t* slice = smem + (size_t)wave * fields_tree_wave_lds_bytes(W);
  float* acc = reinterpret_cast<float*>(slice);  // the outer (required) sum: valid where the count is not 0
  float* gsum = acc + W;                         // the current group's sum and maximum: valid where FIELDS_IN_GROUP is set
  float* gmax = gsum + W;
  float* opt = gmax + W;                         // the optional sum: valid where FIELDS_TREE_OPT_HELD is set
  uint8_t* flag = reinterpret_cast<uint8_t*>(opt + W);
  const int q = (int)(blockIdx.x % (unsigned)n_queries);
  const int g = (int)(blockIdx.x / (unsigned)n_queries) * FIELDS_WAVES + wave;
  const int64_t item = (int64_t)q * items_per_query + g;
  const FieldsTreeQueryDev Q = queries[q];
  const bool has_live = seg.live != nullptr;
  const bool emit = Q.mode == FIELDS_TREE_MODE_RULE;
  const bool add_opt = Q.mode == FIELDS_TREE_MODE_ADD;

  WaveTopK top;
  uint64_t tau = 0, floor = 0;
  int hits_lane = 0;
  SharedTau shared{tau_slots + q};
  shared.fold(shared.peek(), tau, floor);
  const int win0 = g * windows_per_item;
  const int win1 = Q.n_groups > 0 ? min(windows_per_query, win0 + windows_per_item) : win0;
  const int32_t first_doc = win0 * W;

  // ---- cursors, as in k_fields_windows; the lower bounds of the lead group's clauses (the query's first flat clauses) add up to the
  // item's first record slot
  const int c0 = Q.n_groups > 0 ? groups[Q.first_group].first_term : Q.first_not;
  const int n_cl = Q.first_not + Q.n_not - c0;
  int64_t at0 = 0, at1 = 0;
  int32_t next0 = 0x7fffffff, next1 = 0x7fffffff;
  int64_t rec_at = 0;   // wave-uniform: the next record slot of this item
  int64_t rec_end = 0;  // (the end of the query's region: nothing is ever written at or behind it)
  if (win0 < win1) {
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
      const int cl = lane + 64 * slot;
      const bool mine = cl < n_cl;
      const int64_t base = mine ? run_prefix[c0 + cl] : 0;
      int lo = 0, hi = mine ? run_len[c0 + cl] : 0;
      const int len = hi;
      while (__ballot(lo < hi)) {
        if (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (runs[base + mid].doc < first_doc) lo = mid + 1; else hi = mid;
        }
      }
      const int64_t at = base + lo;
      const int32_t next = mine ? runs[at].doc : 0x7fffffff;
      if (slot == 0) {
        at0 = at; next0 = next;
        if (emit) {  // (a lead group has at most nine clauses: all in slot 0)
          const bool lead = lane < Q.lead_terms;
          rec_at = Q.rec_base + (int64_t)wave_reduce_add(lead ? lo : 0);
          rec_end = min(n_records, Q.rec_base + (int64_t)wave_reduce_add(lead ? len : 0));
        }
      } else { at1 = at; next1 = next; }
    }
  }
  for (int i = lane; i < W / 4; i += 64) reinterpret_cast<uint32_t*>(flag)[i] = 0u;
  wave_sync();

  for (int win = win0; win < win1; ++win) {
    const int32_t w0 = win * W;
    const int32_t w1 = min(seg.max_doc, w0 + W);
    const uint32_t wlen = (uint32_t)(w1 - w0);
    const uint64_t active0 = __ballot(next0 < w1), active1 = __ballot(next1 < w1);
    bool touched_any = false;

    auto walk = [&](int cl, bool prohibited) {
      const int src = cl & 63;
      const bool hi_slot = cl >= 64;
      const int64_t at = (int64_t)readlane64((uint64_t)(hi_slot ? at1 : at0), src);
      int taken = 0;
      int32_t next;
      ScoredPosting e = runs[at + lane];
      while (true) {
        const bool in = e.doc < w1;
        const int n = __popcll(__ballot(in));
        const uint32_t o = (uint32_t)(e.doc - w0);
        if (in && o < wlen) {
          const uint32_t f = flag[o];
          if (prohibited) {
            flag[o] = (uint8_t)(f | FIELDS_EXCLUDED);
          } else if (f & FIELDS_IN_GROUP) {
            gsum[o] = gsum[o] + e.score;
            gmax[o] = fmaxf(gmax[o], e.score);
          } else {
            gsum[o] = 0.0f + e.score;
            gmax[o] = e.score;
            flag[o] = (uint8_t)(f | FIELDS_IN_GROUP);
          }
        }
        taken += n;
        if (n < 64) { next = readlane(e.doc, n); break; }
        e = runs[at + taken + lane];
      }
      if (lane == src) {
        if (hi_slot) { at1 += taken; next1 = next; } else { at0 += taken; next0 = next; }
      }
      touched_any = true;
      wave_sync();
    };
    auto is_active = [&](int cl) -> bool { return (((cl >= 64 ? active1 : active0) >> (cl & 63)) & 1ull) != 0ull; };

    for (int i = 0; i < Q.n_not; ++i) {
      const int cl = Q.first_not - c0 + i;
      if (is_active(cl)) walk(cl, true);
    }
    // ---- the groups: the MUST side in its cost order, then the SHOULD side in clause order
    for (int gi = 0; gi < Q.n_groups; ++gi) {
      const FieldsTreeGroupDev G = groups[Q.first_group + gi];
      bool group_touched = false;
      for (int i = 0; i < G.n_terms; ++i) {
        const int cl = G.first_term - c0 + i;
        if (is_active(cl)) { walk(cl, false); group_touched = true; }
      }
      if (!group_touched) continue;
      const float tie = __uint_as_float(G.tie_bits);
      const int kind = G.kind;
      const bool optional = G.optional != 0;
      for (uint32_t i0 = 0; i0 < wlen; i0 += 256) {
        const uint32_t at = i0 + 4u * (uint32_t)lane;
        uint32_t f4 = *reinterpret_cast<const uint32_t*>(flag + at);
        if (f4 & 0x10101010u) {
          const float4 s4 = *reinterpret_cast<const float4*>(gsum + at);
          const float4 m4 = *reinterpret_cast<const float4*>(gmax + at);
          float* into = optional ? opt : acc;
          float4 a4 = *reinterpret_cast<const float4*>(into + at);
          auto fold = [&](int j, float s, float m, float& a) {
            const uint32_t f = (f4 >> (8 * j)) & 0xffu;
            if (!(f & FIELDS_IN_GROUP)) return;
            float gsc = m;  // a term group: the clause's own score
            if (kind == FIELDS_TREE_KIND_DISMAX) {  // three f32 operations (the library is built with -ffp-contract=off)
              const float diff = s - m;
              const float prod = diff * tie;
              gsc = m + prod;
            } else if (kind == FIELDS_TREE_KIND_SUM) {
              gsc = s;
            }
            uint32_t nf;
            if (optional) {
              a = (f & FIELDS_TREE_OPT_HELD) ? a + gsc : 0.0f + gsc;
              nf = (f & ~FIELDS_IN_GROUP) | FIELDS_TREE_OPT_HELD;
            } else {
              a = (f & FIELDS_COUNT_MASK) ? a + gsc : (Q.must ? gsc : 0.0f + gsc);
              nf = (f & ~FIELDS_IN_GROUP) + 1u;
            }
            f4 = (f4 & ~(0xffu << (8 * j))) | ((nf & 0xffu) << (8 * j));
          };
          fold(0, s4.x, m4.x, a4.x);
          fold(1, s4.y, m4.y, a4.y);
          fold(2, s4.z, m4.z, a4.z);
          fold(3, s4.w, m4.w, a4.w);
          *reinterpret_cast<float4*>(into + at) = a4;
          *reinterpret_cast<uint32_t*>(flag + at) = f4;
        }
      }
      wave_sync();
    }

    // ---- scan the window
    if (touched_any) {
      for (uint32_t i0 = 0; i0 < wlen; i0 += 256) {
        const uint32_t at = i0 + 4u * (uint32_t)lane;
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(flag + at);
        if (__ballot(f4 != 0u)) {
          *reinterpret_cast<uint32_t*>(flag + at) = 0u;
          float4 v = *reinterpret_cast<const float4*>(acc + at);
          const int32_t d = w0 + (int32_t)at;
          auto hit = [&](int j) -> bool {
            const uint32_t f = (f4 >> (8 * j)) & 0xffu;
            bool h = !(f & FIELDS_EXCLUDED) && (int)(f & FIELDS_COUNT_MASK) >= Q.need;
            if (h && has_live) h = doc_is_live(seg.live, d + j);
            return h;
          };
          const bool h0 = hit(0), h1 = hit(1), h2 = hit(2), h3 = hit(3);
          if (emit || add_opt) {
            const float4 o4 = *reinterpret_cast<const float4*>(opt + at);
            const float o0 = (f4 & (FIELDS_TREE_OPT_HELD << 0)) ? o4.x : 0.0f, o1 = (f4 & (FIELDS_TREE_OPT_HELD << 8)) ? o4.y : 0.0f,
                        o2 = (f4 & (FIELDS_TREE_OPT_HELD << 16)) ? o4.z : 0.0f, o3 = (f4 & (FIELDS_TREE_OPT_HELD << 24)) ? o4.w : 0.0f;
            if (emit) {  // the step's hits, compactly and in doc order: lane-major, then the lane's four docs
              const int mine = (int)h0 + (int)h1 + (int)h2 + (int)h3;
              const int incl = wave_incl_scan(mine);
              const int step_hits = readlane(incl, 63);
              int64_t slot = rec_at + (int64_t)(incl - mine);
              if (h0) { if (slot < rec_end) records[slot] = SeqRec{d, v.x, o0, 0}; ++slot; }
              if (h1) { if (slot < rec_end) records[slot] = SeqRec{d + 1, v.y, o1, 0}; ++slot; }
              if (h2) { if (slot < rec_end) records[slot] = SeqRec{d + 2, v.z, o2, 0}; ++slot; }
              if (h3) { if (slot < rec_end) records[slot] = SeqRec{d + 3, v.w, o3, 0}; ++slot; }
              rec_at += step_hits;
              continue;
            }
            v.x = v.x + o0; v.y = v.y + o1; v.z = v.z + o2; v.w = v.w + o3;
          }
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
