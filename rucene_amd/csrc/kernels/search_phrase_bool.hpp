// BooleanQuery with exact PhraseQuery clauses among its required clauses (rgpu_search_phrase_bool_batch): +"a b" +c -d.
// The candidates are the conjunction of every required clause's terms (k_search_and in emit mode, MUST_NOT terms removed there);
// the phrase match kernels (search_phrase.hpp) then see one "virtual query" per (query, phrase) — plane j of a query holds the same
// candidates in the same slots as plane 0 — and leave make_key(BM25(phrase_j freq, norm), doc) or 0 in every slot. The kernels
// here sit on both sides of that stage: k_phrase_bool_fanout copies plane 0's candidates to the other planes, k_phrase_bool_score
// forms the f32 sum the reference's ConjunctionScorer forms (conjunction_scorer.rs:87-95: the children's scores in stable cost
// order, the first one as it is, the rest +=) and writes it over plane 0's key for the collectors.
// Virtual queries are plane-major: v = j * n_queries + q. emit_prefix has n_planes * n_queries + 1 entries, its first n_queries + 1
// are plane 0's (a contiguous run of 64-slot groups, none of which straddles two queries).
#pragma once
#include "search_phrase.hpp"

namespace rgpu {

// One query as k_phrase_bool_score reads it. order[]: n_order entries at first_order in the launch's order array — >= 0: a required
// term clause (index into the launch's clause DevTerm array), < 0: ~plane (that phrase's key_score).
struct PhraseBoolDev {
  int32_t n_planes;     // phrases (0: the leaf matches nothing — no slots either)
  int32_t first_order;
  int32_t n_order;
  int32_t pad;
};

// One wavefront per 64-slot group of plane 0. Bounds: group < n_groups = emit_prefix[n_queries] / 64; a lane reads and writes slots
// below its query's candidate count only, at the same offset in every plane (each plane of a query has plane 0's size).
__global__ __launch_bounds__(WG_THREADS) void k_phrase_bool_fanout(const PhraseBoolDev* __restrict__ pb, const int64_t* __restrict__ emit_prefix,
                                                                   unsigned long long* __restrict__ emit_count, int32_t* __restrict__ emit_docs,
                                                                   int n_queries, int64_t n_groups) {
  const int lane = lane_id();
  const int64_t group = (int64_t)blockIdx.x * WG_WAVES + wave_id();
  if (group >= n_groups) return;
  const int q = upper_slot_wave(emit_prefix, n_queries, group * 64, lane);
  const int n_planes = pb[q].n_planes;
  if (n_planes < 2) return;
  const int64_t base = emit_prefix[q];
  const int64_t idx = group * 64 + lane - base;
  const unsigned long long cnt = emit_count[q];
  if (idx == 0)  // the query's first group: the planes' counts
    for (int j = 1; j < n_planes; ++j) emit_count[(int64_t)j * n_queries + q] = cnt;
  if ((unsigned long long)idx >= cnt) return;
  const int32_t doc = emit_docs[base + idx];  // (a deleted candidate keeps its sign bit: no plane checks it)
  for (int j = 1; j < n_planes; ++j) emit_docs[emit_prefix[(int64_t)j * n_queries + q] + idx] = doc;
}

constexpr int PHRASE_BOOL_MAX_PLANES = 4;  // = RGPU_MAX_BOOL_PHRASES

// One wavefront per 64-slot group of plane 0, one candidate per lane. A candidate survives when every plane holds a key for it
// (one ballot per plane); a group without survivors leaves after one coalesced key load per plane. For the survivors every
// required term clause's freq is found the way k_rescore finds it — directory -> block / tail / singleton — but a block is decoded
// once per wavefront into wave-private LDS and every surviving lane whose doc lies in that block's range looks its doc up there:
// the survivors of a group come from one lead block and lie near each other. The conjunction guarantees that every clause holds
// every survivor; one that is not found again raises RGPU_ERR_ILLEGAL_STATE in *err and loses its key.
// Bounds: slots as in k_phrase_bool_fanout; directory indexes inside [dir_base, dir_base + nblocks] (the tail's row only when
// tail_n > 0); staged[] indexes 0..127.
template <bool LEGACY>
__global__ __launch_bounds__(WG_THREADS) void k_phrase_bool_score(SegView seg, const PhraseBoolDev* __restrict__ pb, const int32_t* __restrict__ order,
                                                                  const DevTerm* __restrict__ clauses, const int64_t* __restrict__ emit_prefix,
                                                                  const unsigned long long* __restrict__ emit_count, int n_queries, int64_t n_groups,
                                                                  uint64_t* __restrict__ keys, int* err) {
  __shared__ __attribute__((aligned(16))) uint8_t slabs[WG_WAVES][2 * SLAB_STREAM];
  __shared__ float caches[WG_WAVES][256];
  __shared__ int32_t staged_docs[WG_WAVES][128];
  __shared__ uint32_t staged_freqs[WG_WAVES][128];
  const int lane = lane_id();
  const int wave = wave_id();
  const int64_t group = (int64_t)blockIdx.x * WG_WAVES + wave;
  if (group >= n_groups) return;
  const int q = upper_slot_wave(emit_prefix, n_queries, group * 64, lane);
  const int64_t base = emit_prefix[q];
  const int64_t idx = group * 64 + lane - base;
  const int64_t cnt = (int64_t)emit_count[q];
  if (idx - lane >= cnt) return;  // nothing in these 64 slots (the collectors read the first emit_count[q] slots only)
  const PhraseBoolDev Q = pb[q];
  const bool mine = idx < cnt;
  // ---- survivors: a key in every plane
  uint64_t pkey[PHRASE_BOOL_MAX_PLANES];
  bool alive = mine;
#pragma unroll
  for (int j = 0; j < PHRASE_BOOL_MAX_PLANES; ++j) {
    pkey[j] = 0ull;
    if (j < Q.n_planes) {  // wave-uniform
      pkey[j] = mine ? keys[emit_prefix[(int64_t)j * n_queries + q] + idx] : 0ull;
      alive = alive && pkey[j] != 0ull;
    }
  }
  if (!__ballot(alive)) {
    if (mine) keys[base + idx] = 0ull;
    return;
  }
  const int32_t doc = alive ? key_doc(pkey[0]) : -1;
  // ---- the sum in reference order
  uint8_t* slab = slabs[wave];
  float* cache = caches[wave];
  int32_t* sd = staged_docs[wave];
  uint32_t* sf = staged_freqs[wave];
  const bool has_norms = seg.norms != nullptr;
  const uint32_t nb = (has_norms && alive) ? seg.norms[doc] : 0u;
  int cur_table = -1;
  float k1 = 0.f;
  float sum = 0.0f;
  for (int o = 0; o < Q.n_order; ++o) {
    const int32_t what = readfirstlane(order[Q.first_order + o]);  // wave-uniform: a scalar
    float s = 0.0f;
    if (what < 0) {
      const int j = ~what;
      const uint64_t kj = j == 0 ? pkey[0] : (j == 1 ? pkey[1] : (j == 2 ? pkey[2] : pkey[3]));
      s = key_score(kj);
    } else {
      const DevTerm T = clauses[what];
      uint32_t freq = 0u;
      if (T.df == 1) {
        if (alive && T.singleton_doc == doc) freq = (uint32_t)T.singleton_freq;
      } else {
        bool pend = alive;
        while (true) {
          const uint64_t pm = __ballot(pend);
          if (!pm) break;
          const int32_t d = readlane(doc, (int)__builtin_ctzll(pm));
          const int blk = find_block_wave(seg.dir_last, T.dir_base, 0, T.nblocks, d, lane);
          const int32_t lo = blk == 0 ? -1 : seg.dir_last[T.dir_base + blk - 1];             // docs of this block are > lo ...
          const int32_t hi = blk < T.nblocks ? seg.dir_last[T.dir_base + blk] : 0x7fffffff;  // ... and <= hi
          int32_t e0 = 0x7fffffff, e1 = 0x7fffffff;
          uint32_t g0 = 0u, g1 = 0u;
          if (blk < T.nblocks) {
            const BlockPair bp = decode_block<LEGACY>(seg.bstore + T.bs_base, seg.dir_row[T.dir_base + blk], seg.dir_hdr[T.dir_base + blk], slab, lane);
            deltas_to_docs(bp.d0, bp.d1, blk == 0 ? 0 : lo, e0, e1);
            g0 = bp.f0; g1 = bp.f1;
          } else if (T.tail_n > 0) {
            tail_load(seg.bstore + T.bs_base, seg.dir_row[T.dir_base + T.nblocks], lane, e0, e1, g0, g1);
            if (2 * lane >= T.tail_n) { e0 = 0x7fffffff; g0 = 0u; }
            if (2 * lane + 1 >= T.tail_n) { e1 = 0x7fffffff; g1 = 0u; }
          }
          wave_sync();  // (the lanes' look-ups of the previous block are done)
          sd[2 * lane] = e0; sd[2 * lane + 1] = e1;
          sf[2 * lane] = g0; sf[2 * lane + 1] = g1;
          wave_sync();
          const bool here = pend && doc > lo && doc <= hi;  // the chosen lane's doc is: every round answers a lane
          if (here) {
            int a = 0, b = 128;  // first staged doc >= doc (the staged docs ascend; unused entries are INT_MAX)
            while (a < b) {
              const int mid = (a + b) >> 1;
              if (sd[mid] < doc) a = mid + 1; else b = mid;
            }
            if (a < 128 && sd[a] == doc) freq = sf[a];
            pend = false;
          }
        }
      }
      if (__ballot(alive && freq == 0u)) {  // the conjunction found the doc in this term: it cannot be missing
        if (lane == 0) atomicMin(err, (int)-1 /* RGPU_ERR_ILLEGAL_STATE */);
        alive = alive && freq != 0u;
      }
      if (T.sim_table != cur_table) { load_sim_table(seg, T.sim_table, cache, lane, k1); cur_table = T.sim_table; }
      s = bm25_score(T.weight * (k1 + 1.0f), (float)(int32_t)freq, has_norms ? cache[nb] : k1);
    }
    sum = o == 0 ? s : sum + s;
  }
  if (mine) keys[base + idx] = alive ? make_key(sum, doc) : 0ull;
}

}  // namespace rgpu
