// Single-term queries, one workgroup per QUERY (k_search_term_query): the default kernel of the fused single-term call.
//
// k_search_term (search_term.hpp) cuts every list into work items of at least 8 wavefronts each, and every item pays the same chain
// of dependent loads (term -> table -> sketch -> chunk frontiers) before it looks at its first block, finds its live blocks only by
// position in the list, and hands its partial list to the query's last item across XCDs. Here a query stays inside one workgroup of
// W waves:
//   set-up    once: the term, its score table in LDS (shared by the waves), the sketch threshold;
//   gather    the list's chunk frontiers (SegView::dir_sum), one thread per chunk; for the chunks that survive, the blocks' frontier
//             words (dir_bmax), one lane per block, together with their store row, header and the doc in front of them. Blocks whose
//             bound can still enter the top-k go to an LDS queue of capacity TQ_CAP, in block order;
//   sort      the queue by (bound desc, block asc);
//   drain     the waves pop entries best bound first from an LDS counter and unpack them (term_blocks_fast's per-block body), up
//             to PREFETCH_DEPTH rows in flight per wave: every address comes from the queue, none waits for a directory load.
// The threshold only rises and the queue is sorted by bound, then by block (whose doc in front grows with it): the first popped
// entry that can no longer enter proves that none behind it can, and the round ends there. A list with more candidates than the
// queue holds is gathered and drained in rounds from a chunk cursor, each round's gather filtering with the threshold the
// previous rounds reached. The top-k list lives in LDS (GroupList, shared under its lock) and wave 0 writes the caller's row:
// no partial lists, no per-query counters in memory, no exchange between XCDs.
// Queries off the table path (raw norms, deleted docs, a negative weight, a sim table without TERM_FLAG_MONOTONE) run in the same
// launch: the waves stride over the list's chunks with stream_blocks and offer into the same list.
// One-chunk path (table-path lists of at most `short_blocks` <= 64 FullBlocks; RGPU_TERM_SHORT_BLOCKS, 0: off): such
// a list is one lane per block, so it has no chunk frontier to test, no queue to fill, sort and pop, and — its waves being the only
// writers — needs no shared list:
//   loads     the chunk's directory entries (dir_bmax, dir_row, dir_hdr, dir_last) are requested from the descriptor alone, by waves
//             1 .. W - 1 while wave 0 builds the table (wave 0: behind its build); wave W - 1 also loads the tail (row -> cells ->
//             norms -> the similarity's cache entries) and scores it ahead of the barrier, without the table;
//   deal      behind the barrier every wave computes every block's bound and the same ballot of survivors against the floor; wave w
//             owns the survivors of rank w, w + W, ... and parks their directory entries in the (unused) queue arrays;
//   unpack    the general path's per-block body through a PREFETCH_DEPTH-deep ring, a block re-tested against the WAVE's threshold
//             just before it is unpacked; offers go to a list of the wave's own (LDS over `cq`, checked out per offer, level cut in
//             front: wave_offer2) with tau = max(its k-th best, floor). No lock;
//   merge     one barrier, then wave 0 folds the W sorted lists (topk_merge_sorted) and writes the row, the total and the counters.
// Exact: a subset's k-th best key is a lower bound of the list's, so a block skipped against a private threshold holds no winner;
// keys are unique, so the k best of the union of the private lists are the list's k best.
// On the general path a gather round past the list's last chunk and a block-step slot without a chunk issue no loads and no bound.
#pragma once
#include "search_term.hpp"

namespace rgpu {

#ifndef RGPU_TERMQ_CAP
#define RGPU_TERMQ_CAP 256
#endif
constexpr int TQ_CAP = RGPU_TERMQ_CAP;  // queue entries per round (a whole chunk of 64 blocks always fits an empty queue)
constexpr int TQ_CHUNK_UNROLL = 4;      // chunk frontier words per thread per gather window
#ifndef RGPU_TERMQ_STEP_CHUNKS
#define RGPU_TERMQ_STEP_CHUNKS 2
#endif
constexpr int TQ_STEP_CHUNKS = RGPU_TERMQ_STEP_CHUNKS;  // surviving chunks per wave per gather step
// The bound asks for 6 waves per SIMD (k_search_term's): the scheduler spreads the general path's drain over 73 VGPRs and spills 22
// SGPRs. A bound of 7 holds the headline instantiation to 71 VGPRs and seven waves, pays for it with 44 spilled SGPRs in the general
// path, and its one-stream step measures 5 % slower in every run: -DRGPU_TERMQ_FAST_WAVES=7 builds it. (W = 2 always takes
// k_search_term's bound: two-wave workgroups do not fit seven.)
#ifndef RGPU_TERMQ_FAST_WAVES
#define RGPU_TERMQ_FAST_WAVES 6
#endif
// 1: variant builds whose block gather deals a window's surviving chunks to the waves without a barrier, the queue entries reserved
// from an LDS counter (modelled by tests/test_term_gather_model_cpu.py). 1-1.5 % faster, not separated from noise.
#ifndef RGPU_TERMQ_DEAL
#define RGPU_TERMQ_DEAL 0
#endif
#ifndef RGPU_TERMQ_DEAL_CHUNKS
#define RGPU_TERMQ_DEAL_CHUNKS 4
#endif
constexpr int TQ_DEAL_CHUNKS = RGPU_TERMQ_DEAL_CHUNKS;  // chunks a wave has in flight in the dealt gather (one round trip for them all)
#ifndef RGPU_TERMQ_ONE  // 0: variant builds without the one-chunk path
#define RGPU_TERMQ_ONE 1
#endif
static_assert(TQ_CAP >= 64 && TQ_CAP <= 65536, "queue positions are u16 and a chunk must fit an empty queue");

// the entry test of term_blocks_fast on raw score bits: a block whose postings' best score is `bound` can enter iff
// bound >= term_thr_of(tau, lo), where lo = the last doc in front of the block (strict when none of its docs can win a tie)
__device__ __forceinline__ uint32_t term_thr_of(uint64_t t, int32_t lo) {
  const uint32_t thi = (uint32_t)(t >> 32);
  if (!(thi & 0x80000000u)) return 0u;
  const uint32_t bits = thi & 0x7fffffffu;
  return key_doc(t) <= lo + 1 ? bits + 1u : bits;
}
// the best score any posting behind frontier word w can have under the LDS table (raw bits; all ones: no bound)
__device__ __forceinline__ uint32_t term_bound_of(const float* cache, uint64_t w) {
  const uint32_t fmax = (uint32_t)w & 15u;
  uint32_t bb = 0u;
#pragma unroll
  for (int f = 1; f <= SCORE_TABLE_FREQS; ++f) {
    const uint32_t r = (uint32_t)(w >> (4 + 6 * (f - 1))) & 63u;
    const uint32_t sc = __float_as_uint(table_score(cache, r, (uint32_t)f));
    bb = ((uint32_t)f <= fmax && sc > bb) ? sc : bb;
  }
  return fmax > (uint32_t)SCORE_TABLE_FREQS ? 0xffffffffu : bb;
}

#ifdef RGPU_TERM_TRACE  // developer instrumentation (variant builds only): one record per WORKGROUP of k_search_term_query in g_term_trace
// (three of k_search_term's records each; read back by rgpu_debug_trace, printed by scripts/term_query_timeline.py).
// d[]: 10 ns ticks from t0 to: descriptor in registers, table built, sketch folded, end of the first gather, end of the first sort,
// end of the drain (every wave past its last block), end of the tail. cyc[w]: wave w's shader-clock cycles {waiting for the list's
// lock, holding it, the rest of step()} up to the end of the drain; wave0_cycles: wave 0's shader clock over the same ticks as d[5].
struct TermQueryTraceRec {
  unsigned long long t0, t1;
  int32_t q, nblocks, rounds, entries, unpacked, offers, entered;
  unsigned int d[7];
  unsigned int waves, wave0_cycles;
  unsigned int cyc[8][3];
  unsigned int pad[16];
};
static_assert(sizeof(TermQueryTraceRec) == 3 * sizeof(TermTraceRec), "a workgroup's record takes three slots of g_term_trace");
#define TQ_TR(slot, dep) do { asm volatile("" :: "v"(dep)); tq_d[slot] = (unsigned int)((unsigned long long)wall_clock64() - tq_t0); } while (0)
#else
#define TQ_TR(slot, dep) do {} while (0)
#endif

// a one-chunk list's directory, one lane per block: frontier word, store row, header, the doc in front of the block (-1: none)
struct OneChunkDir {
  uint64_t bm = 0ull;
  uint32_t rw = 0u, hd = 0u;
  int32_t lo = -1;
  __device__ __forceinline__ void load(const SegView& seg, const DevTerm& T, int lane) {
    if (lane < T.nblocks) {
      const uint32_t b = T.dir_base + (uint32_t)lane;
      bm = seg.dir_bmax[b];
      rw = seg.dir_row[b];
      hd = (uint32_t)seg.dir_hdr[b];
      if (lane > 0) lo = seg.dir_last[b - 1u];
    }
  }
};

template <bool LEGACY, bool WIDE, int W>
__global__ __launch_bounds__(64 * W, (LEGACY || WIDE) ? RGPU_TERM_OTHER_WAVES : W == 2 ? RGPU_TERM_FAST_WAVES : RGPU_TERMQ_FAST_WAVES)
void k_search_term_query(SegView seg, const DevQuery* __restrict__ queries, const DevTerm* __restrict__ terms,
                         const int32_t* __restrict__ order, int n_queries, int k, unsigned long long* __restrict__ work_slots,
                         const int32_t* __restrict__ qmap, HitOut* __restrict__ hits, int64_t* __restrict__ totals, int32_t doc_base,
                         const TermLaunch* __restrict__ launch, int short_blocks) {
  // order[i]: the query of workgroup i (heaviest first); work_slots (nullable): [q] = bytes requested for query q, [n_queries + q] =
  // FullBlocks unpacked (rgpu_last_search_counters).
  // launch (nullable; pinned host memory): workgroup i's whole plan is launch[i] — `terms` is then the context's descriptor arena and
  // `queries`, `order` and `qmap` are not read: one read over the bus and one of device memory instead of order -> query -> term
  // short_blocks (0..64, the same in every workgroup): table-path lists of at most this many FullBlocks take the one-chunk path; 0: none
  constexpr int LIST_N = WIDE ? 128 : 64;
  constexpr int NT = 64 * W;
  constexpr int DEPTH = PREFETCH_DEPTH;
  __shared__ __attribute__((aligned(16))) uint8_t slabs[W][TERM_BLOCK_SLAB];
  __shared__ float cache[WAVE_CACHE_FLOATS];  // the norm cache (64 ranks + the score table, or 256 raw norm bytes)
  __shared__ uint64_t list[LIST_N];
  __shared__ uint32_t lock_word;
  __shared__ uint32_t e_blk[TQ_CAP], e_row[TQ_CAP], e_bound[TQ_CAP];  // the queue, in block order
  __shared__ int32_t e_lo[TQ_CAP];
  __shared__ uint16_t e_hdr[TQ_CAP], e_order[TQ_CAP];                 // e_order: queue positions, best bound first
  // cq: surviving chunks of the current gather window; on the one-chunk path (no window, no queue) the waves' private lists
  __shared__ __attribute__((aligned(16))) uint32_t cq[TQ_CHUNK_UNROLL * NT];
  static_assert(sizeof(uint32_t) * TQ_CHUNK_UNROLL * NT >= sizeof(uint64_t) * W * LIST_N, "W private lists of LIST_N keys alias cq");
  __shared__ uint32_t cnt[TQ_CHUNK_UNROLL * NT / 64 > W * TQ_STEP_CHUNKS ? TQ_CHUNK_UNROLL * NT / 64 : W * TQ_STEP_CHUNKS];
  __shared__ uint32_t cursor;
#if RGPU_TERMQ_DEAL
  __shared__ uint32_t q_count, q_end;                       // entries reserved this round; where the first reservation that did not fit starts
  __shared__ uint32_t done_map[TQ_CHUNK_UNROLL * NT / 32];  // one bit per chunk of the gather window: its blocks are queued
#endif
  __shared__ uint32_t sums[3];  // hits, blocks unpacked, bytes requested
  __shared__ uint64_t floor_s;

  const int lane = lane_id();
  const int wave = wave_id();
  const int tid = (int)threadIdx.x;
#ifdef RGPU_TERM_TRACE
  __shared__ uint32_t tq_w[8][5];  // per wave: lock wait, lock hold, step() in all, offers, keys entered
  const unsigned long long tq_t0 = (unsigned long long)wall_clock64();
  const uint64_t tq_c0 = (uint64_t)clock64();
  unsigned int tq_d[7] = {0, 0, 0, 0, 0, 0, 0};
  uint32_t tq_step = 0;
  int tq_rounds = 0, tq_entries = 0;
#endif
  TERM_LK_DECL;
  int q, row, rec;
  if (launch != nullptr) {
    if ((int)blockIdx.x >= n_queries) return;
    const TermLaunch L = launch[blockIdx.x];
    q = row = L.row;
    rec = L.rec;
  } else {
    q = order != nullptr ? order[blockIdx.x] : (int)blockIdx.x;
    if (q >= n_queries) return;
    row = qmap ? qmap[q] : q;
    const DevQuery Q = queries[q];
    rec = Q.n_terms < 1 ? -1 : Q.first_term;
  }
  HitOut* out = hits + (size_t)row * (size_t)k;
  if (rec < 0) {  // clause absent from this leaf: nothing to collect
    if (wave == 0) {
      if (lane < k) out[lane] = HitOut{-1, 0.f};
      if (WIDE && lane + 64 < k) out[lane + 64] = HitOut{-1, 0.f};
      if (lane == 0) {
        totals[row] = 0;
        if (work_slots != nullptr) { work_slots[q] = 0ull; work_slots[n_queries + q] = 0ull; }  // (nobody zeroes them ahead of a launch-record step)
      }
    }
    return;
  }
  const DevTerm T = terms[rec];
  TQ_TR(0, T.df);
  const bool has_norms = seg.norms != nullptr;
  const bool tabled = has_norms && seg.n_norm_ranks > 0;
  const bool fast = tabled && seg.live == nullptr && T.weight >= 0.0f && RGPU_TERM_PRUNE && (T.flags & TERM_FLAG_MONOTONE) != 0u;
  const float k1 = seg.sim_tables[(size_t)T.sim_table * 257 + 256];
  const float wk = T.weight * (k1 + 1.0f);
  const uint8_t* term_rows = seg.bstore + T.bs_base;
  const GroupList group{list, &lock_word};
  const int n_chunks = (T.nblocks + 63) >> 6;
  const uint32_t sum_base = (T.dir_base + 63u) >> 6;

  // One-chunk path: a table-path list of at most short_blocks (<= 64) FullBlocks is one lane per block in every wave. Its directory
  // entries depend on the descriptor alone, so every wave requests them here (the same lines in every wave: L2 hits) and they fly
  // while wave 0 builds the table; wave W - 1 also requests the tail (or the singleton's norm): tail row -> cells -> norms.
  // (workgroup-uniform, and said so: a branch the compiler takes for divergent is laid out as both sides under masks, and what one
  // side keeps in registers then stays live across the other)
  const bool one = readfirstlane((int)(RGPU_TERMQ_ONE && fast && short_blocks > 0 && T.nblocks <= short_blocks)) != 0;
  OneChunkDir oc;
  uint64_t oc_k0 = 0ull, oc_k1 = 0ull;  // wave W - 1: the tail's (or the singleton's) keys
  for (int i = tid; i < LIST_N; i += NT) list[i] = 0ull;
  if (tid == 0) { lock_word = 0u; sums[0] = sums[1] = sums[2] = 0u; floor_s = 0ull; cursor = 0u; }
  uint32_t looked = 0, touched = 0;  // per wave (scalar)
  int count = 0;                     // per wave: hits counted
  if (wave == 0) {
    float k1_;
    load_sim_table(seg, T.sim_table, cache, lane, k1_);
    if (tabled) build_score_table(cache, wk, lane);
    if (one) oc.load(seg, T, lane);
    TQ_TR(1, cache[lane]);
    // the term's block-max sketch: k real postings of k blocks, scored with this query's table — a threshold to start from
    if (fast && T.sketch != 0u && seg.sketch != nullptr && k <= TERM_SKETCH_K) {
      const uint64_t f = sketch_floor<WIDE>(seg.sketch + (size_t)(T.sketch - 1u) * TERM_SKETCH_K, cache, k, lane);
      if (lane == 0) floor_s = f;
      touched += 2u * (uint32_t)k;
    }
  } else if (one) {
    // (an else of wave 0's branch, not a block in front of it: what is loaded here is then not live across the table build, whose
    // eleven divisions in flight want the registers; wave 0 requests its directory entries behind the build)
    oc.load(seg, T, lane);
    if (wave == W - 1 && (T.df == 1 || T.tail_n > 0)) {
      // scored here, without the table: table_score(rank, freq) IS bm25_score(wk, freq, the rank's cache entry), the expression below
      // on the same operands, so the bits are the table's; two keys cross the barrier instead of docs, freqs and norms
      int32_t d0 = T.singleton_doc, d1 = 0;
      uint32_t f0 = (uint32_t)T.singleton_freq, f1 = 1u, n0, n1 = 0u;
      bool v0 = lane == 0, v1 = false;
      if (T.df == 1) {
        n0 = v0 ? norm_at(seg, T.singleton_doc) : 0u;
      } else {
        tail_load(term_rows, seg.dir_row[T.dir_base + T.nblocks], lane, d0, d1, f0, f1);  // decoded and validated at prepare time
        v0 = 2 * lane < T.tail_n;
        v1 = 2 * lane + 1 < T.tail_n;
        n0 = v0 ? seg.norms[d0] : 0u;
        n1 = v1 ? seg.norms[d1] : 0u;
      }
      const float* sim = seg.sim_tables + (size_t)T.sim_table * 257;
      const float c0 = sim[seg.rank_to_norm[n0]], c1 = sim[seg.rank_to_norm[n1]];
      const float s0 = bm25_score(wk, (float)(int32_t)f0, c0), s1 = bm25_score(wk, (float)(int32_t)f1, c1);
      oc_k0 = v0 ? make_key(s0, d0) : 0ull;
      oc_k1 = v1 ? make_key(s1, d1) : 0ull;
    }
  }
  __syncthreads();
  const uint64_t floor = ((uint64_t)(uint32_t)readfirstlane((int)(uint32_t)(floor_s >> 32)) << 32) | (uint32_t)readfirstlane((int)(uint32_t)floor_s);
  auto tau_now = [&]() -> uint64_t {
    const uint64_t kth = group_kth<WIDE>(group, k);
    return kth > floor ? kth : floor;
  };
  uint64_t tau = floor;
  TQ_TR(2, (uint32_t)floor);

  if (one) {
    // ---- one chunk: no chunk frontier, no queue, no sort, no lock ----
    // A ballot is the queue: every wave computes every block's bound and the same survivor mask pm against the floor; wave w takes
    // the survivors of rank w, w + W, ... in pm and keeps a list of its own in registers (tau = max(its k-th best, floor)). A
    // subset's k-th best key is a lower bound of the list's final one, so a block skipped against a private threshold holds no
    // winner, and keys are unique: the merge of the W private top-k lists at the end is the top-k of their union.
    const uint8_t* pn = seg.pnorm + T.pn_base;
    uint8_t* slab = slabs[wave];
    // this wave's private list: LDS over cq, which this path never uses, checked out into registers for an offer (no lock: one owner)
    uint64_t* mine = reinterpret_cast<uint64_t*>(cq) + wave * LIST_N;
    mine[lane] = 0ull;
    if (WIDE) mine[64 + lane] = 0ull;
    if (wave == 0) {
      count = 128 * T.nblocks;  // no deleted docs on this path: every posting is a hit
      touched += 18u * (uint32_t)T.nblocks;
    }
    // the tail or the singleton, beside the other waves' blocks: its loads were requested with the directory's
    if (wave == W - 1) {
      count += T.df == 1 ? 1 : T.tail_n;
      if (__ballot((oc_k0 > oc_k1 ? oc_k0 : oc_k1) > tau)) wave_offer2<WIDE>(mine, oc_k0, oc_k1, tau, k, lane, floor TERM_LK_PASS);
    }
    const uint32_t bd = term_bound_of(cache, oc.bm);
    const uint64_t pm = __ballot(lane < T.nblocks && bd >= term_thr_of(floor, oc.lo));
    // (wave W - 1 has the tail behind it: its threshold may already be above the floor)
    uint64_t todo = __ballot(((pm >> lane) & 1ull) != 0ull && (mbcnt(pm) & (W - 1)) == wave && bd >= term_thr_of(tau, oc.lo));
    const int first = todo ? (int)__builtin_ctzll(todo) : 0;
    // the owner of a block parks its directory entry in the (unused) queue arrays, indexed by block: four registers less across the
    // ring, which then costs what the general path's drain does
    if ((todo >> lane) & 1ull) { e_row[lane] = oc.rw; e_hdr[lane] = (uint16_t)oc.hd; e_lo[lane] = oc.lo; e_bound[lane] = bd; }
    wave_sync();
#ifdef RGPU_TERM_TRACE
    tq_entries = __popcll(pm);
    TQ_TR(3, bd);
    tq_d[4] = tq_d[3];
#endif
    auto take = [&]() -> int {
      if (!todo) return -1;
      const int i = (int)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      return i;
    };
    auto rows_of = [&](int i) -> uint4 { return block_rows_load(block_rows_at(term_rows, e_row[i]), e_hdr[i], lane); };
    auto norms_of = [&](int i) -> uint32_t {
      return *reinterpret_cast<const uint16_t*>(pn + (128u * (uint32_t)i + 2u * (uint32_t)lane));
    };
    // the wave's share, up to DEPTH rows in flight (at most 15 blocks over 4 waves: one ring fill); slots without a block reload the
    // wave's first block instead of being guarded, and a wave without a block requests nothing
    int slot[DEPTH];
    uint4 ring[DEPTH];
    uint32_t nring[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) { slot[j] = -1; ring[j] = uint4{0u, 0u, 0u, 0u}; nring[j] = 0u; }
    if (todo != 0ull) {
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        slot[j] = take();
        const int pj = slot[j] < 0 ? first : slot[j];
        ring[j] = rows_of(pj);
        nring[j] = norms_of(pj);
      }
    }
    auto step = [&](int i, const uint4& rows, uint32_t nn) {
      const uint32_t hdr = (uint32_t)e_hdr[i];
      const int32_t lo = e_lo[i];
      touched += encoded_block_bytes(hdr) + 128u;  // both streams' rows + the posting-order norms were requested
      // against the wave's threshold of the moment, just before the block is unpacked
      if (e_bound[i] < term_thr_of(tau, lo)) return;
      const int bf = hdr_bfreq(hdr);
      stage_rows(rows, slab, lane);
      wave_sync();
      uint32_t f0, f1;
      bool in_table = true;  // wave-uniform: every freq of the block has a table column
      if (bf) {
        extract_pair<LEGACY>(slab + SLAB_STREAM, bf, lane, f0, f1);
        if (bf > 3) in_table = !__ballot((f0 > f1 ? f0 : f1) > (uint32_t)SCORE_TABLE_FREQS);
      } else {
        const uint32_t f = (uint32_t)readlane((int)rows.x, 32);  // all-equal stream: its value
        f0 = f1 = f;
        in_table = f <= (uint32_t)SCORE_TABLE_FREQS;
      }
      const uint32_t nb0 = nn & 0xffu, nb1 = nn >> 8;
      float s0, s1;
      if (in_table) {
        s0 = table_score(cache, nb0, f0);
        s1 = table_score(cache, nb1, f1);
      } else {
        s0 = bm25_score(wk, (float)(int32_t)f0, cache[nb0]);
        s1 = bm25_score(wk, (float)(int32_t)f1, cache[nb1]);
      }
      looked += 1u;
      const uint32_t thr = term_thr_of(tau, lo);
      const uint32_t r0 = __float_as_uint(s0), r1 = __float_as_uint(s1);
      if (__ballot((r0 > r1 ? r0 : r1) >= thr)) {  // the doc deltas only when some posting can still enter
        uint32_t e0, e1;
        staged_doc_deltas<LEGACY>(slab, rows, hdr, lane, e0, e1);
        int32_t d0, d1;
        deltas_to_docs(e0, e1, lo < 0 ? 0 : lo, d0, d1);
        const uint64_t key0 = make_key(s0, d0), key1 = make_key(s1, d1);
        if (__ballot((key0 > key1 ? key0 : key1) > tau)) wave_offer2<WIDE>(mine, key0, key1, tau, k, lane, floor TERM_LK_PASS);
      }
      wave_sync();  // slab is free for the next block
    };
    while (slot[0] >= 0) {  // slots fill in order, so an empty slot 0 means an empty ring
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        const uint4 rows = ring[j];
        const uint32_t nn = nring[j];
        const int i = slot[j];
        slot[j] = i >= 0 ? take() : -1;
        const int pj = slot[j] < 0 ? first : slot[j];
        ring[j] = rows_of(pj);
        nring[j] = norms_of(pj);
        if (i >= 0) {
          TERM_LK_NOW(tq_s0);
          step(i, rows, nn);
#ifdef RGPU_TERM_TRACE
          tq_step += (uint32_t)((uint64_t)clock64() - tq_s0);
#endif
        }
      }
    }
    // (the private lists are in LDS, sorted, 0 = empty: wave 0 folds them behind the barrier below)
  } else if (fast) {
    count = wave == 0 ? 128 * T.nblocks : 0;  // no deleted docs on this path: every posting is a hit
    const uint8_t* pn = seg.pnorm + T.pn_base;
    uint8_t* slab = slabs[wave];
    int cnext = 0;  // workgroup-uniform: the first chunk not gathered yet
#if RGPU_TERMQ_DEAL
    bool redo = false;  // workgroup-uniform: the window at cnext filled a round and is repeated (done_map holds what it queued)
#endif
    while (cnext < n_chunks) {  // rounds
      int nq = 0;  // entries in the queue (workgroup-uniform)
#if RGPU_TERMQ_DEAL
      if (tid == 0) { q_count = 0u; q_end = 0xffffffffu; }  // (the window's barriers lie between this and the first reservation)
#endif
      // ---- gather ----
      while (cnext < n_chunks) {
        // a window of TQ_CHUNK_UNROLL * NT chunks from cnext: one thread per chunk against its frontier word, strict where the doc in
        // front of the chunk is at or past the threshold's doc (the list is the same in every wave: nothing is offered while gathering)
        tau = tau_now();
#if RGPU_TERMQ_DEAL
        if (!redo && tid < TQ_CHUNK_UNROLL * NT / 32) done_map[tid] = 0u;  // a new window (its chunks are marked two barriers on)
#endif
        uint64_t pass_m[TQ_CHUNK_UNROLL];
        uint32_t tb = 0u;
#pragma unroll
        for (int u = 0; u < TQ_CHUNK_UNROLL; ++u) {
          // (a wave whose 64 chunks of this round all lie past the list's end — every wave of a round past it — has nothing to test)
          if (cnext + u * NT + 64 * wave >= n_chunks) { pass_m[u] = 0ull; continue; }
          const int c = cnext + u * NT + tid;
#if RGPU_TERMQ_DEAL  // a repeated window: the chunks an earlier round of it queued are out (this wave's 64 bits of the map, uniform)
          uint64_t dm = 0ull;
          if (redo) {
            const int wd = 2 * (u * W + wave);
            dm = ((uint64_t)(uint32_t)readfirstlane((int)done_map[wd + 1]) << 32) | (uint32_t)readfirstlane((int)done_map[wd]);
          }
          const bool in = c < n_chunks && ((dm >> lane) & 1ull) == 0ull;
#else
          const bool in = c < n_chunks;
#endif
          const bool whole = in && 64 * c + 64 <= T.nblocks;
          const bool worded = whole && seg.dir_sum != nullptr;
          const uint64_t w = worded ? seg.dir_sum[sum_base + (uint32_t)c] : 15ull;
          const int32_t lo = (in && c > 0) ? seg.dir_last[T.dir_base + 64u * (uint32_t)c - 1u] : -1;
          tb += (worded ? 8u : 0u) + ((in && c > 0) ? 4u : 0u);
          pass_m[u] = __ballot(in && term_bound_of(cache, w) >= term_thr_of(tau, lo));
        }
        touched += (uint32_t)wave_reduce_add((int)tb);
#pragma unroll
        for (int u = 0; u < TQ_CHUNK_UNROLL; ++u)
          if (lane == 0) cnt[u * W + wave] = (uint32_t)__popcll(pass_m[u]);
        __syncthreads();
        {  // survivors in chunk order: (u, wave, lane)
          const int nc = TQ_CHUNK_UNROLL * W;
          const int v = lane < nc ? (int)cnt[lane] : 0;
          const int incl = wave_incl_scan(v);
#pragma unroll
          for (int u = 0; u < TQ_CHUNK_UNROLL; ++u) {
            const int at = readlane(incl - v, u * W + wave);
            if ((pass_m[u] >> lane) & 1ull) cq[at + mbcnt(pass_m[u])] = (uint32_t)(cnext + u * NT + tid);
          }
        }
        const int n_cq = (int)readfirstlane(wave_reduce_add(lane < TQ_CHUNK_UNROLL * W ? (int)cnt[lane] : 0));
        const int window_end = min(n_chunks, cnext + TQ_CHUNK_UNROLL * NT);
        __syncthreads();
#if RGPU_TERMQ_DEAL
        // the surviving chunks, dealt to the waves (wave w: cq[w], cq[w + W], ...), no barrier inside: every block's frontier word,
        // store row, header and the doc in front of it, one lane per block, TQ_DEAL_CHUNKS chunks of the wave requested at a time.
        // The blocks that may still enter take queue entries reserved from q_count (consecutive intervals of a counter that only
        // grows): a reservation that fits is written and its chunk marked done; the first that does not fit starts at q_end, every
        // earlier one ends at or below it and every later one starts past TQ_CAP — [0, min(q_count, q_end)) is what was written.
        bool full = false;
        if (n_cq > 0) {
          bool stop = false;  // (wave-uniform) this wave met a full queue
          for (int base = wave; base < n_cq && !stop; base += W * TQ_DEAL_CHUNKS) {
            uint64_t bm[TQ_DEAL_CHUNKS];
            uint32_t rw[TQ_DEAL_CHUNKS], hd[TQ_DEAL_CHUNKS];
            int32_t lo[TQ_DEAL_CHUNKS];
            int ch[TQ_DEAL_CHUNKS];
#pragma unroll
            for (int g = 0; g < TQ_DEAL_CHUNKS; ++g) {
              const int ci = base + g * W;
              ch[g] = ci < n_cq ? (int)cq[ci] : -1;
              if (ch[g] < 0) { bm[g] = 0ull; rw[g] = 0u; hd[g] = 0u; lo[g] = -1; continue; }  // an empty slot requests nothing
              const int nb = min(64, T.nblocks - 64 * ch[g]);
              const bool ok = lane < nb;
              const uint32_t b = T.dir_base + 64u * (uint32_t)ch[g] + (uint32_t)lane;
              bm[g] = ok ? seg.dir_bmax[b] : 0ull;
              rw[g] = ok ? seg.dir_row[b] : 0u;
              hd[g] = ok ? (uint32_t)seg.dir_hdr[b] : 0u;
              lo[g] = (ok && b > T.dir_base) ? seg.dir_last[b - 1u] : -1;
              touched += 18u * (uint32_t)nb;
            }
#pragma unroll
            for (int g = 0; g < TQ_DEAL_CHUNKS; ++g) {
              if (ch[g] < 0 || stop) continue;
              const int nb = min(64, T.nblocks - 64 * ch[g]);
              const uint32_t bd = term_bound_of(cache, bm[g]);
              const uint64_t pm = __ballot(lane < nb && bd >= term_thr_of(tau, lo[g]));
              const int n = __popcll(pm);
              const int wi = ch[g] - cnext;  // the chunk's bit in the window's done map
              uint32_t at = 0u;
              if (n > 0) {  // (a chunk with nothing to queue is done without a reservation)
                if (lane == 0) at = atomicAdd(&q_count, (uint32_t)n);
                at = (uint32_t)readfirstlane((int)at);
                if (at + (uint32_t)n > (uint32_t)TQ_CAP) {  // the round is full; the chunk stays undone and this wave takes no more
                  if (lane == 0) atomicMin(&q_end, at);
                  stop = true;
                  continue;
                }
                if ((pm >> lane) & 1ull) {
                  const uint32_t e = at + (uint32_t)mbcnt(pm);
                  e_blk[e] = (uint32_t)(64 * ch[g] + lane);
                  e_row[e] = rw[g];
                  e_hdr[e] = (uint16_t)hd[g];
                  e_lo[e] = lo[g];
                  e_bound[e] = bd;
                }
              }
              if (lane == 0) atomicOr(&done_map[wi >> 5], 1u << (wi & 31));
            }
          }
          __syncthreads();
          const uint32_t qc = q_count, qe = q_end;
          nq = (int)(qc < qe ? qc : qe);
          full = qe != 0xffffffffu;
        }
        // a full round drains, then repeats this window from its start with the threshold the drain reached: the window test skips
        // the chunks marked done, so no block is queued twice
        redo = full;
        if (full) break;
        cnext = window_end;
      }
#else
        // the surviving chunks, TQ_STEP_CHUNKS per wave per step: every block's frontier word, store row, header and the doc in front
        // of it, one lane per block; the blocks that may still enter are appended to the queue in block order. A step whose blocks
        // do not all fit ends the round at the first chunk that does not fit.
        int pos = 0;
        bool full = false;
        while (pos < n_cq) {
          uint64_t bm[TQ_STEP_CHUNKS];
          uint32_t rw[TQ_STEP_CHUNKS], hd[TQ_STEP_CHUNKS];
          int32_t lo[TQ_STEP_CHUNKS];
          int ch[TQ_STEP_CHUNKS];
#pragma unroll
          for (int s = 0; s < TQ_STEP_CHUNKS; ++s) {
            const int ci = pos + wave * TQ_STEP_CHUNKS + s;
            ch[s] = ci < n_cq ? (int)cq[ci] : -1;
            if (ch[s] < 0) { bm[s] = 0ull; rw[s] = 0u; hd[s] = 0u; lo[s] = -1; continue; }  // an empty slot requests nothing
            const int nb = min(64, T.nblocks - 64 * ch[s]);
            const bool ok = lane < nb;
            const uint32_t b = T.dir_base + 64u * (uint32_t)ch[s] + (uint32_t)lane;
            bm[s] = ok ? seg.dir_bmax[b] : 0ull;
            rw[s] = ok ? seg.dir_row[b] : 0u;
            hd[s] = ok ? (uint32_t)seg.dir_hdr[b] : 0u;
            lo[s] = (ok && b > T.dir_base) ? seg.dir_last[b - 1u] : -1;
            touched += 18u * (uint32_t)nb;
          }
          uint64_t pm[TQ_STEP_CHUNKS];
          uint32_t bd[TQ_STEP_CHUNKS];  // the block's bound: ten table reads, kept for the queue entry
#pragma unroll
          for (int s = 0; s < TQ_STEP_CHUNKS; ++s) {
            if (ch[s] < 0) {  // (wave-uniform) an empty slot: no bound, no candidates
              bd[s] = 0u;
              pm[s] = 0ull;
            } else {
              const int nb = min(64, T.nblocks - 64 * ch[s]);
              bd[s] = term_bound_of(cache, bm[s]);
              pm[s] = __ballot(lane < nb && bd[s] >= term_thr_of(tau, lo[s]));
            }
            if (lane == 0) cnt[wave * TQ_STEP_CHUNKS + s] = (uint32_t)__popcll(pm[s]);
          }
          __syncthreads();
          const int ns = W * TQ_STEP_CHUNKS;
          const int v = lane < ns ? (int)cnt[lane] : 0;
          const int incl = wave_incl_scan(v);
          const int cut = __popcll(__ballot(lane < ns && nq + incl <= TQ_CAP));  // chunks of this step that fit (a prefix)
#pragma unroll
          for (int s = 0; s < TQ_STEP_CHUNKS; ++s) {
            const int i = wave * TQ_STEP_CHUNKS + s;
            if (i < cut && ((pm[s] >> lane) & 1ull)) {
              const int at = nq + readlane(incl - v, i) + mbcnt(pm[s]);
              e_blk[at] = (uint32_t)(64 * ch[s] + lane);
              e_row[at] = rw[s];
              e_hdr[at] = (uint16_t)hd[s];
              e_lo[at] = lo[s];
              e_bound[at] = bd[s];
            }
          }
          nq += cut > 0 ? readlane(incl, cut - 1) : 0;
          pos = min(n_cq, pos + cut);
          __syncthreads();
          if (cut < ns) { full = true; break; }
        }
        if (full && pos < n_cq) { cnext = (int)cq[pos]; break; }  // the round is full: the next one resumes at this chunk
        cnext = window_end;
        if (full) break;
      }
#endif
#ifdef RGPU_TERM_TRACE
      if (tq_rounds == 0) TQ_TR(3, nq);
      tq_rounds += 1;
      tq_entries += nq;
#endif
      if (nq == 0) continue;
#if RGPU_TERMQ_DEAL
      // ---- sort: queue position -> entry, (bound desc, block asc) as one key; the entries lie in the order the waves reserved them ----
      for (int i = tid; i < nq; i += NT) {
        const uint64_t ki = ((uint64_t)e_bound[i] << 32) | (uint64_t)(0xffffffffu - e_blk[i]);
        int r = 0;
        for (int j = 0; j < nq; ++j) {
          const uint64_t kj = ((uint64_t)e_bound[j] << 32) | (uint64_t)(0xffffffffu - e_blk[j]);
          r += kj > ki ? 1 : 0;
        }
        e_order[r] = (uint16_t)i;
      }
#else
      // ---- sort: queue position -> entry, (bound desc, entry asc); entries are in block order ----
      for (int i = tid; i < nq; i += NT) {
        const uint32_t bi = e_bound[i];
        int r = 0;
        for (int j = 0; j < nq; ++j) {
          const uint32_t bj = e_bound[j];
          r += (bj > bi || (bj == bi && j < i)) ? 1 : 0;
        }
        e_order[r] = (uint16_t)i;
      }
#endif
      if (tid == 0) cursor = 0u;
      __syncthreads();
#ifdef RGPU_TERM_TRACE
      if (tq_rounds == 1) TQ_TR(4, e_order[0]);
#endif
      // ---- drain ----
      // An entry is re-tested against the list's k-th best of the moment when it is popped. The threshold only rises, and an entry
      // behind a failed one has a bound at most as large and, at an equal bound, a later block (its doc in front is at least as
      // large: term_thr_of is at least as strict) — so the first failure ends the round for every wave.
      auto pop = [&]() -> int {
        uint32_t p = 0u;
        if (lane == 0) p = atomicAdd(&cursor, 1u);
        p = (uint32_t)readfirstlane((int)p);
        if (p >= (uint32_t)nq) return -1;
        const int i = (int)e_order[p];
        if (e_bound[i] >= term_thr_of(tau_now(), e_lo[i])) return i;
        if (lane == 0) atomicMax(&cursor, (uint32_t)nq);
        return -1;
      };
      auto norms_of = [&](int i) -> uint32_t {
        return *reinterpret_cast<const uint16_t*>(pn + (128u * e_blk[i] + 2u * (uint32_t)lane));
      };
      auto step = [&](int i, const uint4& rows, uint32_t nn) {
        const uint32_t hdr = (uint32_t)e_hdr[i];
        const int32_t lo = e_lo[i];
        touched += encoded_block_bytes(hdr) + 128u;  // both streams' rows + the posting-order norms were requested at the pop
        // once more against the threshold of the moment: up to DEPTH pops of every wave are in flight, and the list may have risen
        // since this one was popped
        tau = tau_now();
        if (e_bound[i] < term_thr_of(tau, lo)) return;
        const int bf = hdr_bfreq(hdr);
        stage_rows(rows, slab, lane);
        wave_sync();
        uint32_t f0, f1;
        bool in_table = true;  // wave-uniform: every freq of the block has a table column
        if (bf) {
          extract_pair<LEGACY>(slab + SLAB_STREAM, bf, lane, f0, f1);
          if (bf > 3) in_table = !__ballot((f0 > f1 ? f0 : f1) > (uint32_t)SCORE_TABLE_FREQS);
        } else {
          const uint32_t f = (uint32_t)readlane((int)rows.x, 32);  // all-equal stream: its value
          f0 = f1 = f;
          in_table = f <= (uint32_t)SCORE_TABLE_FREQS;
        }
        const uint32_t nb0 = nn & 0xffu, nb1 = nn >> 8;
        float s0, s1;
        if (in_table) {
          s0 = table_score(cache, nb0, f0);
          s1 = table_score(cache, nb1, f1);
        } else {
          s0 = bm25_score(wk, (float)(int32_t)f0, cache[nb0]);
          s1 = bm25_score(wk, (float)(int32_t)f1, cache[nb1]);
        }
        looked += 1u;
        tau = tau_now();
        const uint32_t thr = term_thr_of(tau, lo);
        const uint32_t r0 = __float_as_uint(s0), r1 = __float_as_uint(s1);
        if (__ballot((r0 > r1 ? r0 : r1) >= thr)) {  // the doc deltas only when some posting can still enter
          uint32_t e0, e1;
          staged_doc_deltas<LEGACY>(slab, rows, hdr, lane, e0, e1);
          int32_t d0, d1;
          deltas_to_docs(e0, e1, lo < 0 ? 0 : lo, d0, d1);
          const uint64_t key0 = make_key(s0, d0), key1 = make_key(s1, d1);
          tau = tau_now();
          if (__ballot((key0 > key1 ? key0 : key1) > tau)) group_offer2<WIDE>(group, key0, key1, tau, k, lane, floor, slab TERM_LK_PASS);
        }
        wave_sync();  // slab is free for the next block
      };
      // a DEPTH-deep ring of row (and norm) loads per wave; slots without an entry reload entry 0 instead of being guarded
      int slot[DEPTH];
      uint4 ring[DEPTH];
      uint32_t nring[DEPTH];
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        slot[j] = pop();
        const int pj = slot[j] < 0 ? 0 : slot[j];
        ring[j] = block_rows_load(block_rows_at(term_rows, e_row[pj]), e_hdr[pj], lane);
        nring[j] = norms_of(pj);
      }
      while (slot[0] >= 0) {  // slots fill in order, so an empty slot 0 means an empty ring
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
          const uint4 rows = ring[j];
          const uint32_t nn = nring[j];
          const int i = slot[j];
          slot[j] = i >= 0 ? pop() : -1;
          const int pj = slot[j] < 0 ? 0 : slot[j];
          ring[j] = block_rows_load(block_rows_at(term_rows, e_row[pj]), e_hdr[pj], lane);
          nring[j] = norms_of(pj);
          if (i >= 0) {
            TERM_LK_NOW(tq_s0);
            step(i, rows, nn);
#ifdef RGPU_TERM_TRACE
            tq_step += (uint32_t)((uint64_t)clock64() - tq_s0);
#endif
          }
        }
      }
      __syncthreads();  // every offer of this round is in the list; the queue is free
    }
  } else {
    // off the table path: the waves stride over the list's chunks of 64 blocks and share the list
    const bool has_live = seg.live != nullptr;
    uint8_t* slab = slabs[wave];
    auto on_block = [&](int blk, int32_t d0, int32_t d1, uint32_t f0, uint32_t f1, uint32_t nb0, uint32_t nb1) {
      looked += 1u;  // the general path decodes every block
      touched += encoded_block_bytes((uint32_t)seg.dir_hdr[T.dir_base + blk]) + (has_norms ? 128u : 0u);
      bool v0 = true, v1 = true;
      if (has_live) {
        v0 = doc_in_segment(seg, d0) && doc_is_live(seg.live, d0);
        v1 = doc_in_segment(seg, d1) && doc_is_live(seg.live, d1);
      }
      float s0, s1;
      const uint32_t fmax = f0 > f1 ? f0 : f1;
      if (tabled && !__ballot((v0 || v1) && fmax > (uint32_t)SCORE_TABLE_FREQS)) {
        s0 = table_score(cache, nb0, v0 ? f0 : 1u);
        s1 = table_score(cache, nb1, v1 ? f1 : 1u);
      } else {
        s0 = bm25_score(wk, (float)(int32_t)f0, has_norms ? cache[nb0] : k1);
        s1 = bm25_score(wk, (float)(int32_t)f1, has_norms ? cache[nb1] : k1);
      }
      count += __popcll(__ballot(v0)) + __popcll(__ballot(v1));
      const uint64_t key0 = v0 ? make_key(s0, d0) : 0ull, key1 = v1 ? make_key(s1, d1) : 0ull;
      if (__ballot((key0 > key1 ? key0 : key1) > tau)) group_offer2<WIDE>(group, key0, key1, tau, k, lane, floor, slab TERM_LK_PASS);
    };
    for (int c = wave; c < n_chunks; c += W) {
      const int b0 = 64 * c, b1 = min(T.nblocks, b0 + 64);
      int32_t base = b0 == 0 ? 0 : seg.dir_last[T.dir_base + b0 - 1];
      if (has_norms)
        stream_blocks<LEGACY, true>(term_rows, seg.dir_row, seg.dir_hdr, T.dir_base, seg.pnorm + T.pn_base, b0, b1, slab, lane, base, on_block);
      else
        stream_blocks<LEGACY, false>(term_rows, seg.dir_row, seg.dir_hdr, T.dir_base, nullptr, b0, b1, slab, lane, base, on_block);
    }
  }

  if (lane == 0) {
    atomicAdd(&sums[0], (uint32_t)count);
    atomicAdd(&sums[1], looked);
    atomicAdd(&sums[2], touched);
#ifdef RGPU_TERM_TRACE
    if (wave < 8) { tq_w[wave][0] = lk[0]; tq_w[wave][1] = lk[1]; tq_w[wave][2] = tq_step; tq_w[wave][3] = lk[2]; tq_w[wave][4] = lk[3]; }
#endif
  }
  __syncthreads();
  if (wave != 0) return;
#ifdef RGPU_TERM_TRACE
  TQ_TR(5, sums[0]);
  const unsigned int tq_wave0 = (unsigned int)((uint64_t)clock64() - tq_c0);
#endif
  // the tail and the singleton (postings outside FullBlocks), then the caller's row
  {
    const bool has_live = seg.live != nullptr;
    int tcount = 0;
    auto collect = [&](int32_t d0, int32_t d1, uint32_t f0, uint32_t f1, uint32_t nb0, uint32_t nb1, bool v0, bool v1) {
      if (has_live) {
        v0 = v0 && doc_in_segment(seg, d0) && doc_is_live(seg.live, d0);
        v1 = v1 && doc_in_segment(seg, d1) && doc_is_live(seg.live, d1);
      }
      float s0, s1;
      const uint32_t fmax = f0 > f1 ? f0 : f1;
      if (tabled && !__ballot((v0 || v1) && fmax > (uint32_t)SCORE_TABLE_FREQS)) {
        s0 = table_score(cache, nb0, v0 ? f0 : 1u);
        s1 = table_score(cache, nb1, v1 ? f1 : 1u);
      } else {
        s0 = bm25_score(wk, (float)(int32_t)f0, has_norms ? cache[nb0] : k1);
        s1 = bm25_score(wk, (float)(int32_t)f1, has_norms ? cache[nb1] : k1);
      }
      tcount += __popcll(__ballot(v0)) + __popcll(__ballot(v1));
      const uint64_t key0 = v0 ? make_key(s0, d0) : 0ull, key1 = v1 ? make_key(s1, d1) : 0ull;
      tau = tau_now();
      if (__ballot((key0 > key1 ? key0 : key1) > tau)) group_offer2<WIDE>(group, key0, key1, tau, k, lane, floor, slabs[0] TERM_LK_PASS);
    };
    WaveTopK merged;
    if (one) {
      // every wave's list is in LDS (the barrier above), the tail is in wave W - 1's: one bitonic merge per list
      const uint64_t* wl = reinterpret_cast<const uint64_t*>(cq);
      merged.a = wl[lane];
      if (WIDE) merged.b = wl[64 + lane];
#pragma unroll
      for (int w = 1; w < W; ++w) topk_merge_sorted<WIDE>(merged, wl[w * LIST_N + lane], WIDE ? wl[w * LIST_N + 64 + lane] : 0ull, lane);
    } else if (T.df == 1) {
      const bool v0 = lane == 0;
      const uint32_t nb0 = (has_norms && v0) ? norm_at(seg, T.singleton_doc) : 0u;
      collect(T.singleton_doc, 0, (uint32_t)T.singleton_freq, 1u, nb0, 0u, v0, false);
    } else if (T.tail_n > 0) {
      int32_t d0, d1;
      uint32_t f0, f1;
      tail_load(term_rows, seg.dir_row[T.dir_base + T.nblocks], lane, d0, d1, f0, f1);  // decoded and validated at prepare time
      const bool v0 = 2 * lane < T.tail_n, v1 = 2 * lane + 1 < T.tail_n;
      const uint32_t nb0 = (has_norms && v0) ? seg.norms[d0] : 0u, nb1 = (has_norms && v1) ? seg.norms[d1] : 0u;
      collect(d0, d1, f0, f1, nb0, nb1, v0, v1);
    }
    wave_sync();
    const uint64_t a = one ? merged.a : list[lane];
    const uint64_t b = !WIDE ? 0ull : one ? merged.b : list[64 + lane];
    if (lane < k) out[lane] = a ? HitOut{key_doc(a) + doc_base, key_score(a)} : HitOut{-1, 0.f};
    if (WIDE && lane + 64 < k) out[lane + 64] = b ? HitOut{key_doc(b) + doc_base, key_score(b)} : HitOut{-1, 0.f};
    if (lane == 0) {
      totals[row] = (int64_t)sums[0] + tcount;
      if (work_slots != nullptr) {
        work_slots[q] = (unsigned long long)sums[2];
        work_slots[n_queries + q] = (unsigned long long)sums[1];
      }
    }
#ifdef RGPU_TERM_TRACE
    TQ_TR(6, a);
    if (lane == 0 && 3 * (int)blockIdx.x + 2 < TERM_TRACE_CAP) {
      TermQueryTraceRec r{};
      r.t0 = tq_t0; r.t1 = (unsigned long long)wall_clock64();
      r.q = q; r.nblocks = T.nblocks; r.rounds = tq_rounds; r.entries = tq_entries; r.unpacked = (int32_t)sums[1];
      for (int i = 0; i < 7; ++i) r.d[i] = tq_d[i];
      r.waves = (unsigned int)W; r.wave0_cycles = tq_wave0;
      r.pad[0] = one ? 1u : 0u;  // the workgroup took the one-chunk path (rounds 0, entries = the survivors of its ballot)
      int offers = 0, entered = 0;
      for (int w = 0; w < (W < 8 ? W : 8); ++w) {
        r.cyc[w][0] = tq_w[w][0]; r.cyc[w][1] = tq_w[w][1]; r.cyc[w][2] = tq_w[w][2] - tq_w[w][0] - tq_w[w][1];
        offers += (int)tq_w[w][3]; entered += (int)tq_w[w][4];
      }
      r.offers = offers + (int)(lk[2] - tq_w[0][3]); r.entered = entered + (int)(lk[3] - tq_w[0][4]);  // (+ the tail's, wave 0)
      reinterpret_cast<TermQueryTraceRec*>(g_term_trace)[blockIdx.x] = r;
    }
#endif
  }
}

}  // namespace rgpu
