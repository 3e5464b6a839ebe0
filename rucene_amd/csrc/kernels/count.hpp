// Hit counts without scoring: the kernels of rgpu_count_batch (IndexSearcher::count, search/searcher.rs:632-654 - a
// TotalHitCountCollector, collector/mod.rs: needs_scores() is false; TotalHitsCountLeafCollector counts the live docs a scorer
// stops at). No freq is decoded into a score, no norm is read, no list of hits is kept: a row's answer is one u64 in counts[row].
//   k_count_lists     LIST rows (a lone term under deletions or a doc set): the term's prepared list decoded block by block as
//                     k_docset_lists does, every posting looked up in the mask words
//   k_count_windows   WINDOWS rows (unions, min_should_match >= 2, MUST_NOT beside a lone term): a run of consecutive doc-id windows
//                     per wavefront; the window lives in the wavefront's LDS slice as a bit per doc, or as two counters per doc
//   k_count_emitted   CONJ rows: the candidate lists k_search_and leaves in emit mode, counted against the mask
// The mask: FixedBitSet words (bit doc & 63 of u64 word doc >> 6, viewed as u32 like the doc-set kernels do) - the segment's live
// docs, a doc set's words, or `live AND set`; null = every doc below max_doc. Every kernel adds into counts[row] with ONE vector
// atomic per work item (unsigned long long, as k_docset_combine), after a ballot / popcount reduction inside the wavefront.
#pragma once
#include "decode.hpp"
#include "decode_terms.hpp"
#include "docset.hpp"
#include "search_and.hpp"
#include "types.hpp"

namespace rgpu {

constexpr int COUNT_THREADS = 256;
constexpr int COUNT_WAVES = COUNT_THREADS / 64;
// Docs per window of k_count_windows: 64 lanes x 32 bits, so the bit form of a window is ONE u32 per lane - a clause that has a doc
// bitmap hands its window over with one coalesced 256-byte read of TermBitmap::memb and no LDS traffic at all - and the counter
// form (a u8 pair per doc) is 4 KiB per wavefront: with the decoders' slab 4 x (2432 + 4096) = 26112 bytes per workgroup, under the
// 32 KiB that keeps two workgroups' worth of wavefronts per SIMD resident beside the 160 KiB of a CU.
constexpr int COUNT_WINDOW_DOCS = 2048;
constexpr int COUNT_WINDOW_WORDS = COUNT_WINDOW_DOCS / 32;
static_assert(COUNT_WINDOW_WORDS == 64, "the bit form of a window is one u32 per lane");
static_assert(COUNT_WINDOW_WORDS <= BITMAP_PAD_WORDS, "a whole window is read from TermBitmap::memb without a bounds test");
// A counter per doc and side: up to RGPU_MAX_QUERY_TERMS = 64 clauses can hold one doc, so a counter must reach 64 without wrapping
constexpr int COUNT_COUNTER_BITS = 8;
using count_counter_t = uint8_t;
static_assert((1 << COUNT_COUNTER_BITS) > 64 && sizeof(count_counter_t) * 8 == COUNT_COUNTER_BITS, "a counter holds 64");
constexpr int COUNT_COUNTERS_PER_WORD = 32 / COUNT_COUNTER_BITS;                        // 4 docs per u32 of LDS
constexpr int COUNT_SIDE_WORDS = COUNT_WINDOW_DOCS / COUNT_COUNTERS_PER_WORD;           // 512 u32 per side
constexpr int COUNT_LDS_WORDS = 2 * COUNT_SIDE_WORDS;                                   // positive side, negative side (the bit form uses 64 + 64 of them)
static_assert(COUNT_WAVES * (SLAB_BYTES + 4 * COUNT_LDS_WORDS) <= 32768, "static LDS per workgroup stays at or below 32 KiB");

__device__ __forceinline__ bool count_mask_bit(const uint32_t* __restrict__ mask, int32_t max_doc, int32_t d) {
  if ((uint32_t)d >= (uint32_t)max_doc) return false;  // (a damaged list never reads out of bounds)
  return mask == nullptr || ((mask[(uint32_t)d >> 5] >> (d & 31)) & 1u) != 0u;
}
// the mask's u32 word `w` (32 docs from 32 w on), zero at and past max_doc
__device__ __forceinline__ uint32_t count_mask_word(const uint32_t* __restrict__ mask, int32_t max_doc, int64_t w) {
  const int64_t first = w << 5;
  if (first >= (int64_t)max_doc) return 0u;
  const int rest = (int)((int64_t)max_doc - first);
  const uint32_t below = rest >= 32 ? 0xffffffffu : ((1u << rest) - 1u);
  return (mask != nullptr ? mask[w] : 0xffffffffu) & below;  // (w < ceil(max_doc / 32) <= 2 * ceil(max_doc / 64): inside the words)
}

struct CountJob {
  uint32_t term;  // index into the launch's DevTerm array
  uint32_t row;   // the counter the postings go to
};

// Items = (job, chunk of DOCSET_BLOCKS_PER_ITEM blocks) exactly as in k_docset_lists (both .doc formats, all-equal blocks, the
// prepared VInt tail, the singleton of the term-dictionary entry, docs-only fields): the last item of a term also takes its tail.
template <bool LEGACY>
__global__ __launch_bounds__(COUNT_THREADS) void k_count_lists(SegView seg, const DevTerm* __restrict__ terms, const CountJob* __restrict__ jobs,
                                                               const int64_t* __restrict__ item_prefix, int n_jobs, int64_t n_items,
                                                               const uint32_t* __restrict__ mask, unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) uint8_t slabs[COUNT_WAVES][SLAB_BYTES];
  const int lane = lane_id();
  const int wave = wave_id();
  const int64_t item = (int64_t)blockIdx.x * COUNT_WAVES + wave;
  if (item >= n_items) return;
  const int j = upper_slot_wave(item_prefix, n_jobs, item, lane);
  const int chunk = (int)(item - item_prefix[j]);
  const CountJob J = jobs[j];
  const DevTerm T = terms[J.term];
  uint8_t* slab = slabs[wave];
  const int b0 = chunk * DOCSET_BLOCKS_PER_ITEM;
  const int b1 = min(T.nblocks, b0 + DOCSET_BLOCKS_PER_ITEM);
  int32_t base = b0 == 0 ? 0 : seg.dir_last[T.dir_base + b0 - 1];
  const uint8_t* term_rows = seg.bstore + T.bs_base;
  int n = 0;  // (wave-uniform: ballots)
  auto take = [&](int32_t d0, int32_t d1, bool v0, bool v1) {
    n += __popcll(__ballot(v0 && count_mask_bit(mask, seg.max_doc, d0))) + __popcll(__ballot(v1 && count_mask_bit(mask, seg.max_doc, d1)));
  };
  stream_blocks<LEGACY, false, 1>(term_rows, seg.dir_row, seg.dir_hdr, T.dir_base, nullptr, b0, b1, slab, lane, base,
                                  [&](int, int32_t d0, int32_t d1, uint32_t, uint32_t, uint32_t, uint32_t) { take(d0, d1, true, true); });
  if (b1 == T.nblocks) {
    if (T.df == 1) {
      take(T.singleton_doc, 0, lane == 0, false);
    } else if (T.tail_n > 0) {
      int32_t d0, d1;
      uint32_t f0, f1;
      tail_load(term_rows, seg.dir_row[T.dir_base + T.nblocks], lane, d0, d1, f0, f1);  // decoded and validated at prepare time
      take(d0, d1, 2 * lane < T.tail_n, 2 * lane + 1 < T.tail_n);
    }
  }
  if (lane == 0 && n != 0) atomicAdd(counts + J.row, (unsigned long long)n);
}

// One row of k_count_windows: clauses [first_clause, first_clause + n_pos) are positive, the n_neg behind them negative
struct CountRow {
  int32_t first_clause;
  int32_t n_pos, n_neg;
  int32_t need, need_not;  // a doc stands when pos >= need && !(neg >= need_not); both 1: the bit form
  int32_t out;             // the counter the row's docs go to
};
struct CountClauseDev {
  uint32_t term;          // index into the launch's DevTerm array
  uint32_t mult;          // clauses of the row that name the term (the counter form adds it)
  const uint32_t* memb;   // TermBitmap::memb when the term has a doc bitmap (read by the bit form), else null: the list is decoded
};

// smallest value over the 64 lanes of non-negative ints
__device__ __forceinline__ int32_t count_wave_min(int32_t v) { return 0x7fffffff - (int32_t)wave_reduce_max_u32((uint32_t)(0x7fffffff - v)); }

// An item = (row, run of `windows_per_item` consecutive windows of COUNT_WINDOW_DOCS docs), one wavefront each. A row has at most
// RGPU_MAX_QUERY_TERMS = 64 clauses, so lane c keeps clause c's state across the run: `cur` - the first block not yet wholly below
// the window, found ONCE per clause with find_block_wave for the run's first doc and advanced from the directory afterwards - and
// `nxt`, a lower bound of the clause's next doc (a sparse list whose next posting lies windows ahead is not decoded again until
// the run gets there). Per window and decoded clause the blocks from `cur` up to the first one whose last doc is at or past the
// window's end are streamed; of a block or a tail that straddles an edge only the docs inside [w0, w1) are taken, and that block is
// where the cursor stays. The window is then ANDed with the mask words (the bits below max_doc without a mask) and popcounted.
// COUNTERS = false: need == need_not == 1 - positive clauses are ORed in, negative ones cleared; clauses with `memb` never touch LDS.
// COUNTERS = true: a u8 per doc and side, four docs to a u32 of LDS; every clause is decoded.
template <bool LEGACY>
__global__ __launch_bounds__(COUNT_THREADS) void k_count_windows(SegView seg, const DevTerm* __restrict__ terms, const CountRow* __restrict__ rows,
                                                                 const CountClauseDev* __restrict__ clauses, int n_rows, int items_per_row,
                                                                 int windows_per_item, const uint32_t* __restrict__ mask,
                                                                 unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) uint8_t slabs[COUNT_WAVES][SLAB_BYTES];
  __shared__ uint32_t lds[COUNT_WAVES][COUNT_LDS_WORDS];
  const int lane = lane_id();
  const int wave = wave_id();
  const int64_t item = (int64_t)blockIdx.x * COUNT_WAVES + wave;
  if (item >= (int64_t)n_rows * items_per_row) return;
  const int r = (int)(item / items_per_row);
  const CountRow R = rows[r];
  const int64_t n_windows = ((int64_t)seg.max_doc + COUNT_WINDOW_DOCS - 1) / COUNT_WINDOW_DOCS;
  const int64_t win0 = (item - (int64_t)r * items_per_row) * windows_per_item;
  const int64_t win1 = win0 + windows_per_item < n_windows ? win0 + windows_per_item : n_windows;
  if (win0 >= win1) return;
  uint8_t* slab = slabs[wave];
  uint32_t* pos = lds[wave];
  uint32_t* neg = lds[wave] + COUNT_SIDE_WORDS;
  const bool counters = R.need != 1 || R.need_not != 1;
  const int n_clauses = R.n_pos + R.n_neg;  // <= 64
  // lane c: clause c
  const bool mine = lane < n_clauses;
  const CountClauseDev C = mine ? clauses[R.first_clause + lane] : CountClauseDev{0u, 0u, nullptr};
  const DevTerm T = terms[mine ? C.term : clauses[R.first_clause].term];
  const bool use_memb = mine && C.memb != nullptr && !counters;
  const int32_t run_first = (int32_t)(win0 * COUNT_WINDOW_DOCS);
  int cur = 0;
  for (int c = 0; c < n_clauses; ++c) {  // the one search per clause and item
    if (readlane((int)use_memb, c)) continue;
    const int nb = readlane(T.nblocks, c);
    const int at = find_block_wave(seg.dir_last, (uint32_t)readlane((int)T.dir_base, c), 0, nb, run_first, lane);
    if (lane == c) cur = at;
  }
  int32_t nxt = 0;
  unsigned long long total = 0;
  for (int64_t win = win0; win < win1; ++win) {
    const int32_t w0 = (int32_t)(win * COUNT_WINDOW_DOCS);
    const int64_t w1l = (int64_t)w0 + COUNT_WINDOW_DOCS;
    const int32_t w1 = w1l > (int64_t)seg.max_doc ? seg.max_doc : (int32_t)w1l;  // docs of the window: [w0, w1), w1 <= max_doc
    if (counters) {
#pragma unroll
      for (int i = 0; i < COUNT_LDS_WORDS / 64; ++i) lds[wave][i * 64 + lane] = 0u;
    } else {
      pos[lane] = 0u;
      neg[lane] = 0u;
    }
    wave_sync();
    uint32_t acc = 0u, nacc = 0u;  // the bit form's words that came straight from doc bitmaps
    for (int c = 0; c < n_clauses; ++c) {
      const bool negative = c >= R.n_pos;
      if (readlane((int)use_memb, c)) {
        const uint32_t* memb = (const uint32_t*)(((uint64_t)(uint32_t)readlane((int)((uint64_t)C.memb >> 32), c) << 32) | (uint32_t)readlane((int)(uint32_t)(uint64_t)C.memb, c));
        const uint32_t word = memb[(w0 >> 5) + lane];  // (zero padded behind the last real word)
        if (negative) nacc |= word; else acc |= word;
        continue;
      }
      if (readlane(nxt, c) >= w1) continue;  // nothing of this clause before the window's end
      const int nb = readlane(T.nblocks, c);
      const int df = readlane(T.df, c);
      const uint32_t dir_base = (uint32_t)readlane((int)T.dir_base, c);
      const uint64_t bs_base = ((uint64_t)(uint32_t)readlane((int)(T.bs_base >> 32), c) << 32) | (uint32_t)readlane((int)(uint32_t)T.bs_base, c);
      const uint32_t add = (uint32_t)readlane((int)C.mult, c);
      uint32_t* side = negative ? neg : pos;
      int32_t ahead = 0x7fffffff;  // the smallest doc at or past w1 this lane saw
      auto take = [&](int32_t d, bool valid) {
        if (!valid) return;
        if (d >= w1) { ahead = d < ahead ? d : ahead; return; }
        if (d < w0) return;
        const int o = d - w0;
        if (counters) atomicAdd(side + (o >> 2), add << (COUNT_COUNTER_BITS * (o & 3)));
        else atomicOr(side + (o >> 5), 1u << (o & 31));
      };
      const uint8_t* term_rows = seg.bstore + bs_base;
      int b = readlane(cur, c);
      bool open = false;  // a block whose last doc is at or past w1 was decoded: the cursor stays on it
      while (b < nb) {
        const int p = b + lane;
        const int32_t last = p < nb ? seg.dir_last[dir_base + p] : 0x7fffffff;
        const uint64_t m = __ballot(last >= w1);  // (never empty when the directory window reaches past the last block)
        const int e = m ? b + (int)__builtin_ctzll(m) : b + 64;  // <= nb
        const int stop = m ? (e + 1 < nb ? e + 1 : nb) : e;
        if (stop > b) {
          int32_t base = b == 0 ? 0 : seg.dir_last[dir_base + b - 1];
          stream_blocks<LEGACY, false, 1>(term_rows, seg.dir_row, seg.dir_hdr, dir_base, nullptr, b, stop, slab, lane, base,
                                          [&](int, int32_t d0, int32_t d1, uint32_t, uint32_t, uint32_t, uint32_t) { take(d0, true); take(d1, true); });
        }
        b = e;
        if (m) { open = e < nb; break; }
      }
      if (!open) {  // every block is below the window's end: the tail, or the singleton
        if (df == 1) {
          take(readlane(T.singleton_doc, c), lane == 0);
        } else if (df % 128 > 0) {
          int32_t d0, d1;
          uint32_t f0, f1;
          tail_load(term_rows, seg.dir_row[dir_base + nb], lane, d0, d1, f0, f1);
          take(d0, 2 * lane < df % 128);
          take(d1, 2 * lane + 1 < df % 128);
        }
      }
      const int32_t next_doc = count_wave_min(ahead);  // INT_MAX: the list ends in this window
      if (lane == c) { cur = b; nxt = next_doc; }
    }
    wave_sync();
    int n = 0;
    if (counters) {
      // lane l, step i: LDS word i * 64 + l of either side = docs w0 + 4 (i * 64 + l) .. + 3 (consecutive lanes, consecutive banks)
#pragma unroll
      for (int i = 0; i < COUNT_SIDE_WORDS / 64; ++i) {
        const int wi = i * 64 + lane;
        const uint32_t pw = pos[wi], nw = neg[wi];
        const int64_t doc0 = (int64_t)w0 + 4 * wi;
        const uint32_t live = (count_mask_word(mask, seg.max_doc, doc0 >> 5) >> (doc0 & 31)) & 0xfu;
#pragma unroll
        for (int t = 0; t < COUNT_COUNTERS_PER_WORD; ++t) {
          const int p = (int)((pw >> (COUNT_COUNTER_BITS * t)) & 0xffu), q = (int)((nw >> (COUNT_COUNTER_BITS * t)) & 0xffu);
          n += (int)((live >> t) & 1u) & (int)(p >= R.need && !(q >= R.need_not));
        }
      }
    } else {
      const uint32_t word = (acc | pos[lane]) & ~(nacc | neg[lane]);
      n = __popc(word & count_mask_word(mask, seg.max_doc, (int64_t)(w0 >> 5) + lane));
    }
    total += (unsigned long long)wave_reduce_add(n);
    wave_sync();  // (the next window zeroes the slice)
  }
  if (lane == 0 && total != 0ull) atomicAdd(counts + R.out, total);
}

// k_search_and in emit mode leaves row q's matches at docs[emit_prefix[q] .. + emit_count[q]) in any order, deleted docs with the
// sign bit set. One thread per slot; a slot counts when it is below its row's count, its sign bit is clear and its mask bit set.
// A wavefront's slots ascend through the rows, so it adds once per row it touches (almost always one).
__global__ __launch_bounds__(COUNT_THREADS) void k_count_emitted(const int32_t* __restrict__ docs, const int64_t* __restrict__ emit_prefix,
                                                                 const unsigned long long* __restrict__ emit_count, int n_queries, int64_t n_slots,
                                                                 int32_t max_doc, const uint32_t* __restrict__ mask,
                                                                 unsigned long long* __restrict__ counts) {
  const int64_t slot = (int64_t)blockIdx.x * COUNT_THREADS + threadIdx.x;
  bool hit = false;
  int q = -1;
  if (slot < n_slots) {
    q = upper_slot(emit_prefix, n_queries, slot);
    if ((unsigned long long)(slot - emit_prefix[q]) < emit_count[q]) {
      const int32_t d = docs[slot];
      hit = d >= 0 && count_mask_bit(mask, max_doc, d);
    }
  }
  const int lane = lane_id();
  uint64_t left = __ballot(hit);
  while (left != 0ull) {
    const int q0 = readlane(q, (int)__builtin_ctzll(left));
    const uint64_t same = __ballot(hit && q == q0);
    if (lane == (int)__builtin_ctzll(same)) atomicAdd(counts + q0, (unsigned long long)__popcll(same));
    left &= ~same;
  }
}

}  // namespace rgpu
