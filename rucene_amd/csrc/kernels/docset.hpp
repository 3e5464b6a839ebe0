// Doc sets: a set of ONE segment's doc ids in HBM as FixedBitSet words (bit doc & 63 of u64 word doc >> 6, ceil(max_doc / 64)
// words, no bit at or past max_doc) — the layout of SegView::live, so every collecting kernel reads one as its live docs.
// GPU counterpart of the query cache's fill (search/cache/query_cache.rs:301-372: a non-scoring weight's matches collected once per
// leaf into a FixedBitSet, BitSetLeafCollector :520-536) and of the bit-set algebra behind FILTER / MUST_NOT clauses that are not terms.
//   k_docset_from_docs     host-given ids (any order, repeats) -> bits; ids outside the segment are counted, not written
//   k_docset_lists<CLEAR>  (set row, term) jobs: the term's prepared list decoded block by block, bits set — or cleared (MUST_NOT)
//   k_docset_from_emitted  the candidate lists k_search_and leaves in emit mode -> bits (conjunctions)
//   k_docset_combine       AND of sets, minus sets, inside [0, max_doc), optionally AND live docs; counts the result
//   k_docset_chunk_counts, k_docset_head_scan, k_docset_select_head   the head of a set: its cardinality and first n docs (at the end)
//   k_required_set_fill    rows of "SHOULD clauses beside a required doc set" completed from the head at score 0 (at the end)
// The kernels view the words as u32 (little endian: bit doc & 31 of u32 word doc >> 5 is the same bit).
#pragma once
#include "decode.hpp"
#include "decode_terms.hpp"
#include "search.hpp"
#include "types.hpp"

namespace rgpu {

constexpr int DOCSET_THREADS = 256;
constexpr int DOCSET_WAVES = DOCSET_THREADS / 64;
constexpr int DOCSET_BLOCKS_PER_ITEM = 4;   // 128-posting blocks one wavefront of k_docset_lists decodes (the last item of a term: + its tail)
constexpr int DOCSET_MAX_OPERANDS = 16;     // sets on either side of one k_docset_combine launch

// ids outside [0, max_doc) are counted in status[0] (the host refuses the call) and never touch memory. One atomic per id: the ids
// arrive in no order, so there is nothing to combine in registers (repeats of one id are idempotent).
__global__ __launch_bounds__(DOCSET_THREADS) void k_docset_from_docs(const int32_t* __restrict__ docs, int64_t n, int32_t max_doc,
                                                                      uint32_t* __restrict__ words, unsigned int* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * DOCSET_THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t d = docs[i];
  if ((uint32_t)d >= (uint32_t)max_doc) { atomicAdd(status, 1u); return; }
  atomicOr(words + ((uint32_t)d >> 5), 1u << (d & 31));
}

struct DocsetJob {
  uint32_t term;   // index into the launch's DevTerm array
  uint32_t row;    // index into the launch's row pointers (the set the bits go to)
};

constexpr uint32_t DOCSET_NO_WORD = 0xffffffffu;

// The gathering step of docset_block_bits (below) as a variant of its own for callers that bring words and masks (k_points_scan) —
// kept beside it, not under it, so that what k_docset_lists runs compiles to what it was; it sets bits only. Every lane holds a
// first word wa with the bits ma and a last word wb with the bits mb — wb == wa (then mb == ma) when the lane touches one word —
// the words ascending, not strictly, along (lane, first / last). A mask may be ZERO in any lane (a point outside the range keeps its
// word, so the runs of a word stay contiguous); DOCSET_NO_WORD marks lanes that hold nothing and may only stand on a suffix of the lanes.
__device__ __forceinline__ void docset_wave_masks(uint32_t* __restrict__ words, uint32_t wa, uint32_t ma, uint32_t wb, uint32_t mb, int lane) {
  constexpr uint32_t NONE = DOCSET_NO_WORD;
  // s = OR of ma over this lane and the lanes right behind it whose FIRST word is wa
  uint32_t s = ma;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ow = (uint32_t)__shfl_down((int)wa, off), os = (uint32_t)__shfl_down((int)s, off);
    if (lane + off < 64 && ow == wa) s |= os;
  }
  const uint32_t prev_wa = (uint32_t)__shfl_up((int)wa, 1), prev_wb = (uint32_t)__shfl_up((int)wb, 1);
  const uint32_t next_wa = (uint32_t)__shfl_down((int)wa, 1), next_s = (uint32_t)__shfl_down((int)s, 1);
  // the first word: this lane starts its run unless the lane before touches the word (as its first or as its last word)
  const bool head_a = wa != NONE && (lane == 0 || (prev_wa != wa && prev_wb != wa));
  // the last word, when it is another one: its run starts here, and goes on with the next lanes' first words
  const bool head_b = wb != wa && wb != NONE;
  const uint32_t bits_b = mb | ((lane < 63 && next_wa == wb) ? next_s : 0u);
  if (head_a && s != 0u) atomicOr(words + wa, s);
  if (head_b && bits_b != 0u) atomicOr(words + wb, bits_b);
}

// The 128 postings of a block as the wavefront holds them — lane l: postings 2l and 2l + 1, doc ids ascending along that order — to
// ONE atomic per distinct 32-bit word. A word's bits are gathered in registers first: every lane merges its two postings when they
// share a word, a segmented suffix OR over the lanes (keyed on the lane's first word, five shuffles) collects a word's run, and the
// lane that touches a word first issues the atomic — through its second posting when the run starts there. Estimate: a list that holds one doc
// in g has 128 postings over 128 * g / 32 = 4 g words, so g <= 8 gives <= 32 atomics per block (0.25 per posting) where one atomic per
// posting (k_bitmap_memb's shape) gives 128; past g = 32 every posting has a word of its own and the two shapes meet.
// v0 / v1: the posting exists (a prefix of the order); docs outside the segment are dropped (corrupt lists never write out of bounds).
template <bool CLEAR>
__device__ __forceinline__ void docset_block_bits(uint32_t* __restrict__ words, int32_t max_doc, int32_t d0, int32_t d1, bool v0, bool v1, int lane) {
  constexpr uint32_t NONE = 0xffffffffu;
  v0 = v0 && (uint32_t)d0 < (uint32_t)max_doc;
  v1 = v1 && (uint32_t)d1 < (uint32_t)max_doc;
  uint32_t wa = v0 ? (uint32_t)d0 >> 5 : NONE, ma = v0 ? 1u << (d0 & 31) : 0u;
  uint32_t wb = v1 ? (uint32_t)d1 >> 5 : NONE, mb = v1 ? 1u << (d1 & 31) : 0u;
  if (!v0) { wa = wb; ma = mb; }             // (only a damaged list: the lane's one posting is its first and its last)
  if (!v1 || wb == wa) { ma |= (wb == wa ? mb : 0u); wb = wa; mb = ma; }  // one word in this lane: first == last
  // s = OR of ma over this lane and the lanes right behind it whose FIRST word is wa
  uint32_t s = ma;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ow = (uint32_t)__shfl_down((int)wa, off), os = (uint32_t)__shfl_down((int)s, off);
    if (lane + off < 64 && ow == wa) s |= os;
  }
  const uint32_t prev_wa = (uint32_t)__shfl_up((int)wa, 1), prev_wb = (uint32_t)__shfl_up((int)wb, 1);
  const uint32_t next_wa = (uint32_t)__shfl_down((int)wa, 1), next_s = (uint32_t)__shfl_down((int)s, 1);
  // the first word: this lane starts its run unless the lane before touches the word (as its first or as its last word)
  const bool head_a = wa != NONE && (lane == 0 || (prev_wa != wa && prev_wb != wa));
  // the last word, when it is another one: its run starts here, and goes on with the next lanes' first words
  const bool head_b = wb != wa && wb != NONE;
  const uint32_t bits_b = mb | ((lane < 63 && next_wa == wb) ? next_s : 0u);
  if (head_a && s != 0u) { if (CLEAR) atomicAnd(words + wa, ~s); else atomicOr(words + wa, s); }
  if (head_b && bits_b != 0u) { if (CLEAR) atomicAnd(words + wb, ~bits_b); else atomicOr(words + wb, bits_b); }
}

// Items = (job, chunk of DOCSET_BLOCKS_PER_ITEM blocks) as in k_decode_terms, decoded with the same device functions (both .doc
// formats, all-equal blocks, the prepared VInt tail, the singleton of the term-dictionary entry, docs-only fields); live docs are NOT
// consulted (query_cache.rs:335-342). CLEAR runs as a launch of its own behind the setting launch of the same rows.
template <bool LEGACY, bool CLEAR>
__global__ __launch_bounds__(DOCSET_THREADS) void k_docset_lists(SegView seg, const DevTerm* __restrict__ terms, const DocsetJob* __restrict__ jobs,
                                                                 const int64_t* __restrict__ item_prefix, int n_jobs, int64_t n_items,
                                                                 uint32_t* const* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) uint8_t slabs[DOCSET_WAVES][SLAB_BYTES];
  const int lane = lane_id();
  const int wave = wave_id();
  const int64_t item = (int64_t)blockIdx.x * DOCSET_WAVES + wave;
  if (item >= n_items) return;
  const int j = upper_slot_wave(item_prefix, n_jobs, item, lane);
  const int chunk = (int)(item - item_prefix[j]);
  const DocsetJob J = jobs[j];
  const DevTerm T = terms[J.term];
  uint32_t* const words = rows[J.row];
  uint8_t* slab = slabs[wave];
  const int b0 = chunk * DOCSET_BLOCKS_PER_ITEM;
  const int b1 = min(T.nblocks, b0 + DOCSET_BLOCKS_PER_ITEM);
  int32_t base = b0 == 0 ? 0 : seg.dir_last[T.dir_base + b0 - 1];
  const uint8_t* term_rows = seg.bstore + T.bs_base;
  stream_blocks<LEGACY, false, 1>(term_rows, seg.dir_row, seg.dir_hdr, T.dir_base, nullptr, b0, b1, slab, lane, base,
                                  [&](int, int32_t d0, int32_t d1, uint32_t, uint32_t, uint32_t, uint32_t) {
                                    docset_block_bits<CLEAR>(words, seg.max_doc, d0, d1, true, true, lane);
                                  });
  if (b1 == T.nblocks) {
    if (T.df == 1) {
      docset_block_bits<CLEAR>(words, seg.max_doc, T.singleton_doc, 0, lane == 0, false, lane);
    } else if (T.tail_n > 0) {
      int32_t d0, d1;
      uint32_t f0, f1;
      tail_load(term_rows, seg.dir_row[T.dir_base + T.nblocks], lane, d0, d1, f0, f1);  // decoded and validated at prepare time
      docset_block_bits<CLEAR>(words, seg.max_doc, d0, d1, 2 * lane < T.tail_n, 2 * lane + 1 < T.tail_n, lane);
    }
  }
}

// k_search_and in emit mode leaves query q's matches at docs[emit_prefix[q] .. + emit_count[q]) in any order, deleted docs with the
// sign bit set: they belong in the set all the same. One thread per slot; slots behind a query's count are skipped.
__global__ __launch_bounds__(DOCSET_THREADS) void k_docset_from_emitted(const int32_t* __restrict__ docs, const int64_t* __restrict__ emit_prefix,
                                                                         const unsigned long long* __restrict__ emit_count, int n_queries,
                                                                         int64_t n_slots, int32_t max_doc, uint32_t* const* __restrict__ rows) {
  const int64_t slot = (int64_t)blockIdx.x * DOCSET_THREADS + threadIdx.x;
  if (slot >= n_slots) return;
  const int q = upper_slot(emit_prefix, n_queries, slot);
  if ((unsigned long long)(slot - emit_prefix[q]) >= emit_count[q]) return;
  const int32_t d = docs[slot] & 0x7fffffff;
  if ((uint32_t)d >= (uint32_t)max_doc) return;
  atomicOr(rows[q] + ((uint32_t)d >> 5), 1u << (d & 31));
}

struct DocsetCombineArgs {
  const uint64_t* all_of[DOCSET_MAX_OPERANDS];
  const uint64_t* none_of[DOCSET_MAX_OPERANDS];
  const uint64_t* live;   // nullable: AND the segment's live docs (the mask of a masked search)
  int32_t n_all, n_none;
  int32_t max_doc;
};

// out = AND all_of, AND NOT every none_of, AND (doc < max_doc) [AND live]; n_all = 0 starts from all ones. A lane handles two u64
// words with 16-byte loads and one 16-byte store; the last word of an odd count is handled alone with 8-byte accesses (the operands'
// allocations end with their last word). `out` may be one of the operands (element-wise). The result's bits are counted: popcount,
// wave reduction, one atomic add per workgroup into *cardinality (the caller zeroes it).
__global__ __launch_bounds__(DOCSET_THREADS) void k_docset_combine(DocsetCombineArgs a, uint64_t* out,  // (may alias an operand)
                                                                    unsigned long long* __restrict__ cardinality) {
  __shared__ int wave_counts[DOCSET_WAVES];
  const int64_t n_words = ((int64_t)a.max_doc + 63) >> 6;
  const int64_t w0 = 2 * ((int64_t)blockIdx.x * DOCSET_THREADS + threadIdx.x);
  int count = 0;
  if (w0 < n_words) {
    const bool pair = w0 + 1 < n_words;
    uint64_t x = ~0ull, y = ~0ull;
    auto load2 = [&](const uint64_t* p, uint64_t& u, uint64_t& v) {
      if (pair) { const ulonglong2 t = *reinterpret_cast<const ulonglong2*>(p + w0); u = t.x; v = t.y; }
      else { u = p[w0]; v = 0ull; }
    };
    for (int i = 0; i < a.n_all; ++i) { uint64_t u, v; load2(a.all_of[i], u, v); x &= u; y &= v; }
    for (int i = 0; i < a.n_none; ++i) { uint64_t u, v; load2(a.none_of[i], u, v); x &= ~u; y &= ~v; }
    if (a.live != nullptr) { uint64_t u, v; load2(a.live, u, v); x &= u; y &= v; }
    // the bits at and past max_doc of the last word
    const int tail = a.max_doc & 63;
    const uint64_t tail_mask = tail == 0 ? ~0ull : ((1ull << tail) - 1ull);
    if (w0 == n_words - 1) x &= tail_mask;
    if (!pair) y = 0ull;
    else if (w0 + 1 == n_words - 1) y &= tail_mask;
    if (pair) { ulonglong2 t; t.x = x; t.y = y; *reinterpret_cast<ulonglong2*>(out + w0) = t; }
    else out[w0] = x;
    count = __popcll(x) + __popcll(y);
  }
  const int wsum = wave_reduce_add(count);
  if (lane_id() == 0) wave_counts[wave_id()] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int i = 0; i < DOCSET_WAVES; ++i) total += wave_counts[i];
    if (total != 0) atomicAdd(cardinality, (unsigned long long)total);
  }
}

// ---- a doc set as the only required clause (rgpu_docset_head, rgpu_search_batch_required_set) -------------------------------------
// The head of M = live AND set: |M| and its first n docs, ascending. Three launches over the mask's words, no atomics:
//   k_docset_chunk_counts  popcount per chunk of DOCSET_HEAD_CHUNK_WORDS u64 words, one workgroup per chunk
//   k_docset_head_scan     exclusive prefix of the chunk counts and their total; one wavefront (a 2^31-doc leaf has 16384 chunks)
//   k_docset_select_head   every chunk whose prefix is below n writes its docs of rank < n to head[rank]
// The mask's allocation ends on a 16-byte boundary and its padding word is zero (docset_new / docset_mask_locked), so a pair
// load of the last word of an odd count stays inside it.
constexpr int DOCSET_HEAD_CHUNK_WORDS = 2048;  // = RGPU_DOCSET_HEAD_CHUNK_WORDS (include/rucene_gpu.h): 131072 docs per chunk

__global__ __launch_bounds__(DOCSET_THREADS) void k_docset_chunk_counts(const uint64_t* __restrict__ words, int64_t n_words,
                                                                         int* __restrict__ counts) {
  __shared__ int wave_counts[DOCSET_WAVES];
  const int64_t c0 = (int64_t)blockIdx.x * DOCSET_HEAD_CHUNK_WORDS;
  const int64_t c1 = c0 + DOCSET_HEAD_CHUNK_WORDS < n_words ? c0 + DOCSET_HEAD_CHUNK_WORDS : n_words;
  int count = 0;
  for (int64_t w = c0 + 2 * (int64_t)threadIdx.x; w < c1; w += 2 * DOCSET_THREADS) {  // (c0 is even: w + 1 is the pair's second word or the padding)
    const uint4 t = *reinterpret_cast<const uint4*>(words + w);
    count += __popc(t.x) + __popc(t.y) + __popc(t.z) + __popc(t.w);
  }
  const int wsum = wave_reduce_add(count);
  if (lane_id() == 0) wave_counts[wave_id()] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int i = 0; i < DOCSET_WAVES; ++i) total += wave_counts[i];
    counts[blockIdx.x] = total;
  }
}

// prefix[c] = docs of M in the chunks before c; *total = |M|. Launched as ONE wavefront.
__global__ __launch_bounds__(64) void k_docset_head_scan(const int* __restrict__ counts, int n_chunks, long long* __restrict__ prefix,
                                                         long long* __restrict__ total) {
  const int lane = lane_id();
  long long carry = 0;
  for (int base = 0; base < n_chunks; base += 64) {
    const int c = base + lane;
    const int v = c < n_chunks ? counts[c] : 0;
    const int incl = wave_incl_scan(v);  // (64 chunks hold at most 2^23 docs)
    if (c < n_chunks) prefix[c] = carry + (long long)(incl - v);
    carry += (long long)readlane(incl, 63);
  }
  if (lane == 0) *total = carry;
}

// One workgroup per chunk; a chunk at or past rank n has nothing to write. A step takes DOCSET_THREADS words, one per lane: the
// word's popcount, an inclusive scan inside the wavefront, the wavefronts' totals through LDS — the rank of the lane's first doc —
// and the lane peels its word's bits while rank < n. head holds n slots.
__global__ __launch_bounds__(DOCSET_THREADS) void k_docset_select_head(const uint64_t* __restrict__ words, int64_t n_words,
                                                                        const long long* __restrict__ prefix, int n,
                                                                        int32_t* __restrict__ head) {
  __shared__ int wave_totals[2][DOCSET_WAVES];
  long long rank_base = prefix[blockIdx.x];
  if (rank_base >= (long long)n) return;  // (uniform in the workgroup)
  const int lane = lane_id(), wave = wave_id();
  const int64_t c0 = (int64_t)blockIdx.x * DOCSET_HEAD_CHUNK_WORDS;
  const int64_t c1 = c0 + DOCSET_HEAD_CHUNK_WORDS < n_words ? c0 + DOCSET_HEAD_CHUNK_WORDS : n_words;
  int buf = 0;
  for (int64_t w0 = c0; w0 < c1 && rank_base < (long long)n; w0 += DOCSET_THREADS, buf ^= 1) {
    const int64_t w = w0 + threadIdx.x;
    uint64_t x = w < c1 ? words[w] : 0ull;
    const int cnt = __popcll(x);
    const int incl = wave_incl_scan(cnt);
    if (lane == 63) wave_totals[buf][wave] = incl;
    __syncthreads();  // (two buffers: a wavefront a step ahead writes the other one)
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < DOCSET_WAVES; ++i) { const int t = wave_totals[buf][i]; all += t; if (i < wave) before += t; }
    long long rank = rank_base + (long long)(before + incl - cnt);
    while (x != 0ull && rank < (long long)n) {
      head[rank] = (int32_t)((w << 6) + __builtin_ctzll(x));
      x &= x - 1ull;
      ++rank;
    }
    rank_base += (long long)all;
  }
}

// Rows of "SHOULD clauses beside a required doc set": the masked disjunction has left query q's scored docs (the docs of O, best
// first, {-1, 0} behind them) in its row; every doc of M matches, the unscored ones at +0.0 in doc order. One wavefront per query.
// A full row stands (every scored doc's score is > 0: the host refuses other weights). Otherwise all n_q docs of O are in the row
// and the first k docs of M hold at least k - n_q docs outside O: the scored docs are looked up in the ascending head (binary
// search) and flagged in LDS, the unflagged head docs are appended in order from slot n_q on. total_hits = |M| for every row.
constexpr int REQUIRED_SET_FILL_WAVES = 4;
constexpr int REQUIRED_SET_MAX_HEAD = 1024;  // = RGPU_MAX_K

__global__ __launch_bounds__(64 * REQUIRED_SET_FILL_WAVES) void k_required_set_fill(HitOut* __restrict__ hits, int64_t* __restrict__ totals,
                                                                                     int n_queries, int k, const int32_t* __restrict__ head,
                                                                                     int head_len, int64_t cardinality, int32_t doc_base) {
  __shared__ uint32_t flags[REQUIRED_SET_FILL_WAVES][REQUIRED_SET_MAX_HEAD / 32];
  const int lane = lane_id(), wave = wave_id();
  const int q = (int)blockIdx.x * REQUIRED_SET_FILL_WAVES + wave;
  if (q >= n_queries) return;
  if (lane == 0) totals[q] = cardinality;
  HitOut* row = hits + (int64_t)q * k;
  if (row[k - 1].doc >= 0) return;  // k scored docs: the row stands
  const int hn = head_len < k ? head_len : k;  // (head_len <= REQUIRED_SET_MAX_HEAD)
  uint32_t* fl = flags[wave];
  if (lane < REQUIRED_SET_MAX_HEAD / 32) fl[lane] = 0u;
  wave_sync();
  int n_q = 0;
  for (int base = 0; base < k; base += 64) {
    const int i = base + lane;
    const int32_t doc = i < k ? row[i].doc : -1;
    const bool valid = doc >= 0;
    if (valid) {
      const int32_t d = doc - doc_base;
      int lo = 0, hi = hn;  // first slot whose doc is >= d
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (head[mid] < d) lo = mid + 1; else hi = mid; }
      if (lo < hn && head[lo] == d) atomicOr(&fl[lo >> 5], 1u << (lo & 31));
    }
    const uint64_t m = __ballot(valid);
    n_q += __popcll(m);
    if (m != ~0ull) break;  // (scored docs are a prefix of the row)
  }
  wave_sync();
  int out = n_q;
  for (int base = 0; base < hn && out < k; base += 64) {
    const int p = base + lane;
    const bool keep = p < hn && ((fl[p >> 5] >> (p & 31)) & 1u) == 0u;
    const uint64_t m = __ballot(keep);
    const int slot = out + mbcnt(m);
    if (keep && slot < k) row[slot] = HitOut{head[p] + doc_base, 0.0f};
    out += __popcll(m);
  }
  for (int i = (out < k ? out : k) + lane; i < k; i += 64) row[i] = HitOut{-1, 0.0f};
}

}  // namespace rgpu
