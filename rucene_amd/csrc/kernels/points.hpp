// Point ranges: the docs of ONE segment that hold a one-dimensional point inside a closed range, as a doc set. GPU counterpart of
// PointRangeQuery's scorer (search/query/point_range_query.rs:503-561: every point of the field is visited, visit_by_packed_value
// :626-640 keeps a doc when lower <= value <= upper in unsigned byte order; live docs are not consulted). The sortable bytes of a
// value (IntPoint::encode_dimension etc.) are held as an unsigned key loaded big-endian, so one unsigned compare IS the byte compare.
//   k_points_scan<K, DENSE>   one pass over the keys in doc order answers up to POINTS_SCAN_RANGES ranges of a call
// (the value-ordered scatter of narrow ranges is k_docset_from_docs over a slice of the docs in value order: kernels/docset.hpp).
// A streaming kernel: its bound is the bytes of the column, n_points * sizeof(K) (+ 4 per point when the field is not dense), read
// once per pass with 16-byte loads per lane, however many ranges ride on the pass.
#pragma once
#include "docset.hpp"
#include "types.hpp"
#include "wave.hpp"

namespace rgpu {

constexpr int POINTS_SCAN_RANGES = 16;      // ranges one launch of k_points_scan answers (more: passes, host side)
constexpr int POINTS_SCAN_MAX_BLOCKS = 2048;  // workgroups of a launch; a wavefront strides over the chunks beyond

template <typename K>
struct PointsScanArgs {
  K lower[POINTS_SCAN_RANGES];              // lower <= key <= lower + span; the host sends no empty range (lower > upper)
  K span[POINTS_SCAN_RANGES];
  uint32_t* rows[POINTS_SCAN_RANGES];       // the sets' words as u32
  int32_t n_ranges;
  int32_t max_doc;
  int64_t n_points;
};

// bit i of x -> bit i * PER (PER = 4: the low 8 bits; PER = 2: the low 16 bits)
template <int PER>
__device__ __forceinline__ uint32_t points_spread(uint32_t x) {
  if (PER == 4) {
    x = (x | (x << 12)) & 0x000f000fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
  } else {
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
  }
  return x;
}

// A lane holds PER = 16 / sizeof(K) consecutive points (one 16-byte load), a wavefront a chunk of 64 * PER. `keys` (and `docs`) are
// allocated to whole chunks, so every load is inside its allocation whatever n_points is.
//
// DENSE (point i belongs to doc i, n_points == max_doc): the chunk is 64 * PER consecutive docs = 2 * PER whole 32-bit words of a
// set. Per range the compare of a lane's j-th key is a ballot b_j (bit l: doc PER * l + j of the chunk); lane w < 2 * PER cuts the
// 32 / PER lanes of word w out of every b_j, spreads them to every PER-th bit and stores the word. Every 32-bit word of every set,
// the upper half of the last u64 word included, has exactly ONE writer: plain stores, no atomics, nothing zeroed beforehand; bits at
// and past max_doc (the zero padding of the keys may lie inside a range) are masked.
//
// Not DENSE (`docs` ascend, not strictly: a sparse or multi-valued field): a lane's points touch up to PER words. Its first and its
// last word go through docset_wave_masks with the bits of the points inside the range — a point outside keeps its word and carries
// no bit, so a word's run over the lanes stays contiguous; a word strictly between them belongs to this lane alone (every other
// lane's words are <= the first or >= the last) and is written by the lane itself. The sets are zeroed beforehand.
template <typename K, bool DENSE>
__global__ __launch_bounds__(DOCSET_THREADS) void k_points_scan(const K* __restrict__ keys, const int32_t* __restrict__ docs, PointsScanArgs<K> a) {
  constexpr int PER = 16 / (int)sizeof(K);
  constexpr int CHUNK = 64 * PER;
  static_assert(PER == 4 || PER == 2, "keys of 4 or 8 bytes");
  struct alignas(16) KeyVec { K k[PER]; };
  struct alignas(4 * PER) DocVec { int32_t d[PER]; };
  const int lane = lane_id();
  const int64_t n_chunks = DENSE ? ((((int64_t)a.max_doc + 63) >> 6) * 64 + CHUNK - 1) / CHUNK : (a.n_points + CHUNK - 1) / CHUNK;
  const int64_t n_waves = (int64_t)gridDim.x * DOCSET_WAVES;
  for (int64_t c = (int64_t)blockIdx.x * DOCSET_WAVES + wave_id(); c < n_chunks; c += n_waves) {
    const int64_t p0 = c * CHUNK + (int64_t)lane * PER;
    const KeyVec kv = *reinterpret_cast<const KeyVec*>(keys + p0);
    if (DENSE) {
      constexpr int LPW = 32 / PER;                                  // lanes per 32-bit word
      const int64_t w32 = c * (2 * PER) + lane;                      // the word lane < 2 * PER stores
      const int64_t n_w32 = (((int64_t)a.max_doc + 63) >> 6) * 2;
      const int64_t first_doc = w32 * 32;
      const uint32_t keep = first_doc + 32 <= a.max_doc ? 0xffffffffu : (first_doc >= a.max_doc ? 0u : (1u << (uint32_t)(a.max_doc - first_doc)) - 1u);
      const bool writer = lane < 2 * PER && w32 < n_w32;
      for (int r = 0; r < a.n_ranges; ++r) {
        const K lo = a.lower[r], span = a.span[r];
        uint32_t word = 0u;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const uint64_t b = __ballot((K)(kv.k[j] - lo) <= span);
          const uint32_t mine = (uint32_t)(b >> ((LPW * lane) & 63)) & ((1u << LPW) - 1u);
          word |= points_spread<PER>(mine) << j;
        }
        if (writer) a.rows[r][w32] = word & keep;
      }
    } else {
      const DocVec dv = *reinterpret_cast<const DocVec*>(docs + p0);
      uint32_t w[PER], bit[PER];
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const bool have = p0 + j < a.n_points;
        w[j] = have ? (uint32_t)dv.d[j] >> 5 : (j == 0 ? DOCSET_NO_WORD : w[j - 1]);   // past the end: the word before, no bit
        bit[j] = have ? 1u << (dv.d[j] & 31) : 0u;
      }
      const uint32_t wa = w[0], wb = w[PER - 1];
      for (int r = 0; r < a.n_ranges; ++r) {
        const K lo = a.lower[r], span = a.span[r];
        uint32_t m[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) m[j] = (K)(kv.k[j] - lo) <= span ? bit[j] : 0u;
        uint32_t ma = 0u, mb = 0u;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          if (w[j] == wa) ma |= m[j];
          if (w[j] == wb) mb |= m[j];
        }
        if (PER == 4) {   // the words strictly between the first and the last: this lane's alone
          const bool mid1 = w[1] != wa && w[1] != wb, mid2 = w[2] != wa && w[2] != wb;
          const uint32_t m1 = m[1] | (w[2] == w[1] ? m[2] : 0u);
          if (mid1 && m1 != 0u) atomicOr(a.rows[r] + w[1], m1);
          if (mid2 && w[2] != w[1] && m[2] != 0u) atomicOr(a.rows[r] + w[2], m[2]);
        }
        docset_wave_masks(a.rows[r], wa, ma, wb, mb, lane);
      }
    }
  }
}

}  // namespace rgpu
