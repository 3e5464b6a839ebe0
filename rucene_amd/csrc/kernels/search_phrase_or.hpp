// BooleanQuery whose clauses are all SHOULD / MUST_NOT with exact PhraseQuery clauses among the SHOULD ones
// (rgpu_search_phrase_or_batch): "a b" "c d" e -f. Inside a DisjunctionSumScorer an ExactPhraseScorer is a plain iterator over its
// matching docs that scores BM25(phrase freq, norm) (phrase_scorer.rs:245-294), so a phrase clause can ride through the clause-order
// disjunction (search_or.hpp) as one more {doc, score} run. The phrase match stage (search_phrase.hpp) has left one
// make_key(score, doc) or 0 per candidate slot of every "virtual query" v = (query, phrase); the kernels here turn v's keys into
// that clause's run inside the OR launch's run buffer: the matching docs ascending, then {INT_MAX, 0} up to capacity + OR_RUN_PAD.
//
// The candidates arrive in whatever order the conjunction's wavefronts appended them (search_and.hpp: an atomic cursor per query),
// so the run is built by a method whose OUTPUT does not depend on arrival order — docs of one clause are distinct:
//   k_phrase_run_fill      every slot of every phrase run <- the sentinel (the matches overwrite a prefix of it);
//   k_phrase_run_place<0>  count the matches per (clause, bucket of PHRASE_OR_BUCKET docs);
//   k_phrase_run_scan      one wavefront per clause: exclusive scan of its bucket counts -> each bucket's first slot in the run;
//   k_phrase_run_place<1>  scatter {doc, score} into the bucket's slots (order inside a bucket: arrival order — not kept);
//   k_phrase_run_sort      one wavefront per (clause, 64 buckets), bucket by non-empty bucket: every score to doc - bucket_base in
//                          wave-private LDS with an occupancy bitmap, then the bucket is written back over its own slots in doc
//                          order by ballot / popcount rank.
// One code path whatever the sizes. A match that scores 0.0 (a boost-0 phrase) is a match: its key is non-zero (the low word is
// ~doc) and the bitmap, not the score, says which docs are there. Deleted candidates never get a key (the exact match kernels do
// not check a doc whose sign bit the conjunction set); a key whose doc lies outside [0, max_doc) is dropped all the same.
//
// How the runs reach k_or_windows unchanged: a phrase clause is a pseudo DevTerm with df = capacity, nblocks = 0, tail_n = 0 and no
// flags — the window kernel takes the run's length from df, binary-searches [0, df) and reads 64 entries from its cursor, so every
// slot up to capacity + OR_RUN_PAD holds a doc (sentinels ascend trivially). The host gives a pseudo term NO k_score_terms item
// (search_or_group's plan): that kernel never sees it, so neither its sentinel store nor its df == 1 singleton branch can write a
// bogus posting, and a capacity of 1 needs no special case. The runs are filled between k_score_terms and the window kernel.
#pragma once
#include "search_or.hpp"

namespace rgpu {

constexpr int PHRASE_OR_BUCKET = 1024;  // docs per bucket (a power of two <= 4096): 4 KB of scores + 128 B of bits per wavefront
static_assert((PHRASE_OR_BUCKET & (PHRASE_OR_BUCKET - 1)) == 0 && PHRASE_OR_BUCKET >= 64 && PHRASE_OR_BUCKET <= 4096, "bucket size");
constexpr int PHRASE_OR_FILL_SPLIT = 16;  // workgroups that share one clause's sentinel fill

// One phrase clause = one virtual query of the match stage. Virtual query v's buckets are [v * n_buckets, (v + 1) * n_buckets).
struct PhraseRunDev {
  int32_t term;      // index of the clause's pseudo DevTerm in the OR launch's term array (run_prefix[term] = the run's first slot)
  int32_t capacity;  // slots for matches: the phrase's cost (0: the clause does not exist in this leaf — no run, no slots)
};

// Bounds: v < n_virtual (grid.x); i < capacity + OR_RUN_PAD, the length search_or_group's run plan gave the pseudo term.
__global__ __launch_bounds__(WG_THREADS) void k_phrase_run_fill(const PhraseRunDev* __restrict__ pr, const int64_t* __restrict__ run_prefix,
                                                                ScoredPosting* __restrict__ runs) {
  const PhraseRunDev R = pr[blockIdx.x];
  if (R.capacity <= 0) return;
  ScoredPosting* run = runs + run_prefix[R.term];
  const int64_t n = (int64_t)R.capacity + OR_RUN_PAD;
  for (int64_t i = (int64_t)blockIdx.y * WG_THREADS + threadIdx.x; i < n; i += (int64_t)PHRASE_OR_FILL_SPLIT * WG_THREADS)
    run[i] = ScoredPosting{0x7fffffff, 0.0f};
}

// One wavefront per 64-slot group of the match stage's candidate slots (a group belongs to one virtual query), one slot per lane.
// SCATTER = false: counts[v * n_buckets + doc / B] += 1 per match. SCATTER = true (after the scan, which zeroed the counts again):
// the match goes to the bucket's next free slot, counts[] is the cursor and ends at the bucket's count once more.
// Bounds: group < n_groups = emit_prefix[n_virtual] / 64; a lane reads keys[slot] only below its query's candidate count; bucket
// < n_buckets because doc < max_doc is checked; a scatter lands at offsets[bucket] + cursor < the clause's match count <= its
// candidate count <= capacity (the conjunction is led by the phrase's rarest term) — checked again before the store.
template <bool SCATTER>
__global__ __launch_bounds__(WG_THREADS) void k_phrase_run_place(const PhraseRunDev* __restrict__ pr, const int64_t* __restrict__ emit_prefix,
                                                                 const unsigned long long* __restrict__ emit_count, const uint64_t* __restrict__ keys,
                                                                 int n_virtual, int64_t n_groups, int32_t max_doc, int n_buckets,
                                                                 uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                                 const int64_t* __restrict__ run_prefix, ScoredPosting* __restrict__ runs) {
  const int lane = lane_id();
  const int64_t group = (int64_t)blockIdx.x * WG_WAVES + wave_id();
  if (group >= n_groups) return;
  const int v = upper_slot_wave(emit_prefix, n_virtual, group * 64, lane);
  const int64_t idx = group * 64 + lane - emit_prefix[v];
  const int64_t cnt = (int64_t)emit_count[v];
  if (idx - lane >= cnt) return;  // nothing in these 64 slots
  const uint64_t key = idx < cnt ? keys[group * 64 + lane] : 0ull;
  const int32_t doc = key_doc(key);
  if (key == 0ull || (uint32_t)doc >= (uint32_t)max_doc) return;  // no match (or a doc no segment holds)
  const PhraseRunDev R = pr[v];
  const int64_t b = (int64_t)v * n_buckets + doc / PHRASE_OR_BUCKET;
  if (!SCATTER) {
    atomicAdd(&counts[b], 1u);
  } else {
    const int64_t at = (int64_t)offsets[b] + (int64_t)atomicAdd(&counts[b], 1u);
    if (at < (int64_t)R.capacity) runs[run_prefix[R.term] + at] = ScoredPosting{doc, key_score(key)};
  }
}

// One wavefront per virtual query: offsets[b] = matches in the buckets before b (64 buckets per step, a DPP scan), counts[b] <- 0.
// Bounds: v < n_virtual; bucket indexes v * n_buckets + i with i < n_buckets.
__global__ __launch_bounds__(WG_THREADS) void k_phrase_run_scan(int n_virtual, int n_buckets, uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets) {
  const int lane = lane_id();
  const int v = blockIdx.x * WG_WAVES + wave_id();
  if (v >= n_virtual) return;
  uint32_t* cn = counts + (int64_t)v * n_buckets;
  uint32_t* of = offsets + (int64_t)v * n_buckets;
  int running = 0;
  for (int i0 = 0; i0 < n_buckets; i0 += 64) {  // uniform trip count: the scan is a wave-wide operation
    const int i = i0 + lane;
    const int n = i < n_buckets ? (int)cn[i] : 0;
    const int incl = wave_incl_scan(n);
    if (i < n_buckets) { of[i] = (uint32_t)(running + incl - n); cn[i] = 0u; }
    running += readlane(incl, 63);
  }
}

// One wavefront per (virtual query, group of 64 buckets): lane i reads bucket i's count, and the wavefront goes through the
// non-empty buckets of its group one after the other (at 10 M docs a clause has ~10 k buckets, nearly all of them empty: one
// wavefront per bucket spent the launch starting wavefronts that left at once — 1.13 ms for a 1024-query batch against 0.20). A bucket's n scattered entries go through
// wave-private LDS — score at doc - bucket_base, one occupancy bit per doc — and come back over the same n slots in doc order: 64
// docs per step, a lane's rank among the occupied docs of its step from the ballot (mbcnt), the steps' popcounts added up. Nothing
// is shared between wavefronts; the order inside the wavefront is wave_sync's (LDS operations of a wave complete in issue order).
// Bounds: w < n_virtual * groups_per_clause; bucket < n_buckets (lanes past it hold a count of 0); the bucket's slots are
// [offsets[cell], offsets[cell] + n) of the clause's run, below its capacity (k_phrase_run_place stored nothing beyond it) — n is cut
// to the slots that lie below it; LDS indexes o = doc - bucket_base are checked against PHRASE_OR_BUCKET; at most n bits are set, so
// at most n entries are written back.
__global__ __launch_bounds__(WG_THREADS) void k_phrase_run_sort(const PhraseRunDev* __restrict__ pr, int64_t n_items, int n_buckets,
                                                                int groups_per_clause, const uint32_t* __restrict__ counts,
                                                                const uint32_t* __restrict__ offsets, const int64_t* __restrict__ run_prefix,
                                                                ScoredPosting* __restrict__ runs) {
  __shared__ float scores[WG_WAVES][PHRASE_OR_BUCKET];
  __shared__ uint32_t bitmaps[WG_WAVES][PHRASE_OR_BUCKET / 32];
  const int lane = lane_id();
  const int wave = wave_id();
  const int64_t w = (int64_t)blockIdx.x * WG_WAVES + wave;
  if (w >= n_items) return;
  const int v = (int)(w / groups_per_clause);
  const int bucket0 = (int)(w % groups_per_clause) * 64;
  const int64_t cell0 = (int64_t)v * n_buckets + bucket0;
  const int my_count = bucket0 + lane < n_buckets ? (int)counts[cell0 + lane] : 0;
  uint64_t todo = __ballot(my_count > 0);
  if (todo == 0ull) return;
  const PhraseRunDev R = pr[v];
  float* sc = scores[wave];
  uint32_t* bits = bitmaps[wave];
  ScoredPosting* clause_run = runs + run_prefix[R.term];
  while (todo != 0ull) {  // wave-uniform
    const int s = (int)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    const int32_t base = (bucket0 + s) * PHRASE_OR_BUCKET;
    const int64_t first = (int64_t)offsets[cell0 + s];
    const int n = (int)min((int64_t)readlane(my_count, s), max((int64_t)0, (int64_t)R.capacity - first));
    if (n <= 0) continue;
    ScoredPosting* run = clause_run + first;
    if (lane < PHRASE_OR_BUCKET / 32) bits[lane] = 0u;
    wave_sync();
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      if (i < n) {
        const ScoredPosting e = run[i];
        const uint32_t o = (uint32_t)(e.doc - base);
        if (o < (uint32_t)PHRASE_OR_BUCKET) {  // (docs of one clause are distinct: no two lanes meet in one cell)
          sc[o] = e.score;
          atomicOr(&bits[o >> 5], 1u << (o & 31u));
        }
      }
    }
    wave_sync();  // every entry has been read (its score sits in LDS) before the first slot is written again
    int written = 0;
    for (int step = 0; step < PHRASE_OR_BUCKET / 64; ++step) {
      const uint32_t o = (uint32_t)(step * 64 + lane);
      const bool has = ((bits[o >> 5] >> (o & 31u)) & 1u) != 0u;
      const uint64_t m = __ballot(has);
      if (m == 0ull) continue;  // wave-uniform
      if (has) run[written + mbcnt(m)] = ScoredPosting{base + (int32_t)o, sc[o]};
      written += __popcll(m);
    }
    wave_sync();  // the bitmap and the scores are free for the next bucket
  }
}

}  // namespace rgpu
