// BooleanQuery of required and optional clauses with exact PhraseQuery clauses on either side (rgpu_search_phrase_opt_batch):
// +a +b "a b", +"a b" c, +"a b" +c "b c" d -n #f. The stages in front of the kernels here leave, per query, one doc-ascending
// {doc, req} run for the required side (the phrase-bool stages: candidate conjunction, match planes, k_phrase_bool_score, then the
// order-independent run builder k_phrase_run_* of search_phrase_or.hpp) and one doc-ascending {doc, score} run per optional clause
// that exists in the leaf (k_score_terms for a term, the run builder for a phrase). Every run is closed by OR_RUN_PAD sentinel entries
// {INT_MAX, 0}; the slots of a phrase run behind its matches hold the sentinel too (k_phrase_run_fill).
//   k_phrase_opt_seed  a required side of term clauses alone has no phrase plane to say which candidates are alive: its plane 0 gets
//                      make_key(0.0f, doc) for every live candidate, so that k_phrase_bool_score runs over it as over a phrase's keys
//                      (the seeded score is never read: the query's order[] names term clauses only);
//   k_req_opt_join     required run x optional runs -> the SeqRec{doc, req, opt} stream k_req_opt_scan (search_and.hpp) walks.
#pragma once
#include "search_phrase_bool.hpp"
#include "search_phrase_or.hpp"

namespace rgpu {

// One wavefront per 64-slot group of plane 0 (plane 0's slots are the first emit_prefix[n_queries] of the launch). seeded[q] != 0:
// query q's required side names no phrase. Bounds: group < n_groups = emit_prefix[n_queries] / 64; q < n_queries; a lane reads
// emit_docs[slot] and writes keys[slot] only below its query's candidate count, slot < emit_prefix[q + 1].
__global__ __launch_bounds__(WG_THREADS) void k_phrase_opt_seed(const int32_t* __restrict__ seeded, const int64_t* __restrict__ emit_prefix,
                                                                const unsigned long long* __restrict__ emit_count,
                                                                const int32_t* __restrict__ emit_docs, int n_queries, int64_t n_groups,
                                                                uint64_t* __restrict__ keys) {
  const int lane = lane_id();
  const int64_t group = (int64_t)blockIdx.x * WG_WAVES + wave_id();
  if (group >= n_groups) return;
  const int q = upper_slot_wave(emit_prefix, n_queries, group * 64, lane);
  if (seeded[q] == 0) return;
  const int64_t slot = group * 64 + lane;
  const int64_t idx = slot - emit_prefix[q];
  if ((unsigned long long)idx >= emit_count[q]) return;
  const int32_t doc = emit_docs[slot];  // (a deleted candidate keeps its sign bit: it gets no key and never reaches the run)
  keys[slot] = doc >= 0 ? make_key(0.0f, doc) : 0ull;
}

// One query as k_req_opt_join reads it: its required run and its optional runs (n_opt entries at first_opt of the launch's opt_runs
// array, in clause order). A run is named by its index into run_prefix / run_len.
struct ReqOptJoinDev {
  int32_t req_run;
  int32_t first_opt;
  int32_t n_opt;   // 0..9
  int32_t add_all; // rgpu_config.req_opt_rule = -1: the record carries req + opt as its required score and 0.0 as its optional one
};

// First index in [0, n) whose doc is >= target (n when there is none), searched by the whole wavefront: 64 probes per step.
// Bounds: every probe index is < hi <= n. `target` is wave-uniform.
__device__ __forceinline__ int64_t run_lower_bound_wave(const ScoredPosting* __restrict__ run, int64_t n, int32_t target, int lane) {
  int64_t lo = 0, hi = n;
  while (hi > lo) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t at = lo + (int64_t)lane * step;
    const bool less = at < hi && run[at].doc < target;  // true on a prefix of the lanes (the run ascends)
    const int p = __popcll(__ballot(less));
    if (p == 0) { hi = lo; break; }
    const int64_t new_hi = min(hi, lo + (int64_t)p * step);  // (probe p, where there is one, is >= target)
    lo = lo + (int64_t)(p - 1) * step + 1;
    hi = new_hi;
  }
  return lo;
}

// One wavefront per 64 consecutive records of a query's required run, one record per lane. The wavefront first narrows every optional
// run of the query to the range that can hold its 64 docs - one lane-parallel lower bound at the group's first doc and one at its
// last - then each lane looks its own doc up in the narrowed ranges in clause order and forms opt = 0.0f + s_i ... in f32 (the library
// is built with -ffp-contract=off; an add is an add). The record goes to the required entry's own index; a sentinel entry
// (doc == INT_MAX: behind the run's matches) leaves doc = -1, which k_req_opt_scan passes over.
// Bounds: group < n_groups = seq_prefix[n_queries] / 64; q < n_queries; i = group * 64 + lane - seq_prefix[q] < round_up_64(capacity)
// <= capacity + 63 < capacity + OR_RUN_PAD, the required run's length, so run[i] is inside the run and seq[seq_prefix[q] + i] inside the
// query's records; an optional run is read at indexes < run_len[r] only (run_lower_bound_wave's probes are < n = run_len[r]; a
// lane's own search stays inside [lo, hi) with hi <= run_len[r]); opt_runs indexes first_opt + c with c < n_opt.
__global__ __launch_bounds__(WG_THREADS) void k_req_opt_join(const ReqOptJoinDev* __restrict__ jq, const int32_t* __restrict__ opt_runs,
                                                             const int64_t* __restrict__ run_prefix, const int32_t* __restrict__ run_len,
                                                             const ScoredPosting* __restrict__ runs, const int64_t* __restrict__ seq_prefix,
                                                             int n_queries, int64_t n_groups, SeqRec* __restrict__ seq) {
  const int lane = lane_id();
  const int64_t group = (int64_t)blockIdx.x * WG_WAVES + wave_id();
  if (group >= n_groups) return;
  const int q = upper_slot_wave(seq_prefix, n_queries, group * 64, lane);
  const ReqOptJoinDev Q = jq[q];
  const int64_t i = group * 64 + lane - seq_prefix[q];
  const ScoredPosting mine = runs[run_prefix[Q.req_run] + i];
  const bool valid = mine.doc != 0x7fffffff;
  const uint64_t vm = __ballot(valid);  // a prefix of the lanes: the run ascends and its sentinels stand behind the matches
  float opt = 0.0f;
  if (vm != 0ull) {
    const int32_t first = readlane(mine.doc, (int)__builtin_ctzll(vm));
    const int32_t last = readlane(mine.doc, 63 - (int)__builtin_clzll(vm));
    for (int c = 0; c < Q.n_opt; ++c) {  // wave-uniform
      const int r = opt_runs[Q.first_opt + c];
      const ScoredPosting* run = runs + run_prefix[r];
      const int64_t n = (int64_t)run_len[r];
      int64_t lo = run_lower_bound_wave(run, n, first, lane);
      int64_t hi = run_lower_bound_wave(run, n, last, lane);
      if (hi < n) ++hi;  // (the entry at the bound may be `last` itself)
      if (valid) {
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (run[mid].doc < mine.doc) lo = mid + 1; else hi = mid;
        }
        // lo <= the narrowed range's end <= n: an entry is read only when it exists
        if (lo < n) {
          const ScoredPosting e = run[lo];
          if (e.doc == mine.doc) opt = opt + e.score;
        }
      }
    }
  }
  SeqRec rec;
  rec.doc = valid ? mine.doc : -1;
  rec.req = Q.add_all ? mine.score + opt : mine.score;
  rec.opt = Q.add_all ? 0.0f : opt;
  rec.pad = 0;
  seq[seq_prefix[q] + i] = rec;
}

}  // namespace rgpu
