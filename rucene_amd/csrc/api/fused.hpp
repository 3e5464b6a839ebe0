// Plan + search in one call. HostLaps, TermHot; the single-term step with its descriptors resident on the device
// (term_batch_resident) and staged per call (term_batch_fast); search_uniform_locked (declared in sharded.hpp); uniform_args_ok. Entry
// points: rgpu_planner_search_uniform_ids_device, rgpu_planner_search_uniform_ids_sharded.
// Uses: rgpu_api.hip itself (the arena, scratch slots, stage_h2d, k_stage_term_plan / TermPlanLayout, RGPU_LAUNCH_WITH_STOP, stat_slot_once,
// HostClock, launch_merge, term_item_blocks, term_query_item_blocks, term_item_shift, fill_term_item_desc, search_impl), sharded.hpp
// (rgpu_comm, UniformBatch, ShardedCall, sharded_*), planner.hpp (rgpu_planner, plan_uniform).
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- plan + search in ONE call ------------------------------------------------------------------------------------------------
// A serving host's steady state is "a batch of term ids arrives -> rows": rgpu_plan_uniform_ids writes rgpu_query[] /
// rgpu_query_term[] (40 B a clause), rgpu_search_batch_device reads them back, validates them as foreign input, looks every
// clause's prepared structures up, sorts the queries into groups and only then builds the device descriptors — 63 us of one
// host thread per 1024-query TERM batch against 47 us of GPU time (round 5). The fused form keeps the ids inside the library:
// for single-term batches the planner's per-clause result (term state, idf) and the prepared-term table entry go straight
// into the staged DevQuery / DevTerm arrays — one pass, no intermediate arrays, nothing to validate (the planner's own
// tables are trusted; an id outside them is an absent term) — and the zeroed per-query counters travel with the same staged
// copy (three enqueues per batch: copy, k_search_term, k_merge_items). Anything the fast pass does not handle — another op,
// a term that is not prepared yet or lacks its block-max sketch, k > 128, a prepared-term budget, a dictionary planner — goes
// through plan() + search_impl() inside the same call: same rows either way (tests/test_gpu_parity.py).
// RGPU_HOST_TIME=1 in the environment: where the calling thread's time goes inside term_batch_fast, averaged over 256 calls (stderr)
struct HostLaps {
  static constexpr int N = 7;
  long long ns[N] = {0, 0, 0, 0, 0, 0, 0};
  int calls = 0;
  std::chrono::steady_clock::time_point last;
  void start() { last = std::chrono::steady_clock::now(); }
  void lap(int i) { const auto t = std::chrono::steady_clock::now(); ns[i] += std::chrono::duration_cast<std::chrono::nanoseconds>(t - last).count(); last = t; }
  void done() {
    if (++calls < 256) return;
    std::fprintf(stderr, "[term_batch_fast host, us per call] slot + stage room %.2f | term states -> descriptors %.2f | items %.2f | item descriptors + zeroes %.2f | "
                         "stage copy enqueue %.2f | reserve + kernel enqueue %.2f | status + mark %.2f\n",
                 ns[0] / 256e3, ns[1] / 256e3, ns[2] / 256e3, ns[3] / 256e3, ns[4] / 256e3, ns[5] / 256e3, ns[6] / 256e3);
    *this = HostLaps{};
  }
};
// what term_batch_resident's memo pass needs of a DevTerm besides its arena index: the digest of the planner's hot entry
// (host/batch_planner.hpp for_each_flat_memo_hot). bucket: clz(nblocks), 32 for a list without FullBlocks
struct TermHot { int32_t df, nblocks, bucket; };
// The fused single-term step with the term descriptors RESIDENT on the device (the default; RGPU_TERM_PLAN=staged: the staged plan
// below). What a step sends is 8 bytes per query — TermLaunch{record, row} in launch order, which k_search_term_query reads straight
// from the pinned stage — and nothing is copied: no stage kernel, no DevQuery / DevTerm / order / qmap arrays. The descriptors live in
// the context's arena (host/term_arena.hpp has the ownership rules), written once each:
//   * a memo miss appends the record to the current generation and to this call's stage; the call then runs k_stage_term_plan — the
//     stage copy, with the arena as its destination — on ITS stream ahead of its search kernel, and records an event behind it;
//   * a call on another stream that names records of an upload not known complete makes its stream wait for that event
//     (hipStreamWaitEvent) before its search kernel. Uploads become known complete when a slot marked behind them on their stream
//     is waited for, which scratch_take does anyway: a steady state makes no event call for the arena;
//   * nothing in a generation is ever overwritten, and a generation's buffer is handed back only when no busy scratch slot carries
//     its number — so a launch in flight on either stream reads what its plan named, whatever the memo does meanwhile.
// *staged: the call is not for this path after all (more distinct terms than the arena holds): the caller stages the plan.
template <class Make>
static int32_t term_batch_resident(rgpu_segment* seg, rucene::BatchPlanner* P, int32_t nq, const int64_t* ids, int32_t k, HitOut* hits_dev,
                                   int64_t* totals_dev, hipStream_t stream, const rucene::BatchPlanner::MemoKey& memo_key, Make& make_term,
                                   HostLaps* laps, bool* taken, bool* staged) {
  rgpu_ctx* c = seg->ctx;
  rucene::TermArena& A = c->arena;
  *staged = false;
  if (A.begin(rucene::TermArena::Key{{memo_key.w[0], memo_key.w[1], memo_key.w[2], memo_key.w[3]}})) HIP_TRY(arena_new_buffer(c));
  Stager st(c);
  const size_t o_l = st.add((size_t)nq * sizeof(TermLaunch));
  const size_t o_up = st.add((size_t)nq * sizeof(DevTerm));  // records this call places (at most one per query)
  HIP_TRY(c->S->h_stage.reserve(st.used));
  HIP_TRY(c->S->d_stage.reserve((size_t)nq * 16, 0, stream));  // the launch's counters: the kernel stores every one of them
  if (laps) laps->lap(0);
  TermLaunch* hl = reinterpret_cast<TermLaunch*>(c->S->h_stage.p + o_l);
  DevTerm* hup = reinterpret_cast<DevTerm*>(c->S->h_stage.p + o_up);
  static thread_local std::vector<int32_t> recs;
  static thread_local std::vector<uint8_t> buckets;
  recs.resize((size_t)nq);
  buckets.resize((size_t)nq);
  int64_t postings = 0, total_blocks = 0, loose = 0;
  int32_t start[34];
  int32_t n_up = 0;
  int64_t first_up = -1;
  uint32_t lo = 0xffffffffu, hi = 0u;
  // records placed by a pass whose upload is never enqueued (a term the fast pass does not take, a failed call) must not be named by
  // a later call: the generation ends with them
  struct Unplace {
    rucene::TermArena& A;
    const int32_t& n_up;
    bool armed = true;
    ~Unplace() { if (armed && n_up > 0) A.turn_over(); }
  } unplace{A, n_up};
  for (int attempt = 0;; ++attempt) {
    postings = total_blocks = loose = 0;
    std::memset(start, 0, sizeof start);
    n_up = 0;
    first_up = -1;
    lo = 0xffffffffu;
    hi = 0u;
    bool full = false;
    auto place = [&](const DevTerm* t) -> int64_t {
      const int64_t at = A.append();
      if (at < 0) { full = true; return -1; }
      if (first_up < 0) first_up = at;  // (appends of one pass are consecutive: the context's lock is held)
      hup[n_up++] = *t;
      return at;
    };
    // the memo pass counts the launch order's buckets (0: the longest lists; floor(log2(nblocks))) on the way. What it needs of a term —
    // its record's index, df, nblocks, the bucket — comes from the planner's hot entry (one cache line per query; RGPU_TERM_HOT=0: from
    // the memo's record, as before)
    const bool ok = c->term_hot ? P->for_each_flat_memo_hot<DevTerm, TermHot>(ids, nq, memo_key, A.generation(), make_term, place, [](const DevTerm& t) {
      return TermHot{t.df, t.nblocks, t.nblocks > 0 ? __builtin_clz((uint32_t)t.nblocks) : 32};
    }, [&](int64_t q, int32_t rec, const TermHot& t) {
      int b = 32;
      if (rec >= 0) {
        postings += t.df;
        total_blocks += t.nblocks;
        loose += t.df == 1 ? 1 : t.df % 128;  // (make_term's tail_n)
        b = t.bucket;
        lo = std::min(lo, (uint32_t)rec);
        hi = std::max(hi, (uint32_t)rec);
      }
      recs[(size_t)q] = rec;
      buckets[(size_t)q] = (uint8_t)b;
      ++start[b + 1];
    }) : P->for_each_flat_memo_placed<DevTerm>(ids, nq, memo_key, A.generation(), make_term, place, [&](int64_t q, const DevTerm* t, int32_t rec) {
      int b = 32;
      if (t) {
        postings += t->df;
        total_blocks += t->nblocks;
        loose += t->df == 1 ? 1 : t->tail_n;
        if (t->nblocks > 0) b = __builtin_clz((uint32_t)t->nblocks);
        lo = std::min(lo, (uint32_t)rec);
        hi = std::max(hi, (uint32_t)rec);
      }
      recs[(size_t)q] = rec;
      buckets[(size_t)q] = (uint8_t)b;
      ++start[b + 1];
    });
    if (ok) break;
    if (!full) return RGPU_OK;  // (the full path takes the call; the slot was taken and not marked: it is simply free again)
    // the generation is full: a fresh one, and the pass again (every entry misses). A batch that does not fit an empty arena is staged.
    n_up = 0;
    A.turn_over();
    if (attempt == 1) { *staged = true; return RGPU_OK; }
    HIP_TRY(arena_new_buffer(c));
  }
  if (laps) laps->lap(1);
  for (int b = 0; b < 33; ++b) start[b + 1] += start[b];
  for (int q = 0; q < nq; ++q) hl[start[buckets[(size_t)q]]++] = TermLaunch{recs[(size_t)q], q};
  if (laps) { laps->lap(2); laps->lap(3); }
  const DevTerm* d_arena = static_cast<const DevTerm*>(A.buffer());
  if (n_up > 0) {
    {
      // k_stage_term_plan's second job: the new records, from the stage to their place in the arena (no zero range, no item descriptors)
      TimedLaunch tl(c, stream, "k_stage_term_plan", 0);
      const size_t n16 = (size_t)n_up * (sizeof(DevTerm) / 16);
      const TermPlanLayout L{0u, 0u, 0u, 0u, 0u, 0u, 0};
      const unsigned grid = (unsigned)std::min<size_t>(1024, (n16 + 255) / 256);
      RGPU_LAUNCH(k_stage_term_plan, dim3(grid), dim3(256), 0, stream, c->S->h_stage.p + o_up,
                  reinterpret_cast<uint8_t*>(const_cast<DevTerm*>(d_arena + first_up)), n16, L);
    }
    HIP_TRY(launch_status());
    void* ev = A.take_spare_event();
    if (!ev) {
      hipEvent_t e = nullptr;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      ev = e;
    }
    const hipError_t er = hipEventRecord((hipEvent_t)ev, stream);
    if (er != hipSuccess) { A.give_spare_event(ev); HIP_TRY(er); }
    A.note_upload((uint32_t)first_up, (uint32_t)(first_up + n_up), (uint64_t)(uintptr_t)stream, ev);
  }
  unplace.armed = false;  // (what this pass placed is on its way)
  if (A.pending_uploads() != 0 && lo <= hi) {
    hipError_t ew = hipSuccess;
    A.for_each_wait((uint64_t)(uintptr_t)stream, lo, hi, [&](void* ev) {
      const hipError_t e = hipStreamWaitEvent(stream, (hipEvent_t)ev, 0);
      if (ew == hipSuccess) ew = e;
    });
    HIP_TRY(ew);
  }
  if (laps) laps->lap(4);
  unsigned long long* d_work = reinterpret_cast<unsigned long long*>(c->S->d_stage.p);
  c->last_counted = c->S;
  c->last_counted_words = d_work;
  c->last_counted_op = RGPU_OP_TERM;
  c->last_counted_queries = nq;
  c->last_counted_postings = postings;
  c->last_counted_dir_blocks = total_blocks;
  c->last_counted_loose = loose;
  const bool wide = k > 64;
  const bool legacy = seg->version < 1;
  // the slot's mark travels with the step's only launch: `done` is the kernel's stop event, and no hipEventRecord follows it
  const bool bound = c->term_slot_event_bound;
  if (bound && !c->S->done) HIP_TRY(hipEventCreateWithFlags(&c->S->done, hipEventDisableTiming));
  {
    TimedLaunch tl(c, stream, stat_slot_once(c, &c->stat_k_search_term, "k_search_term"), postings);  // (under the TERM search's name, like the staged plan's launch below)
    const SegView sv = seg_view(seg);
    auto go = [&](auto kern, int waves) -> hipError_t {
      // (hipExtLaunchKernelGGL passes the arguments as they are typed here: each one has its parameter's type exactly)
      if (bound) RGPU_LAUNCH_WITH_STOP(kern, dim3((unsigned)nq), dim3(64 * waves), 0, stream, c->S->done, sv, (const DevQuery*)nullptr, d_arena, (const int32_t*)nullptr,
                                       (int)nq, (int)k, d_work, (const int32_t*)nullptr, hits_dev, totals_dev, (int32_t)seg->doc_base, (const TermLaunch*)hl,
                                       (int)c->term_short_blocks);
      else RGPU_LAUNCH(kern, dim3((unsigned)nq), dim3(64 * waves), 0, stream, sv, (const DevQuery*)nullptr, d_arena, (const int32_t*)nullptr, nq, (int)k, d_work,
                       (const int32_t*)nullptr, hits_dev, totals_dev, seg->doc_base, (const TermLaunch*)hl, c->term_short_blocks);
      return hipSuccess;
    };
    auto pick = [&](auto legacy_c, auto wide_c) -> hipError_t {
      constexpr bool LG = decltype(legacy_c)::value, WD = decltype(wide_c)::value;
      if (c->term_query_waves == 2) return go(k_search_term_query<LG, WD, 2>, 2);
      if (c->term_query_waves == 8) return go(k_search_term_query<LG, WD, 8>, 8);
      return go(k_search_term_query<LG, WD, 4>, 4);
    };
    hipError_t e;
    if (legacy) e = wide ? pick(std::true_type{}, std::true_type{}) : pick(std::true_type{}, std::false_type{});
    else e = wide ? pick(std::false_type{}, std::true_type{}) : pick(std::false_type{}, std::false_type{});
    HIP_TRY(e);
    c->stats[(size_t)stat_slot_once(c, &c->stat_term_query_launches, "term_query_launches")].launches += 1;
  }
  if (laps) laps->lap(5);
  HIP_TRY(launch_status());  // (a refused launch: the slot stays unmarked, `busy` false)
  if (bound) c->S->busy = true;
  else HIP_TRY(scratch_mark(c, stream));
  A.slot_marked((int)(c->S - c->scr), (uint64_t)(uintptr_t)stream);
  c->stats[(size_t)stat_slot_once(c, &c->stat_fused_term_batches, "fused_term_batches")].launches += 1;
  if (laps) { laps->lap(6); laps->done(); }
  *taken = true;
  return RGPU_OK;
}
static int32_t term_batch_fast(rgpu_segment* seg, rucene::BatchPlanner* P, int32_t nq, const int64_t* ids, int32_t k, HitOut* hits_dev,
                               int64_t* totals_dev, hipStream_t stream, bool* taken) {
  rgpu_ctx* c = seg->ctx;
  *taken = false;
  static thread_local HostLaps laps;
  const bool timed = c->host_time;
  if (timed) laps.start();
  const int32_t sim_table = P->sim_table();
  if (!P->flat() || k > RGPU_PASS_K || c->prepared_budget != 0 || sim_table < 0 || sim_table >= c->n_sim_tables || seg->dir_used == 0) return RGPU_OK;
  const bool want_sketch = c->term_sketches && seg->d_norms && seg->n_norm_ranks > 0 && !live_words(seg);
  const bool need_norms = seg->d_norms != nullptr;
  const uint32_t flags = c->sim_monotone[(size_t)sim_table] ? TERM_FLAG_MONOTONE : 0u;
  c->pass = rgpu_ctx::Pass{};
  SCRATCH_TAKE(c);
  const int32_t max_doc = seg->max_doc;
  const bool has_freqs = seg->has_freqs;
  // term id -> finished descriptor through the planner's memo (host/batch_planner.hpp for_each_flat_memo): a descriptor is a function
  // of the planner's tables (immutable), the segment and what its prepared store holds (uid, epoch), and the flags below
  const rucene::BatchPlanner::MemoKey memo_key{{seg->uid, seg->prepared.epoch, (uint64_t)(uint32_t)sim_table | ((uint64_t)flags << 32),
                                                (uint64_t)want_sketch | ((uint64_t)need_norms << 1) | ((uint64_t)has_freqs << 2) | ((uint64_t)(uint32_t)max_doc << 8)}};
  auto make_term = [&](const rgpu_term_state& s0, float idf, DevTerm* out) -> int32_t {
    DevTerm t;
    t.start_fp = (uint64_t)std::max<int64_t>(0, s0.doc_start_fp);
    t.pn_base = 0;
    t.bs_base = 0;
    t.dir_base = 0;
    t.nblocks = 0;
    t.df = s0.doc_freq;
    t.tail_n = s0.doc_freq > 1 ? s0.doc_freq % 128 : 0;
    t.singleton_doc = s0.singleton_doc_id;
    t.singleton_freq = has_freqs ? (int32_t)s0.total_term_freq : 1;
    t.weight = idf;
    t.sim_table = sim_table;
    t.flags = flags;
    t.sketch = 0;
    if (s0.doc_freq == 1) {
      if (s0.singleton_doc_id < 0 || s0.singleton_doc_id >= max_doc) return -1;  // (the full path names the error)
    } else {
      const TermInfo* info = seg->prepared.find(s0.doc_start_fp);
      if (!info || info->df != s0.doc_freq || (need_norms && !info->norms) ||
          (want_sketch && info->sketch == 0 && info->nblocks >= TERM_SKETCH_MIN_BLOCKS)) return -1;  // (the full path prepares it: another epoch)
      t.dir_base = info->dir_base;
      t.nblocks = info->nblocks;
      t.pn_base = info->pn_base;
      t.bs_base = info->bs_base;
      t.sketch = info->sketch;
    }
    *out = t;
    return 1;
  };
  // k_search_term_query: one workgroup per query, no work items
  const bool per_query = c->term_query_kernel && c->blocks_per_item_auto && c->term_fold;
  if (per_query && c->term_plan_resident && c->stage_by_kernel && !c->upload_aside) {
    bool staged_after_all = false;
    const int32_t rc = term_batch_resident(seg, P, nq, ids, k, hits_dev, totals_dev, stream, memo_key, make_term, timed ? &laps : nullptr, taken, &staged_after_all);
    if (!staged_after_all) return rc;
  }
  Stager st(c);
  const size_t o_q = st.add((size_t)nq * sizeof(DevQuery));
  const size_t o_t = st.add((size_t)nq * sizeof(DevTerm));
  const size_t o_p = st.add((size_t)(nq + 1) * 8);
  const size_t o_m = st.add((size_t)nq * 4);
  const size_t o_sh = st.add((size_t)nq);            // log2 of every query's own item size (0: the launch's)
  const size_t o_ord = st.add((size_t)nq * 4);       // k_search_term_query: the query of every workgroup, heaviest first
  const size_t o_tau = st.add((size_t)nq * 8);       // per-query shared thresholds ...
  const size_t o_w = st.add((size_t)nq * 16);        // ... and the launch's counters: zeroed by the copy that brings the plan
  const size_t o_done = st.add((size_t)nq * 4);      // ... and the per-query counts of finished items (TermMerge::done)
  const size_t o_zero_end = st.add(0);               // (the three above are one range: [o_tau, o_zero_end))
  // ... and the item descriptors, LAST: their number is known only once the terms have been read (at most 262144 + nq, the item
  // loop's cap), the stage has room for the worst case and the copy takes what is used
  const size_t o_id = st.add(((size_t)262144 + (size_t)nq) * sizeof(int4));
  HIP_TRY(c->S->h_stage.reserve(st.used));
  HIP_TRY(c->S->d_stage.reserve(st.used, 0, stream));
  if (timed) laps.lap(0);
  DevQuery* hq = reinterpret_cast<DevQuery*>(c->S->h_stage.p + o_q);
  DevTerm* ht = reinterpret_cast<DevTerm*>(c->S->h_stage.p + o_t);
  int64_t* hp = reinterpret_cast<int64_t*>(c->S->h_stage.p + o_p);
  int32_t* hm = reinterpret_cast<int32_t*>(c->S->h_stage.p + o_m);
  int32_t nt = 0;
  int64_t postings = 0, total_blocks = 0, loose = 0;
  bool bail = false;
  bail = !P->for_each_flat_memo<DevTerm>(ids, nq, memo_key, make_term, [&](int64_t q, const DevTerm* t) {
    hm[q] = (int32_t)q;
    if (!t) { hq[q] = DevQuery{RGPU_OP_TERM, 0, nt, 0}; return; }  // TermWeight::create_scorer -> None for this leaf
    hq[q] = DevQuery{RGPU_OP_TERM, 1, nt, 0};
    ht[nt++] = *t;
    postings += t->df;
    total_blocks += t->nblocks;
    loose += t->df == 1 ? 1 : t->tail_n;
  });
  if (bail) return RGPU_OK;  // (the slot was taken and not marked: it is simply free again)
  if (timed) laps.lap(1);
  // k_search_term_query — the plan is the queries, their terms and a launch order, longest lists first (a counting sort on
  // floor(log2(nblocks)))
  if (per_query) {
    int32_t* ho = reinterpret_cast<int32_t*>(c->S->h_stage.p + o_ord);
    int32_t start[34] = {0};
    auto bucket = [&](int q) -> int {  // 0: the longest lists
      const int32_t nb = hq[q].n_terms >= 1 ? ht[hq[q].first_term].nblocks : 0;
      return nb <= 0 ? 32 : __builtin_clz((uint32_t)nb);
    };
    for (int q = 0; q < nq; ++q) ++start[bucket(q) + 1];
    for (int b = 0; b < 33; ++b) start[b + 1] += start[b];
    for (int q = 0; q < nq; ++q) ho[start[bucket(q)]++] = q;
  }
  // items: chunks of a term's blocks; every query's first chunk is scheduled first (search_pass's rule, to the letter)
  int blocks_per_item = c->cfg.blocks_per_item;
  int term_split = 1;
  if (c->blocks_per_item_auto) {
    blocks_per_item = term_item_blocks(total_blocks, c->term_target_items);
    term_split = c->term_split;
  }
  int64_t items = 0;
  uint8_t* hsh = c->S->h_stage.p + o_sh;
  while (!per_query) {
    items = 0;
    const int base_sh = term_item_shift(blocks_per_item);  // 0: not a power of two (a caller's own size) — no per-query sizes then
    const int floor_sh = std::max(1, term_item_shift(c->term_min_item_blocks));
    for (int q = 0; q < nq; ++q) {
      hp[q] = items;
      hsh[q] = 0;
      if (hq[q].n_terms >= 1) {
        const int32_t nb = ht[hq[q].first_term].nblocks;
        if (base_sh > 0) {  // term_query_item_blocks in shifts: halve while the query has fewer than `split` items
          int sh = base_sh;
          if (term_split > 1) while (sh > floor_sh && ((nb + (1 << sh) - 1) >> sh) < term_split) --sh;
          hsh[q] = (uint8_t)sh;
          items += (nb == 0 ? 1 : (nb + (1 << sh) - 1) >> sh) - 1;
        } else {
          items += (nb == 0 ? 1 : (nb + blocks_per_item - 1) / blocks_per_item) - 1;
        }
      }
    }
    hp[nq] = items;
    if (items <= 262144 || blocks_per_item >= (1 << 17)) break;
    blocks_per_item *= 2;
  }
  if (!per_query) items += nq;
  if (timed) laps.lap(2);
  if (items > 262144 + (int64_t)nq) return RGPU_OK;  // (blocks_per_item hit its ceiling on an absurd batch: the full path takes it)
  const bool plan_on_device = c->stage_by_kernel && !c->upload_aside && o_id + (size_t)items * sizeof(int4) <= 0xffffffffull;
  if (plan_on_device) {
    // zeroes and item descriptors are the copy kernel's work (k_stage_term_plan)
    if (timed) laps.lap(3);
    const size_t n16 = (o_id + 15) / 16;  // (o_id is 256-aligned: everything in front of the descriptors)
    const TermPlanLayout L{(uint32_t)o_q, (uint32_t)o_p, (uint32_t)o_sh, (uint32_t)o_id, (uint32_t)o_tau, (uint32_t)o_zero_end, per_query ? 0 : nq};
    TimedLaunch tl(c, stream, "k_stage_term_plan", 0);
    const unsigned grid = (unsigned)std::min<size_t>(1024, std::max<size_t>((n16 + 255) / 256, per_query ? 0 : ((size_t)nq + 255) / 256));
    RGPU_LAUNCH(k_stage_term_plan, dim3(grid), dim3(256), 0, stream, c->S->h_stage.p, c->S->d_stage.p, n16, L);
  } else {
    std::memset(c->S->h_stage.p + o_tau, 0, o_zero_end - o_tau);
    int4* hd = reinterpret_cast<int4*>(c->S->h_stage.p + o_id);
    for (int q = 0; q < (per_query ? 0 : nq); ++q) {  // fill_term_item_desc with the sizes the item loop chose
      const int n_mine = 1 + (int)(hp[q + 1] - hp[q]);
      const int ft = hq[q].n_terms >= 1 ? hq[q].first_term : -1;
      const int w = n_mine | ((int)hsh[q] << 24);
      hd[q] = make_int4(q, 0, ft, w);
      int4* rest = hd + nq + hp[q];
      for (int ch = 1; ch < n_mine; ++ch) rest[ch - 1] = make_int4(q, ch, ft, w);
    }
    const size_t staged = o_id + (size_t)items * sizeof(int4);
    if (timed) laps.lap(3);
    HIP_TRY(stage_h2d(c, staged, stream));
  }
  if (timed) laps.lap(4);
  if (!per_query) {
    HIP_TRY(c->S->d_partial_keys.reserve((size_t)items * (size_t)k, 0, stream));
    HIP_TRY(c->S->d_partial_counts.reserve((size_t)items, 0, stream));
  }
  unsigned long long* d_tau = reinterpret_cast<unsigned long long*>(c->S->d_stage.p + o_tau);
  unsigned long long* d_work = reinterpret_cast<unsigned long long*>(c->S->d_stage.p + o_w);
  const DevQuery* dq = reinterpret_cast<const DevQuery*>(c->S->d_stage.p + o_q);
  const DevTerm* dt = reinterpret_cast<const DevTerm*>(c->S->d_stage.p + o_t);
  const int64_t* dp = reinterpret_cast<const int64_t*>(c->S->d_stage.p + o_p);
  const int32_t* dm = reinterpret_cast<const int32_t*>(c->S->d_stage.p + o_m);
  c->last_counted = c->S;
  c->last_counted_words = d_work;
  c->last_counted_op = RGPU_OP_TERM;
  c->last_counted_queries = nq;
  c->last_counted_postings = postings;
  c->last_counted_dir_blocks = total_blocks;
  c->last_counted_loose = loose;
  const bool wide = k > 64;
  const bool legacy = seg->version < 1;
  // the fold of every query's item lists happens inside k_search_term (TermMerge), unless RGPU_TERM_FOLD=0 asks for k_merge_items
  const TermMerge fold = c->term_fold ? TermMerge{reinterpret_cast<unsigned int*>(c->S->d_stage.p + o_done), dp, hits_dev, totals_dev, nullptr, seg->doc_base, 0, 0}
                                      : TermMerge{};
  if (per_query) {
    // (timed under the TERM search's name: what reads the stats — bench.py's roofline among them — asks for "k_search_term"; the
    // term_query_launches stat below tells the two kernels apart)
    TimedLaunch tl(c, stream, "k_search_term", postings);
    const SegView sv = seg_view(seg);
    const int32_t* dord = reinterpret_cast<const int32_t*>(c->S->d_stage.p + o_ord);
    auto go = [&](auto kern, int waves) -> hipError_t {
      RGPU_LAUNCH(kern, dim3((unsigned)nq), dim3(64 * waves), 0, stream, sv, dq, dt, dord, nq, (int)k, d_work, dm, hits_dev, totals_dev, seg->doc_base,
                  (const TermLaunch*)nullptr, c->term_short_blocks);
      return hipSuccess;
    };
    auto pick = [&](auto legacy_c, auto wide_c) -> hipError_t {
      constexpr bool LG = decltype(legacy_c)::value, WD = decltype(wide_c)::value;
      if (c->term_query_waves == 2) return go(k_search_term_query<LG, WD, 2>, 2);
      if (c->term_query_waves == 8) return go(k_search_term_query<LG, WD, 8>, 8);
      return go(k_search_term_query<LG, WD, 4>, 4);
    };
    hipError_t e;
    if (legacy) e = wide ? pick(std::true_type{}, std::true_type{}) : pick(std::true_type{}, std::false_type{});
    else e = wide ? pick(std::false_type{}, std::true_type{}) : pick(std::false_type{}, std::false_type{});
    HIP_TRY(e);
    c->stats[(size_t)stat_slot(c, "term_query_launches")].launches += 1;
  } else {
    TimedLaunch tl(c, stream, "k_search_term", postings);
    const unsigned grid = wg_count((items + TERM_WAVES - 1) / TERM_WAVES);
    const size_t lds = term_lds_bytes(wide);
    const SegView sv = seg_view(seg);
    auto go = [&](auto kern) -> hipError_t {
      hipError_t e = set_dynamic_lds_once(c, reinterpret_cast<const void*>(kern), lds);
      if (e != hipSuccess) return e;
      RGPU_LAUNCH(kern, dim3(grid), dim3(TERM_THREADS), lds, stream, sv, dq, dt, reinterpret_cast<const int4*>(c->S->d_stage.p + o_id), nq, items,
                         blocks_per_item, (int)k, c->S->d_partial_keys.p, c->S->d_partial_counts.p, d_tau, d_work, (const unsigned long long*)nullptr, dm, fold);
      return hipSuccess;
    };
    hipError_t e;
    if (legacy) e = wide ? go(k_search_term<true, true>) : go(k_search_term<true, false>);
    else e = wide ? go(k_search_term<false, true>) : go(k_search_term<false, false>);
    HIP_TRY(e);
  }
  if (!per_query && !c->term_fold) {
    if (wide) launch_merge<true>(c, stream, nq, k, dp, seg->doc_base, hits_dev, totals_dev, nq, nullptr, nullptr, dm);
    else launch_merge<false>(c, stream, nq, k, dp, seg->doc_base, hits_dev, totals_dev, nq, nullptr, nullptr, dm);
  }
  if (timed) laps.lap(5);
  HIP_TRY(launch_status());
  HIP_TRY(scratch_mark(c, stream));
  c->stats[(size_t)stat_slot(c, "fused_term_batches")].launches += 1;  // (tests ask whether this path ran: rgpu_kernel_stats)
  if (timed) { laps.lap(6); laps.done(); }
  *taken = true;
  return RGPU_OK;
}

// context mutex held by the caller; c->defer_or as the caller set it
static int32_t search_uniform_locked(rgpu_segment* seg, const UniformBatch& ub, int32_t n_queries, int32_t k, HitOut* hits_dev, int64_t* totals_dev,
                                     hipStream_t stream) {
  const int32_t op = ub.op & 0xff;
  // BooleanQuery::build: a lone clause IS that clause (boolean_query.rs:56-68) — as plan() rewrites it
  if (ub.n_clauses == 1 && (ub.op >> 8) == 0 && op >= RGPU_OP_TERM && op <= RGPU_OP_OR) {
    bool taken = false;
    const int32_t rc = term_batch_fast(seg, ub.planner->p.get(), n_queries, ub.ids, k, hits_dev, totals_dev, stream, &taken);
    if (rc != RGPU_OK || taken) return rc;
  }
  thread_local std::vector<rgpu_query> queries;
  thread_local std::vector<rgpu_query_term> terms;
  queries.resize((size_t)n_queries);
  terms.resize((size_t)n_queries * (size_t)ub.n_clauses);
  const int32_t rc = plan_uniform(ub.planner, ub.op, n_queries, ub.n_clauses, ub.ids, nullptr, nullptr, queries.data(), terms.data());
  if (rc != RGPU_OK) return rc;
  return search_impl(seg, queries.data(), n_queries, terms.data(), (int32_t)terms.size(), k, hits_dev, totals_dev, stream);
}

static int32_t uniform_args_ok(rgpu_planner* p, rgpu_segment* seg, int32_t op, int32_t n_queries, int32_t n_clauses, const int64_t* ids, int32_t k,
                               const void* hits_dev, const void* totals_dev) {
  if (!p || !seg || !ids || !hits_dev || !totals_dev) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  if (n_queries <= 0 || n_clauses <= 0 || n_clauses > RGPU_MAX_QUERY_TERMS || (int64_t)n_queries * n_clauses > 0x7fffffff) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad batch shape");
  if ((op & 0xff) == RGPU_OP_DISMAX) return fail(RGPU_ERR_UNSUPPORTED, "the planner does not plan RGPU_OP_DISMAX: pack rgpu_query / rgpu_query_term and call rgpu_search_batch*");
  if ((op >> 16) != 0 || (op & 0xff) < RGPU_OP_TERM || (op & 0xff) > RGPU_OP_OR || ((op & 0xff) == RGPU_OP_TERM && n_clauses != 1))
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "a uniform batch is TERM (one clause), AND or OR (optionally RGPU_OP_OR_MSM)");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  if (!p->p->flat()) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "this planner names terms by their bytes (rgpu_planner_create): plan with rgpu_plan_uniform_bytes, then rgpu_search_batch_device");
  return RGPU_OK;
}

extern "C" int32_t rgpu_planner_search_uniform_ids_device(rgpu_planner* p, rgpu_segment* seg, int32_t op, int32_t n_queries, int32_t n_clauses,
                                                          const int64_t* term_ids, int32_t k, void* hits_dev, void* totals_dev, void* hip_stream) {
  const int32_t ok = uniform_args_ok(p, seg, op, n_queries, n_clauses, term_ids, k, hits_dev, totals_dev);
  if (ok != RGPU_OK) return ok;
  rgpu_ctx* c = seg->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const UniformBatch ub{p, op, n_clauses, term_ids};
  c->defer_or = c->cfg.or_deferred != 0;
  const int32_t rc = search_uniform_locked(seg, ub, n_queries, k, (HitOut*)hits_dev, (int64_t*)totals_dev, s);
  c->defer_or = false;
  return rc;
}

// ... and its sharded form: rgpu_search_batch_sharded with the batch named by ids (local plan + search -> all-gather -> merge)
extern "C" int32_t rgpu_planner_search_uniform_ids_sharded(rgpu_comm* comm, rgpu_planner* p, rgpu_segment* seg, int32_t op, int32_t n_queries,
                                                           int32_t n_clauses, const int64_t* term_ids, int32_t k, void* hits_dev, void* totals_dev,
                                                           void* hip_stream) {
  if (!comm) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  const int32_t ok = uniform_args_ok(p, seg, op, n_queries, n_clauses, term_ids, k, hits_dev, totals_dev);
  if (ok != RGPU_OK) return ok;
  if (seg->ctx != comm->ctx) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "segment and communicator belong to different contexts");
  rgpu_ctx* c = comm->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const UniformBatch ub{p, op, n_clauses, term_ids};
  ShardedCall call;
  int32_t rc = sharded_reserve(comm, n_queries, k, s, &call);
  if (rc != RGPU_OK) return rc;
  sharded_local(comm, seg, nullptr, n_queries, nullptr, 0, k, s, &call, false, &ub);
  rc = sharded_gather(comm, s, call);
  if (rc != RGPU_OK) return rc;
  rc = sharded_merge(comm, n_queries, k, hits_dev, totals_dev, s, call);
  if (rc != RGPU_OK) return rc;
  if (call.local_rc != RGPU_OK) return fail(call.local_rc, call.local_why);
  if (call.pre_rc != RGPU_OK) return fail(call.pre_rc, call.pre_why);
  return RGPU_OK;
}

