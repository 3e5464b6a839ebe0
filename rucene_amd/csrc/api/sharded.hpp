// Segment-sharded search: an RCCL all-gather of per-shard records and a device merge. CommSlot, rgpu_comm, NCCL_TRY; records
// (record_bytes, search_into_record, merge_records); one sharded call in steps (ShardedCall, sharded_reserve / _local / _settle / _gather /
// _merge). Entry points: rgpu_comm_unique_id, rgpu_comm_init, rgpu_comm_init_all, rgpu_comm_destroy, rgpu_record_bytes,
// rgpu_search_batch_record_device, rgpu_merge_records_device, rgpu_search_batch_sharded, rgpu_comm_reserve, rgpu_comm_gathers_issued,
// rgpu_search_batch_sharded_all, rgpu_comm_status.
// Uses from rgpu_api.hip itself: rgpu_ctx, rgpu_segment, DevVec, fail, HIP_TRY, RGPU_LAUNCH, TimedLaunch, settle_pending, search_impl.
// Wart: UniformBatch and the declaration of search_uniform_locked stand here, for search_into_record; fused.hpp defines the function.
// Not a stand-alone header: part of the one translation unit rgpu_api.hip, included there once and in this order.

// ---- segment-sharded search: RCCL all-gather of per-shard top-k + device merge -------------------------------------------
constexpr int N_COMM_SLOTS = 4;
struct CommSlot {
  // One record (record_bytes: hits, counts, status word) per rank. The all-gather is IN PLACE: this rank's search writes its
  // record straight into its own region, recv + rank * record (ncclAllGather with sendbuff == recvbuff + rank * count moves
  // nothing locally: no send buffer, no device copy of the rank's own record).
  DevVec<uint8_t> recv;
  size_t record = 0;           // the record size the status words below were prepared for
  bool status_zero = false;    // this rank's status word already reads RGPU_OK (zeroed with the buffer, never dirtied since): a
                               // successful search then needs no extra launch to say so
  hipEvent_t done = nullptr;
  bool busy = false;
};
struct rgpu_comm {
  rgpu_ctx* ctx = nullptr;
  ncclComm_t nccl = nullptr;
  int n_ranks = 1, rank = 0;
  CommSlot slots[N_COMM_SLOTS];
  int next = 0;
  // collectives of one communicator must not run side by side: when consecutive calls come on different streams, the
  // later all-gather waits for the earlier one (an event), while the searches in front of them still overlap
  hipStream_t last_stream = nullptr;
  hipEvent_t last_collective = nullptr;
  bool have_last = false;
  CommSlot* last_slot = nullptr;  // the most recent batch's records (rgpu_comm_status)
  int32_t last_queries = 0, last_k = 0;
  int64_t gathers_issued = 0;     // ncclAllGather calls enqueued on this communicator (rgpu_comm_gathers_issued)
};
#define NCCL_TRY(expr)                                                                                          \
  do {                                                                                                          \
    ncclResult_t _r = (expr);                                                                                   \
    if (_r != ncclSuccess) return fail(RGPU_ERR_RUNTIME, std::string(#expr) + ": " + ncclGetErrorString(_r)); \
  } while (0)
static_assert(RGPU_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "rgpu_comm ids are ncclUniqueIds");

extern "C" int32_t rgpu_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "id_out is null");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  std::memcpy(id_out, id.internal, RGPU_COMM_ID_BYTES);
  return RGPU_OK;
}

extern "C" int32_t rgpu_comm_init(rgpu_ctx* c, int32_t n_ranks, int32_t rank, const uint8_t* id_bytes, rgpu_comm** out) {
  if (!out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "out_comm is null");
  *out = nullptr;
  if (!c || !id_bytes) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "rank outside [0, n_ranks)");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId id;
  std::memcpy(id.internal, id_bytes, RGPU_COMM_ID_BYTES);
  auto comm = std::make_unique<rgpu_comm>();
  comm->ctx = c;
  comm->n_ranks = n_ranks;
  comm->rank = rank;
  NCCL_TRY(ncclCommInitRank(&comm->nccl, n_ranks, id, rank));
  *out = comm.release();
  return RGPU_OK;
}

// One process, one thread, n contexts (Rucene itself is one process: search_parallel hands leaves to threads,
// searcher.rs:527-630): ncclCommInitRank blocks until every rank of the id has joined, so n of them issued one after the
// other from one thread would never return — they have to sit inside one ncclGroupStart / ncclGroupEnd.
extern "C" int32_t rgpu_comm_init_all(rgpu_ctx* const* ctxs, int32_t n, rgpu_comm** out_comms) {
  if (!ctxs || !out_comms || n < 1) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  for (int32_t r = 0; r < n; ++r) {
    out_comms[r] = nullptr;
    if (!ctxs[r]) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null context");
    for (int32_t j = 0; j < r; ++j)
      if (ctxs[j] == ctxs[r] || ctxs[j]->device == ctxs[r]->device) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "every rank needs its own context on its own device");
  }
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  std::vector<std::unique_ptr<rgpu_comm>> comms;
  for (int32_t r = 0; r < n; ++r) {
    comms.emplace_back(new rgpu_comm());
    comms.back()->ctx = ctxs[r];
    comms.back()->n_ranks = n;
    comms.back()->rank = r;
  }
  ncclResult_t res = ncclGroupStart();
  for (int32_t r = 0; r < n && res == ncclSuccess; ++r) {
    if (hipSetDevice(ctxs[r]->device) != hipSuccess) { res = ncclUnhandledCudaError; break; }
    res = ncclCommInitRank(&comms[(size_t)r]->nccl, n, id, r);
  }
  const ncclResult_t end = ncclGroupEnd();
  if (res == ncclSuccess) res = end;
  if (res != ncclSuccess) {
    for (auto& cm : comms) if (cm->nccl) (void)ncclCommAbort(cm->nccl);
    return fail(RGPU_ERR_RUNTIME, std::string("ncclCommInitRank (grouped): ") + ncclGetErrorString(res));
  }
  for (int32_t r = 0; r < n; ++r) out_comms[r] = comms[(size_t)r].release();
  return RGPU_OK;
}

extern "C" void rgpu_comm_destroy(rgpu_comm* comm) {
  if (!comm) return;
  (void)hipSetDevice(comm->ctx->device);
  for (auto& sl : comm->slots) {
    if (sl.busy) (void)hipEventSynchronize(sl.done);
    if (sl.done) (void)hipEventDestroy(sl.done);
    sl.recv.release();
  }
  if (comm->last_collective) (void)hipEventDestroy(comm->last_collective);
  if (comm->nccl) (void)ncclCommDestroy(comm->nccl);
  delete comm;
}

// ---- a shard's record: what one rank contributes to the all-gather ---------------------------------------------------------
// [n_queries x k rgpu_hit][n_queries x int64 hit count][int64 status] — the status word is the rank's rgpu_status for the
// batch: a rank whose local search failed still takes part in the collective (with empty rows), so that the other ranks
// neither hang in the all-gather nor silently merge a stale record; every rank can read everybody's status afterwards.
static size_t record_hits_bytes(int32_t n_queries, int32_t k) { return (size_t)n_queries * (size_t)k * sizeof(HitOut); }
static size_t record_bytes(int32_t n_queries, int32_t k) { return record_hits_bytes(n_queries, k) + (size_t)n_queries * 8 + 8; }
extern "C" int64_t rgpu_record_bytes(int32_t n_queries, int32_t k) {
  if (n_queries <= 0 || k <= 0) return 0;
  return (int64_t)record_bytes(n_queries, k);
}

__global__ void k_set_i64(int64_t* p, int64_t v) { *p = v; }

// local search of one shard straight into a record (device memory, record_bytes long); enqueue-only. The call's own status
// is returned AND left in the record's status word; on failure the record holds empty rows.
// `status_zero` (in / out, may be null): the record's status word is known to hold RGPU_OK already — a successful search then
// leaves it alone (one launch less per batch on the serving path); a failure writes it and clears the flag.
// `defer`: >= 10-clause disjunctions leave their hand-back flags for settle_pending (the caller runs it before the record is
// read by anybody: before the collective) — the one-process form enqueues every shard's search before it waits for any.
// A uniform batch that is still to be planned (the fused plan + search entry points): n_queries x n_clauses flat-table ids
struct UniformBatch {
  rgpu_planner* planner;
  int32_t op, n_clauses;
  const int64_t* ids;
};
static int32_t search_uniform_locked(rgpu_segment* seg, const UniformBatch& ub, int32_t n_queries, int32_t k, HitOut* hits_dev, int64_t* totals_dev,
                                     hipStream_t stream);
static int32_t search_into_record(rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries, const rgpu_query_term* terms,
                                  int32_t n_terms_total, int32_t k, uint8_t* record, hipStream_t s, bool* status_zero = nullptr, bool defer = false,
                                  const UniformBatch* uniform = nullptr) {
  const size_t hits_bytes = record_hits_bytes(n_queries, k);
  seg->ctx->defer_or = defer;
  int32_t rc = uniform ? search_uniform_locked(seg, *uniform, n_queries, k, (HitOut*)record, (int64_t*)(record + hits_bytes), s)
                       : search_impl(seg, queries, n_queries, terms, n_terms_total, k, (HitOut*)record, (int64_t*)(record + hits_bytes), s);
  seg->ctx->defer_or = false;
  std::string why = rc == RGPU_OK ? std::string() : g_last_error;
  // No early return below: the status word is written whatever else fails (a peer that merged a record without one would
  // take stale rows for this shard's answer), and the first error is the one reported.
  auto note = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && rc == RGPU_OK) { rc = RGPU_ERR_RUNTIME; why = std::string(what) + ": " + hipGetErrorString(e); }
  };
  if (rc != RGPU_OK) {  // whatever was enqueued before the failure is overwritten behind it on the same stream
    note(hipMemsetAsync(record + hits_bytes, 0, (size_t)n_queries * 8, s), "hipMemsetAsync(record counts)");
    RGPU_LAUNCH(k_init_hits, dim3(wg_count(((size_t)n_queries * k + 255) / 256)), dim3(256), 0, s, (HitOut*)record, (int64_t)n_queries, (int)k, (int)k, 0);
    note(launch_status(), "k_init_hits");
  }
  if (rc == RGPU_OK && status_zero != nullptr && *status_zero) return RGPU_OK;  // the word says RGPU_OK already
  if (status_zero != nullptr) *status_zero = false;  // (set again by the caller once it has zeroed the word)
  RGPU_LAUNCH(k_set_i64, dim3(1), dim3(1), 0, s, (int64_t*)(record + hits_bytes + (size_t)n_queries * 8), (int64_t)rc);
  const hipError_t e_status = launch_status();
  if (e_status != hipSuccess) {  // the launch itself was refused: put the word there with a copy from the host instead
    const int64_t word = rc != RGPU_OK ? (int64_t)rc : (int64_t)RGPU_ERR_RUNTIME;
    (void)hipMemcpyAsync(record + hits_bytes + (size_t)n_queries * 8, &word, 8, hipMemcpyHostToDevice, s);
    (void)hipStreamSynchronize(s);  // (`word` lives on this frame)
    note(e_status, "k_set_i64");
  }
  if (rc != RGPU_OK) return fail(rc, why);
  return RGPU_OK;
}

extern "C" int32_t rgpu_search_batch_record_device(rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries,
                                                   const rgpu_query_term* terms, int32_t n_terms_total, int32_t k, void* record_dev,
                                                   void* hip_stream) {
  if (!seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !record_dev) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  std::lock_guard<std::mutex> g(seg->ctx->mu);
  HIP_TRY(hipSetDevice(seg->ctx->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : seg->ctx->stream;
  return search_into_record(seg, queries, n_queries, terms, n_terms_total, k, (uint8_t*)record_dev, s);
}

// the canonical k-way merge over `n_ranks` gathered records (k_merge_lists reading them in place, with the record stride)
static int32_t merge_records(rgpu_ctx* c, const uint8_t* records, int32_t n_ranks, int32_t n_queries, int32_t k, HitOut* hits_dev,
                             int64_t* totals_dev, hipStream_t s) {
  const size_t hits_bytes = record_hits_bytes(n_queries, k), record = record_bytes(n_queries, k);
  {
    TimedLaunch tl(c, s, "k_merge_lists", 0);
    const unsigned grid = wg_count((n_queries + WG_WAVES - 1) / WG_WAVES);
    auto go = [&](auto kern) {
      RGPU_LAUNCH(kern, dim3(grid), dim3(WG_THREADS), 0, s, (const HitOut*)records, (const int64_t*)(records + hits_bytes),
                         (int64_t)(record / sizeof(HitOut)), (int64_t)(record / 8), n_ranks, n_queries, (int)k, hits_dev, totals_dev);
    };
    if (k > 64) go(k_merge_lists<true>); else go(k_merge_lists<false>);
  }
  HIP_TRY(launch_status());
  return RGPU_OK;
}

extern "C" int32_t rgpu_merge_records_device(rgpu_ctx* c, const void* records_dev, int32_t n_ranks, int32_t n_queries, int32_t k,
                                             void* hits_out_dev, void* totals_out_dev, void* hip_stream) {
  if (!c || !records_dev || !hits_out_dev || !totals_out_dev || n_ranks <= 0 || n_queries <= 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return merge_records(c, (const uint8_t*)records_dev, n_ranks, n_queries, k, (HitOut*)hits_out_dev, (int64_t*)totals_out_dev,
                       hip_stream ? (hipStream_t)hip_stream : c->stream);
}

// ---- the three phases of a sharded batch (context mutex held by the caller) -------------------------------------------------
struct ShardedCall {
  CommSlot* sl = nullptr;
  size_t record = 0;
  int32_t local_rc = RGPU_OK;
  std::string local_why;
  int32_t pre_rc = RGPU_OK;  // a failure in front of the collective that did not keep this rank from joining it
  std::string pre_why;
};
// phase 0: the slot and its buffers. The ONE thing that can fail here and leave the communicator out of step with its peers
// is the allocation of the record buffer itself (nowhere to gather into): rgpu_comm_reserve does it at start-up, so a serving
// host never allocates on the data path. Everything else that goes wrong (a wait on the slot's previous batch, the status
// word's memset) is remembered in call->pre_rc and reported AFTER the collective has been joined.
static int32_t sharded_reserve(rgpu_comm* comm, int32_t n_queries, int32_t k, hipStream_t s, ShardedCall* call) {
  CommSlot& sl = comm->slots[comm->next];
  auto note = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && call->pre_rc == RGPU_OK) { call->pre_rc = RGPU_ERR_RUNTIME; call->pre_why = std::string(what) + ": " + hipGetErrorString(e); }
  };
  if (sl.busy) { note(hipEventSynchronize(sl.done), "hipEventSynchronize(slot)"); sl.busy = false; }
  const size_t record = record_bytes(n_queries, k);
  const uint8_t* before = sl.recv.p;
  HIP_TRY(sl.recv.reserve(record * (size_t)comm->n_ranks, 0, s));
  if (sl.recv.p != before || sl.record != record || !sl.status_zero) {
    // this rank's status word, zeroed once per (buffer, record size): a batch that succeeds never touches it again
    const hipError_t e = hipMemsetAsync(sl.recv.p + (size_t)comm->rank * record + record - 8, 0, 8, s);
    sl.record = record;
    sl.status_zero = e == hipSuccess;  // not zeroed: search_into_record writes the word with a launch instead
  }
  call->sl = &sl;
  call->record = record;
  return RGPU_OK;
}
// phase 1: from here on this rank WILL enqueue the collective, whatever its local search does (search_into_record leaves the
// status in the record)
static void sharded_local(rgpu_comm* comm, rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries, const rgpu_query_term* terms,
                          int32_t n_terms_total, int32_t k, hipStream_t s, ShardedCall* call, bool defer = false, const UniformBatch* uniform = nullptr) {
  comm->next = (comm->next + 1) % N_COMM_SLOTS;
  call->local_rc = search_into_record(seg, queries, n_queries, terms, n_terms_total, k, call->sl->recv.p + (size_t)comm->rank * call->record, s,
                                      &call->sl->status_zero, defer, uniform);
  if (call->local_rc != RGPU_OK) call->local_why = g_last_error;
}
// phase 1b (after a deferred sharded_local): whatever the shard's disjunctions still have to run again runs now, before the
// record is gathered; a failure becomes the shard's status like a failure of the search itself
static void sharded_settle(rgpu_comm* comm, int32_t n_queries, int32_t k, hipStream_t s, ShardedCall* call) {
  const int32_t rc = settle_pending(comm->ctx);
  if (rc == RGPU_OK || call->local_rc != RGPU_OK) return;
  call->local_rc = rc;
  call->local_why = g_last_error;
  uint8_t* record = call->sl->recv.p + (size_t)comm->rank * call->record;
  const size_t hits_bytes = record_hits_bytes(n_queries, k);
  call->sl->status_zero = false;
  (void)hipMemsetAsync(record + hits_bytes, 0, (size_t)n_queries * 8, s);
  RGPU_LAUNCH(k_init_hits, dim3(wg_count(((size_t)n_queries * k + 255) / 256)), dim3(256), 0, s, (HitOut*)record, (int64_t)n_queries, (int)k, (int)k, 0);
  RGPU_LAUNCH(k_set_i64, dim3(1), dim3(1), 0, s, (int64_t*)(record + hits_bytes + (size_t)n_queries * 8), (int64_t)rc);
  (void)launch_status();
}
static int32_t sharded_gather(rgpu_comm* comm, hipStream_t s, ShardedCall& call) {
  // A communicator of one rank has nothing to gather: its record is already where the merge reads it. (Before round 5 this
  // path cost a device copy of the record, a one-thread launch for the status word and an event wait between consecutive
  // batches on different streams: 0.157 ms per 1024-query TERM step against 0.093 for the local search.)
  // rgpu_config.comm_force_gather issues the in-place all-gather all the same: the N > 1 path on a one-GPU box.
  if (comm->n_ranks == 1 && comm->ctx->cfg.comm_force_gather == 0) return RGPU_OK;
  auto note = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && call.pre_rc == RGPU_OK) { call.pre_rc = RGPU_ERR_RUNTIME; call.pre_why = std::string(what) + ": " + hipGetErrorString(e); }
    return e;
  };
  // collectives of one communicator run one after the other; when the stream changed, the later one waits for the earlier
  // one's event. If that wait cannot be enqueued the host waits instead — this rank still joins the collective (its peers
  // are in it already): nothing between sharded_reserve and ncclAllGather returns
  if (comm->have_last && comm->last_stream != s)
    if (note(hipStreamWaitEvent(s, comm->last_collective, 0), "hipStreamWaitEvent(last collective)") != hipSuccess)
      (void)hipEventSynchronize(comm->last_collective);
  uint8_t* const mine = call.sl->recv.p + (size_t)comm->rank * call.record;  // in place: sendbuff == recvbuff + rank * count
  NCCL_TRY(ncclAllGather(mine, call.sl->recv.p, call.record, ncclInt8, comm->nccl, s));
  comm->gathers_issued++;
  if (!comm->last_collective) (void)note(hipEventCreateWithFlags(&comm->last_collective, hipEventDisableTiming), "hipEventCreate(last collective)");
  if (comm->last_collective && note(hipEventRecord(comm->last_collective, s), "hipEventRecord(last collective)") == hipSuccess) {
    comm->last_stream = s;
    comm->have_last = true;
  } else {  // no event to order the next collective behind this one: the host waits for this one now
    (void)hipStreamSynchronize(s);
    comm->have_last = false;
  }
  return RGPU_OK;
}
static int32_t sharded_merge(rgpu_comm* comm, int32_t n_queries, int32_t k, void* hits_dev, void* totals_dev, hipStream_t s, const ShardedCall& call) {
  int32_t rc = merge_records(comm->ctx, call.sl->recv.p, comm->n_ranks, n_queries, k, (HitOut*)hits_dev, (int64_t*)totals_dev, s);
  if (rc != RGPU_OK) return rc;
  if (!call.sl->done) HIP_TRY(hipEventCreateWithFlags(&call.sl->done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(call.sl->done, s));
  call.sl->busy = true;
  comm->last_slot = call.sl;
  comm->last_queries = n_queries;
  comm->last_k = k;
  return RGPU_OK;
}

extern "C" int32_t rgpu_search_batch_sharded(rgpu_comm* comm, rgpu_segment* seg, const rgpu_query* queries, int32_t n_queries,
                                             const rgpu_query_term* terms, int32_t n_terms_total, int32_t k, void* hits_dev,
                                             void* totals_dev, void* hip_stream) {
  if (!comm || !seg || !queries || n_queries <= 0 || !terms || n_terms_total <= 0 || !hits_dev || !totals_dev)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (seg->ctx != comm->ctx) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "segment and communicator belong to different contexts");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  rgpu_ctx* c = comm->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
  ShardedCall call;
  int32_t rc = sharded_reserve(comm, n_queries, k, s, &call);
  if (rc != RGPU_OK) return rc;
  sharded_local(comm, seg, queries, n_queries, terms, n_terms_total, k, s, &call);
  rc = sharded_gather(comm, s, call);
  if (rc != RGPU_OK) return rc;
  rc = sharded_merge(comm, n_queries, k, hits_dev, totals_dev, s, call);
  if (rc != RGPU_OK) return rc;
  // the collective has been honoured; now this rank's own failure, if any, is reported (its peers see it in the status words)
  if (call.local_rc != RGPU_OK) return fail(call.local_rc, call.local_why);
  if (call.pre_rc != RGPU_OK) return fail(call.pre_rc, call.pre_why);
  return RGPU_OK;
}

// Start-up sizing: every slot's gather buffer for batches of up to n_queries x k, allocated now — the data path then never
// allocates, and the one failure that would leave a rank out of a collective (no buffer to gather into) cannot happen there.
// Not a collective; every rank calls it with the shapes it will serve.
extern "C" int32_t rgpu_comm_reserve(rgpu_comm* comm, int32_t n_queries, int32_t k) {
  if (!comm || n_queries <= 0) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  rgpu_ctx* c = comm->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = record_bytes(n_queries, k) * (size_t)comm->n_ranks;
  for (auto& sl : comm->slots) {
    if (sl.busy) { HIP_TRY(hipEventSynchronize(sl.done)); sl.busy = false; }
    const uint8_t* before = sl.recv.p;
    HIP_TRY(sl.recv.reserve(bytes, 0, c->stream));
    if (sl.recv.p != before) sl.status_zero = false;
    if (!sl.done) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  }
  if (!comm->last_collective) HIP_TRY(hipEventCreateWithFlags(&comm->last_collective, hipEventDisableTiming));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RGPU_OK;
}

// ncclAllGather calls this communicator has enqueued so far (a communicator of one rank issues none unless
// rgpu_config.comm_force_gather is set): tests and bench.py assert that the collective really ran.
extern "C" int64_t rgpu_comm_gathers_issued(rgpu_comm* comm) {
  if (!comm) return -1;
  std::lock_guard<std::mutex> g(comm->ctx->mu);
  return comm->gathers_issued;
}

// The one-process form: rank r = comms[r] / segs[r] (from rgpu_comm_init_all), one thread issues the whole batch. The n
// all-gathers sit in one NCCL group (issued one by one from one thread the first would wait for peers that this very
// thread has not reached yet).
extern "C" int32_t rgpu_search_batch_sharded_all(rgpu_comm* const* comms, rgpu_segment* const* segs, int32_t n, const rgpu_query* queries,
                                                 int32_t n_queries, const rgpu_query_term* const* terms_per_rank, int32_t n_terms_total,
                                                 int32_t k, void* const* hits_dev, void* const* totals_dev, void* const* hip_streams) {
  if (!comms || !segs || n < 1 || !queries || n_queries <= 0 || !terms_per_rank || n_terms_total <= 0 || !hits_dev || !totals_dev)
    return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "bad arguments");
  if (k <= 0 || k > RGPU_MAX_K) return fail(k <= 0 ? RGPU_ERR_ILLEGAL_ARGUMENT : RGPU_ERR_UNSUPPORTED, "k must be in 1..RGPU_MAX_K");
  for (int32_t r = 0; r < n; ++r) {
    if (!comms[r] || !segs[r] || !terms_per_rank[r] || !hits_dev[r] || !totals_dev[r]) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null per-rank argument");
    if (segs[r]->ctx != comms[r]->ctx || comms[r]->rank != r || comms[r]->n_ranks != n)
      return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "comms[r] / segs[r] must be rank r of an n-rank rgpu_comm_init_all group");
  }
  std::vector<ShardedCall> calls((size_t)n);
  std::vector<hipStream_t> ss((size_t)n);
  for (int32_t r = 0; r < n; ++r) {  // phase 0 for every rank: a failure here returns before ANY rank has moved on
    rgpu_ctx* c = comms[r]->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    ss[(size_t)r] = (hip_streams && hip_streams[r]) ? (hipStream_t)hip_streams[r] : c->stream;
    int32_t rc = sharded_reserve(comms[r], n_queries, k, ss[(size_t)r], &calls[(size_t)r]);
    if (rc != RGPU_OK) return rc;
  }
  // From here to ncclGroupEnd nothing returns: every rank advances its slot, searches (a failing shard leaves its status in
  // its record) and issues its all-gather — a rank left out would leave the others hanging in theirs.
  int32_t first_rc = RGPU_OK;
  std::string first_why;
  auto note = [&](int32_t rc, const std::string& why) { if (rc != RGPU_OK && first_rc == RGPU_OK) { first_rc = rc; first_why = why; } };
  for (int32_t r = 0; r < n; ++r) {  // every shard's search is enqueued before any collective: the GPUs work side by side
    rgpu_ctx* c = comms[r]->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) {  // the search cannot run: an empty record with a status would need the device too
      comms[r]->next = (comms[r]->next + 1) % N_COMM_SLOTS;
      calls[(size_t)r].local_rc = RGPU_ERR_RUNTIME;
      calls[(size_t)r].local_why = "hipSetDevice";
      continue;
    }
    sharded_local(comms[r], segs[r], queries, n_queries, terms_per_rank[r], n_terms_total, k, ss[(size_t)r], &calls[(size_t)r], true);
  }
  // (round 5: every shard's kernels are enqueued by now — disjunctions included, whose groups used to end in a stream sync and so
  // ran shard after shard; only here does the thread wait, shard by shard, for flags that are back by then as a rule)
  for (int32_t r = 0; r < n; ++r) {
    rgpu_ctx* c = comms[r]->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) continue;
    sharded_settle(comms[r], n_queries, k, ss[(size_t)r], &calls[(size_t)r]);
  }
  {
    const ncclResult_t gs = ncclGroupStart();
    if (gs != ncclSuccess) note(RGPU_ERR_RUNTIME, std::string("ncclGroupStart: ") + ncclGetErrorString(gs));
    for (int32_t r = 0; r < n; ++r) {
      rgpu_ctx* c = comms[r]->ctx;
      std::lock_guard<std::mutex> g(c->mu);
      if (hipSetDevice(c->device) != hipSuccess) { note(RGPU_ERR_RUNTIME, "hipSetDevice"); continue; }
      const int32_t rc = sharded_gather(comms[r], ss[(size_t)r], calls[(size_t)r]);
      if (rc != RGPU_OK) note(rc, "rank " + std::to_string(r) + ": " + g_last_error);
    }
    const ncclResult_t ge = ncclGroupEnd();
    if (ge != ncclSuccess) note(RGPU_ERR_RUNTIME, std::string("ncclGroupEnd: ") + ncclGetErrorString(ge));
  }
  if (first_rc != RGPU_OK) return fail(first_rc, first_why);  // a collective that could not be issued: rgpu_comm_destroy / a new communicator
  for (int32_t r = 0; r < n; ++r) {
    rgpu_ctx* c = comms[r]->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) { note(RGPU_ERR_RUNTIME, "hipSetDevice"); continue; }
    const int32_t rc = sharded_merge(comms[r], n_queries, k, hits_dev[r], totals_dev[r], ss[(size_t)r], calls[(size_t)r]);
    if (rc != RGPU_OK) note(rc, "rank " + std::to_string(r) + ": " + g_last_error);
    if (calls[(size_t)r].local_rc != RGPU_OK) note(calls[(size_t)r].local_rc, "rank " + std::to_string(r) + ": " + calls[(size_t)r].local_why);
    if (calls[(size_t)r].pre_rc != RGPU_OK) note(calls[(size_t)r].pre_rc, "rank " + std::to_string(r) + ": " + calls[(size_t)r].pre_why);
  }
  if (first_rc != RGPU_OK) return fail(first_rc, first_why);
  return RGPU_OK;
}

// Every rank's status word of the most recent sharded batch on this communicator (waits for that batch): 0, or the
// rgpu_status its local search failed with — the merged rows then lack that shard's hits.
extern "C" int32_t rgpu_comm_status(rgpu_comm* comm, int32_t* status_out) {
  if (!comm || !status_out) return fail(RGPU_ERR_ILLEGAL_ARGUMENT, "null argument");
  rgpu_ctx* c = comm->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  for (int r = 0; r < comm->n_ranks; ++r) status_out[r] = RGPU_OK;
  if (!comm->last_slot) return RGPU_OK;
  if (comm->last_slot->busy) { HIP_TRY(hipEventSynchronize(comm->last_slot->done)); comm->last_slot->busy = false; }
  const size_t record = record_bytes(comm->last_queries, comm->last_k);
  for (int r = 0; r < comm->n_ranks; ++r) {
    int64_t v = 0;
    HIP_TRY(hipMemcpy(&v, comm->last_slot->recv.p + (size_t)r * record + record - 8, 8, hipMemcpyDeviceToHost));
    status_out[r] = (int32_t)v;
  }
  return RGPU_OK;
}

