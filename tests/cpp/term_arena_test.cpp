// csrc/host/term_arena.hpp (the bookkeeping of the device-resident term descriptors) and csrc/host/batch_planner.hpp
// for_each_flat_memo_placed (the memo that names them): a generation turns over on a full arena and on another key and gets a buffer of
// its own; a retired generation's buffer comes back only after the last slot tagged with it has been waited for; an upload makes other
// streams wait until a slot marked behind it on its own stream has been waited for, and never its own stream; an evicted memo entry
// only orphans its record — no index is handed out twice within a generation, and what a record says never changes.
#include "../../rucene_amd/csrc/host/batch_planner.hpp"
#include "../../rucene_amd/csrc/host/term_arena.hpp"

#include <cstdio>
#include <map>
#include <set>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

using rucene::TermArena;

struct Rec { int64_t fp; int32_t df; float idf; };

static void* ptr(uintptr_t v) { return reinterpret_cast<void*>(v); }

static void generations_and_retirement() {
  TermArena A(4);
  const TermArena::Key k1{{1, 1, 0, 0}}, k2{{1, 2, 0, 0}};
  std::vector<void*> freed;
  auto release = [&]() { A.release_retired([&](void* b) { freed.push_back(b); }); };
  CHECK(A.generation() == 0 && A.append() == -1);  // no generation, no buffer: nothing to append to
  CHECK(A.begin(k1));                               // the first call starts one ...
  CHECK(A.append() == -1);                          // ... which takes records once it has its buffer
  A.set_buffer(ptr(0x1000));
  const uint32_t g1 = A.generation();
  CHECK(g1 != 0 && !A.begin(k1) && A.generation() == g1);  // the same key: the same generation
  for (int i = 0; i < 4; ++i) CHECK(A.append() == i);
  CHECK(A.append() == -1 && A.used() == 4);         // full
  A.slot_marked(0, 7);                              // two calls in flight read generation g1
  A.slot_marked(1, 8);
  A.turn_over();                                    // full: the next generation, a buffer of its own
  CHECK(A.generation() != g1 && A.buffer() == nullptr && A.used() == 0 && A.retired() == 1);
  A.set_buffer(ptr(0x2000));
  CHECK(A.append() == 0);
  CHECK(A.slot_holds_retired(0) && A.slot_holds_retired(1) && !A.slot_holds_retired(2));
  release();
  CHECK(freed.empty());                             // both slots still carry g1
  A.slot_waited(0);
  release();
  CHECK(freed.empty());                             // one still does
  A.slot_marked(0, 7);                              // (slot 0 comes round again under the new generation: that does not hold g1)
  release();
  CHECK(freed.empty());
  A.slot_waited(1);
  release();
  CHECK(freed.size() == 1 && freed[0] == ptr(0x1000) && A.retired() == 0);
  // another key: a new generation although this one has room
  const uint32_t g2 = A.generation();
  CHECK(A.begin(k2) && A.generation() != g2 && A.generation() != g1 && A.buffer() == nullptr && A.retired() == 1);
  A.set_buffer(ptr(0x3000));
  CHECK(!A.begin(k2) && A.begin(k1));               // ... and back: generations are never resumed
  A.set_buffer(ptr(0x4000));
  CHECK(A.retired() == 2);
  release();
  CHECK(freed.size() == 2 && freed[1] == ptr(0x3000) && A.retired() == 1);  // 0x3000 was never read by a slot; 0x2000 is slot 0's
  A.all_waited();                                   // a device-wide wait
  release();
  CHECK(freed.size() == 3 && freed[2] == ptr(0x2000));
  // closing: the current generation goes too, once its slots have been waited for
  A.slot_marked(2, 7);
  A.retire_current();
  release();
  CHECK(freed.size() == 3 && A.buffer() == nullptr);
  A.slot_waited(2);
  release();
  CHECK(freed.size() == 4 && freed[3] == ptr(0x4000) && A.retired() == 0);
  // a generation that lost its buffer (a pass whose records were never uploaded) is not resumed either
  CHECK(A.begin(k1));
}

static void upload_sequences() {
  TermArena A(1000);
  const TermArena::Key k{{5, 5, 5, 5}};
  A.begin(k);
  A.set_buffer(ptr(0x1000));
  const uint64_t sa = 0xA, sb = 0xB;
  std::vector<void*> waited;
  auto waits = [&](uint64_t stream, uint32_t lo, uint32_t hi) {
    waited.clear();
    A.for_each_wait(stream, lo, hi, [&](void* e) { waited.push_back(e); });
    return waited.size();
  };
  CHECK(waits(sb, 0, 999) == 0 && A.pending_uploads() == 0);  // steady state: nothing pending, nothing to wait for
  // call 1 on stream A uploads records [0, 10) in slot 0
  for (int i = 0; i < 10; ++i) A.append();
  const uint64_t q1 = A.note_upload(0, 10, sa, ptr(0xE1));
  A.slot_marked(0, sa);
  CHECK(q1 == 1 && A.last_sequence() == 1);
  CHECK(waits(sa, 0, 9) == 0);                      // its own stream is ordered behind it already
  CHECK(waits(sb, 10, 20) == 0);                    // records of no pending upload
  CHECK(waits(sb, 3, 4) == 1 && waited[0] == ptr(0xE1));  // first touch on A, use on B: B waits for A's event
  A.slot_marked(1, sb);
  CHECK(waits(sb, 3, 4) == 0);                      // ... once: B is ordered behind it from then on
  // call 3 on stream B uploads [10, 15); a call on A reading 8..12 waits for it, not for its own upload
  for (int i = 0; i < 5; ++i) A.append();
  const uint64_t q2 = A.note_upload(10, 15, sb, ptr(0xE2));
  A.slot_marked(2, sb);
  CHECK(q2 == 2);
  CHECK(waits(sa, 8, 12) == 1 && waited[0] == ptr(0xE2));
  // slot 1 (marked on B BEFORE upload 2) is waited for: that proves nothing about upload 2, and nothing about A's upload 1
  A.slot_waited(1);
  CHECK(A.pending_uploads() == 2);
  // slot 0 (marked on A behind upload 1) is waited for: upload 1 is complete, its event is spare
  A.slot_waited(0);
  CHECK(A.pending_uploads() == 1 && A.take_spare_event() == ptr(0xE1) && A.take_spare_event() == nullptr);
  CHECK(waits(0xC, 0, 9) == 0);                     // a third stream reads upload 1's records without a wait
  CHECK(waits(0xC, 0, 14) == 1 && waited[0] == ptr(0xE2));
  A.slot_waited(2);
  CHECK(A.pending_uploads() == 0 && A.take_spare_event() == ptr(0xE2));
  // a turnover forgets the uploads still pending (nobody names their records any more) and hands their events back
  A.append();
  A.note_upload(15, 16, sa, ptr(0xE3));
  A.turn_over();
  CHECK(A.pending_uploads() == 0 && A.take_spare_event() == ptr(0xE3));
  A.set_buffer(ptr(0x2000));
  A.append();
  A.note_upload(0, 1, sa, ptr(0xE4));
  A.all_waited();
  CHECK(A.pending_uploads() == 0 && A.take_spare_event() == ptr(0xE4));
}

// the memo and the arena together, as term_batch_resident drives them
static void memo_places_records_once() {
  const int64_t n_leaf = 300000;
  std::vector<rgpu_term_state> states((size_t)n_leaf);
  for (int64_t i = 0; i < n_leaf; ++i) {
    rgpu_term_state s{};
    s.doc_freq = (i % 17 == 3) ? 0 : (int32_t)(2 + i % 1000);
    s.doc_start_fp = 1000 + 13 * i;
    s.total_term_freq = s.doc_freq * 2;
    s.skip_offset = -1;
    s.singleton_doc_id = -1;
    states[(size_t)i] = s;
  }
  rgpu_plan_stats ps{};
  ps.max_doc = 10000000;
  ps.doc_count = 10000000;
  ps.sum_total_term_freq = 1000000000;
  ps.k1 = 1.2f;
  ps.b = 0.75f;
  rucene::BatchPlanner P(ps, 0, states.data(), n_leaf, nullptr, 0);
  // pairs of ids that share a memo slot (they evict each other call after call), a hot set, an absent term, ids outside the table
  std::vector<int64_t> first(65536, -1), a, b;
  for (int64_t id = 0; id < n_leaf && a.size() < 40; ++id) {
    if (id % 17 == 3) continue;
    const size_t slot = (size_t)(((uint64_t)id * 0x9E3779B97F4A7C15ull) >> 48);
    if (first[slot] < 0) first[slot] = id;
    else { a.push_back(first[slot]); b.push_back(id); }
  }
  CHECK(a.size() == 40);
  for (int64_t id = 100; id < 130; ++id) { a.push_back(id); b.push_back(id); }
  a.push_back(3); b.push_back(-1); a.push_back(n_leaf); b.push_back(20);

  TermArena A(96);
  std::map<uint32_t, std::vector<Rec>> device;      // generation -> the records "on the device", by index
  std::map<uint32_t, std::set<int64_t>> issued;     // generation -> indices handed out
  int turnovers = 0;
  auto call = [&](const std::vector<int64_t>& ids, const rucene::BatchPlanner::MemoKey& key) {
    if (A.begin(TermArena::Key{{key.w[0], key.w[1], key.w[2], key.w[3]}})) { A.set_buffer(ptr(0x1000 + A.generation())); ++turnovers; }
    for (int attempt = 0; attempt < 2; ++attempt) {
      bool full = false;
      size_t seen = 0;
      const uint32_t gen = A.generation();
      const bool ok = P.for_each_flat_memo_placed<Rec>(ids.data(), (int64_t)ids.size(), key, gen, [&](const rgpu_term_state& s, float idf, Rec* out) -> int32_t {
        *out = Rec{s.doc_start_fp, s.doc_freq, idf};
        return 1;
      }, [&](const Rec* r) -> int64_t {
        const int64_t at = A.append();
        if (at < 0) { full = true; return -1; }
        CHECK(issued[gen].insert(at).second);       // never issued before within this generation
        std::vector<Rec>& d = device[gen];
        if (d.size() <= (size_t)at) d.resize((size_t)at + 1);
        d[(size_t)at] = *r;                         // written exactly once
        return at;
      }, [&](int64_t i, const Rec* r, int32_t index) {
        ++seen;
        const int64_t id = ids[(size_t)i];
        const bool held = id >= 0 && id < n_leaf && states[(size_t)id].doc_freq > 0;
        CHECK(held == (r != nullptr) && held == (index >= 0));
        if (!r || index < 0) return;
        CHECK((size_t)index < device[gen].size());
        const Rec& on_device = device[gen][(size_t)index];  // what a launch of this call would read
        CHECK(on_device.fp == states[(size_t)id].doc_start_fp && on_device.df == states[(size_t)id].doc_freq && on_device.idf == r->idf);
      });
      if (ok) { CHECK(seen == ids.size()); return; }
      CHECK(full && attempt == 0);
      A.turn_over();
      A.set_buffer(ptr(0x1000 + A.generation()));
      ++turnovers;
    }
  };
  const rucene::BatchPlanner::MemoKey k1{{7, 1, 0, 0}}, k2{{7, 2, 0, 0}};
  call(a, k1);
  const uint32_t used_once = A.used();
  CHECK(turnovers == 1 && used_once >= 60 && used_once <= 70);
  call(a, k1);
  CHECK(A.used() == used_once);                     // a steady state places nothing
  // b's pairs evict a's: each alternation orphans 40 records and appends 40, until the arena is full and turns over
  const uint32_t g_before = A.generation();
  for (int i = 0; i < 6; ++i) { call(b, k1); call(a, k1); }
  CHECK(A.generation() != g_before && turnovers > 2);
  // another key: another generation, every record made and placed again
  const int t0 = turnovers;
  call(a, k2);
  CHECK(turnovers == t0 + 1 && A.used() == used_once);
  // entries for_each_flat_memo made or re-made carry no place: placed on their next use here, under the same generation
  size_t n = 0;
  CHECK(P.for_each_flat_memo<Rec>(b.data(), (int64_t)b.size(), k2, [&](const rgpu_term_state& s, float idf, Rec* out) -> int32_t { *out = Rec{s.doc_start_fp, s.doc_freq, idf}; return 1; },
                                  [&](int64_t, const Rec*) { ++n; }));
  CHECK(n == b.size());
  call(b, k2);
  call(a, k2);
}

int main() {
  generations_and_retirement();
  upload_sequences();
  memo_places_records_once();
  if (failures) return 1;
  std::printf("term_arena OK\n");
  return 0;
}
