// The bookkeeping of a context's device-resident term descriptors (api/fused.hpp term_batch_resident). Host-only: no HIP calls, the
// device buffers and events are opaque pointers the owner allocates, frees and records.
//
// A fused single-term step names the same terms call after call, and a term's descriptor depends only on things that stay put between
// calls (the planner's tables, the segment's prepared store, the similarity table): it is written to the device once and the per-step
// plan names it by a 32-bit index. What makes that safe with launches in flight on several streams is that nothing is ever rewritten:
//
//   generation   one device buffer of `capacity` records, filled from index 0 upwards. A record is written exactly once, by the call
//                whose memo pass missed; an evicted memo entry only orphans its record. A generation ends when the key changes (segment,
//                prepared-store epoch, similarity table, flags: everything a record depends on outside the planner) or the buffer is
//                full; the next one gets a FRESH buffer, so a launch that still reads the old one is not disturbed.
//   retirement   every scratch slot whose call read a generation carries its number until the slot's event has been waited for. A
//                retired generation's buffer goes back to the owner only when no busy slot carries its number.
//   uploads      new records travel on the caller's stream, ahead of the search kernel that reads them: the same stream needs no
//                more. Each upload gets a sequence number and an event; a call on ANOTHER stream that names a record of an upload
//                not known complete waits for that event first. An upload is known complete once a slot marked on its stream at or
//                after it has been waited for — which happens anyway when the slot comes round again, so a steady state (no uploads
//                pending) makes no event call at all.
#pragma once
#include <cstdint>
#include <vector>

namespace rucene {

class TermArena {
 public:
  struct Key {
    uint64_t w[4];
    bool operator==(const Key& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
  };
  static constexpr int MAX_SLOTS = 16;

  explicit TermArena(uint32_t capacity = 262144) : capacity_(capacity < 1 ? 1 : capacity) {}

  uint32_t capacity() const { return capacity_; }
  uint32_t generation() const { return gen_; }  // 0: none yet
  uint32_t used() const { return used_; }
  void* buffer() const { return buf_; }
  const Key& key() const { return key_; }

  // A call under `key` is about to append / read records: false when the current generation serves it; true when a new one was started
  // (another key, or none yet) — the owner then hands it a buffer with set_buffer() before anything else.
  bool begin(const Key& key) {
    if (gen_ != 0 && buf_ != nullptr && key_ == key) return false;
    key_ = key;
    turn_over();
    return true;
  }
  // The current generation ends here (full, or its records can no longer be trusted): its buffer is retired, uploads still pending are
  // forgotten (their records are no longer named by anybody; their events go back to the owner). The owner gives the new one a buffer.
  void turn_over() {
    if (buf_ != nullptr) retired_.push_back(Retired{gen_, buf_});
    buf_ = nullptr;
    for (const Upload& u : pending_) spare_events_.push_back(u.event);
    pending_.clear();
    ++gen_;
    if (gen_ == 0) gen_ = 1;  // (0 is "no generation": what a memo entry that was never placed carries)
    used_ = 0;
  }
  void set_buffer(void* buf) { buf_ = buf; }

  // the next free index, or -1 when the generation is full (the caller turns it over and starts its pass again)
  int64_t append() {
    if (buf_ == nullptr || used_ >= capacity_) return -1;
    return (int64_t)used_++;
  }

  // ---- uploads ----
  // records [first, end) were enqueued on `stream` with `event` recorded behind them; returns the upload's sequence number
  uint64_t note_upload(uint32_t first, uint32_t end, uint64_t stream, void* event) {
    pending_.push_back(Upload{next_seq_, first, end, stream, stream, event});
    return next_seq_++;
  }
  // A call on `stream` reads records within [lo, hi]: wait(event) for every upload not known complete that another stream carries and
  // that may hold one of them. (A stream that has waited for an upload is not asked again while it stays the latest to have done so.)
  template <class Wait>
  void for_each_wait(uint64_t stream, uint32_t lo, uint32_t hi, Wait&& wait) {
    for (Upload& u : pending_) {
      if (u.stream == stream || u.ordered_on == stream || u.first > hi || u.end <= lo) continue;
      wait(u.event);
      u.ordered_on = stream;
    }
  }
  size_t pending_uploads() const { return pending_.size(); }
  uint64_t last_sequence() const { return next_seq_ - 1; }
  // an event the owner may record again (nullptr: none spare, create one)
  void* take_spare_event() {
    if (spare_events_.empty()) return nullptr;
    void* e = spare_events_.back();
    spare_events_.pop_back();
    return e;
  }
  void give_spare_event(void* e) { spare_events_.push_back(e); }

  // ---- scratch slots ----
  // slot `slot`'s call read the current generation and was marked (its event recorded) on `stream`
  void slot_marked(int slot, uint64_t stream) {
    slots_[slot] = Slot{gen_, stream, next_seq_ - 1};
  }
  // slot `slot`'s event has been waited for: everything enqueued on its stream before the mark has finished — the launches that read
  // its generation, and the uploads that stream carried up to then
  void slot_waited(int slot) {
    const Slot s = slots_[slot];
    slots_[slot] = Slot{};
    if (s.gen == 0) return;
    if (s.gen == gen_) {
      size_t keep = 0;
      for (size_t i = 0; i < pending_.size(); ++i) {
        if (pending_[i].stream == s.stream && pending_[i].seq <= s.seq) spare_events_.push_back(pending_[i].event);
        else pending_[keep++] = pending_[i];
      }
      pending_.resize(keep);
    }
  }
  // every slot has been waited for (a device-wide wait)
  void all_waited() {
    for (int i = 0; i < MAX_SLOTS; ++i) slots_[i] = Slot{};
    for (const Upload& u : pending_) spare_events_.push_back(u.event);
    pending_.clear();
  }
  bool slot_tagged(int slot) const { return slots_[slot].gen != 0; }
  // does a busy slot still carry a RETIRED generation's number? (what rgpu_synchronize waits for)
  bool slot_holds_retired(int slot) const { return slots_[slot].gen != 0 && slots_[slot].gen != gen_; }

  // ---- retirement ----
  size_t retired() const { return retired_.size(); }
  // free_buffer(buf) for every retired generation no busy slot carries
  template <class Free>
  void release_retired(Free&& free_buffer) {
    size_t keep = 0;
    for (size_t i = 0; i < retired_.size(); ++i) {
      bool held = false;
      for (int s = 0; s < MAX_SLOTS; ++s) held = held || slots_[s].gen == retired_[i].gen;
      if (held) retired_[keep++] = retired_[i];
      else free_buffer(retired_[i].buf);
    }
    retired_.resize(keep);
  }
  // the current generation too (segment close, context close): call after the slots that read it have been waited for
  void retire_current() {
    if (buf_ != nullptr) turn_over();
  }

 private:
  struct Upload { uint64_t seq; uint32_t first, end; uint64_t stream, ordered_on; void* event; };
  struct Slot { uint32_t gen = 0; uint64_t stream = 0; uint64_t seq = 0; };
  struct Retired { uint32_t gen; void* buf; };
  uint32_t capacity_;
  uint32_t gen_ = 0, used_ = 0;
  void* buf_ = nullptr;
  Key key_{{0, 0, 0, 0}};
  uint64_t next_seq_ = 1;
  std::vector<Upload> pending_;
  std::vector<void*> spare_events_;
  std::vector<Retired> retired_;
  Slot slots_[MAX_SLOTS];
};

}  // namespace rucene
