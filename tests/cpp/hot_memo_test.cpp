// csrc/host/batch_planner.hpp for_each_flat_memo_hot (the 32-byte hot entries in front of the planner's memo; csrc/api/fused.hpp
// term_batch_resident) against for_each_flat_memo_placed on a second planner over the same table, and against for_each_flat: for every
// id the same held / absent verdict, the same record behind the returned index, the same digest — over a hot set asked again and again,
// ids that share a hot slot, ids that share a memo slot, ids outside the table and absent terms, new arena generations, new keys,
// refusals (with and without records placed), for_each_flat_memo calls in between, and a stamp that wraps.
#include "../../rucene_amd/csrc/host/batch_planner.hpp"

#include <cstdio>
#include <map>
#include <random>
#include <set>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

using rucene::BatchPlanner;
struct Rec { int64_t fp; int32_t df; float idf; int32_t nblocks; uint32_t keytag; };
struct Digest { int32_t df, nblocks, bucket; };
static bool same(const Rec& a, const Rec& b) { return a.fp == b.fp && a.df == b.df && a.idf == b.idf && a.nblocks == b.nblocks && a.keytag == b.keytag; }
static Digest digest_of(const Rec& r) { return Digest{r.df, r.nblocks, r.nblocks > 0 ? __builtin_clz((uint32_t)r.nblocks) : 32}; }
static size_t memo_slot(int64_t id) { return (size_t)(((uint64_t)id * 0x9E3779B97F4A7C15ull) >> 48); }

// one planner with the arena its records are placed in: append-only within a generation, a fresh "device buffer" per generation
struct Side {
  BatchPlanner P;
  uint32_t gen = 1;
  std::map<uint32_t, std::vector<Rec>> device;  // generation -> records by index (written exactly once each)
  std::map<int64_t, int> made, placed;          // fp -> how often make / place ran since the last clear_counts()
  int64_t refuse_fp = -1;                       // make refuses this term
  size_t capacity = (size_t)1 << 30;
  Side(const rgpu_plan_stats& ps, const std::vector<rgpu_term_state>& st) : P(ps, 0, st.data(), (int64_t)st.size(), nullptr, 0) {}
  void turn_over() { ++gen; }
  void clear_counts() { made.clear(); placed.clear(); }
  auto maker(const BatchPlanner::MemoKey& key) {
    return [this, key](const rgpu_term_state& s, float idf, Rec* out) -> int32_t {
      if (s.doc_start_fp == refuse_fp) return -1;
      ++made[s.doc_start_fp];
      *out = Rec{s.doc_start_fp, s.doc_freq, idf, s.doc_freq / 128, (uint32_t)key.w[1]};
      return 1;
    };
  }
  auto placer() {
    return [this](const Rec* r) -> int64_t {
      std::vector<Rec>& d = device[gen];
      if (d.size() >= capacity) return -1;
      ++placed[r->fp];
      d.push_back(*r);
      return (int64_t)d.size() - 1;
    };
  }
  size_t placed_now() { return device[gen].size(); }
};

int main() {
  std::mt19937_64 rng(23);
  const int64_t n_leaf = 200000;
  std::vector<rgpu_term_state> states((size_t)n_leaf);
  for (int64_t i = 0; i < n_leaf; ++i) {
    rgpu_term_state s{};
    s.doc_freq = (i % 17 == 3) ? 0 : (int32_t)(1 + rng() % 500000);  // every 17th term is absent from the leaf
    s.doc_start_fp = 1000 + 13 * i;
    s.total_term_freq = s.doc_freq * 2;
    s.skip_offset = -1;
    s.singleton_doc_id = s.doc_freq == 1 ? (int32_t)(rng() % 1000) : -1;
    states[(size_t)i] = s;
  }
  rgpu_plan_stats ps{};
  ps.max_doc = 10000000;
  ps.doc_count = 10000000;
  ps.sum_total_term_freq = 1000000000;
  ps.k1 = 1.2f;
  ps.b = 0.75f;
  Side H(ps, states), M(ps, states);  // H: hot entries in front of the memo; M: the memo alone
  BatchPlanner F(ps, 0, states.data(), n_leaf, nullptr, 0);
  auto fp_of = [&](int64_t id) { return states[(size_t)id].doc_start_fp; };
  auto held = [&](int64_t id) { return id >= 0 && id < n_leaf && states[(size_t)id].doc_freq > 0; };

  // one call of each function over the same ids; false when the hot one gave up (then nothing is compared)
  auto run = [&](const std::vector<int64_t>& ids, const BatchPlanner::MemoKey& key) -> bool {
    const int64_t n = (int64_t)ids.size();
    struct Got { int32_t index = -2; Digest d{}; };
    std::vector<Got> got((size_t)n);
    size_t seen = 0;
    const bool ok = H.P.for_each_flat_memo_hot<Rec, Digest>(ids.data(), n, key, H.gen, H.maker(key), H.placer(), digest_of, [&](int64_t i, int32_t index, const Digest& d) {
      ++seen;
      got[(size_t)i] = Got{index, d};
    });
    if (!ok) return false;
    CHECK(seen == ids.size());
    std::vector<Rec> want((size_t)n);
    F.for_each_flat(ids.data(), n, [&](int64_t i, const rgpu_term_state& s, float idf) { want[(size_t)i] = Rec{s.doc_start_fp, s.doc_freq, idf, s.doc_freq / 128, (uint32_t)key.w[1]}; });
    const std::vector<Rec>& hd = H.device[H.gen];
    const bool ok_m = M.P.for_each_flat_memo_placed<Rec>(ids.data(), n, key, M.gen, M.maker(key), M.placer(), [&](int64_t i, const Rec* r, int32_t index) {
      const Got& g = got[(size_t)i];
      CHECK((r != nullptr) == (g.index >= 0) && (r != nullptr) == (index >= 0) && (r != nullptr) == (want[(size_t)i].df > 0));
      if (!r || g.index < 0) {
        CHECK(g.index == -1 && g.d.df == 0 && g.d.nblocks == 0 && g.d.bucket == 0);  // absent: index -1 and a zero digest
        return;
      }
      CHECK((size_t)g.index < hd.size());
      if ((size_t)g.index >= hd.size()) return;
      CHECK(same(hd[(size_t)g.index], *r) && same(*r, want[(size_t)i]) && same(M.device[M.gen][(size_t)index], *r));
      const Digest d = digest_of(*r);
      CHECK(g.d.df == d.df && g.d.nblocks == d.nblocks && g.d.bucket == d.bucket);
    });
    CHECK(ok_m);
    return true;
  };
  auto count = [](const std::map<int64_t, int>& m, int64_t fp) { const auto it = m.find(fp); return it == m.end() ? 0 : it->second; };

  const BatchPlanner::MemoKey k1{{7, 1, 0, 0}}, k2{{7, 2, 0, 0}}, k3{{7, 3, 0, 0}};
  const std::vector<int64_t> odd = {-1, n_leaf, n_leaf + 5, 3, 20, -77, INT64_MAX, INT64_MIN};  // outside the table; 3, 20: absent terms

  // ---- a hot set asked again and again (ids below 5000: no two share a slot of either table): make and place run once per term
  std::vector<int64_t> hot_set;
  for (int i = 0; i < 3000; ++i) hot_set.push_back((int64_t)(rng() % 5000));
  hot_set.insert(hot_set.end(), odd.begin(), odd.end());
  std::set<int64_t> hot_fps;
  for (int64_t id : hot_set) if (held(id)) hot_fps.insert(fp_of(id));
  for (int pass = 0; pass < 4; ++pass) {
    CHECK(run(hot_set, k1));
    std::shuffle(hot_set.begin(), hot_set.end(), rng);
  }
  CHECK(H.made.size() == hot_fps.size() && H.placed.size() == hot_fps.size() && H.placed_now() == hot_fps.size());
  for (int64_t fp : hot_fps) CHECK(count(H.made, fp) == 1 && count(H.placed, fp) == 1);

  // ---- pairs that share a hot slot (and no memo slot), asked alternately: both stay right; the memo still holds the one the hot
  // table dropped, so nothing is made or placed twice
  std::vector<int64_t> pa, pb;
  for (int64_t a = 6000; a < 6400; ++a) {
    const int64_t b = a + (int64_t)BatchPlanner::HOT_SLOTS;
    CHECK(BatchPlanner::hot_slot(a) == BatchPlanner::hot_slot(b));
    if (memo_slot(a) == memo_slot(b)) continue;
    pa.push_back(a);
    pb.push_back(b);
  }
  pa.insert(pa.end(), odd.begin(), odd.end());
  H.clear_counts();
  for (int pass = 0; pass < 3; ++pass) { CHECK(run(pa, k1)); CHECK(run(pb, k1)); }
  { std::vector<int64_t> both;  // ... and within one call
    for (size_t i = 0; i < pb.size(); ++i) { both.push_back(pa[i]); both.push_back(pb[i]); both.push_back(pa[i]); }
    CHECK(run(both, k1)); }
  for (size_t i = 0; i < pb.size(); ++i) {
    if (held(pa[i])) CHECK(count(H.made, fp_of(pa[i])) == 1 && count(H.placed, fp_of(pa[i])) == 1);
    if (held(pb[i])) CHECK(count(H.made, fp_of(pb[i])) == 1 && count(H.placed, fp_of(pb[i])) == 1);
  }

  // ---- pairs that share a memo slot (and no hot slot), asked alternately: the memo evicts, the hot entries stay — placed once each
  std::vector<int64_t> by_slot_first(65536, -1), ma, mb;
  for (int64_t id = 7000; id < n_leaf && ma.size() < 300; ++id) {
    if (!held(id)) continue;
    const size_t slot = memo_slot(id);
    if (by_slot_first[slot] < 0) by_slot_first[slot] = id;
    else if (BatchPlanner::hot_slot(by_slot_first[slot]) != BatchPlanner::hot_slot(id)) { ma.push_back(by_slot_first[slot]); mb.push_back(id); by_slot_first[slot] = -1; }
  }
  CHECK(ma.size() == 300);
  H.clear_counts();
  M.clear_counts();
  for (int pass = 0; pass < 3; ++pass) { CHECK(run(ma, k1)); CHECK(run(mb, k1)); }
  for (size_t i = 0; i < ma.size(); ++i) {
    CHECK(count(H.placed, fp_of(ma[i])) == 1 && count(H.placed, fp_of(mb[i])) == 1);
    CHECK(count(M.placed, fp_of(ma[i])) == 3 && count(M.placed, fp_of(mb[i])) == 3);  // (the memo alone places them every time)
  }
  // ... and `place` runs again only when the memo entry is gone too: a loses its hot entry to b (same hot slot) and its memo entry
  // to c (same memo slot)
  {
    int64_t a = -1, b = -1, c = -1;
    for (size_t i = 0; i < ma.size() && a < 0; ++i) {
      const int64_t cand = ma[i] + (int64_t)BatchPlanner::HOT_SLOTS;
      if (cand < n_leaf && held(cand) && memo_slot(cand) != memo_slot(ma[i])) { a = ma[i]; c = mb[i]; b = cand; }
    }
    CHECK(a >= 0);
    CHECK(run({b}, k1));
    CHECK(run({a}, k1));             // (a hot miss: a is in both tables now)
    H.clear_counts();
    CHECK(run({b}, k1));             // a's hot entry goes; its memo entry stays
    CHECK(run({a}, k1));
    CHECK(count(H.placed, fp_of(a)) == 0 && count(H.made, fp_of(a)) == 0);
    // a's memo entry goes (c takes the slot, through the pass that looks at the memo for every id); its hot entry stays
    CHECK(H.P.for_each_flat_memo<Rec>(&c, 1, k1, H.maker(k1), [&](int64_t, const Rec* r) { CHECK(r != nullptr); }));
    CHECK(run({a}, k1));
    CHECK(count(H.placed, fp_of(a)) == 0 && count(H.made, fp_of(a)) == 0);
    CHECK(run({b}, k1));             // both gone
    const size_t before = H.placed_now();
    CHECK(run({a, a, a}, k1));
    CHECK(count(H.placed, fp_of(a)) == 1 && count(H.made, fp_of(a)) == 1 && H.placed_now() == before + 1);  // (the old record: an orphan)
  }

  // ---- a new arena generation: every held term is placed again, into the new buffer
  std::vector<int64_t> all = hot_set;
  all.insert(all.end(), pa.begin(), pa.end());
  all.insert(all.end(), pb.begin(), pb.end());
  all.insert(all.end(), ma.begin(), ma.end());
  all.insert(all.end(), mb.begin(), mb.end());
  std::set<int64_t> all_fps;
  for (int64_t id : all) if (held(id)) all_fps.insert(fp_of(id));
  H.turn_over(); M.turn_over();
  H.clear_counts();
  CHECK(H.placed_now() == 0);
  CHECK(run(all, k1));
  for (int64_t fp : all_fps) CHECK(count(H.placed, fp) >= 1);
  CHECK(H.placed_now() >= all_fps.size());
  // ---- a new key: made again under it (the records carry the key's tag), placed in the caller's new generation
  H.turn_over(); M.turn_over();
  H.clear_counts();
  CHECK(run(all, k2));
  for (int64_t fp : all_fps) CHECK(count(H.made, fp) >= 1 && count(H.placed, fp) >= 1);
  CHECK(run(hot_set, k2));
  // ... and a key that changes under ONE arena generation (the memo's own generation moves): nothing of the old key comes back
  CHECK(run(hot_set, k3));
  CHECK(run(hot_set, k2));
  CHECK(run(all, k2));

  // ---- make refuses midway, after records have been placed: false at once; the caller's arena generation turns over, and the next
  // pass is right under the new one
  {
    std::vector<int64_t> fresh;
    for (int64_t id = 100000; id < 100400; ++id) fresh.push_back(id);
    const int64_t victim = 100250;
    CHECK(held(victim));
    H.refuse_fp = fp_of(victim);
    const size_t before = H.placed_now();
    H.clear_counts();
    CHECK(!run(fresh, k2));
    CHECK(H.placed_now() > before && count(H.made, fp_of(victim)) == 0);
    H.refuse_fp = -1;
    H.turn_over(); M.turn_over();     // (term_batch_resident's Unplace)
    CHECK(run(fresh, k2));
    CHECK(run(all, k2));
    CHECK(run(fresh, k2));
    // ---- a refusal with nothing placed: the generation stays, and earlier hot entries stay valid (no make, no place)
    const int64_t victim2 = 100600;
    CHECK(held(victim2));
    H.refuse_fp = fp_of(victim2);
    const size_t placed_before = H.placed_now();
    std::vector<int64_t> known_then_refused(fresh.begin(), fresh.begin() + 100);
    known_then_refused.push_back(victim2);
    known_then_refused.push_back(100601);
    CHECK(!run(known_then_refused, k2));
    CHECK(H.placed_now() == placed_before);
    H.refuse_fp = -1;
    H.clear_counts();
    CHECK(run(fresh, k2));
    CHECK(H.made.empty() && H.placed.empty() && H.placed_now() == placed_before);
    CHECK(run(known_then_refused, k2));   // (the refused term was not kept: made and placed now)
    CHECK(count(H.made, fp_of(victim2)) == 1 && count(H.placed, fp_of(victim2)) == 1);
    // place refuses (a full arena): false, turn over, right again
    H.capacity = H.placed_now() + 3;
    std::vector<int64_t> more;
    for (int64_t id = 101000; id < 101050; ++id) more.push_back(id);
    CHECK(!run(more, k2));
    H.capacity = (size_t)1 << 30;
    H.turn_over(); M.turn_over();
    CHECK(run(more, k2));
    CHECK(run(all, k2));
  }

  // ---- for_each_flat_memo (the staged plan's pass) over the same ids in between, under the same key: it rewrites memo entries
  // without placing them; the hot entries stay right, and a hot miss places what for_each_flat_memo left unplaced
  for (int pass = 0; pass < 3; ++pass) {
    for (Side* s : {&H, &M}) {
      const std::vector<int64_t>& ids = pass == 1 ? mb : ma;
      CHECK(s->P.for_each_flat_memo<Rec>(ids.data(), (int64_t)ids.size(), k2, s->maker(k2), [&](int64_t, const Rec* r) { CHECK(r != nullptr); }));
      std::vector<int64_t> unseen;
      for (int64_t id = 120000 + 100 * pass; id < 120050 + 100 * pass; ++id) unseen.push_back(id);
      CHECK(s->P.for_each_flat_memo<Rec>(unseen.data(), (int64_t)unseen.size(), k2, s->maker(k2), [&](int64_t, const Rec*) {}));
    }
    std::vector<int64_t> unseen;
    for (int64_t id = 120000 + 100 * pass; id < 120050 + 100 * pass; ++id) unseen.push_back(id);
    CHECK(run(unseen, k2));
    CHECK(run(ma, k2));
    CHECK(run(mb, k2));
    CHECK(run(all, k2));
  }
  // ... and under another key and record size, as another caller of the same planner would
  CHECK(H.P.for_each_flat_memo<int64_t>(ma.data(), (int64_t)ma.size(), k3, [](const rgpu_term_state& s, float, int64_t* out) -> int32_t { *out = s.doc_start_fp; return 1; },
                                        [&](int64_t, const int64_t* r) { CHECK(r != nullptr); }));
  CHECK(run(all, k2));

  // ---- the stamp wraps: the table is cleared, nothing stamped before the wrap is taken for current
  H.P.hot_stamp_set(0xfffffffdu);
  CHECK(run(all, k2));               // 0xfffffffe
  H.turn_over(); M.turn_over();
  CHECK(run(all, k2));               // 0xffffffff
  CHECK(run(hot_set, k2));
  H.turn_over(); M.turn_over();
  H.clear_counts();
  CHECK(run(all, k2));               // wrapped: 1, after a clear
  for (int64_t fp : all_fps) CHECK(count(H.placed, fp) >= 1);
  H.turn_over(); M.turn_over();
  CHECK(run(all, k2));               // 2
  CHECK(run(all, k2));
  H.clear_counts();
  CHECK(run(hot_set, k2));
  CHECK(H.made.empty() && H.placed.empty());

  if (failures) return 1;
  std::printf("hot_memo OK\n");
  return 0;
}
