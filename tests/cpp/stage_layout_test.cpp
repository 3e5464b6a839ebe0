// csrc/host/stage_layout.hpp (the layout of a staged plan and the typed view of its two buffers) against a straight re-statement of
// the rule the byte arithmetic followed: used = (used + 255) & ~255; off = used; used += bytes.
#include "../../rucene_amd/csrc/host/stage_layout.hpp"

#include <cstdio>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

using rucene::StageLayout;
using rucene::StageRegion;
using rucene::StageView;

struct OldRule {
  size_t used = 0;
  size_t add(size_t bytes) {
    used = (used + 255) & ~size_t(255);
    const size_t off = used;
    used += bytes;
    return off;
  }
};
struct Sixteen { uint32_t w[4]; };
struct Odd { uint8_t b[52]; };  // (a DevTerm-sized record: no power of two)

template <typename T>
static void same(StageLayout& st, OldRule& old, size_t n) {
  const StageRegion<T> r = st.add<T>(n);
  CHECK(r.off == old.add(n * sizeof(T)) && r.n == n && r.bytes() == n * sizeof(T) && r.off % 256 == 0 && st.used == old.used);
}

static void mixed_types_and_counts() {
  StageLayout st;
  OldRule old;
  same<Sixteen>(st, old, 1024);
  same<Odd>(st, old, 3);
  same<int64_t>(st, old, 1025);
  same<int32_t>(st, old, 1);
  same<uint8_t>(st, old, 7);
  same<uint8_t>(st, old, 0);    // nothing: the next region starts where this one does
  same<int64_t>(st, old, 0);
  same<int32_t>(st, old, 64);   // 256 bytes: the next region follows without padding
  const size_t end_of_256 = st.used;
  same<Sixteen>(st, old, 32);   // 512 bytes
  CHECK(st.used - 512 == end_of_256);
  same<Odd>(st, old, 1);
  CHECK(st.add(5) == old.add(5) && st.used == old.used);  // the raw overload
}

static void end_marker() {  // add<T>(0) behind the last region: the aligned end, as the fused TERM path reads it
  StageLayout st;
  OldRule old;
  same<Odd>(st, old, 5);
  const StageRegion<uint8_t> end = st.add<uint8_t>(0);
  CHECK(end.off == old.add(0) && end.n == 0 && end.off == 512 && st.used == 512);
  const StageRegion<uint8_t> again = st.add<uint8_t>(0);
  CHECK(again.off == 512 && st.used == 512);
}

// search_pass: queries, terms (at least one), item prefix, row map, thresholds, then — each only when its path is taken — the finished-item
// counts, ReqOptScorer's record prefix, the clause bitmaps and k_search_term's item descriptors
static void search_pass_sequence(size_t nq, size_t nt, bool term_fold, bool req_opt, size_t n_bitmaps, bool term, size_t items) {
  StageLayout st;
  OldRule old;
  same<Sixteen>(st, old, nq);
  same<Odd>(st, old, nt > 0 ? nt : 1);
  same<int64_t>(st, old, nq + 1);
  same<int32_t>(st, old, nq);
  same<unsigned long long>(st, old, nq);
  const StageRegion<unsigned> r_done = st.add_if<unsigned>(term_fold, nq);
  const size_t o_done = term_fold ? old.add(nq * 4) : 0;
  const StageRegion<int64_t> r_sp = st.add_if<int64_t>(req_opt, nq + 1);
  const size_t o_sp = req_opt ? old.add((nq + 1) * 8) : 0;
  const StageRegion<Odd> r_bm = st.add_if<Odd>(n_bitmaps > 0, n_bitmaps);
  const size_t o_bm = n_bitmaps > 0 ? old.add(n_bitmaps * sizeof(Odd)) : 0;
  const StageRegion<Sixteen> r_id = st.add_if<Sixteen>(term, items);
  const size_t o_id = term ? old.add(items * sizeof(Sixteen)) : 0;
  CHECK(r_done.off == o_done && r_sp.off == o_sp && r_bm.off == o_bm && r_id.off == o_id && st.used == old.used);
  CHECK(r_done.n == (term_fold ? nq : 0) && r_sp.n == (req_opt ? nq + 1 : 0) && r_bm.n == n_bitmaps && r_id.n == (term ? items : 0));
}

static void view_puts_and_fills() {
  StageLayout st;
  const StageRegion<int32_t> a = st.add<int32_t>(3);
  const StageRegion<int64_t> b = st.add<int64_t>(2);
  const StageRegion<uint8_t> z = st.add<uint8_t>(5);
  const StageRegion<int32_t> none = st.add_if<int32_t>(false, 9);
  std::vector<uint8_t> hbuf(st.used + 64, 0xaa), dbuf(8);
  uint8_t *hp = hbuf.data(), *dp = dbuf.data();
  StageView v;
  v.h = &hp;
  v.d = &dp;
  CHECK(reinterpret_cast<uint8_t*>(v.host(b)) == hp + 256 && reinterpret_cast<uint8_t*>(v.dev(b)) == dp + 256);
  v.put(a, std::vector<int32_t>{1, 2, 3});
  v.put(b, std::vector<int64_t>{7});        // shorter than its region: what it holds, no more
  v.put(b, std::vector<int64_t>{});         // nothing
  v.put(none, std::vector<int32_t>{});      // a region that was left out takes an empty vector
  v.fill(none, 0);
  CHECK(!v.overrun && v.host(a)[2] == 3 && v.host(b)[0] == 7 && hbuf[256 + 8] == 0xaa && hbuf[12] == 0xaa);
  v.fill(st.from(b), 0);                     // from b to the end of the layout: b, the padding behind it, z
  CHECK(v.host(b)[0] == 0 && hbuf[256 + 16] == 0 && hbuf[511] == 0 && v.host(z)[4] == 0 && hbuf[st.used] == 0xaa && hbuf[255] == 0xaa);
  v.fill(z, 0xff);
  CHECK(v.host(z)[0] == 0xff && v.host(z)[4] == 0xff && hbuf[st.used] == 0xaa && hbuf[511] == 0);
  v.put(a, std::vector<int32_t>{9, 9, 9, 9});  // longer than its region: refused whole, nothing written
  CHECK(v.overrun && v.host(a)[0] == 1 && hbuf[12] == 0xaa);
  std::vector<uint8_t> grown(st.used, 0);    // the owner's buffer grew: the view follows the owner's pointer
  hp = grown.data();
  CHECK(reinterpret_cast<uint8_t*>(v.host(a)) == grown.data());
}

int main() {
  mixed_types_and_counts();
  end_marker();
  for (size_t nq : {size_t(1), size_t(31), size_t(32), size_t(64), size_t(1024)})
    for (size_t nt : {size_t(0), size_t(1), size_t(5), size_t(3072)})
      for (int mask = 0; mask < 16; ++mask)
        search_pass_sequence(nq, nt, mask & 1, mask & 2, (mask & 4) ? nt : 0, mask & 8, (mask & 8) ? nq * 3 + 1 : 0);
  view_puts_and_fills();
  if (failures) return 1;
  std::printf("stage_layout OK\n");
  return 0;
}
