// The layout of a staged plan (rgpu_api.hip Stager): several host arrays packed into one pinned buffer that travels to the device
// in one copy. Host-only: no HIP calls, the two buffers are plain pointers their owner sizes.
//
// A region is named once, by element type and count; its bytes on the host side, its address on the device side and the size of a
// copy into it all come from that one handle. Regions start on 256-byte boundaries, in the order they were added.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rucene {

template <typename T> struct StageRegion {  // `n` elements of T at byte `off` of the stage; {0, 0}: a conditional region that was left out
  size_t off = 0, n = 0;
  size_t bytes() const { return n * sizeof(T); }
};

struct StageLayout {
  size_t used = 0;
  size_t add(size_t bytes) {  // raw bytes: for plans that carry their own layout struct to the device (TermPlanLayout)
    used = (used + 255) & ~size_t(255);
    const size_t off = used;
    used += bytes;
    return off;
  }
  template <typename T> StageRegion<T> add(size_t n) { return StageRegion<T>{add(n * sizeof(T)), n}; }  // add<T>(0): the aligned offset, an end marker
  template <typename T> StageRegion<T> add_if(bool wanted, size_t n) { return wanted ? add<T>(n) : StageRegion<T>{}; }
  // everything from a region's first byte to the end of the layout, the padding between regions included
  template <typename T> StageRegion<uint8_t> from(const StageRegion<T>& r) const { return StageRegion<uint8_t>{r.off, used - r.off}; }
};

// The two buffers once both hold a layout's `used` bytes. The base pointers are read at every call, not kept: a view never
// outlives a buffer that grew.
struct StageView {
  uint8_t* const* h = nullptr;
  uint8_t* const* d = nullptr;
  bool overrun = false;  // some put() was refused: its vector was longer than its region
  template <typename T> T* host(const StageRegion<T>& r) const { return reinterpret_cast<T*>(*h + r.off); }
  template <typename T> T* dev(const StageRegion<T>& r) const { return reinterpret_cast<T*>(*d + r.off); }
  // copies v.size() elements at once (an empty vector: nothing); never past the region
  template <typename T> void put(const StageRegion<T>& r, const std::vector<T>& v) {
    if (v.size() > r.n) overrun = true;
    else if (!v.empty()) std::memcpy(host(r), v.data(), v.size() * sizeof(T));
  }
  template <typename T> void fill(const StageRegion<T>& r, int byte) { if (r.n) std::memset(host(r), byte, r.bytes()); }
};

}  // namespace rucene
