// device_layout.h -- how the host code lays out one device allocation: every block is requested once, with its byte count, and
// that one request gives its 256-byte aligned offset; the running total is the size to allocate.  No caller adds offsets up.
// Plain C++ (no HIP include): tests/emu/device_layout_main.cpp exercises it on host memory.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rgbdfe_host {

constexpr size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Block {  // a block of a layout: where it starts in the allocation, and the bytes that were asked for
  size_t off = 0, bytes = 0;
};

class DeviceLayout {
 public:
  // a working block: it only takes room
  Block room(size_t bytes) {
    const Block b{total_, bytes};
    total_ += round256(bytes);
    return b;
  }
  // an uploaded block: its bytes (zeros when src is NULL) also go to the staging vector, at the block's own offset.  The
  // vector reaches from offset 0 to the end of the latest uploaded block, padding zeroed, so the uploaded blocks come first
  // and go up in one copy of staged_bytes() from staged()
  Block put(const void* src, size_t bytes) {
    const Block b = room(bytes);
    stage_.resize(total_, 0);
    if (src && bytes) memcpy(stage_.data() + b.off, src, bytes);
    return b;
  }
  size_t total() const { return total_; }
  const char* staged() const { return stage_.data(); }
  size_t staged_bytes() const { return stage_.size(); }
  // an uploaded block's bytes in the staging vector (valid until the next put)
  template <class T> T* staged(Block b) { return reinterpret_cast<T*>(stage_.data() + b.off); }

 private:
  size_t total_ = 0;
  std::vector<char> stage_;
};

// the block in an allocation of the layout's total() bytes at `base`
template <class T> T* at(void* base, Block b) { return reinterpret_cast<T*>(static_cast<char*>(base) + b.off); }

// the workspace of launch_vox_sort for n (key, index) pairs, by the rule at its declaration (rgbdfe_internal.h): two key and
// two index buffers of n words, 256 counters per sort tile, 256 digit totals
constexpr size_t kSortTilePairs = 4096;  // == kVoxSortTile (static_assert in rgbdfe_host.h)
struct SortWorkspace {
  Block keys[2], idx[2], hist, digits;
};
inline SortWorkspace sort_workspace(DeviceLayout& lay, size_t n) {
  SortWorkspace w;
  for (Block& b : w.keys) b = lay.room(4 * n);
  for (Block& b : w.idx) b = lay.room(4 * n);
  w.hist = lay.room(4 * 256 * ((n + kSortTilePairs - 1) / kSortTilePairs));
  w.digits = lay.room(4 * 256);
  return w;
}

}  // namespace rgbdfe_host
