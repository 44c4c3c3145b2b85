// tests/emu/emu_octomap_tree.cpp -- TEST INFRASTRUCTURE ONLY: csrc/octomap_tree.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_octomap_tree_kernels.py builds it: the kernel SOURCE of the product runs, one OS
// thread per HIP thread).  The vocabulary the shared header lacks is added here: __float_as_uint, __clzll, and a __shfl_up for
// workgroups of several waves (through the workgroup barrier: every thread of the workgroup must call it, which holds for
// the scans of octomap_tree.hip: a workgroup leaves them whole or not at all).  The radix sort of voxel_filter.hip is built
// on mbcnt and wave barriers and cannot run here: launch_vox_sort is a host stand-in with the same contract.
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include <algorithm>
#include <numeric>

static inline unsigned __float_as_uint(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
static inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }

namespace {
int g_val[1024];
int block_shfl_up(int v, int delta) {  // lane l of a wave takes lane l - delta's value, its own when there is none
  const unsigned t = threadIdx.x;
  g_val[t] = v;
  hipemu_barrier();
  const int r = (t & 63u) >= (unsigned)delta ? g_val[t - (unsigned)delta] : v;
  hipemu_barrier();
  return r;
}
}  // namespace
#define __shfl_up(v, d) block_shfl_up(v, d)

#include "octomap_tree.hip"

namespace rgbdfe {
int launch_vox_sort(uint32_t n, int passes, uint32_t* keys[2], uint32_t* idx[2], uint32_t*, uint32_t*, hipStream_t) {
  const uint32_t mask = passes >= 4 ? 0xffffffffu : (1u << (8 * passes)) - 1u;
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (keys[0][a] & mask) < (keys[0][b] & mask); });
  for (uint32_t i = 0; i < n; ++i) {
    keys[1][i] = keys[0][order[i]];
    idx[1][i] = idx[0][order[i]];
  }
  return 1;
}
}  // namespace rgbdfe

namespace {
struct Work {
  std::vector<unsigned long long> code, scode;
  std::vector<uint32_t> u[13], hist, digits, tile_count, tile_first;
  rgbdfe::TreeHdr hdr{};
  rgbdfe::TreeScratch view(uint32_t n, uint32_t cap) {
    const uint32_t tiles = (std::max(n, cap) + rgbdfe::kTreeTile - 1) / rgbdfe::kTreeTile;
    code.assign(n, 0); scode.assign(n, 0);
    for (auto& v : u) v.assign(n, 0xdeadbeefu);
    digits.assign(256, 0); hist.assign(1, 0); tile_count.assign(tiles, 0); tile_first.assign(tiles + 1, 0);
    hdr = rgbdfe::TreeHdr{};
    rgbdfe::TreeScratch t{};
    t.hdr = &hdr; t.code = code.data(); t.scode = scode.data(); t.slot = u[0].data();
    t.keys[0] = u[1].data(); t.keys[1] = u[2].data(); t.idx[0] = u[3].data(); t.idx[1] = u[4].data();
    t.top = u[5].data(); t.off = u[6].data();
    for (int l = 0; l < 2; ++l) {
      t.level[l].value = reinterpret_cast<float*>(u[7 + 3 * l].data());
      t.level[l].colour = u[8 + 3 * l].data();
      t.level[l].first = u[9 + 3 * l].data();
    }
    t.hist = hist.data(); t.digits = digits.data(); t.tile_count = tile_count.data(); t.tile_first = tile_first.data();
    return t;
  }
};
}  // namespace

// The table (key / value / colour of `cap` slots, n_leaves of them leaves) through the stages as api_octomap.hip drives them:
// the records of the whole tree (records: room for 17 * n_leaves; *n_nodes), then the nodes of `depth` with value >=
// min_log_odds as 16-byte leaf records (level_out: room for n_leaves; *n_level).  counts_out: TreeHdr::cnt of the first run.
extern "C" int emu_octomap_tree(unsigned long long* key, float* value, uint32_t* colour, uint32_t cap, uint32_t n_leaves,
                                void* records, uint32_t* n_nodes, int depth, float min_log_odds, void* level_out, uint32_t* n_level,
                                uint32_t* counts_out) {
  rgbdfe::OctoTable tb{};
  tb.key = key; tb.value = value; tb.colour = colour; tb.mark = nullptr; tb.cap = cap;
  Work w;
  rgbdfe::TreeScratch t = w.view(n_leaves, cap);
  int launches = rgbdfe::launch_tree_leaves(tb, n_leaves, t, nullptr);
  if (w.hdr.cnt[16] != n_leaves) return -1;
  *n_nodes = 0;
  *n_level = 0;
  if (n_leaves == 0) return launches;
  launches += rgbdfe::launch_tree_chain(n_leaves, t, nullptr);
  *n_nodes = w.hdr.n_nodes;
  launches += rgbdfe::launch_tree_levels(n_leaves, 0u, t, records, nullptr);
  memcpy(counts_out, w.hdr.cnt, sizeof(w.hdr.cnt));
  t = w.view(n_leaves, cap);
  rgbdfe::launch_tree_leaves(tb, n_leaves, t, nullptr);
  rgbdfe::launch_tree_levels(n_leaves, (uint32_t)depth, t, nullptr, nullptr);
  rgbdfe::launch_tree_filter(n_leaves, (uint32_t)depth, min_log_odds, t, level_out, nullptr);
  *n_level = w.hdr.n_out;
  return launches;
}
