// tests/emu/emu_octomap.cpp -- TEST INFRASTRUCTURE ONLY: csrc/octomap.hip compiled as host C++ over tests/emu/hip/hip_runtime.h
// (tests/test_emu_octomap_kernels.py builds it: the kernel SOURCE of the product runs, one OS thread per HIP thread, so the
// 256 lanes of a workgroup race for the table's slots through the compare-and-swap as they do on the device).
// The vocabulary the shared header lacks is added here: 32-bit atomicMax / atomicAdd, the 64-bit compare-and-swap, the
// relaxed atomic load, and a ballot for workgroups of several waves (through the workgroup barrier: every thread of the
// workgroup must call it, which holds for octo_apply_kernel).  The radix sort and the head kernels of voxel_filter.hip are
// built on mbcnt and wave barriers and cannot run here: launch_vox_sort / launch_vox_heads are host stand-ins with the same
// contract (a stable sort by key; the first position of every run of equal keys).
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include <algorithm>
#include <numeric>

static inline unsigned atomicMax(unsigned* p, unsigned v) {
  unsigned old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return old;
}
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long expected, unsigned long long desired) {
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return expected;  // the word before the exchange
}
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, __ATOMIC_SEQ_CST)
#define __HIP_MEMORY_SCOPE_AGENT 0
static inline unsigned __float_as_uint(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

namespace {
int g_pred[1024];
unsigned long long block_ballot(int pred) {
  const unsigned t = threadIdx.x;
  g_pred[t] = pred ? 1 : 0;
  hipemu_barrier();
  unsigned long long m = 0;
  for (unsigned l = 0; l < 64; ++l)
    if ((t & ~63u) + l < blockDim.x && g_pred[(t & ~63u) + l]) m |= 1ull << l;
  hipemu_barrier();
  return m;
}
}  // namespace
#define __ballot(p) block_ballot(p)

#include "octomap.hip"

namespace rgbdfe {
int launch_vox_sort(uint32_t n, int, uint32_t* keys[2], uint32_t* idx[2], uint32_t*, uint32_t*, hipStream_t) {
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[0][a] < keys[0][b]; });
  for (uint32_t i = 0; i < n; ++i) {
    keys[1][i] = keys[0][order[i]];
    idx[1][i] = idx[0][order[i]];
  }
  return 1;
}
void launch_vox_heads(const uint32_t* keys, uint32_t n, uint32_t*, uint32_t*, uint32_t* cell_start, VoxHeader* hdr, hipStream_t) {
  uint32_t cells = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (i == 0 || keys[i] != keys[i - 1]) cell_start[cells++] = i;
  cell_start[cells] = n;
  hdr->n_cells = cells;
}
}  // namespace rgbdfe

namespace {
struct Table {
  std::vector<unsigned long long> key;
  std::vector<uint32_t> value, colour, mark;
  rgbdfe::OctoTable view() {
    rgbdfe::OctoTable t;
    t.key = key.data(); t.value = reinterpret_cast<float*>(value.data()); t.colour = colour.data(); t.mark = mark.data();
    t.cap = (uint32_t)key.size();
    return t;
  }
  explicit Table(uint32_t cap) : key(cap, rgbdfe::kOctoEmptyKey), value(cap, rgbdfe::kOctoNoLeaf), colour(cap, 0xffffffffu), mark(cap, 0u) {}
};
}  // namespace

// n_clouds clouds (cloud k: counts[k] rows of 4 floats behind the earlier ones, transforms + 16 k column-major) into a fresh
// table of `cap` slots through launch_octo_cloud, as api_octomap.hip drives it; rehash != 0: the leaves then move to a table
// of `rehash` slots through launch_octo_rehash.  prm: resolution, max_range, hit, miss, clamp_min, clamp_max.
// out_*: the table's arrays (max(cap, rehash) entries each); ctl_out: overflow, n_done, n_leaves.  Returns the final slots.
extern "C" int emu_octomap(const float* points, const int32_t* counts, int n_clouds, const float* transforms, const double* prm,
                           uint32_t cap, uint32_t rehash, unsigned long long* out_key, uint32_t* out_value, uint32_t* out_colour,
                           uint32_t* ctl_out) {
  Table tb(cap);
  rgbdfe::OctoCtl ctl{};
  uint32_t n_max = 1;
  for (int k = 0; k < n_clouds; ++k) n_max = std::max(n_max, (uint32_t)counts[k]);
  std::vector<uint32_t> k0(n_max), k1(n_max), i0(n_max), i1(n_max), cells(n_max + 1);
  rgbdfe::VoxHeader hdr{};
  rgbdfe::OctoScratch s{};
  s.keys[0] = k0.data(); s.keys[1] = k1.data(); s.idx[0] = i0.data(); s.idx[1] = i1.data();
  s.cell_start = cells.data(); s.hdr = &hdr;
  rgbdfe::OctoCloud oc{};
  oc.res = prm[0]; oc.inv_res = 1.0 / prm[0]; oc.max_range = prm[1];
  oc.hit = (float)prm[2]; oc.miss = (float)prm[3]; oc.clamp_min = (float)prm[4]; oc.clamp_max = (float)prm[5];
  const float4* at = reinterpret_cast<const float4*>(points);
  for (int k = 0; k < n_clouds; ++k) {
    oc.epoch = (uint32_t)k + 1u;
    const float* T = transforms + 16 * k;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) oc.R[r * 3 + c] = T[c * 4 + r];
      oc.t[r] = T[12 + r];
    }
    rgbdfe::launch_octo_cloud(tb.view(), &ctl, at, (uint32_t)counts[k], oc, 4, s, nullptr);
    at += counts[k];
  }
  ctl_out[0] = ctl.overflow; ctl_out[1] = ctl.n_done; ctl_out[2] = ctl.n_leaves;
  Table* fin = &tb;
  Table moved(rehash ? rehash : 1u);
  if (rehash) {
    rgbdfe::OctoCtl c2{};
    rgbdfe::launch_octo_rehash(tb.view(), moved.view(), &c2, nullptr);
    ctl_out[0] |= c2.overflow << 1;
    fin = &moved;
  }
  const size_t n = fin->key.size();
  memcpy(out_key, fin->key.data(), 8 * n);
  memcpy(out_value, fin->value.data(), 4 * n);
  memcpy(out_colour, fin->colour.data(), 4 * n);
  return (int)n;
}
