// tests/emu/emu_render.cpp -- TEST INFRASTRUCTURE ONLY: csrc/render.hip compiled as host C++ over tests/emu/hip/hip_runtime.h
// (tests/test_emu_render_kernels.py builds it: the kernel SOURCE of the product runs, one OS thread per HIP thread).  The kernels
// use no barrier and no wave-level operation, so every one of them runs here.  The groups are formed as api_render.hip forms
// them: consecutive nodes, each group's rows, strip records and node firsts counted from the group's first vertex.
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

// not in the vocabulary: the pixel type and the two atomics render.hip uses (one address space here)
struct uchar4 { unsigned char x, y, z, w; };
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
  }
  return old;
}
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }

#include "render.hip"

// The whole stream as rgbdfe_display_geometry gives it (vertices [n_vertices][4], node_offsets [n_nodes + 1], strips
// [n_strips][2] into the whole stream, node_strip_offsets [n_nodes + 1], node_types [n_nodes]); group_first [n_groups + 1]: the
// first node of every group, then n_nodes.  view / projection column-major.  ids / node_index may be NULL.  stats: NULL, or two
// counters (fragments offered, fragments that lowered a word on arrival) filled by the counting kernels.  Returns the kernel
// launches.
extern "C" int emu_render(int32_t n_nodes, const float* vertices, const int64_t* node_offsets, const int64_t* strips,
                          const int64_t* node_strip_offsets, const int32_t* node_types, int32_t n_groups,
                          const int32_t* group_first, const double* view, const double* projection, int32_t W, int32_t H,
                          int32_t point_n, int32_t cull, const uint8_t* clear_rgba, uint8_t* rgba, float* depth, int64_t* ids,
                          int32_t* node_index, uint64_t* stats) {
  using namespace rgbdfe;
  RenderCamera cam;
  memcpy(cam.view, view, sizeof(cam.view));
  memcpy(cam.proj, projection, sizeof(cam.proj));
  cam.W = W;
  cam.H = H;
  cam.point_n = point_n;
  cam.cull = cull;
  RenderImages img{reinterpret_cast<uchar4*>(rgba), depth, ids, node_index};
  std::vector<unsigned long long> vis((size_t)W * (size_t)H);
  uint32_t queue_count = 77u;  // the clear resets it
  unsigned long long counters[2] = {77ull, 77ull};
  int launches = launch_render_clear(cam, uchar4{clear_rgba[0], clear_rgba[1], clear_rgba[2], clear_rgba[3]}, vis.data(), img,
                                     &queue_count, counters, nullptr);
  for (int32_t gi = 0; gi < n_groups; ++gi) {
    const int32_t k0 = group_first[gi], k1 = group_first[gi + 1];
    const int64_t v0 = node_offsets[k0], v1 = node_offsets[k1], s0 = node_strip_offsets[k0], s1 = node_strip_offsets[k1];
    std::vector<int64_t> first((size_t)(k1 - k0) + 1), recs(2 * (size_t)(s1 - s0) + 2);
    for (int32_t k = k0; k <= k1; ++k) first[(size_t)(k - k0)] = node_offsets[k] - v0;
    for (int64_t s = s0; s < s1; ++s) {
      recs[2 * (size_t)(s - s0)] = strips[2 * s] - v0;
      recs[2 * (size_t)(s - s0) + 1] = strips[2 * s + 1];
    }
    // exact-size copies, so that a read past the group's rows is a read past a heap block
    std::vector<float4> rows((size_t)(v1 - v0));
    if (v1 > v0) memcpy(rows.data(), vertices + 4 * v0, sizeof(float4) * rows.size());
    std::vector<uint32_t> queue((size_t)(v1 - v0));
    RenderGroup g;
    g.vertices = rows.data();
    g.strips = recs.data();
    g.node_first = first.data();
    g.node_type = node_types + k0;
    g.n_vertices = (uint32_t)(v1 - v0);
    g.n_strips = (uint32_t)(s1 - s0);
    g.n_nodes = (uint32_t)(k1 - k0);
    g.node0 = k0;
    g.base = (uint64_t)v0;
    launches += launch_render_group(g, cam, vis.data(), queue.data(), &queue_count, img, 3u, counters, stats != nullptr,
                                    nullptr);  // three workgroups: entries b, b + 3, ...
    if (queue_count != 0u) return -1;  // the shading pass leaves the queue empty for the next group
  }
  if (stats) {
    stats[0] = counters[0];
    stats[1] = counters[1];
  } else if (counters[0] != 0ull || counters[1] != 0ull) {
    return -2;  // the product kernels count nothing
  }
  return launches;
}
