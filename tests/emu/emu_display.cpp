// tests/emu/emu_display.cpp -- TEST INFRASTRUCTURE ONLY: csrc/display_geometry.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_display_kernels.py builds it: the kernel SOURCE of the product runs, one OS
// thread per HIP thread).  The kernels use workgroup barriers only, so every one of them runs here.  The node table is built
// as api_display.hip builds it, and the call runs as it runs there: count + scan, the sizes, then the write.
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }  // not in the vocabulary

#include "display_geometry.hip"

// clouds[k]: hw[2k] x hw[2k + 1] points.  transforms: n x 16 floats, column-major, or NULL.  totals[2], node_first[2 * (n + 1)]
// (vertices, strip records) are always set; vertices / strips are written when both capacities suffice.  Returns the kernel
// launches, or -1 when a capacity is too small.
extern "C" int emu_display(int32_t n_nodes, const float* const* clouds, const int32_t* hw, const float* transforms,
                           int32_t display_type, int32_t step, double squared_meshing_threshold, double maximum_depth,
                           float* vertices, int64_t vertex_capacity, int64_t* strips, int64_t strip_capacity, int64_t* totals,
                           int64_t* node_first, int32_t* node_types) {
  using namespace rgbdfe;
  const size_t n = (size_t)n_nodes;
  std::vector<DispNode> table(n + 1);
  memset(table.data(), 0, sizeof(DispNode) * (n + 1));
  int64_t tiles = 0, rows = 0;
  bool have_items = false, have_rows = false;
  for (size_t k = 0; k < n; ++k) {
    const int64_t h = hw[2 * k], w = hw[2 * k + 1];
    DispNode& m = table[k];
    m.cloud = reinterpret_cast<const float4*>(clouds[k]);
    m.w = (int32_t)w;
    m.h = (int32_t)h;
    m.type = (h <= 1 || squared_meshing_threshold < 0) ? kDispPoints : display_type;
    m.step = step;
    int64_t items = 0, tile = kDispItemTile;
    if (m.type == kDispPoints) {
      items = w * h;
      m.items_h = (uint32_t)h;
    } else if (m.type == kDispTriangles) {
      items = w >= 2 ? (w - 1) * (h - 1) : 0;
      m.items_h = (uint32_t)(h - 1);
    } else {
      items = (h > step && w > step) ? (h - 1) / step : 0;
      tile = kDispRowTile;
      m.first_row = (uint32_t)rows;
      rows += items;
    }
    m.n_items = (uint32_t)items;
    m.first_tile = (uint32_t)tiles;
    if (items > 0) (m.type == kDispStrip ? have_rows : have_items) = true;
    if (transforms) {
      const float* T = transforms + k * 16;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m.R[r * 3 + c] = T[c * 4 + r];
        m.t[r] = T[12 + r];
      }
    }
    tiles += (items + tile - 1) / tile;
    node_types[k] = m.type;
  }
  table[n].first_tile = (uint32_t)tiles;
  table[n].first_row = (uint32_t)rows;
  const uint32_t n_tiles = (uint32_t)tiles;
  std::vector<uint32_t> tile_node(n_tiles + 1);
  for (size_t k = 0; k < n; ++k)
    for (uint32_t t = table[k].first_tile; t < table[k + 1].first_tile; ++t) tile_node[t] = (uint32_t)k;
  DispParams prm;
  prm.mesh_thresh = (float)squared_meshing_threshold;
  prm.max_depth = (float)maximum_depth;
  prm.transform = transforms ? 1u : 0u;
  std::vector<uint2> tile_count(n_tiles + 1), row_count((size_t)rows + 1);
  std::vector<int64_t> tile_first(2 * ((size_t)n_tiles + 1));
  int launches = launch_display_count_scan(table.data(), tile_node.data(), (uint32_t)n, n_tiles, prm, have_items, have_rows,
                                           tile_count.data(), row_count.data(), tile_first.data(), node_first, nullptr);
  totals[0] = node_first[2 * n];
  totals[1] = node_first[2 * n + 1];
  if (vertex_capacity < totals[0] || strip_capacity < totals[1]) return -1;
  launches += launch_display_write(table.data(), tile_node.data(), n_tiles, prm, have_items, have_rows, row_count.data(),
                                   tile_first.data(), reinterpret_cast<float4*>(vertices), strips, nullptr);
  return launches;
}

// The one-workgroup scan alone over given tile counts (n_tiles pairs) and the nodes' first tiles (n_nodes + 1 entries, the
// last one n_tiles): tile_first[2 * (n_tiles + 1)], node_first[2 * (n_nodes + 1)].
extern "C" void emu_display_scan(const uint32_t* tile_count, uint32_t n_tiles, const uint32_t* first_tile, uint32_t n_nodes,
                                 int64_t* tile_first, int64_t* node_first) {
  using namespace rgbdfe;
  std::vector<DispNode> table((size_t)n_nodes + 1);
  memset(table.data(), 0, sizeof(DispNode) * table.size());
  for (uint32_t k = 0; k <= n_nodes; ++k) table[k].first_tile = first_tile[k];
  hipLaunchKernelGGL(disp_scan_kernel, dim3(1), dim3(kDispScanBlock), 0, nullptr, reinterpret_cast<const uint2*>(tile_count),
                     n_tiles, tile_first, table.data(), n_nodes, node_first);
}
