// render.h -- what render.hip (kernels) and api_render.hip (host side) share: the camera, the device view of a group of
// nodes whose display-geometry stream is resident, and the launch functions.  The contract is the "rendering" block of
// include/rgbdfe.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbdfe {

constexpr uint32_t kRenderBlock = 256;        // threads of every workgroup here
constexpr uint32_t kRenderSmallBox = 64;      // a primitive whose box holds at most this many pixels is walked by its own lane
constexpr uint32_t kRenderLargeBlocks = 1024; // workgroups of the second pass on the device at most: each takes entries b, b + grid, ...
constexpr int32_t kRenderMaxSize = 4096;      // W, H at most
constexpr int32_t kRenderMaxPoint = 64;       // the point size is clamped to [1, kRenderMaxPoint]
constexpr double kRenderGuard = 16384.0;      // |x_w|, |y_w| of a drawn triangle's vertices at most
constexpr int64_t kRenderMaxGroup = (int64_t)1 << 30;  // vertices resident at once at most
constexpr unsigned long long kRenderEmpty = ~0ull;     // a pixel nothing has been drawn to

struct RenderCamera {
  double view[16], proj[16];  // column-major
  int32_t W, H;
  int32_t point_n;            // the point size, rounded and clamped
  int32_t cull;
};

// The nodes [node0, node0 + n_nodes) of the call, whose vertex rows [base, base + n_vertices) of the whole stream are in
// `vertices`.  node_first (n_nodes + 1 entries) and the strip records count from the group's first vertex.
struct RenderGroup {
  const float4* vertices;
  const int64_t* strips;      // (first vertex, vertex count) per record, ascending
  const int64_t* node_first;
  const int32_t* node_type;
  uint32_t n_vertices, n_strips, n_nodes;
  int32_t node0;
  uint64_t base;
};

// the images, H x W, row 0 at the top; ids / node_index may be NULL
struct RenderImages {
  uchar4* rgba;
  float* depth;
  int64_t* ids;
  int32_t* node_index;
};

// each returns its number of kernel launches
// vis = kRenderEmpty, the images = background, *queue_count = 0, stats[0] = stats[1] = 0
int launch_render_clear(const RenderCamera& cam, uchar4 clear_rgba, unsigned long long* vis, RenderImages img,
                        uint32_t* queue_count, unsigned long long* stats, hipStream_t st);
// a group's primitives into vis (the lane pass, then the workgroup pass: large_blocks >= 1 workgroups over `queue`, which has
// room for n_vertices entries), then the pixels the group owns into the images; leaves *queue_count = 0.  count
// (diagnostics): the kernels that also add the fragments they offered to stats[0] and those that lowered a word on arrival
// to stats[1].
int launch_render_group(const RenderGroup& g, const RenderCamera& cam, unsigned long long* vis, uint32_t* queue,
                        uint32_t* queue_count, RenderImages img, uint32_t large_blocks, unsigned long long* stats, bool count,
                        hipStream_t st);
inline uint32_t render_large_blocks(uint32_t n_vertices) { return n_vertices < kRenderLargeBlocks ? n_vertices : kRenderLargeBlocks; }

}  // namespace rgbdfe
