// render.hip -- the display-geometry stream rasterised into images, gfx950: what GL does with the vertex rows in
// GLViewer::paintGL / drawClouds / drawOneCloud (src/glviewer.cpp:291-425) under the state of initializeGL (:195-211).
// The contract is the "rendering" block of include/rgbdfe.h; tests/render_oracle.py restates it literally
// and the bytes must agree.
//
// A visibility buffer: one 64-bit word per pixel, (float32 bits of z_w) << 32 | primitive id, all ones where nothing was
// drawn.  z_w >= 0, so the bits order as the values do and the id breaks ties: an integer atomicMin per fragment makes the
// word -- and with it every image -- independent of the order in which the device meets the primitives.
//   clear   vis and the images
//   small   a lane per vertex row v of the resident group.  The row's node (binary search over the nodes' firsts) says
//           whether v starts a primitive: every row of a POINTS node; rows 0, 3, 6, ... of a TRIANGLES node; every row of a
//           strip record that has two more behind it.  A primitive whose pixel box holds at most kRenderSmallBox pixels is
//           walked by the lane; the others are queued (an atomicAdd on the queue's length; their order does not matter).
//   large   a workgroup per queued primitive, its threads over the box
//   shade   a lane per pixel, 8 x 8 pixels per wave: the pixel's winner, if it is of this group, is set up again and its
//           colour, depth, id and node written.  Behind a kernel boundary, so vis is final for the group's vertices; a later
//           group that wins the pixel again simply overwrites it.
// A fragment loads the word plainly first (a hint: most fragments of a map lose) and the atomic decides.  No float atomics,
// nothing waits on another workgroup, no wave-level operation (tests/emu runs this source on the host).
// Everything behind the float32 world point is double with one rounding per operation (-ffp-contract=off); coverage is
// 64-bit integer arithmetic.
#include "render.h"

#include <float.h>
#include <string.h>

namespace rgbdfe {

namespace {

struct RenderVert {
  double xw, yw, zw, w;
  uint32_t word;
  bool depth_ok;  // w positive and finite, -w <= z <= w
  bool xy_in;     // -w <= x, y <= w
};

__device__ __forceinline__ RenderVert render_vertex(const float4& p, const RenderCamera& c) {
  const double x = p.x, y = p.y, z = p.z;
  double e[4], q[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) e[r] = ((c.view[r] * x + c.view[4 + r] * y) + c.view[8 + r] * z) + c.view[12 + r];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = ((c.proj[r] * e[0] + c.proj[4 + r] * e[1]) + c.proj[8 + r] * e[2]) + c.proj[12 + r] * e[3];
  RenderVert o;
  const double w = q[3];
  o.w = w;
  o.depth_ok = w > 0.0 && w <= DBL_MAX && -w <= q[2] && q[2] <= w;
  o.xy_in = -w <= q[0] && q[0] <= w && -w <= q[1] && q[1] <= w;
  o.xw = (q[0] / w + 1.0) * (double)c.W / 2.0;
  o.yw = (q[1] / w + 1.0) * (double)c.H / 2.0;
  o.zw = q[2] / w / 2.0 + 0.5;
  memcpy(&o.word, &p.w, 4);
  return o;
}

__device__ __forceinline__ int64_t render_min(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t render_max(int64_t a, int64_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t render_float_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

struct RenderPrim {
  int32_t kind;            // 0: nothing, 1: a point, 2: a triangle
  int32_t x0, y0, x1, y1;  // the pixels it may cover (window coordinates, inclusive, inside the viewport)
  uint32_t node;           // of the group
  uint32_t zbits;          // a point's z_w
  int64_t X[3], Y[3];      // a triangle's vertices in 1/256 pixel, counter-clockwise
  double z[3], w[3];
  uint32_t word[3];        // word[0]: a point's colour
};

// the largest k in [0, n) with first[stride * k] <= v (0 when there is none)
__device__ __forceinline__ uint32_t render_owner(const int64_t* __restrict__ first, uint32_t stride, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (first[(size_t)stride * mid] <= (int64_t)v) lo = mid; else hi = mid;
  }
  return lo;
}

// an edge owns the samples on it when it is a left edge (it runs downwards: the interior of a counter-clockwise triangle is
// to its right in the image) or a top edge (horizontal, running to the left): y_w points up
__device__ __forceinline__ bool render_edge_owns(int64_t dx, int64_t dy) { return dy < 0 || (dy == 0 && dx < 0); }

// The primitive that starts at row v of the group, set up; false when v starts none or the primitive draws nothing.
__device__ __forceinline__ bool render_fetch(const RenderGroup& g, const RenderCamera& c, uint32_t v, RenderPrim& pr) {
  pr.kind = 0;
  const uint32_t k = render_owner(g.node_first, 1u, g.n_nodes, v);
  pr.node = k;
  const int32_t type = g.node_type[k];
  if (type == 0) {  // POINTS
    const RenderVert p = render_vertex(g.vertices[v], c);
    if (!(p.depth_ok && p.xy_in)) return false;
    const int32_t n = c.point_n;
    const int32_t sx = (n & 1) ? (int32_t)floor(p.xw) - (n - 1) / 2 : (int32_t)floor(p.xw + 0.5) - n / 2;
    const int32_t sy = (n & 1) ? (int32_t)floor(p.yw) - (n - 1) / 2 : (int32_t)floor(p.yw + 0.5) - n / 2;
    pr.x0 = (int32_t)render_max(sx, 0);
    pr.y0 = (int32_t)render_max(sy, 0);
    pr.x1 = (int32_t)render_min(sx + n - 1, c.W - 1);
    pr.y1 = (int32_t)render_min(sy + n - 1, c.H - 1);
    if (pr.x0 > pr.x1 || pr.y0 > pr.y1) return false;
    pr.zbits = render_float_bits((float)p.zw);
    pr.word[0] = p.word;
    pr.kind = 1;
    return true;
  }
  uint32_t at[3] = {v, v + 1u, v + 2u};
  if (type == 1) {  // TRIANGLES
    const int64_t first = g.node_first[k], end = g.node_first[k + 1];
    if (((int64_t)v - first) % 3 != 0 || (int64_t)v + 2 >= end) return false;
  } else {  // TRIANGLE_STRIP
    if (g.n_strips == 0u) return false;
    const uint32_t r = render_owner(g.strips, 2u, g.n_strips, v);
    const int64_t s = g.strips[2 * (size_t)r], cnt = g.strips[2 * (size_t)r + 1];
    if (s > (int64_t)v || (int64_t)v + 2 >= s + cnt) return false;
    if (((int64_t)v - s) & 1) {  // odd triangles of a strip: (i + 1, i, i + 2)
      at[0] = v + 1u;
      at[1] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const RenderVert p = render_vertex(g.vertices[at[i]], c);
    if (!p.depth_ok || !(fabs(p.xw) <= kRenderGuard) || !(fabs(p.yw) <= kRenderGuard)) return false;
    pr.X[i] = (int64_t)floor(p.xw * 256.0 + 0.5);
    pr.Y[i] = (int64_t)floor(p.yw * 256.0 + 0.5);
    pr.z[i] = p.zw;
    pr.w[i] = p.w;
    pr.word[i] = p.word;
  }
  const int64_t area = (pr.X[1] - pr.X[0]) * (pr.Y[2] - pr.Y[0]) - (pr.Y[1] - pr.Y[0]) * (pr.X[2] - pr.X[0]);
  if (area == 0 || (area < 0 && c.cull)) return false;
  if (area < 0) {  // drawn from behind: vertices 1 and 2 change places
    const int64_t tx = pr.X[1], ty = pr.Y[1];
    const double tz = pr.z[1], tw = pr.w[1];
    const uint32_t tc = pr.word[1];
    pr.X[1] = pr.X[2]; pr.Y[1] = pr.Y[2]; pr.z[1] = pr.z[2]; pr.w[1] = pr.w[2]; pr.word[1] = pr.word[2];
    pr.X[2] = tx; pr.Y[2] = ty; pr.z[2] = tz; pr.w[2] = tw; pr.word[2] = tc;
  }
  const int64_t min_x = render_min(pr.X[0], render_min(pr.X[1], pr.X[2])), max_x = render_max(pr.X[0], render_max(pr.X[1], pr.X[2]));
  const int64_t min_y = render_min(pr.Y[0], render_min(pr.Y[1], pr.Y[2])), max_y = render_max(pr.Y[0], render_max(pr.Y[1], pr.Y[2]));
  // the pixels whose centre 256 p + 128 lies in [min, max] (>> floors)
  const int64_t x0 = render_max((min_x + 127) >> 8, 0), x1 = render_min((max_x - 128) >> 8, (int64_t)c.W - 1);
  const int64_t y0 = render_max((min_y + 127) >> 8, 0), y1 = render_min((max_y - 128) >> 8, (int64_t)c.H - 1);
  if (x0 > x1 || y0 > y1) return false;
  pr.x0 = (int32_t)x0; pr.x1 = (int32_t)x1; pr.y0 = (int32_t)y0; pr.y1 = (int32_t)y1;
  pr.kind = 2;
  return true;
}

// the three edge functions of a triangle at the centre of pixel (px, py); true when the sample is covered
__device__ __forceinline__ bool render_tri_sample(const RenderPrim& t, int32_t px, int32_t py, int64_t e[3]) {
  const int64_t sx = (int64_t)px * 256 + 128, sy = (int64_t)py * 256 + 128;
  bool in = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int a = (i + 1) % 3, b = (i + 2) % 3;
    const int64_t dx = t.X[b] - t.X[a], dy = t.Y[b] - t.Y[a];
    e[i] = dx * (sy - t.Y[a]) - dy * (sx - t.X[a]);
    in = in && (e[i] > 0 || (e[i] == 0 && render_edge_owns(dx, dy)));
  }
  return in;
}

__device__ __forceinline__ float render_tri_depth(const RenderPrim& t, const int64_t e[3]) {
  const double e0 = (double)e[0], e1 = (double)e[1], e2 = (double)e[2];
  return (float)(((e0 * t.z[0] + e1 * t.z[1]) + e2 * t.z[2]) / ((e0 + e1) + e2));
}

// pixel (px, py) of the primitive's box against the visibility buffer.  kStats (diagnostics, rgbdfe_render_fragment_stats): the
// fragments offered and those that lowered the word when they arrived (the second depends on the order of arrival).
template <bool kStats>
__device__ __forceinline__ void render_pixel(const RenderPrim& pr, const RenderCamera& c, int32_t px, int32_t py, uint32_t id,
                                             unsigned long long* vis, uint32_t& tested, uint32_t& won) {
  uint32_t zbits = pr.zbits;
  if (pr.kind == 2) {
    int64_t e[3];
    if (!render_tri_sample(pr, px, py, e)) return;
    zbits = render_float_bits(render_tri_depth(pr, e));
  }
  const size_t pix = (size_t)(c.H - 1 - py) * (size_t)c.W + (size_t)px;
  const unsigned long long word = ((unsigned long long)zbits << 32) | (unsigned long long)id;
  if (kStats) {
    ++tested;
    if (word < vis[pix] && atomicMin(&vis[pix], word) > word) ++won;
  } else {
    if (word < vis[pix]) atomicMin(&vis[pix], word);
  }
}

template <bool kStats>
__device__ __forceinline__ void render_count(unsigned long long* stats, uint32_t tested, uint32_t won) {
  if (kStats) {
    if (tested) atomicAdd(&stats[0], (unsigned long long)tested);
    if (won) atomicAdd(&stats[1], (unsigned long long)won);
  }
}

__global__ __launch_bounds__(kRenderBlock) void render_clear_kernel(RenderCamera c, uchar4 clear_rgba, unsigned long long* __restrict__ vis,
                                                                   RenderImages img, uint32_t* __restrict__ queue_count,
                                                                   unsigned long long* __restrict__ stats) {
  const size_t n = (size_t)c.W * (size_t)c.H, p = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (p == 0) {
    *queue_count = 0u;
    stats[0] = stats[1] = 0ull;
  }
  if (p >= n) return;
  vis[p] = kRenderEmpty;
  img.rgba[p] = clear_rgba;
  img.depth[p] = 1.0f;
  if (img.ids) img.ids[p] = -1;
  if (img.node_index) img.node_index[p] = -1;
}

template <bool kStats>
__global__ __launch_bounds__(kRenderBlock) void render_small_kernel(RenderGroup g, RenderCamera c, unsigned long long* vis,
                                                                   uint32_t* __restrict__ queue, uint32_t* queue_count,
                                                                   unsigned long long* stats) {
  const uint32_t v = blockIdx.x * kRenderBlock + threadIdx.x;
  if (v >= g.n_vertices) return;
  RenderPrim pr;
  if (!render_fetch(g, c, v, pr)) return;
  const uint32_t nx = (uint32_t)(pr.x1 - pr.x0 + 1), ny = (uint32_t)(pr.y1 - pr.y0 + 1);
  if (nx * ny > kRenderSmallBox) {  // at most 4096 x 4096
    queue[atomicAdd(queue_count, 1u)] = v;
    return;
  }
  const uint32_t id = (uint32_t)(g.base + v);
  uint32_t tested = 0, won = 0;
  for (int32_t py = pr.y0; py <= pr.y1; ++py)
    for (int32_t px = pr.x0; px <= pr.x1; ++px) render_pixel<kStats>(pr, c, px, py, id, vis, tested, won);
  render_count<kStats>(stats, tested, won);
}

template <bool kStats>
__global__ __launch_bounds__(kRenderBlock) void render_large_kernel(RenderGroup g, RenderCamera c, unsigned long long* vis,
                                                                   const uint32_t* __restrict__ queue,
                                                                   const uint32_t* __restrict__ queue_count, unsigned long long* stats) {
  const uint32_t n = *queue_count;
  uint32_t tested = 0, won = 0;
  for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
    const uint32_t v = queue[q];
    RenderPrim pr;
    if (!render_fetch(g, c, v, pr)) continue;  // (it was queued, so it draws)
    const uint32_t nx = (uint32_t)(pr.x1 - pr.x0 + 1), np = nx * (uint32_t)(pr.y1 - pr.y0 + 1);
    const uint32_t id = (uint32_t)(g.base + v);
    for (uint32_t i = threadIdx.x; i < np; i += kRenderBlock)
      render_pixel<kStats>(pr, c, pr.x0 + (int32_t)(i % nx), pr.y0 + (int32_t)(i / nx), id, vis, tested, won);
  }
  render_count<kStats>(stats, tested, won);
}

__device__ __forceinline__ uint8_t render_channel(const RenderPrim& t, const double q[3], double den, uint32_t shift) {
  const double c0 = (double)((t.word[0] >> shift) & 255u), c1 = (double)((t.word[1] >> shift) & 255u),
               c2 = (double)((t.word[2] >> shift) & 255u);
  const double v = floor(((q[0] * c0 + q[1] * c1) + q[2] * c2) / den + 0.5);
  return (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

// a workgroup is four waves, a wave one 8 x 8 tile: tile = 4 * blockIdx.x + wave, tiles row by row
__global__ __launch_bounds__(kRenderBlock) void render_shade_kernel(RenderGroup g, RenderCamera c, const unsigned long long* __restrict__ vis,
                                                                   RenderImages img, uint32_t* __restrict__ queue_count) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *queue_count = 0u;  // the next group's queue starts empty
  const uint32_t tiles_x = ((uint32_t)c.W + 7u) / 8u, tiles_y = ((uint32_t)c.H + 7u) / 8u;
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (tile >= tiles_x * tiles_y) return;
  const uint32_t u = (tile % tiles_x) * 8u + (lane & 7u), r = (tile / tiles_x) * 8u + (lane >> 3);
  if (u >= (uint32_t)c.W || r >= (uint32_t)c.H) return;
  const size_t pix = (size_t)r * (size_t)c.W + u;
  const unsigned long long word = vis[pix];
  if (word == kRenderEmpty) return;
  const uint64_t id = word & 0xffffffffull;
  if (id < g.base || id >= g.base + g.n_vertices) return;  // another group's
  RenderPrim pr;
  if (!render_fetch(g, c, (uint32_t)(id - g.base), pr)) return;
  uchar4 o;
  o.w = 255;
  if (pr.kind == 1) {
    o.x = (uint8_t)((pr.word[0] >> 16) & 255u);
    o.y = (uint8_t)((pr.word[0] >> 8) & 255u);
    o.z = (uint8_t)(pr.word[0] & 255u);
  } else {
    int64_t e[3];
    render_tri_sample(pr, (int32_t)u, c.H - 1 - (int32_t)r, e);
    const double q[3] = {(double)e[0] / pr.w[0], (double)e[1] / pr.w[1], (double)e[2] / pr.w[2]};
    const double den = (q[0] + q[1]) + q[2];
    o.x = render_channel(pr, q, den, 16u);
    o.y = render_channel(pr, q, den, 8u);
    o.z = render_channel(pr, q, den, 0u);
  }
  const uint32_t zbits = (uint32_t)(word >> 32);
  float z;
  memcpy(&z, &zbits, 4);
  img.rgba[pix] = o;
  img.depth[pix] = z;
  if (img.ids) img.ids[pix] = (int64_t)id;
  if (img.node_index) img.node_index[pix] = g.node0 + (int32_t)pr.node;
}

}  // namespace

int launch_render_clear(const RenderCamera& cam, uchar4 clear_rgba, unsigned long long* vis, RenderImages img,
                        uint32_t* queue_count, unsigned long long* stats, hipStream_t st) {
  const size_t n = (size_t)cam.W * (size_t)cam.H;
  hipLaunchKernelGGL(render_clear_kernel, dim3((uint32_t)((n + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0, st, cam,
                     clear_rgba, vis, img, queue_count, stats);
  return 1;
}

int launch_render_group(const RenderGroup& g, const RenderCamera& cam, unsigned long long* vis, uint32_t* queue,
                        uint32_t* queue_count, RenderImages img, uint32_t large_blocks, unsigned long long* stats,
                        bool count, hipStream_t st) {
  if (g.n_vertices == 0u) return 0;
  const dim3 small_grid((g.n_vertices + kRenderBlock - 1u) / kRenderBlock), block(kRenderBlock);
  if (count) {
    hipLaunchKernelGGL(render_small_kernel<true>, small_grid, block, 0, st, g, cam, vis, queue, queue_count, stats);
    hipLaunchKernelGGL(render_large_kernel<true>, dim3(large_blocks), block, 0, st, g, cam, vis, queue, queue_count, stats);
  } else {
    hipLaunchKernelGGL(render_small_kernel<false>, small_grid, block, 0, st, g, cam, vis, queue, queue_count, stats);
    hipLaunchKernelGGL(render_large_kernel<false>, dim3(large_blocks), block, 0, st, g, cam, vis, queue, queue_count, stats);
  }
  const uint32_t tiles = (((uint32_t)cam.W + 7u) / 8u) * (((uint32_t)cam.H + 7u) / 8u);
  hipLaunchKernelGGL(render_shade_kernel, dim3((tiles + 3u) / 4u), dim3(kRenderBlock), 0, st, g, cam, vis, img, queue_count);
  return 3;
}

}  // namespace rgbdfe
