// display_geometry.hip -- resident node clouds as GL vertex streams, gfx950.
//
//   GLViewer::pointCloud2GLPoints (src/glviewer.cpp:955-987), pointCloud2GLTriangleList (:989-1042) and pointCloud2GLStrip
//   (:776-906) in the plain form of setGLColor (:91-93), chosen per node as GLViewer::addPointCloud (:693-711) chooses:
//   the sequence of glVertex3f calls of every listed node as rows of (x, y, z, rgb word), and one record per
//   glBegin(GL_TRIANGLE_STRIP).  The contract is the "display geometry" block of include/rgbdfe.h;
//   tests/display_oracle.py restates it literally and the bytes must agree.
//
// All tests are float32 with one rounding per operation (-ffp-contract=off): validXYZ (:44-47), squaredEuclideanDistance
// (:768-773) as (dx*dx + dy*dy) + dz*dz, an IEEE division per test; NaN and inf ratios decide as the comparisons decide.
//
// A node's items are cut into tiles that never cross a node (display_geometry.h):
//   POINTS / TRIANGLES   an item is a point / a cell in the reference's loop order (x outer, y inner): item j is column
//                        j / items_h, row j % items_h.  A tile is 1024 consecutive items, so it emits a contiguous piece of
//                        the stream; its threads read the items row by row over the tile's columns (disp_tile_items).
//   TRIANGLE_STRIP       an item is a visited row (y = r * step): the row's state machine is serial, a lane runs it.  A
//                        tile is 64 rows, one wave.
//   count   every tile's (vertices, strip records); the strip rows' own counts go to row_count, so the machine runs twice
//           in all (count, write) and not three times
//   scan    one workgroup: the exclusive scan of the tiles' counts, the nodes' first vertex / first record, the totals
//   write   a thread's place = tile base + the exclusive scan over the workgroup of the threads' counts (LDS).  Items: the
//           threads leave one slot per vertex in LDS, then a lane is a vertex and the rows go out coalesced.  Strip rows: a
//           lane writes its row's vertices and records as its machine sends them.
// Order is fixed by position alone: no atomics, nothing waits on another workgroup; the scans inside a workgroup are
// Hillis-Steele in LDS behind workgroup barriers (no wave-level operation: tests/emu runs this source on the host).
#include "display_geometry.h"

#include <float.h>

namespace rgbdfe {

namespace {

__device__ __forceinline__ bool disp_finite(float v) { return fabsf(v) <= FLT_MAX; }

// validXYZ (:44-47)
__device__ __forceinline__ bool disp_valid(const float4& p, float max_depth) {
  if (max_depth < p.z) return false;
  return disp_finite(p.z) && disp_finite(p.y) && disp_finite(p.x);
}

// squaredEuclideanDistance (:768-773)
__device__ __forceinline__ float disp_sq(const float4& p1, const float4& p2) {
  const float dx = p1.x - p2.x;
  const float dy = p1.y - p2.y;
  const float dz = p1.z - p2.z;
  return dx * dx + dy * dy + dz * dz;
}

// map_assembly.hip's point_transformed: ((R0 x + R1 y) + R2 z) + t per row, the fourth word as it is
__device__ __forceinline__ float4 disp_transformed(const float4& p, const DispNode& nd) {
  float4 o;
  o.x = nd.R[0] * p.x + nd.R[1] * p.y + nd.R[2] * p.z + nd.t[0];
  o.y = nd.R[3] * p.x + nd.R[4] * p.y + nd.R[5] * p.z + nd.t[1];
  o.z = nd.R[6] * p.x + nd.R[7] * p.y + nd.R[8] * p.z + nd.t[2];
  o.w = p.w;
  return o;
}

// where the vertices of an item go: nowhere (they are counted), or the rows from `at` on
struct DispCount {
  uint32_t nv = 0, ns = 0;
  __device__ __forceinline__ void vertex(const float4&) { ++nv; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void end() { ++ns; }
};
struct DispWrite {
  const DispNode& nd;
  uint32_t transform;
  float4* vertices;
  int64_t* strips;
  int64_t v_at, s_at, strip_first;
  __device__ __forceinline__ void vertex(const float4& p) { vertices[v_at++] = transform ? disp_transformed(p, nd) : p; }
  __device__ __forceinline__ void begin() { strip_first = v_at; }
  __device__ __forceinline__ void end() {
    strips[2 * s_at] = strip_first;
    strips[2 * s_at + 1] = v_at - strip_first;
    ++s_at;
  }
};

// The item in column x, row y of a POINTS node (:975-983) or a TRIANGLES node (:1010-1037): `at` = the index of its point pi; the result says
// what it sends -- POINTS: bit 0 = the point; TRIANGLES: bit 0 = (pi, pl, pj) (:1028), bit 1 = (pi, pk, pl) (:1035), in that order.
__device__ __forceinline__ uint32_t disp_item_code(const DispNode& nd, const DispParams& prm, uint32_t x, uint32_t y, uint32_t& at) {
  const uint32_t w = (uint32_t)nd.w;
  const float4* __restrict__ pc = nd.cloud;
  at = x + y * w;
  const float4 pi = pc[at];  // current point
  if (!disp_valid(pi, prm.max_depth)) return 0u;  // :979, :1016
  if (nd.type == kDispPoints) return 1u;
  const float4 origin = make_float4(0.f, 0.f, 0.f, 0.f);
  const float mesh_thresh = prm.mesh_thresh;
  const float depth = disp_sq(pi, origin);  // :1017
  const float4 pl = pc[at + w + 1];  // one right-down
  if (!disp_valid(pl, prm.max_depth) || disp_sq(pi, pl) / depth > mesh_thresh) return 0u;  // :1020
  uint32_t code = 0;
  const float4 pj = pc[at + 1];  // one right
  if (disp_valid(pj, prm.max_depth) && disp_sq(pi, pj) / depth <= mesh_thresh && disp_sq(pj, pl) / depth <= mesh_thresh)
    code |= 1u;  // :1024-1028
  const float4 pk = pc[at + w];  // one down
  if (disp_valid(pk, prm.max_depth) && disp_sq(pi, pk) / depth <= mesh_thresh && disp_sq(pk, pl) / depth <= mesh_thresh)
    code |= 2u;  // :1032-1035
  return code;
}
__device__ __forceinline__ uint32_t disp_code_vertices(const DispNode& nd, uint32_t code) {
  return nd.type == kDispPoints ? code : 3u * ((code & 1u) + (code >> 1));
}

// The row y of pointCloud2GLStrip's outer loop (:799-897).  Which of the six points around column x a step reads depends on
// the machine's state, and the lanes of a wave are in different states: all six are loaded at the top of the step, in one
// batch and whatever the state, so that a step waits for memory once and not once per branch.  (x - step is clamped to the
// row: a running strip, the only reader of that column, has x >= step.)
template <class Sink>
__device__ __forceinline__ void disp_strip_row(const DispNode& nd, const DispParams& prm, int y, Sink& out) {
  const float4* __restrict__ up = nd.cloud + (size_t)y * (size_t)nd.w;            // the row of `ul`, `ur`
  const float4* __restrict__ lo = nd.cloud + (size_t)(y + nd.step) * (size_t)nd.w;  // the row of `ll`, `lr`
  const int w = nd.w, step = nd.step;
  const float mesh_thresh = prm.mesh_thresh, max_depth = prm.max_depth;
  const float4 origin = make_float4(0.f, 0.f, 0.f, 0.f);
  float depth;
  bool strip_on = false, flip = false;
  for (int x = 0; x < w - step; x += step) {
    const int xm = x >= step ? x - step : x;
    const float4 u0 = up[x], l0 = lo[x], u1 = up[x + step], l1 = lo[x + step], um = up[xm], lm = lo[xm];
    if (!strip_on) {
      const float4 ll = l0;  // one down (lower left corner)
      if (!disp_valid(ll, max_depth)) continue;  // :803
      const float4 ur = u1;  // one right (upper right corner)
      if (!disp_valid(ur, max_depth)) continue;  // :805
      const float4 ul = u0;  // current point
      if (disp_valid(ul, max_depth)) {  // :808
        depth = disp_sq(ul, origin);
        if (disp_sq(ul, ll) / depth <= mesh_thresh && disp_sq(ul, ll) / depth <= mesh_thresh &&  // :810-811, the doubled test
            disp_sq(ur, ll) / depth <= mesh_thresh) {
          out.begin();
          strip_on = true;
          flip = false;
          out.vertex(ul);  // :818-821
        }
      }
      if (!strip_on) {  // :824
        const float4 lr = l1;  // one right-down (lower right)
        if (!disp_valid(lr, max_depth)) {
          x++;  // :829
          continue;
        } else {
          depth = disp_sq(ur, origin);
          if (disp_sq(ur, ll) / depth <= mesh_thresh && disp_sq(lr, ll) / depth <= mesh_thresh &&
              disp_sq(ur, lr) / depth <= mesh_thresh) {  // :833-835
            out.begin();
            strip_on = true;
            flip = true;
          }
        }
      }
      if (strip_on) out.vertex(ll);  // :842-847
      continue;
    } else {
      const float4 ul = flip ? l0 : u0, ul_left = flip ? lm : um;  // :853-854, *(ul-step)
      if (disp_valid(ul, max_depth)) {
        depth = disp_sq(ul, origin);
        if (disp_sq(ul, ul_left) / depth > mesh_thresh) {  // :857
          out.end();
          strip_on = false;
          continue;
        }
        out.vertex(ul);  // :864-867
      } else {
        out.end();
        strip_on = false;
        continue;
      }
      const float4 ll = flip ? u0 : l0, ll_left = flip ? um : lm;  // :875-876, *(ll-step)
      if (disp_valid(ll, max_depth)) {
        depth = disp_sq(ll, origin);
        if (disp_sq(ul, ll) / depth > mesh_thresh || disp_sq(ul, ul_left) / depth > mesh_thresh ||
            disp_sq(ll, ll_left) / depth > mesh_thresh) {  // :879-881
          out.end();
          strip_on = false;
          continue;
        }
        float4 v = ll;
        v.w = ul.w;  // :886, setGLColor(*ul) before ll's glVertex3f
        out.vertex(v);
      } else {
        out.end();
        strip_on = false;
        continue;
      }
    }
  }
  if (strip_on) out.end();  // :896
}

// the inclusive scan of one pair per thread over a workgroup of n threads (Hillis-Steele in LDS, lds[2][n])
__device__ __forceinline__ uint2 disp_block_scan(uint2 v, uint2* lds, uint32_t n) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  uint32_t cur = 0;
  for (uint32_t d = 1; d < n; d <<= 1) {
    uint2 x = lds[cur * n + t];
    if (t >= d) {
      const uint2 o = lds[cur * n + t - d];
      x.x += o.x;
      x.y += o.y;
    }
    cur ^= 1u;
    lds[cur * n + t] = x;
    __syncthreads();
  }
  const uint2 r = lds[cur * n + t];
  __syncthreads();
  return r;
}

// The items of a tile are the range [jb, jb + n) of the node's column-major sequence: some whole columns and a partial one at
// either end.  The threads walk the bounding box of those columns row by row, so neighbouring lanes read neighbouring points
// of a cloud row (the stream's own order would put a whole cloud row between two lanes); f(x, y, item of the tile) is called
// for the items of the box that belong to the tile.
template <class F>
__device__ __forceinline__ void disp_tile_items(const DispNode& nd, uint32_t jb, uint32_t n, F&& f) {
  const uint32_t H = nd.items_h;
  const uint32_t x0 = jb / H, nc = (jb + n - 1u) / H - x0 + 1u;
  const uint32_t nb = nc * H;  // < n + 2 H
  for (uint32_t b = threadIdx.x; b < nb; b += kDispBlock) {
    const uint32_t y = b / nc, x = x0 + (b - y * nc);
    const uint32_t j = x * H + y;
    if (j >= jb && j - jb < n) f(x, y, j - jb);
  }
}

__global__ __launch_bounds__(kDispBlock) void disp_item_count_kernel(const DispNode* __restrict__ nodes,
                                                                    const uint32_t* __restrict__ tile_node, DispParams prm,
                                                                    uint2* __restrict__ tile_count) {
  __shared__ uint2 lds[2 * kDispBlock];
  const uint32_t tile = blockIdx.x;
  const DispNode nd = nodes[tile_node[tile]];
  if (nd.type == kDispStrip) return;
  const uint32_t jb = (tile - nd.first_tile) * kDispItemTile, n = min(kDispItemTile, nd.n_items - jb);
  uint32_t c = 0;
  disp_tile_items(nd, jb, n, [&](uint32_t x, uint32_t y, uint32_t) {
    uint32_t at;
    c += disp_code_vertices(nd, disp_item_code(nd, prm, x, y, at));
  });
  const uint2 incl = disp_block_scan(make_uint2(c, 0u), lds, kDispBlock);
  if (threadIdx.x == kDispBlock - 1) tile_count[tile] = incl;
}

__global__ __launch_bounds__(kDispRowTile) void disp_row_count_kernel(const DispNode* __restrict__ nodes,
                                                                     const uint32_t* __restrict__ tile_node, DispParams prm,
                                                                     uint2* __restrict__ tile_count,
                                                                     uint2* __restrict__ row_count) {
  __shared__ uint2 lds[2 * kDispRowTile];
  const uint32_t tile = blockIdx.x;
  const DispNode nd = nodes[tile_node[tile]];
  if (nd.type != kDispStrip) return;
  const uint32_t r = (tile - nd.first_tile) * kDispRowTile + threadIdx.x;
  DispCount c;
  if (r < nd.n_items) {
    disp_strip_row(nd, prm, (int)r * nd.step, c);
    row_count[nd.first_row + r] = make_uint2(c.nv, c.ns);
  }
  const uint2 incl = disp_block_scan(make_uint2(c.nv, c.ns), lds, kDispRowTile);
  if (threadIdx.x == kDispRowTile - 1) tile_count[tile] = incl;
}

// one workgroup: tile_first[t] = the (vertices, records) in front of tile t, tile_first[n_tiles] = the totals; then the
// nodes' firsts
__global__ __launch_bounds__(kDispScanBlock) void disp_scan_kernel(const uint2* __restrict__ tile_count, uint32_t n_tiles,
                                                                  int64_t* __restrict__ tile_first,
                                                                  const DispNode* __restrict__ nodes, uint32_t n_nodes,
                                                                  int64_t* __restrict__ node_first) {
  __shared__ uint2 lds[2 * kDispScanBlock];
  const uint32_t tid = threadIdx.x;
  int64_t base_v = 0, base_s = 0;  // the same in every thread
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kDispScanBlock) {
    const uint32_t t = t0 + tid;
    const uint2 c = t < n_tiles ? tile_count[t] : make_uint2(0u, 0u);
    const uint2 incl = disp_block_scan(c, lds, kDispScanBlock);
    if (t < n_tiles) {
      tile_first[2 * (size_t)t] = base_v + (int64_t)(incl.x - c.x);
      tile_first[2 * (size_t)t + 1] = base_s + (int64_t)(incl.y - c.y);
    }
    if (tid == kDispScanBlock - 1) lds[0] = incl;
    __syncthreads();
    base_v += (int64_t)lds[0].x;
    base_s += (int64_t)lds[0].y;
    __syncthreads();
  }
  if (tid == 0) {
    tile_first[2 * (size_t)n_tiles] = base_v;
    tile_first[2 * (size_t)n_tiles + 1] = base_s;
  }
  __syncthreads();  // the workgroup's own stores to tile_first are visible to it behind the barrier
  for (uint32_t k = tid; k <= n_nodes; k += kDispScanBlock) {  // nodes[n_nodes]: the sentinel
    const size_t t = nodes[k].first_tile;
    node_first[2 * (size_t)k] = tile_first[2 * t];
    node_first[2 * (size_t)k + 1] = tile_first[2 * t + 1];
  }
}

// Three phases.  The threads work out the tile's items in the order of disp_tile_items and leave each one's code and point
// in LDS.  Then a thread takes kDispPerThread consecutive items in stream order and leaves, for every vertex of the tile, a
// slot in LDS: (item of the tile) << 2 | corner, corner bit 0 = one right, bit 1 = one down (pi 0, pj 1, pk 2, pl 3).  Then a
// lane is a vertex: neighbouring lanes write neighbouring rows, whatever the items sent.
__global__ __launch_bounds__(kDispBlock) void disp_item_write_kernel(const DispNode* __restrict__ nodes,
                                                                    const uint32_t* __restrict__ tile_node, DispParams prm,
                                                                    const int64_t* __restrict__ tile_first,
                                                                    float4* __restrict__ vertices) {
  __shared__ uint2 lds[2 * kDispBlock];
  __shared__ uint32_t item_at[kDispItemTile];
  __shared__ uint8_t item_code[kDispItemTile];
  __shared__ uint16_t slot[6 * kDispItemTile];
  const uint32_t tile = blockIdx.x;
  const DispNode nd = nodes[tile_node[tile]];
  if (nd.type == kDispStrip) return;
  const uint32_t jb = (tile - nd.first_tile) * kDispItemTile, n = min(kDispItemTile, nd.n_items - jb);
  disp_tile_items(nd, jb, n, [&](uint32_t x, uint32_t y, uint32_t l) {
    uint32_t at;
    item_code[l] = (uint8_t)disp_item_code(nd, prm, x, y, at);
    item_at[l] = at;
  });
  __syncthreads();
  const uint32_t l0 = threadIdx.x * kDispPerThread;
  uint32_t code[kDispPerThread], c = 0;
#pragma unroll
  for (uint32_t i = 0; i < kDispPerThread; ++i) {
    code[i] = l0 + i < n ? item_code[l0 + i] : 0u;
    c += disp_code_vertices(nd, code[i]);
  }
  const uint2 incl = disp_block_scan(make_uint2(c, 0u), lds, kDispBlock);
  uint32_t o = incl.x - c;
#pragma unroll
  for (uint32_t i = 0; i < kDispPerThread; ++i) {
    const uint32_t it = (l0 + i) << 2;
    if (nd.type == kDispPoints) {
      if (code[i]) slot[o++] = (uint16_t)it;
    } else {
      if (code[i] & 1u) {  // (pi, pl, pj)
        slot[o] = (uint16_t)it; slot[o + 1] = (uint16_t)(it | 3u); slot[o + 2] = (uint16_t)(it | 1u);
        o += 3;
      }
      if (code[i] & 2u) {  // (pi, pk, pl)
        slot[o] = (uint16_t)it; slot[o + 1] = (uint16_t)(it | 2u); slot[o + 2] = (uint16_t)(it | 3u);
        o += 3;
      }
    }
  }
  __syncthreads();
  const int64_t first = tile_first[2 * (size_t)tile];
  const uint32_t total = (uint32_t)(tile_first[2 * (size_t)tile + 2] - first);  // at most 6 * kDispItemTile
  const float4* __restrict__ pc = nd.cloud;
  for (uint32_t v = threadIdx.x; v < total; v += kDispBlock) {
    const uint32_t s = slot[v];
    const float4 p = pc[item_at[s >> 2] + (s & 1u) + ((s >> 1) & 1u) * (uint32_t)nd.w];
    vertices[first + (int64_t)v] = prm.transform ? disp_transformed(p, nd) : p;
  }
}

__global__ __launch_bounds__(kDispRowTile) void disp_row_write_kernel(const DispNode* __restrict__ nodes,
                                                                     const uint32_t* __restrict__ tile_node, DispParams prm,
                                                                     const uint2* __restrict__ row_count,
                                                                     const int64_t* __restrict__ tile_first,
                                                                     float4* __restrict__ vertices, int64_t* __restrict__ strips) {
  __shared__ uint2 lds[2 * kDispRowTile];
  const uint32_t tile = blockIdx.x;
  const DispNode nd = nodes[tile_node[tile]];
  if (nd.type != kDispStrip) return;
  const uint32_t r = (tile - nd.first_tile) * kDispRowTile + threadIdx.x;
  const uint2 c = r < nd.n_items ? row_count[nd.first_row + r] : make_uint2(0u, 0u);
  const uint2 incl = disp_block_scan(c, lds, kDispRowTile);
  if (c.x == 0) return;  // no vertex, so no glBegin either (behind the last barrier)
  DispWrite out{nd, prm.transform, vertices, strips, tile_first[2 * (size_t)tile] + (int64_t)(incl.x - c.x),
                tile_first[2 * (size_t)tile + 1] + (int64_t)(incl.y - c.y), 0};
  disp_strip_row(nd, prm, (int)r * nd.step, out);
}

}  // namespace

int launch_display_count_scan(const DispNode* nodes, const uint32_t* tile_node, uint32_t n_nodes, uint32_t n_tiles,
                              DispParams prm, bool have_items, bool have_rows, uint2* tile_count, uint2* row_count,
                              int64_t* tile_first, int64_t* node_first, hipStream_t st) {
  int launches = 0;
  if (n_tiles > 0 && have_items) {
    hipLaunchKernelGGL(disp_item_count_kernel, dim3(n_tiles), dim3(kDispBlock), 0, st, nodes, tile_node, prm, tile_count);
    ++launches;
  }
  if (n_tiles > 0 && have_rows) {
    hipLaunchKernelGGL(disp_row_count_kernel, dim3(n_tiles), dim3(kDispRowTile), 0, st, nodes, tile_node, prm, tile_count, row_count);
    ++launches;
  }
  hipLaunchKernelGGL(disp_scan_kernel, dim3(1), dim3(kDispScanBlock), 0, st, tile_count, n_tiles, tile_first, nodes, n_nodes,
                     node_first);
  return launches + 1;
}

int launch_display_write(const DispNode* nodes, const uint32_t* tile_node, uint32_t n_tiles, DispParams prm, bool have_items,
                         bool have_rows, const uint2* row_count, const int64_t* tile_first, float4* vertices,
                         int64_t* strips, hipStream_t st) {
  int launches = 0;
  if (n_tiles > 0 && have_items) {
    hipLaunchKernelGGL(disp_item_write_kernel, dim3(n_tiles), dim3(kDispBlock), 0, st, nodes, tile_node, prm, tile_first, vertices);
    ++launches;
  }
  if (n_tiles > 0 && have_rows) {
    hipLaunchKernelGGL(disp_row_write_kernel, dim3(n_tiles), dim3(kDispRowTile), 0, st, nodes, tile_node, prm, row_count,
                       tile_first, vertices, strips);
    ++launches;
  }
  return launches;
}

}  // namespace rgbdfe
