// map_assembly.hip -- the resident node clouds as one world-frame cloud, gfx950.
//
//   transformAndAppendPointCloud (src/misc.cpp:183-238, the non-HEMACLOUDS form) over a list of nodes: what
//   GraphManager::saveAllCloudsToFile's loop (src/graph_mgr_io.cpp:529-552) builds before it writes the file.
//
// Per point: the range clip (`squaredEuclideanDistance > max_Depth * max_Depth` in float, only when max_Depth >= 0), the
// NaN skip, `rot * p + trans` in the operation order emm_kernel uses for pcl::transformPointCloud; compiled with
// -ffp-contract=off, so every product and sum is rounded on its own as on the host.
//
// The (node, point) sequence is cut into tiles of kMapTile points that never cross a node: node k owns the tiles
// [first_tile[k], first_tile[k + 1]), the last of them partial.  A workgroup is one tile; it finds its node in a
// tile -> node map that travels in the same upload as the node table.
//   raster mode   map_raster_kernel: one streaming pass, out row = first_point[node] + index in the node.
//   compact mode  map_count_kernel (ballot popcounts, one count per tile) -> map_scan_kernel (one workgroup: exclusive scan
//                 of the counts, the nodes' first rows, the total) -> map_write_kernel (rank of a lane = tile base + the
//                 kept points of the tile's earlier waves, from LDS, + mbcnt of the lane's ballot).
// Order is fixed by position alone: no atomics, nothing waits on another workgroup.  Points move as float4.
#include "rgbdfe_internal.h"

namespace rgbdfe {

namespace {

constexpr uint32_t kWaves = kMapTile / 256u;  // point p of a tile: round p / 256 of lane p % 256

__device__ __forceinline__ bool point_clipped(const float4& p, uint32_t clip_on, float md2) {
  const float sq = (p.x * p.x + p.y * p.y) + p.z * p.z;  // pcl::squaredEuclideanDistance(p, origin)
  return clip_on && sq > md2;                            // misc.cpp:217-218 (a NaN distance is not greater)
}
__device__ __forceinline__ bool point_nan(const float4& p) { return p.x != p.x || p.y != p.y || p.z != p.z; }  // :226
__device__ __forceinline__ float4 point_transformed(const float4& p, const MapNode& nd) {  // :230
  float4 o;
  o.x = nd.R[0] * p.x + nd.R[1] * p.y + nd.R[2] * p.z + nd.t[0];
  o.y = nd.R[3] * p.x + nd.R[4] * p.y + nd.R[5] * p.z + nd.t[1];
  o.z = nd.R[6] * p.x + nd.R[7] * p.y + nd.R[8] * p.z + nd.t[2];
  o.w = p.w;  // the rgb word, bit for bit
  return o;
}

// preserve_raster_on_save: every point keeps its row
__global__ __launch_bounds__(256) void map_raster_kernel(const MapNode* __restrict__ nodes, const uint32_t* __restrict__ tile_node,
                                                        uint32_t clip_on, float md2, float4* __restrict__ out) {
  const uint32_t tile = blockIdx.x;
  const MapNode nd = nodes[tile_node[tile]];
  const uint32_t p0 = (tile - nd.first_tile) * kMapTile + threadIdx.x;
  float4 p[kWaves];
#pragma unroll
  for (uint32_t j = 0; j < kWaves; ++j) {
    const uint32_t i = p0 + j * 256u;
    p[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < nd.n_points) p[j] = nd.cloud[i];
  }
#pragma unroll
  for (uint32_t j = 0; j < kWaves; ++j) {
    const uint32_t i = p0 + j * 256u;
    if (i >= nd.n_points) continue;
    float4 o = p[j];  // `cloud_to_append_to += cloud_in`: a skipped point stays as it is
    if (point_clipped(p[j], clip_on, md2)) {
      o.x = o.y = o.z = __uint_as_float(0x7fc00000u);
    } else if (!point_nan(p[j])) {
      o = point_transformed(p[j], nd);
    }
    out[nd.first_point + (int64_t)i] = o;
  }
}

// kept points of every tile
__global__ __launch_bounds__(256) void map_count_kernel(const MapNode* __restrict__ nodes, const uint32_t* __restrict__ tile_node,
                                                       uint32_t clip_on, float md2, uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t wave_cnt[4];
  const uint32_t tile = blockIdx.x;
  const uint32_t k = tile_node[tile];
  const float4* __restrict__ cloud = nodes[k].cloud;
  const uint32_t n = nodes[k].n_points;
  const uint32_t p0 = (tile - nodes[k].first_tile) * kMapTile + threadIdx.x;
  float4 p[kWaves];
#pragma unroll
  for (uint32_t j = 0; j < kWaves; ++j) {
    const uint32_t i = p0 + j * 256u;
    p[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) p[j] = cloud[i];
  }
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < kWaves; ++j) {
    const bool keep = p0 + j * 256u < n && !point_clipped(p[j], clip_on, md2) && !point_nan(p[j]);
    c += (uint32_t)__popcll(__ballot(keep));
  }
  if ((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[tile] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// one workgroup: tile_first[t] = kept points in front of tile t, tile_first[n_tiles] = the total; then the nodes' first rows
__global__ __launch_bounds__(1024) void map_scan_kernel(const uint32_t* __restrict__ tile_count, uint32_t n_tiles,
                                                        int64_t* __restrict__ tile_first, const MapNode* __restrict__ nodes,
                                                        uint32_t n_nodes, int64_t* __restrict__ node_first) {
  __shared__ uint32_t wave_tot[16];
  __shared__ int64_t base;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 1024u) {
    const uint32_t t = t0 + tid;
    const uint32_t c = t < n_tiles ? tile_count[t] : 0u;
    uint32_t incl = c;  // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t w = 0; w < wv; ++w) off += wave_tot[w];
    if (t < n_tiles) tile_first[t] = base + (int64_t)(off + incl - c);
    __syncthreads();
    if (tid == 0) {
      uint32_t s = 0;
      for (int w = 0; w < 16; ++w) s += wave_tot[w];
      base += (int64_t)s;
    }
    __syncthreads();
  }
  if (tid == 0) tile_first[n_tiles] = base;
  __syncthreads();  // the workgroup's own stores to tile_first are visible to it behind the barrier
  for (uint32_t k = tid; k <= n_nodes; k += 1024u) node_first[k] = tile_first[nodes[k].first_tile];  // nodes[n_nodes]: the sentinel
}

// the kept points of every tile, transformed, at tile_first[tile] + rank
__global__ __launch_bounds__(256) void map_write_kernel(const MapNode* __restrict__ nodes, const uint32_t* __restrict__ tile_node,
                                                       const int64_t* __restrict__ tile_first, uint32_t clip_on, float md2,
                                                       float4* __restrict__ out) {
  __shared__ uint32_t cnt[kWaves][4];  // [round][wave]: the order of the points in the tile
  const uint32_t tile = blockIdx.x;
  const MapNode nd = nodes[tile_node[tile]];
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t p0 = (tile - nd.first_tile) * kMapTile + threadIdx.x;
  float4 p[kWaves];
#pragma unroll
  for (uint32_t j = 0; j < kWaves; ++j) {
    const uint32_t i = p0 + j * 256u;
    p[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < nd.n_points) p[j] = nd.cloud[i];
  }
  bool keep[kWaves];
  uint32_t rank[kWaves];
#pragma unroll
  for (uint32_t j = 0; j < kWaves; ++j) {
    keep[j] = p0 + j * 256u < nd.n_points && !point_clipped(p[j], clip_on, md2) && !point_nan(p[j]);
    const uint64_t m = __ballot(keep[j]);
    rank[j] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if ((threadIdx.x & 63u) == 0) cnt[j][wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  int64_t at = tile_first[tile];
#pragma unroll
  for (uint32_t j = 0; j < kWaves; ++j) {
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = cnt[j][w];
      if (w == wv && keep[j]) out[at + (int64_t)rank[j]] = point_transformed(p[j], nd);
      at += (int64_t)c;
    }
  }
}

}  // namespace

void launch_map_raster(const MapNode* nodes, const uint32_t* tile_node, uint32_t n_tiles, bool clip, float md2, float4* out,
                       hipStream_t stream) {
  if (n_tiles == 0) return;
  hipLaunchKernelGGL(map_raster_kernel, dim3(n_tiles), dim3(256), 0, stream, nodes, tile_node, clip ? 1u : 0u, md2, out);
}

void launch_map_count_scan(const MapNode* nodes, const uint32_t* tile_node, uint32_t n_nodes, uint32_t n_tiles, bool clip,
                           float md2, uint32_t* tile_count, int64_t* tile_first, int64_t* node_first, hipStream_t stream) {
  if (n_tiles > 0)
    hipLaunchKernelGGL(map_count_kernel, dim3(n_tiles), dim3(256), 0, stream, nodes, tile_node, clip ? 1u : 0u, md2, tile_count);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_count, n_tiles, tile_first, nodes, n_nodes, node_first);
}

void launch_map_write(const MapNode* nodes, const uint32_t* tile_node, uint32_t n_tiles, const int64_t* tile_first, bool clip,
                      float md2, float4* out, hipStream_t stream) {
  if (n_tiles == 0) return;
  hipLaunchKernelGGL(map_write_kernel, dim3(n_tiles), dim3(256), 0, stream, nodes, tile_node, tile_first, clip ? 1u : 0u, md2, out);
}

}  // namespace rgbdfe
