// voxel_filter.hip -- a cloud reduced to one centroid per occupied cell of a cubic grid, gfx950.
//
//   Node::reducePointCloud (src/node.cpp:1448-1460): pcl::VoxelGrid<PointXYZRGB>::applyFilter with the filter's defaults,
//   restated in include/rgbdfe.h ("voxel filter").  A point is valid when x, y and z are finite; the others take part in
//   nothing.  The cell of a point: ijk[a] = (int)(floorf(p[a] * inv) - (float)min_b[a]), idx = ijk0 + ijk1 * mul1 + ijk2 * mul2.
//   One output row per occupied cell in ascending idx: the members' x, y, z, r, g, b summed in float in ascending input
//   index, starting from the first member, then divided by (float)count.  Compiled with -ffp-contract=off.
//
//   point passes (tiles of kVoxTile points)
//     vox_stats_kernel    per tile: the bounding box of its valid points and their number
//     vox_finish_kernel   one workgroup: the box of the cloud, the exclusive scan of the tiles' counts -> VoxHeader (read by the host)
//     vox_keys_kernel     the valid points as (key, point index) pairs in index order: rank = tile base + the valid points of
//                         the tile's earlier rounds and waves + mbcnt of the lane's ballot (as map_write_kernel)
//   stable LSD radix sort by key, 8 bits a pass, only the passes the grid needs (tiles of kVoxSortTile pairs)
//     vox_hist_kernel     per tile the digit histogram, stored digit-major: hist[digit * n_tiles + tile]
//     vox_digit_scan_kernel  workgroup d: the exclusive scan of digit d's row over the tiles, and the digit's total
//     vox_scatter_kernel  wave w of a tile owns the pairs [w * 1024, (w + 1) * 1024) in steps of 64.  Rank of a lane = digits in
//                         front of its digit + its digit in earlier tiles + in earlier waves of the tile + in earlier steps of
//                         the wave + its rank among the lanes of the step with the same digit (8 ballots, mbcnt)
//   cells (tiles of kVoxTile sorted pairs)
//     vox_head_count / vox_head_scan / vox_head_write   key[i] != key[i - 1] starts a cell: the cells' first sorted positions,
//                         cell_start[n_cells] = the number of pairs; n_cells -> VoxHeader (the second read by the host)
//     vox_centroid_kernel a lane per cell: one accumulation chain over the members in sorted order = input index order
//
// Every rank comes from position alone.  The only atomics are LDS integer counters whose totals are used, never their
// arrival order; no float atomics; no workgroup waits for another.
#include "rgbdfe_internal.h"

namespace rgbdfe {

namespace {

constexpr uint32_t kRounds = kVoxTile / 256u;       // point p of a tile: round p / 256 of lane p % 256
constexpr uint32_t kSteps = kVoxSortTile / 256u;    // pair q of a wave's quarter of a sort tile: step q / 64 of lane q % 64

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool point_valid(const float4& p) { return finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z); }
__device__ __forceinline__ float lower(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float upper(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Exclusive scan of count[0, n) into first[0, n) by one workgroup of 1024 threads (first may be count); returns the total
// to every thread.
__device__ uint32_t block_scan_1024(const uint32_t* count, uint32_t n, uint32_t* first) {
  __shared__ uint32_t wave_tot[16];
  __shared__ uint32_t base;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < n; t0 += 1024u) {
    const uint32_t t = t0 + tid;
    const uint32_t c = t < n ? count[t] : 0u;
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
    if (t < n) first[t] = base + off + incl - c;
    __syncthreads();
    if (tid == 0) {
      uint32_t s = 0;
      for (int w = 0; w < 16; ++w) s += wave_tot[w];
      base += s;
    }
    __syncthreads();
  }
  return base;
}

__device__ __forceinline__ void load_tile(const float4* __restrict__ pts, uint32_t n, uint32_t tile, float4 (&p)[kRounds],
                                          bool (&ok)[kRounds]) {
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) {
    const uint32_t i = tile * kVoxTile + j * 256u + threadIdx.x;  // n < 2^31: no wrap
    p[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) p[j] = pts[i];
    ok[j] = i < n && point_valid(p[j]);
  }
}

__global__ __launch_bounds__(256) void vox_stats_kernel(const float4* __restrict__ pts, uint32_t n, float* __restrict__ tile_box,
                                                       uint32_t* __restrict__ tile_count) {
  __shared__ float box[4][6];
  __shared__ uint32_t wave_cnt[4];
  const uint32_t tile = blockIdx.x, wv = threadIdx.x >> 6;
  float4 p[kRounds];
  bool ok[kRounds];
  load_tile(pts, n, tile, p, ok);
  float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) {
    if (ok[j]) {
      b[0] = lower(b[0], p[j].x); b[1] = lower(b[1], p[j].y); b[2] = lower(b[2], p[j].z);
      b[3] = upper(b[3], p[j].x); b[4] = upper(b[4], p[j].y); b[5] = upper(b[5], p[j].z);
    }
    c += (uint32_t)__popcll(__ballot(ok[j]));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      b[a] = lower(b[a], __shfl_xor(b[a], d));
      b[3 + a] = upper(b[3 + a], __shfl_xor(b[3 + a], d));
    }
  }
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) box[wv][a] = b[a];
    wave_cnt[wv] = c;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const uint32_t a = threadIdx.x;
    float v = box[0][a];
    for (int w = 1; w < 4; ++w) v = a < 3 ? lower(v, box[w][a]) : upper(v, box[w][a]);
    tile_box[(size_t)tile * 6 + a] = v;
  }
  if (threadIdx.x == 0) tile_count[tile] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

__global__ __launch_bounds__(1024) void vox_finish_kernel(const float* __restrict__ tile_box, const uint32_t* __restrict__ tile_count,
                                                          uint32_t n_tiles, uint32_t* __restrict__ tile_first,
                                                          VoxHeader* __restrict__ hdr) {
  __shared__ float box[16][6];
  const uint32_t tid = threadIdx.x;
  float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (uint32_t t = tid; t < n_tiles; t += 1024u) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      b[a] = lower(b[a], tile_box[(size_t)t * 6 + a]);
      b[3 + a] = upper(b[3 + a], tile_box[(size_t)t * 6 + 3 + a]);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      b[a] = lower(b[a], __shfl_xor(b[a], d));
      b[3 + a] = upper(b[3 + a], __shfl_xor(b[3 + a], d));
    }
  }
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) box[tid >> 6][a] = b[a];
  }
  __syncthreads();
  if (tid < 6) {
    float v = box[0][tid];
    for (int w = 1; w < 16; ++w) v = tid < 3 ? lower(v, box[w][tid]) : upper(v, box[w][tid]);
    if (tid < 3) hdr->min_p[tid] = v; else hdr->max_p[tid - 3] = v;
  }
  const uint32_t total = block_scan_1024(tile_count, n_tiles, tile_first);
  if (tid == 0) {
    tile_first[n_tiles] = total;
    hdr->n_valid = total;
    hdr->n_cells = 0;
  }
}

__global__ __launch_bounds__(256) void vox_keys_kernel(const float4* __restrict__ pts, uint32_t n, VoxGrid g,
                                                      const uint32_t* __restrict__ tile_first, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ idx) {
  __shared__ uint32_t cnt[kRounds][4];  // [round][wave]: the order of the points in the tile
  const uint32_t tile = blockIdx.x, wv = threadIdx.x >> 6;
  float4 p[kRounds];
  bool ok[kRounds];
  load_tile(pts, n, tile, p, ok);
  uint32_t rank[kRounds];
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) {
    const uint64_t m = __ballot(ok[j]);
    rank[j] = lanes_below(m);
    if ((threadIdx.x & 63u) == 0) cnt[j][wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  uint32_t at = tile_first[tile];
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) {
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = cnt[j][w];
      if (w == wv && ok[j]) {
        const int i0 = (int)(floorf(p[j].x * g.inv) - g.min_b[0]);
        const int i1 = (int)(floorf(p[j].y * g.inv) - g.min_b[1]);
        const int i2 = (int)(floorf(p[j].z * g.inv) - g.min_b[2]);
        const uint32_t key = (uint32_t)i0 + (uint32_t)i1 * g.mul1 + (uint32_t)i2 * g.mul2;  // int32 arithmetic, wrapping
        keys[at + rank[j]] = key ^ g.flip;
        idx[at + rank[j]] = tile * kVoxTile + j * 256u + threadIdx.x;
      }
      at += c;
    }
  }
}

__global__ __launch_bounds__(256) void vox_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t n_tiles,
                                                      uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t tile = blockIdx.x;
  h[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < kSteps; ++j) {
    const uint64_t e = (uint64_t)tile * kVoxSortTile + j * 256u + threadIdx.x;
    if (e < n) atomicAdd(&h[(keys[e] >> shift) & 255u], 1u);  // a count: its total is used, not the order of arrival
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * n_tiles + tile] = h[threadIdx.x];
}

__global__ __launch_bounds__(1024) void vox_digit_scan_kernel(uint32_t* __restrict__ hist, uint32_t n_tiles,
                                                              uint32_t* __restrict__ digit_total) {
  uint32_t* row = hist + (size_t)blockIdx.x * n_tiles;
  const uint32_t total = block_scan_1024(row, n_tiles, row);
  if (threadIdx.x == 0) digit_total[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void vox_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in,
                                                         uint32_t n, uint32_t shift, uint32_t n_tiles,
                                                         const uint32_t* __restrict__ hist, const uint32_t* __restrict__ digit_total,
                                                         uint32_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out) {
  __shared__ uint32_t cnt[4][256];  // [wave][digit]: first the wave's count of the digit, then the next free row for it
  __shared__ uint32_t wave_tot[4];
  const uint32_t tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  // thread d: the rows in front of digit d of this tile = smaller digits anywhere + digit d in earlier tiles
  const uint32_t tot = digit_total[tid];
  uint32_t incl = tot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= (uint32_t)d) incl += o;
  }
  if (lane == 63) wave_tot[wv] = incl;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) cnt[w][tid] = 0;
  __syncthreads();
  uint32_t first = incl - tot + hist[(size_t)tid * n_tiles + tile];
  for (uint32_t w = 0; w < wv; ++w) first += wave_tot[w];

  uint32_t k[kSteps], v[kSteps];
  bool act[kSteps];
  const uint64_t e0 = (uint64_t)tile * kVoxSortTile + wv * (kVoxSortTile / 4u) + lane;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) {
    const uint64_t e = e0 + s * 64u;
    act[s] = e < n;
    k[s] = act[s] ? keys_in[e] : 0u;
    v[s] = act[s] ? idx_in[e] : 0u;
    if (act[s]) atomicAdd(&cnt[wv][(k[s] >> shift) & 255u], 1u);  // a count again
  }
  __syncthreads();
  {
    uint32_t at = first;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = cnt[w][tid];
      cnt[w][tid] = at;
      at += c;
    }
  }
  __syncthreads();
  volatile uint32_t* next = cnt[wv];  // this wave's alone from here on; a wave's LDS accesses complete in program order
#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) {
    const uint32_t d = (k[s] >> shift) & 255u;
    uint64_t same = __ballot(act[s]);  // the active lanes of the step with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    const uint32_t rank = lanes_below(same);
    uint32_t pos = 0;
    if (act[s]) pos = next[d] + rank;
    __builtin_amdgcn_wave_barrier();
    if (act[s] && rank == 0) next[d] = pos + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
    if (act[s]) {
      keys_out[pos] = k[s];
      idx_out[pos] = v[s];
    }
  }
}

__device__ __forceinline__ void load_heads(const uint32_t* __restrict__ keys, uint32_t n, uint32_t tile, bool (&head)[kRounds]) {
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) {
    const uint32_t i = tile * kVoxTile + j * 256u + threadIdx.x;
    head[j] = i < n && (i == 0 || keys[i] != keys[i - 1]);
  }
}

__global__ __launch_bounds__(256) void vox_head_count_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                            uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t wave_cnt[4];
  bool head[kRounds];
  load_heads(keys, n, blockIdx.x, head);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) c += (uint32_t)__popcll(__ballot(head[j]));
  if ((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

__global__ __launch_bounds__(1024) void vox_head_scan_kernel(const uint32_t* __restrict__ tile_count, uint32_t n_tiles,
                                                             uint32_t* __restrict__ tile_first, uint32_t n,
                                                             uint32_t* __restrict__ cell_start, VoxHeader* __restrict__ hdr) {
  const uint32_t total = block_scan_1024(tile_count, n_tiles, tile_first);
  if (threadIdx.x == 0) {
    cell_start[total] = n;  // the end of the last cell
    hdr->n_cells = total;
  }
}

__global__ __launch_bounds__(256) void vox_head_write_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                            const uint32_t* __restrict__ tile_first, uint32_t* __restrict__ cell_start) {
  __shared__ uint32_t cnt[kRounds][4];
  const uint32_t tile = blockIdx.x, wv = threadIdx.x >> 6;
  bool head[kRounds];
  load_heads(keys, n, tile, head);
  uint32_t rank[kRounds];
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) {
    const uint64_t m = __ballot(head[j]);
    rank[j] = lanes_below(m);
    if ((threadIdx.x & 63u) == 0) cnt[j][wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  uint32_t at = tile_first[tile];
#pragma unroll
  for (uint32_t j = 0; j < kRounds; ++j) {
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = cnt[j][w];
      if (w == wv && head[j]) cell_start[at + rank[j]] = tile * kVoxTile + j * 256u + threadIdx.x;
      at += c;
    }
  }
}

__global__ __launch_bounds__(256) void vox_centroid_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ idx,
                                                          const uint32_t* __restrict__ cell_start, uint32_t n_cells,
                                                          float4* __restrict__ out, float* __restrict__ zplane) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_cells) return;
  const uint32_t s = cell_start[c], e = cell_start[c + 1];
  float4 p = pts[idx[s]];
  uint32_t w = __float_as_uint(p.w);
  float sx = p.x, sy = p.y, sz = p.z;  // the sums start from the first member, not from 0
  float sr = (float)((w >> 16) & 255u), sg = (float)((w >> 8) & 255u), sb = (float)(w & 255u);
  for (uint32_t m = s + 1; m < e; ++m) {
    p = pts[idx[m]];
    w = __float_as_uint(p.w);
    sx += p.x; sy += p.y; sz += p.z;
    sr += (float)((w >> 16) & 255u); sg += (float)((w >> 8) & 255u); sb += (float)(w & 255u);
  }
  const float cn = (float)(e - s);
  float4 o;
  o.x = sx / cn; o.y = sy / cn; o.z = sz / cn;
  const int r = (int)(sr / cn), g = (int)(sg / cn), b = (int)(sb / cn);
  o.w = __uint_as_float(((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b);
  out[c] = o;
  if (zplane) zplane[c] = o.z;
}

inline uint32_t tiles_of(uint32_t n, uint32_t tile) { return (uint32_t)(((uint64_t)n + tile - 1) / tile); }

}  // namespace

void launch_vox_stats(const float4* pts, uint32_t n, float* tile_box, uint32_t* tile_count, uint32_t* tile_first, VoxHeader* hdr,
                      hipStream_t stream) {
  const uint32_t n_tiles = tiles_of(n, kVoxTile);
  if (n_tiles > 0) hipLaunchKernelGGL(vox_stats_kernel, dim3(n_tiles), dim3(256), 0, stream, pts, n, tile_box, tile_count);
  hipLaunchKernelGGL(vox_finish_kernel, dim3(1), dim3(1024), 0, stream, tile_box, tile_count, n_tiles, tile_first, hdr);
}

void launch_vox_keys(const float4* pts, uint32_t n, const VoxGrid& g, const uint32_t* tile_first, uint32_t* keys, uint32_t* idx,
                     hipStream_t stream) {
  const uint32_t n_tiles = tiles_of(n, kVoxTile);
  if (n_tiles > 0) hipLaunchKernelGGL(vox_keys_kernel, dim3(n_tiles), dim3(256), 0, stream, pts, n, g, tile_first, keys, idx);
}

int launch_vox_sort(uint32_t n, int passes, uint32_t* keys[2], uint32_t* idx[2], uint32_t* hist, uint32_t* digit_total,
                    hipStream_t stream) {
  const uint32_t n_tiles = tiles_of(n, kVoxSortTile);
  int cur = 0;
  if (n_tiles == 0) return cur;
  for (int p = 0; p < passes; ++p, cur ^= 1) {
    const uint32_t shift = 8u * (uint32_t)p;
    hipLaunchKernelGGL(vox_hist_kernel, dim3(n_tiles), dim3(256), 0, stream, keys[cur], n, shift, n_tiles, hist);
    hipLaunchKernelGGL(vox_digit_scan_kernel, dim3(256), dim3(1024), 0, stream, hist, n_tiles, digit_total);
    hipLaunchKernelGGL(vox_scatter_kernel, dim3(n_tiles), dim3(256), 0, stream, keys[cur], idx[cur], n, shift, n_tiles, hist,
                       digit_total, keys[cur ^ 1], idx[cur ^ 1]);
  }
  return cur;
}

void launch_vox_heads(const uint32_t* keys, uint32_t n, uint32_t* tile_count, uint32_t* tile_first, uint32_t* cell_start,
                      VoxHeader* hdr, hipStream_t stream) {
  const uint32_t n_tiles = tiles_of(n, kVoxTile);
  if (n_tiles > 0) hipLaunchKernelGGL(vox_head_count_kernel, dim3(n_tiles), dim3(256), 0, stream, keys, n, tile_count);
  hipLaunchKernelGGL(vox_head_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_count, n_tiles, tile_first, n, cell_start, hdr);
  if (n_tiles > 0) hipLaunchKernelGGL(vox_head_write_kernel, dim3(n_tiles), dim3(256), 0, stream, keys, n, tile_first, cell_start);
}

void launch_vox_centroids(const float4* pts, const uint32_t* idx, const uint32_t* cell_start, uint32_t n_cells, float4* out,
                          float* zplane, hipStream_t stream) {
  if (n_cells == 0) return;
  hipLaunchKernelGGL(vox_centroid_kernel, dim3(tiles_of(n_cells, 256u)), dim3(256), 0, stream, pts, idx, cell_start, n_cells, out,
                     zplane);
}

}  // namespace rgbdfe
