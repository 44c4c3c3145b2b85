// icp.hip -- the ICP fallback on the device, gfx950: filterCloud and icpAlignment (icp.cpp:20-89) for icp_method "icp",
// PCL's point-to-point IterativeClosestPoint with an exact brute-force nearest neighbour.  The contract is the "ICP
// fallback" block of include/rgbdfe.h; tests/icp_oracle.py restates it literally and the bytes must agree.
//
//   compact    count (a tile of 256 rows: how many have a z that is not NaN) -> scan (one workgroup per cloud: the valid rows
//              in front of every tile, the cloud's total).  The list of valid rows is never written out.
//   gather     a lane per sample: the valid row of rank pos[s], found by a search over the tiles' offsets and a count inside
//              one tile (the positions come from the host: they depend on the total alone)
//   nn         a lane per source row, the grid is (source block, job).  Iteration 1 makes the working copy P = G S, a later
//              one applies the previous increment at load and writes P back.  The target's xyz passes through LDS in tiles
//              of 512 rows in ascending order, every lane reads a row as a broadcast; the running strict < minimum keeps
//              the first of equal distances.  Then the seventeen values of the row (zero without a kept pair) are summed over
//              the workgroup's four leaves of 64 rows.
//   finish     one workgroup per job: the second level of the tree over the leaf sums, H, the SVD, the increment, F, the
//              stop rules, the job's record.
//
// A job's record is double-buffered by iteration parity.  Both kernels of an iteration return at once for a job whose
// previous record is `done` (finish copies the record forward), so the host enqueues iterations in chunks and reads the
// records once per chunk.  No atomics, no workgroup waits for another: every hand-off is a kernel boundary, and every loop
// has a bound that is a kernel argument or a field the host wrote before the launch.
#include "icp.h"

#include "tfc_device.h"

namespace rgbdfe {

namespace {

__device__ __forceinline__ bool icp_finite(float v) { return fabsf(v) <= FLT_MAX; }

// map_assembly.hip's point_transformed: ((R0 x + R1 y) + R2 z) + t per row, the fourth word as it is
__device__ __forceinline__ float4 icp_transformed(const float* R, const float* t, const float4& p) {
  float4 o;
  o.x = R[0] * p.x + R[1] * p.y + R[2] * p.z + t[0];
  o.y = R[3] * p.x + R[4] * p.y + R[5] * p.z + t[1];
  o.z = R[6] * p.x + R[7] * p.y + R[8] * p.z + t[2];
  o.w = p.w;
  return o;
}

// the inclusive scan of one value per thread over a workgroup of 256 (Hillis-Steele in LDS, lds[2][256])
__device__ __forceinline__ uint32_t icp_block_scan(uint32_t v, uint32_t* lds) {
  const unsigned t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  unsigned cur = 0;
  for (unsigned d = 1; d < (unsigned)kIcpScanTile; d <<= 1) {
    uint32_t x = lds[cur * kIcpScanTile + t];
    if (t >= d) x += lds[cur * kIcpScanTile + t - d];
    cur ^= 1u;
    lds[cur * kIcpScanTile + t] = x;
    __syncthreads();
  }
  const uint32_t r = lds[cur * kIcpScanTile + t];
  __syncthreads();
  return r;
}

__device__ __forceinline__ bool icp_row_valid(const IcpCloud& c, uint32_t i) {
  if (i >= c.n) return false;
  const float z = c.d[i].z;
  return !(z != z);  // icp.cpp:27
}

// grid (tile, cloud)
__global__ void __launch_bounds__(kIcpScanTile) icp_count_kernel(const IcpCloud* __restrict__ clouds, uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t lds[2 * kIcpScanTile];
  const IcpCloud c = clouds[blockIdx.y];
  const uint32_t row0 = blockIdx.x * (uint32_t)kIcpScanTile;
  if (row0 >= c.n) return;
  const uint32_t incl = icp_block_scan(icp_row_valid(c, row0 + threadIdx.x) ? 1u : 0u, lds);
  if (threadIdx.x == kIcpScanTile - 1) tile_count[c.first_tile + blockIdx.x] = incl;
}

// grid (cloud): tile_first[t] = valid rows in front of tile t of the cloud, n_valid[cloud] = the total
__global__ void __launch_bounds__(kIcpScanTile) icp_scan_kernel(const IcpCloud* __restrict__ clouds, const uint32_t* __restrict__ tile_count,
                                                                uint32_t* __restrict__ tile_first, uint32_t* __restrict__ n_valid) {
  __shared__ uint32_t lds[2 * kIcpScanTile];
  const IcpCloud c = clouds[blockIdx.x];
  const uint32_t n_tiles = (c.n + (uint32_t)kIcpScanTile - 1u) / (uint32_t)kIcpScanTile;
  uint32_t base = 0;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += (uint32_t)kIcpScanTile) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < n_tiles ? tile_count[c.first_tile + t] : 0u;
    const uint32_t incl = icp_block_scan(v, lds);
    if (t < n_tiles) tile_first[c.first_tile + t] = base + (incl - v);
    if (threadIdx.x == kIcpScanTile - 1) lds[0] = incl;
    __syncthreads();
    base += lds[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_valid[blockIdx.x] = base;
}

// grid (sample block, cloud): sample s is the valid row of rank pos[s].  Its tile is the last one with tile_first <= the rank
// (a binary search over the cloud's tiles); inside the tile the valid rows are counted up to it (at most 256 rows).
__global__ void __launch_bounds__(256) icp_gather_kernel(const IcpCloud* __restrict__ clouds, const uint32_t* __restrict__ tile_first) {
  const IcpCloud c = clouds[blockIdx.y];
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= c.n_samples) return;
  const uint32_t rank = c.pos[s];
  const uint32_t n_tiles = (c.n + (uint32_t)kIcpScanTile - 1u) / (uint32_t)kIcpScanTile;
  const uint32_t* __restrict__ first = tile_first + c.first_tile;
  uint32_t lo = 0, hi = n_tiles;   // first[lo] <= rank; the answer is in [lo, hi)
  for (int step = 0; step < 32 && hi - lo > 1u; ++step) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (first[mid] <= rank) lo = mid; else hi = mid;
  }
  uint32_t left = rank - first[lo], row = c.n;
  for (uint32_t i = 0; i < (uint32_t)kIcpScanTile; ++i) {
    const uint32_t r = lo * (uint32_t)kIcpScanTile + i;
    if (icp_row_valid(c, r)) {
      if (left == 0u && row == c.n) row = r;
      if (left > 0u) --left;
    }
  }
  if (row >= c.n) return;   // (a position past the valid rows: the host never makes one)
  float4 p = c.d[row];
  if (c.poison && !(icp_finite(p.x) && icp_finite(p.y))) {
    const float nan = __builtin_nanf("");
    p.x = nan; p.y = nan; p.z = nan;
  }
  c.samples[s] = p;
  if (c.sample_index) c.sample_index[s] = row;
}

// grid (source block, job)
__global__ void __launch_bounds__(kIcpBlock) icp_nn_kernel(const IcpJob* __restrict__ jobs, int32_t k, double maxdist2) {
  __shared__ double sums[kIcpSums][kIcpBlock];
  float4* tile = reinterpret_cast<float4*>(&sums[0][0]);  // the target tile lives in the sums' first 8 KiB: used before them
  static_assert(sizeof(float4) * kIcpTile <= sizeof(double) * kIcpSums * kIcpBlock, "the tile fits into the sums");
  const IcpJob& job = jobs[blockIdx.y];
  const int32_t ns = job.ns, nt = job.nt;
  const int32_t row0 = (int32_t)blockIdx.x * kIcpBlock;
  if (row0 >= ns) return;
  const IcpRecord& prev = job.rec[(k - 1) & 1];
  if (prev.done) return;
  const int tid = (int)threadIdx.x;
  const int32_t i = row0 + tid;
  const bool live = i < ns;
  float4 p;
  p.x = p.y = p.z = p.w = 0.0f;
  if (live) {
    if (k == 1) {
      p = icp_transformed(job.GR, job.Gt, job.S[i]);
    } else {
      p = icp_transformed(prev.R, prev.t, job.P[i]);
    }
    job.P[i] = p;
  }
  float best = __builtin_inff();
  int32_t bj = -1;
  for (int32_t t0 = 0; t0 < nt; t0 += kIcpTile) {
    const int32_t cnt = nt - t0 < kIcpTile ? nt - t0 : kIcpTile;
    __syncthreads();  // the previous tile has been read
    for (int32_t j = tid; j < cnt; j += kIcpBlock) tile[j] = job.T[t0 + j];
    __syncthreads();
#pragma unroll 8
    for (int32_t j = 0; j < cnt; ++j) {
      const float4 q = tile[j];
      const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < best) {
        best = d2;
        bj = t0 + j;
      }
    }
  }
  const bool kept = live && bj >= 0 && !((double)best > maxdist2);
  if (live) {
    job.nn_j[i] = bj;
    job.nn_d2[i] = best;
  }
  double v[kIcpSums];
#pragma unroll
  for (int q = 0; q < kIcpSums; ++q) v[q] = 0.0;
  if (kept) {
    const float4 tq = job.T[bj];
    const double P3[3] = {(double)p.x, (double)p.y, (double)p.z};
    const double T3[3] = {(double)tq.x, (double)tq.y, (double)tq.z};
    v[0] = 1.0;
    v[1] = (double)best;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[2 + a] = P3[a];
      v[5 + a] = T3[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) v[8 + 3 * a + b] = T3[a] * P3[b];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kIcpSums; ++q) sums[q][tid] = v[q];
  __syncthreads();
  const int lane = tid & (kIcpLeaf - 1);
  for (int s = kIcpLeaf / 2; s >= 1; s >>= 1) {
    if (lane < s) {
#pragma unroll
      for (int q = 0; q < kIcpSums; ++q) sums[q][tid] = sums[q][tid] + sums[q][tid + s];
    }
    __syncthreads();
  }
  const int32_t leaves = (ns + kIcpLeaf - 1) / kIcpLeaf;
  const int32_t leaf = i / kIcpLeaf;
  if (lane == 0 && leaf < leaves) {
#pragma unroll
    for (int q = 0; q < kIcpSums; ++q) job.part[(size_t)q * (size_t)leaves + (size_t)leaf] = sums[q][tid];
  }
}

// grid (job), one workgroup of 64
__global__ void __launch_bounds__(kIcpLeaf) icp_finish_kernel(const IcpJob* __restrict__ jobs, int32_t k, IcpStop stop) {
  __shared__ double sums[kIcpSums][kIcpLeaf];
  const IcpJob& job = jobs[blockIdx.x];
  const IcpRecord& prev = job.rec[(k - 1) & 1];
  IcpRecord& cur = job.rec[k & 1];
  const int tid = (int)threadIdx.x;
  if (prev.done) {
    if (tid == 0) cur = prev;
    return;
  }
  const int32_t leaves = (job.ns + kIcpLeaf - 1) / kIcpLeaf;
#pragma unroll
  for (int q = 0; q < kIcpSums; ++q) {
    double acc = 0.0;
    for (int32_t l = tid; l < leaves; l += kIcpLeaf) acc = acc + job.part[(size_t)q * (size_t)leaves + (size_t)l];
    sums[q][tid] = acc;
  }
  __syncthreads();
  for (int s = kIcpLeaf / 2; s >= 1; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int q = 0; q < kIcpSums; ++q) sums[q][tid] = sums[q][tid] + sums[q][tid + s];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  IcpRecord r = prev;
  r.k = k;
  const double cd = sums[0][0];
  const int32_t c = (int32_t)cd;
  r.c = c;
  if (c < 3) {
    r.mse = c > 0 ? sums[1][0] / cd : 0.0;
    r.done = 1;
    r.state = kIcpNoCorrespondences;
    cur = r;
    return;
  }
  const double mse = sums[1][0] / cd;
  Tfc s;
  s.W = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    s.m1[a] = (float)(sums[2 + a][0] / cd);
    s.m2[a] = (float)(sums[5 + a][0] / cd);
#pragma unroll
    for (int b = 0; b < 3; ++b) s.C[3 * a + b] = (float)((sums[8 + 3 * a + b][0] - (sums[5 + a][0] * sums[2 + b][0]) / cd) / cd);
  }
  tfc_get_transformation(s, r.R, r.t);
  // F <- increment * F
  float FR[9], Ft[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
      FR[3 * a + b] = (r.R[3 * a] * prev.FR[b] + r.R[3 * a + 1] * prev.FR[3 + b]) + r.R[3 * a + 2] * prev.FR[6 + b];
    Ft[a] = ((r.R[3 * a] * prev.Ft[0] + r.R[3 * a + 1] * prev.Ft[1]) + r.R[3 * a + 2] * prev.Ft[2]) + r.t[a];
  }
#pragma unroll
  for (int a = 0; a < 9; ++a) r.FR[a] = FR[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) r.Ft[a] = Ft[a];
  r.mse = mse;
  const double cos_angle = 0.5 * ((((double)r.R[0] + (double)r.R[4]) + (double)r.R[8]) - 1.0);
  const double tx = (double)r.t[0], ty = (double)r.t[1], tz = (double)r.t[2];
  const double t2 = (tx * tx + ty * ty) + tz * tz;
  double diff = mse - prev.mse;
  if (diff < 0.0) diff = -diff;
  int32_t state = kIcpRunning;
  if (k >= stop.max_iterations) state = kIcpIterations;
  else if (cos_angle >= 1.0 - stop.transformation_epsilon && t2 <= stop.transformation_epsilon) state = kIcpTransform;
  else if (diff < 1e-12) state = kIcpAbsMse;
  else if (diff / prev.mse < stop.euclidean_fitness_epsilon) state = kIcpRelMse;
  r.state = state;
  r.done = state != kIcpRunning ? 1 : 0;
  cur = r;
}

}  // namespace

int launch_icp_compact(const IcpCloud* clouds, uint32_t n_clouds, uint32_t max_tiles, uint32_t* tile_count, uint32_t* tile_first,
                       uint32_t* n_valid, hipStream_t st) {
  if (n_clouds == 0) return 0;
  int launches = 1;
  if (max_tiles > 0) {
    hipLaunchKernelGGL(icp_count_kernel, dim3(max_tiles, n_clouds), dim3(kIcpScanTile), 0, st, clouds, tile_count);
    ++launches;
  }
  hipLaunchKernelGGL(icp_scan_kernel, dim3(n_clouds), dim3(kIcpScanTile), 0, st, clouds, tile_count, tile_first, n_valid);
  return launches;
}

int launch_icp_gather(const IcpCloud* clouds, uint32_t n_clouds, uint32_t max_samples, const uint32_t* tile_first,
                      hipStream_t st) {
  if (n_clouds == 0 || max_samples == 0) return 0;
  hipLaunchKernelGGL(icp_gather_kernel, dim3((max_samples + 255u) / 256u, n_clouds), dim3(256), 0, st, clouds, tile_first);
  return 1;
}

int launch_icp_nn(const IcpJob* jobs, uint32_t n_jobs, uint32_t max_ns, IcpStop stop, int32_t k, hipStream_t st) {
  const uint32_t blocks = (max_ns + (uint32_t)kIcpBlock - 1u) / (uint32_t)kIcpBlock;
  if (n_jobs == 0 || blocks == 0) return 0;
  hipLaunchKernelGGL(icp_nn_kernel, dim3(blocks, n_jobs), dim3(kIcpBlock), 0, st, jobs, k, stop.maxdist2);
  return 1;
}

int launch_icp_finish(const IcpJob* jobs, uint32_t n_jobs, IcpStop stop, int32_t k, hipStream_t st) {
  if (n_jobs == 0) return 0;
  hipLaunchKernelGGL(icp_finish_kernel, dim3(n_jobs), dim3(kIcpLeaf), 0, st, jobs, k, stop);
  return 1;
}

int launch_icp_iterations(const IcpJob* jobs, uint32_t n_jobs, uint32_t max_ns, IcpStop stop, int32_t first, int32_t count,
                          hipStream_t st) {
  int launches = 0;
  for (int32_t k = first; k < first + count; ++k) {
    launches += launch_icp_nn(jobs, n_jobs, max_ns, stop, k, st);
    launches += launch_icp_finish(jobs, n_jobs, stop, k, st);
  }
  return launches;
}

}  // namespace rgbdfe
