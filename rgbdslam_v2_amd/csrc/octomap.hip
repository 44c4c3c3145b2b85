// octomap.hip -- ColorOctomapServer::insertCloudCallback (ColorOctomapServer.cpp:61-129) on the device, gfx950: one cloud
// ray-cast into the leaves (depth 16) of an occupancy map.  The contract is the "occupancy map" block of include/rgbdfe.h;
// every statement of it is one rounding here (-ffp-contract=off).
//
//   octo_ray_kernel     a lane per point: the transform, the range rule, the two keys, then Amanatides & Woo in double.  Every
//                       visited cell is found or claimed in the table (a 64-bit compare-and-swap on the key word, linear
//                       probing, at most `cap` probes: a lane never waits for another) and marked with an integer
//                       atomicMax(mark, 2 * epoch + occupied): "occupied wins" is the maximum, a set and not an order.
//                       A lane keeps its ray from start to end.  (A wave-level queue of rays would even out the 2x spread of
//                       ray lengths inside a wave; it was not built: the fixed assignment has no cross-lane state to get
//                       wrong, and nothing has been measured yet that says the spread matters -- DESIGN.md 4.19.)
//   octo_apply_kernel   a lane per slot: a slot whose mark carries this epoch takes its one update; a claimed key becomes a
//                       leaf here (0, white) and is counted.  Thread 0 counts the cloud as done.
//   octo_colour_keys_kernel  a lane per point: (slot of the leaf at the point's key, point index), `cap` for a point that
//                       contributes no colour.  The slot stands for the cell: it is unique per key, so the 32-bit stable sort
//                       of voxel_filter.hip groups the rows by cell with the index order kept inside.
//   launch_vox_sort, launch_vox_heads   (voxel_filter.hip, unchanged)
//   octo_colour_kernel  a lane per cell: averageNodeColor over its rows in index order.
//   octo_rehash_kernel  the leaves of one table into another (reserve, and the tidy-up after a cloud that did not fit).
//
// A key that finds no slot sets ctl->overflow.  The apply / colour kernels of that cloud and every kernel of a later cloud
// read the flag and change nothing: the map is then the map after ctl->n_done clouds, without a host read in between.
// Which slot a key lands in depends on arrival; nothing that leaves the device does (the leaves go out sorted by key).
// No float atomics, no workgroup waits for another, the launches of a cloud do not depend on its size.
#include "rgbdfe_internal.h"
#include "octomap_table.h"

#include <cfloat>

namespace rgbdfe {

namespace {

// the world-frame point of a row; false: the row contributes nothing
__device__ __forceinline__ bool octo_point(const float4& p, const OctoCloud& c, float& x, float& y, float& z) {
  if (!(finite_bits(p.x) && finite_bits(p.y) && finite_bits(p.z))) return false;
  x = ((c.R[0] * p.x + c.R[1] * p.y) + c.R[2] * p.z) + c.t[0];
  y = ((c.R[3] * p.x + c.R[4] * p.y) + c.R[5] * p.z) + c.t[1];
  z = ((c.R[6] * p.x + c.R[7] * p.y) + c.R[8] * p.z) + c.t[2];
  return finite_bits(x) && finite_bits(y) && finite_bits(z);
}

// the slot of `key`, claimed if it has none; kNoSlot when `cap` probes found neither the key nor a free slot
// (or, on a long probe sequence, when another lane has already raised the overflow flag: the cloud changes nothing then, and
// a table that is full must not keep every lane of the kernel scanning it from end to end)
__device__ __forceinline__ uint32_t find_or_claim(const OctoTable& tb, OctoCtl* ctl, unsigned long long key) {
  uint32_t i = home_slot(key, tb.cap);
  for (uint32_t probe = 0; probe < tb.cap; ++probe) {
    if ((probe & 255u) == 255u && __hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
    unsigned long long k = __hip_atomic_load(&tb.key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kOctoEmptyKey) k = atomicCAS(&tb.key[i], kOctoEmptyKey, key);  // the word before the exchange
    if (k == key || k == kOctoEmptyKey) return i;
    i = i + 1u == tb.cap ? 0u : i + 1u;
  }
  return kNoSlot;
}

__device__ __forceinline__ bool touch(const OctoTable& tb, OctoCtl* ctl, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t mark) {
  const uint32_t s = find_or_claim(tb, ctl, pack_key(k0, k1, k2));
  if (s == kNoSlot) {
    atomicMax(&ctl->overflow, 1u);
    return false;
  }
  atomicMax(&tb.mark[s], mark);
  return true;
}

__global__ __launch_bounds__(256) void octo_ray_kernel(OctoTable tb, OctoCtl* __restrict__ ctl, const float4* __restrict__ pts,
                                                      uint32_t n, OctoCloud c) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  if (__hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
  float px, py, pz;
  if (!octo_point(pts[i], c, px, py, pz)) return;
  const float ox = c.t[0], oy = c.t[1], oz = c.t[2];
  const uint32_t free_mark = 2u * c.epoch, occ_mark = free_mark + 1u;

  // computeUpdate: the end of the ray, and whether its cell is occupied
  float ex = px, ey = py, ez = pz;
  {
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    const double norm = sqrt((double)((dx * dx + dy * dy) + dz * dz));
    if (c.max_range < 0.0 || norm <= c.max_range) {
      uint32_t k0, k1, k2;
      if (octo_key(c.inv_res, px, py, pz, k0, k1, k2) && !touch(tb, ctl, k0, k1, k2, occ_mark)) return;
    } else {
      const float fn = (float)norm, fm = (float)c.max_range;
      ex = ox + (dx / fn) * fm;
      ey = oy + (dy / fn) * fm;
      ez = oz + (dz / fn) * fm;
    }
  }

  // computeRayKeys(origin, end)
  uint32_t k0, k1, k2, e0, e1, e2;
  if (!octo_key(c.inv_res, ox, oy, oz, k0, k1, k2) || !octo_key(c.inv_res, ex, ey, ez, e0, e1, e2)) return;
  if (k0 == e0 && k1 == e1 && k2 == e2) return;
  if (!touch(tb, ctl, k0, k1, k2, free_mark)) return;
  const float dx = ex - ox, dy = ey - oy, dz = ez - oz;
  const float length = (float)sqrt((double)((dx * dx + dy * dy) + dz * dz));
  const float ux = dx / length, uy = dy / length, uz = dz / length;
  const int s0 = ux > 0.0f ? 1 : (ux < 0.0f ? -1 : 0), s1 = uy > 0.0f ? 1 : (uy < 0.0f ? -1 : 0),
            s2 = uz > 0.0f ? 1 : (uz < 0.0f ? -1 : 0);
  double tM0 = DBL_MAX, tM1 = DBL_MAX, tM2 = DBL_MAX, tD0 = DBL_MAX, tD1 = DBL_MAX, tD2 = DBL_MAX;
  if (s0 != 0) {
    const double border = ((double)((int)k0 - 32768) + 0.5) * c.res + (double)(float)((double)s0 * c.res * 0.5);
    tM0 = (border - (double)ox) / (double)ux;
    tD0 = c.res / fabs((double)ux);
  }
  if (s1 != 0) {
    const double border = ((double)((int)k1 - 32768) + 0.5) * c.res + (double)(float)((double)s1 * c.res * 0.5);
    tM1 = (border - (double)oy) / (double)uy;
    tD1 = c.res / fabs((double)uy);
  }
  if (s2 != 0) {
    const double border = ((double)((int)k2 - 32768) + 0.5) * c.res + (double)(float)((double)s2 * c.res * 0.5);
    tM2 = (border - (double)oz) / (double)uz;
    tD2 = c.res / fabs((double)uz);
  }
  const double dlen = (double)length;
  for (uint32_t step = 0; step < kOctoMaxSteps; ++step) {
    const int dim = tM0 < tM1 ? (tM0 < tM2 ? 0 : 2) : (tM1 < tM2 ? 1 : 2);
    if (dim == 0) { k0 = (k0 + (uint32_t)s0) & 0xffffu; tM0 += tD0; }
    else if (dim == 1) { k1 = (k1 + (uint32_t)s1) & 0xffffu; tM1 += tD1; }
    else { k2 = (k2 + (uint32_t)s2) & 0xffffu; tM2 += tD2; }
    if (k0 == e0 && k1 == e1 && k2 == e2) break;
    const double m12 = tM1 < tM2 ? tM1 : tM2;  // std::min(tMax0, std::min(tMax1, tMax2)); no NaN can be here
    const double dist = tM0 < m12 ? tM0 : m12;
    if (dist > dlen) break;
    if (!touch(tb, ctl, k0, k1, k2, free_mark)) return;
  }
}

__global__ __launch_bounds__(256) void octo_apply_kernel(OctoTable tb, OctoCtl* __restrict__ ctl, OctoCloud c) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (ctl->overflow != 0u) return;  // (set by the ray kernel of this cloud or an earlier one, never from here on)
  if (i == 0) ctl->n_done += 1u;
  bool fresh = false;
  if (i < tb.cap) {
    const uint32_t m = tb.mark[i];
    if ((m >> 1) == c.epoch) {
      float v = tb.value[i];
      fresh = __float_as_uint(v) == kOctoNoLeaf;
      if (fresh) {
        v = 0.0f;
        tb.colour[i] = 0x00ffffffu;
      }
      v = v + ((m & 1u) ? c.hit : c.miss);
      if (v < c.clamp_min) v = c.clamp_min;
      if (v > c.clamp_max) v = c.clamp_max;
      tb.value[i] = v;
    }
  }
  const uint64_t b = __ballot(fresh);
  if ((threadIdx.x & 63u) == 0 && b != 0) atomicAdd(&ctl->n_leaves, (uint32_t)__popcll(b));  // a count
}

__global__ __launch_bounds__(256) void octo_colour_keys_kernel(OctoTable tb, const OctoCtl* __restrict__ ctl,
                                                              const float4* __restrict__ pts, uint32_t n, OctoCloud c,
                                                              uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t slot = tb.cap;
  float x, y, z;
  uint32_t k0, k1, k2;
  if (ctl->overflow == 0u && octo_point(pts[i], c, x, y, z) && octo_key(c.inv_res, x, y, z, k0, k1, k2)) {
    const uint32_t s = find_slot(tb, pack_key(k0, k1, k2));
    if (s != kNoSlot && __float_as_uint(tb.value[s]) != kOctoNoLeaf) slot = s;
  }
  keys[i] = slot;
  idx[i] = i;
}

__global__ __launch_bounds__(256) void octo_colour_kernel(OctoTable tb, const OctoCtl* __restrict__ ctl,
                                                         const float4* __restrict__ pts, const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ idx, const uint32_t* __restrict__ cell_start,
                                                         const VoxHeader* __restrict__ hdr) {
  const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
  if (ctl->overflow != 0u || cell >= hdr->n_cells) return;
  const uint32_t s = cell_start[cell], e = cell_start[cell + 1];
  const uint32_t slot = keys[s];
  if (slot >= tb.cap) return;  // the rows without a leaf
  const uint32_t col = tb.colour[slot];
  uint32_t r = (col >> 16) & 255u, g = (col >> 8) & 255u, b = col & 255u;
  for (uint32_t m = s; m < e; ++m) {
    const uint32_t w = __float_as_uint(pts[idx[m]].w);
    const uint32_t nr = (w >> 16) & 255u, ng = (w >> 8) & 255u, nb = w & 255u;
    if (r != 255u || g != 255u || b != 255u) {  // isColorSet
      r = (r + nr) / 2u; g = (g + ng) / 2u; b = (b + nb) / 2u;
    } else {
      r = nr; g = ng; b = nb;
    }
  }
  tb.colour[slot] = (r << 16) | (g << 8) | b;
}

__global__ __launch_bounds__(256) void octo_rehash_kernel(OctoTable from, OctoTable to, OctoCtl* __restrict__ ctl) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= from.cap) return;
  const unsigned long long key = from.key[i];
  const float v = from.value[i];
  if (key == kOctoEmptyKey || __float_as_uint(v) == kOctoNoLeaf) return;
  const uint32_t s = find_or_claim(to, ctl, key);
  if (s == kNoSlot) {
    atomicMax(&ctl->overflow, 1u);
    return;
  }
  to.value[s] = v;
  to.colour[s] = from.colour[i];
}

// rgbdfe_octomap_set_leaves: a claim pass as octo_rehash_kernel over given leaves.  `to` holds no key when it starts, so a
// key that is met in the table is a repeated one, whichever of its lanes comes second.
__global__ __launch_bounds__(256) void octo_set_leaves_kernel(const OctoLeafIn* __restrict__ src, uint32_t n, OctoTable to,
                                                             OctoCtl* __restrict__ ctl, uint32_t* __restrict__ dup) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const OctoLeafIn in = src[r];
  uint32_t i = home_slot(in.key, to.cap);
  for (uint32_t probe = 0; probe < to.cap; ++probe) {
    unsigned long long k = __hip_atomic_load(&to.key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kOctoEmptyKey) {
      k = atomicCAS(&to.key[i], kOctoEmptyKey, in.key);
      if (k == kOctoEmptyKey) {  // claimed: the slot is this lane's
        to.value[i] = in.value;
        to.colour[i] = in.colour;
        return;
      }
    }
    if (k == in.key) {
      atomicMax(dup, 1u);
      return;
    }
    i = i + 1u == to.cap ? 0u : i + 1u;
  }
  atomicMax(&ctl->overflow, 1u);
}

inline uint32_t blocks_of(uint32_t n) { return (uint32_t)(((uint64_t)n + 255u) / 256u); }

}  // namespace

void launch_octo_cloud(const OctoTable& tb, OctoCtl* ctl, const float4* pts, uint32_t n, const OctoCloud& c, int sort_passes,
                       const OctoScratch& s, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(octo_ray_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, tb, ctl, pts, n, c);
  hipLaunchKernelGGL(octo_apply_kernel, dim3(blocks_of(tb.cap)), dim3(256), 0, stream, tb, ctl, c);
  if (n == 0) return;
  hipLaunchKernelGGL(octo_colour_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, tb, ctl, pts, n, c, s.keys[0], s.idx[0]);
  uint32_t* keys[2] = {s.keys[0], s.keys[1]};
  uint32_t* idx[2] = {s.idx[0], s.idx[1]};
  const int cur = launch_vox_sort(n, sort_passes, keys, idx, s.hist, s.digits, stream);
  launch_vox_heads(keys[cur], n, s.tile_count, s.tile_first, s.cell_start, s.hdr, stream);
  hipLaunchKernelGGL(octo_colour_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, tb, ctl, pts, keys[cur], idx[cur], s.cell_start,
                     s.hdr);
}

void launch_octo_rehash(const OctoTable& from, const OctoTable& to, OctoCtl* ctl, hipStream_t stream) {
  hipLaunchKernelGGL(octo_rehash_kernel, dim3(blocks_of(from.cap)), dim3(256), 0, stream, from, to, ctl);
}

void launch_octo_set_leaves(const OctoLeafIn* src, uint32_t n, const OctoTable& to, OctoCtl* ctl, uint32_t* dup, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(octo_set_leaves_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, src, n, to, ctl, dup);
}

}  // namespace rgbdfe
