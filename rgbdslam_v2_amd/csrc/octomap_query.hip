// octomap_query.hip -- the read side of the occupancy map on the device, gfx950: OcTreeBaseImpl::search,
// OccupancyOcTreeBase::castRay and the map seen from a camera pose.  The contract is the block "occupancy map: the read
// side" of include/rgbdfe.h; every statement of it is one rounding here (-ffp-contract=off).
//
//   octo_search_kernel  a lane per point: the key, the lookup, the leaf record.
//   octo_cast_kernel    a lane per ray: the origin's cell, the normalised direction, then Amanatides & Woo in double; every
//                       cell reached is looked up (find_slot: linear probing that claims nothing), the value and colour words
//                       are loaded only when the key was found.
//   octo_view_kernel    a lane per pixel: the pixel's ray from the pose, the same walk, one row of the node-cloud format.  A
//                       wave covers an 8 x 8 tile of pixels, not 64 pixels of a row: neighbouring rays have similar lengths
//                       and read the same neighbourhood of the table.
//
// The kernels read the table and write their own output rows: no atomics, no write to the table, no LDS, no cross-lane
// state.  A walk is a chain of dependent loads (the next cell is known only after the comparison of this one), so what
// hides the latency is the number of resident waves, not instruction-level parallelism; the register counts are in
// DESIGN.md 4.25.  The host refuses a table loaded above 3/4 before anything is launched (api_octomap.hip): a missing key
// costs a probe run to the next free slot.
#include "rgbdfe_internal.h"
#include "octomap_table.h"

#include <cfloat>

namespace rgbdfe {

namespace {

// the leaf in slot s, if the slot holds one: the value word is loaded here, after the key was found
__device__ __forceinline__ bool leaf_at(const OctoTable& tb, uint32_t s, float& value) {
  if (s == kNoSlot) return false;
  value = tb.value[s];
  return __float_as_uint(value) != kOctoNoLeaf;
}

// centre of key k as the float the records and clouds carry
__device__ __forceinline__ float centre_of(uint32_t k, double res) { return (float)(((double)((int)k - 32768) + 0.5) * res); }

struct RayEnd {
  int32_t status;
  uint32_t steps;
  uint32_t k0, k1, k2;   // the last cell reached (valid unless BAD_ORIGIN)
  float c0, c1, c2;      // its centre
  float value;           // HIT only
  uint32_t colour;       // HIT only
};

// castRay of the contract: origin o, direction d
__device__ __forceinline__ RayEnd cast_ray(const OctoTable& tb, const OctoQuery& q, float ox, float oy, float oz, float dx, float dy,
                                           float dz) {
  RayEnd r;
  r.status = RGBDFE_OCTOMAP_RAY_BAD_ORIGIN;
  r.steps = 0u;
  r.k0 = r.k1 = r.k2 = 0u;
  r.c0 = r.c1 = r.c2 = 0.0f;
  r.value = 0.0f;
  r.colour = 0u;
  // 1. the origin
  uint32_t k0, k1, k2;
  if (!(finite_bits(ox) && finite_bits(oy) && finite_bits(oz)) || !octo_key(q.inv_res, ox, oy, oz, k0, k1, k2)) return r;
  r.k0 = k0; r.k1 = k1; r.k2 = k2;
  r.c0 = centre_of(k0, q.res); r.c1 = centre_of(k1, q.res); r.c2 = centre_of(k2, q.res);
  // 2. the origin's cell
  {
    const uint32_t s = find_slot(tb, pack_key(k0, k1, k2));
    float v;
    if (leaf_at(tb, s, v)) {
      if (v >= q.occupied) {
        r.status = RGBDFE_OCTOMAP_RAY_HIT;
        r.value = v;
        r.colour = tb.colour[s];
        return r;
      }
    } else if (q.ignore_unknown == 0u) {
      r.status = RGBDFE_OCTOMAP_RAY_UNKNOWN;
      return r;
    }
  }
  // 3. the direction
  r.status = RGBDFE_OCTOMAP_RAY_BAD_DIRECTION;
  const double n = sqrt((double)((dx * dx + dy * dy) + dz * dz));
  if (!(n > 0.0)) return r;
  const float fn = (float)n;
  const float ux = dx / fn, uy = dy / fn, uz = dz / fn;
  if (!(finite_bits(ux) && finite_bits(uy) && finite_bits(uz))) return r;
  const int s0 = ux > 0.0f ? 1 : (ux < 0.0f ? -1 : 0), s1 = uy > 0.0f ? 1 : (uy < 0.0f ? -1 : 0),
            s2 = uz > 0.0f ? 1 : (uz < 0.0f ? -1 : 0);
  if (s0 == 0 && s1 == 0 && s2 == 0) return r;  // an infinite norm: every component divided to zero
  // 4. the walk's set-up
  double tM0 = DBL_MAX, tM1 = DBL_MAX, tM2 = DBL_MAX, tD0 = DBL_MAX, tD1 = DBL_MAX, tD2 = DBL_MAX;
  if (s0 != 0) {
    const double border = ((double)((int)k0 - 32768) + 0.5) * q.res + ((double)s0 * q.res) * 0.5;
    tM0 = (border - (double)ox) / (double)ux;
    tD0 = q.res / fabs((double)ux);
  }
  if (s1 != 0) {
    const double border = ((double)((int)k1 - 32768) + 0.5) * q.res + ((double)s1 * q.res) * 0.5;
    tM1 = (border - (double)oy) / (double)uy;
    tD1 = q.res / fabs((double)uy);
  }
  if (s2 != 0) {
    const double border = ((double)((int)k2 - 32768) + 0.5) * q.res + ((double)s2 * q.res) * 0.5;
    tM2 = (border - (double)oz) / (double)uz;
    tD2 = q.res / fabs((double)uz);
  }
  // 5. the iterations; every one moves one key one cell in a fixed direction or ends the walk, so 3 * 65535 moves are the most
  for (uint32_t step = 0; step < kOctoMaxSteps; ++step) {
    const int dim = tM0 < tM1 ? (tM0 < tM2 ? 0 : 2) : (tM1 < tM2 ? 1 : 2);
    const uint32_t kd = dim == 0 ? k0 : (dim == 1 ? k1 : k2);
    const int sd = dim == 0 ? s0 : (dim == 1 ? s1 : s2);
    if ((sd < 0 && kd == 0u) || (sd > 0 && kd == 65535u)) {
      r.status = RGBDFE_OCTOMAP_RAY_OUT_OF_BOUNDS;
      return r;
    }
    if (dim == 0) { k0 += (uint32_t)s0; tM0 += tD0; r.k0 = k0; r.c0 = centre_of(k0, q.res); }
    else if (dim == 1) { k1 += (uint32_t)s1; tM1 += tD1; r.k1 = k1; r.c1 = centre_of(k1, q.res); }
    else { k2 += (uint32_t)s2; tM2 += tD2; r.k2 = k2; r.c2 = centre_of(k2, q.res); }
    r.steps = step + 1u;
    if (q.max_range2 >= 0.0) {
      const float q0 = r.c0 - ox, q1 = r.c1 - oy, q2 = r.c2 - oz;
      const double s = ((double)(q0 * q0) + (double)(q1 * q1)) + (double)(q2 * q2);
      if (s > q.max_range2) {
        r.status = RGBDFE_OCTOMAP_RAY_OUT_OF_RANGE;
        return r;
      }
    }
    const uint32_t s = find_slot(tb, pack_key(k0, k1, k2));
    float v;
    if (leaf_at(tb, s, v)) {
      if (v >= q.occupied) {
        r.status = RGBDFE_OCTOMAP_RAY_HIT;
        r.value = v;
        r.colour = tb.colour[s];
        return r;
      }
    } else if (q.ignore_unknown == 0u) {
      r.status = RGBDFE_OCTOMAP_RAY_UNKNOWN;
      return r;
    }
  }
  // 6. unreachable by the bounds rule; the loop is finite without that argument
  r.status = RGBDFE_OCTOMAP_RAY_STEP_LIMIT;
  return r;
}

__global__ __launch_bounds__(256) void octo_search_kernel(OctoTable tb, const float* __restrict__ points, uint32_t n, double inv_res,
                                                         int32_t* __restrict__ found, uint4* __restrict__ leaves) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  uint4 rec = make_uint4(0u, 0u, 0u, 0u);  // key[0] | key[1] << 16, key[2], log-odds bits, r | g << 8 | b << 16
  int32_t st = 2;
  uint32_t k0, k1, k2;
  if (finite_bits(x) && finite_bits(y) && finite_bits(z) && octo_key(inv_res, x, y, z, k0, k1, k2)) {
    st = 0;
    rec.x = k0 | (k1 << 16);
    rec.y = k2;
    const uint32_t s = find_slot(tb, pack_key(k0, k1, k2));
    float v;
    if (leaf_at(tb, s, v)) {
      st = 1;
      const uint32_t c = tb.colour[s];
      rec.z = __float_as_uint(v);
      rec.w = ((c >> 16) & 255u) | (c & 0xff00u) | ((c & 255u) << 16);
    }
  }
  found[i] = st;
  leaves[i] = rec;
}

__device__ __forceinline__ void put_hit(rgbdfe_octomap_ray_hit* __restrict__ out, const RayEnd& e) {
  rgbdfe_octomap_ray_hit h;
  h.status = e.status;
  h.steps = e.steps;
  h.key[0] = (uint16_t)e.k0; h.key[1] = (uint16_t)e.k1; h.key[2] = (uint16_t)e.k2;
  h.zero0 = 0;
  h.centre[0] = e.c0; h.centre[1] = e.c1; h.centre[2] = e.c2;
  h.log_odds = e.value;
  h.rgb[0] = (uint8_t)((e.colour >> 16) & 255u); h.rgb[1] = (uint8_t)((e.colour >> 8) & 255u); h.rgb[2] = (uint8_t)(e.colour & 255u);
  h.zero1 = 0;
  *out = h;
}

__global__ __launch_bounds__(256) void octo_cast_kernel(OctoTable tb, const float* __restrict__ origins,
                                                       const float* __restrict__ directions, uint32_t n, OctoQuery q,
                                                       rgbdfe_octomap_ray_hit* __restrict__ hits) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const size_t at = 3 * (size_t)i;
  const RayEnd e = cast_ray(tb, q, origins[at], origins[at + 1], origins[at + 2], directions[at], directions[at + 1], directions[at + 2]);
  put_hit(hits + i, e);
}

// a workgroup is four waves, a wave one 8 x 8 tile: tile = 4 * blockIdx.x + wave, tiles row by row
__global__ __launch_bounds__(256) void octo_view_kernel(OctoTable tb, OctoView w, OctoQuery q, float4* __restrict__ cloud,
                                                       uint8_t* __restrict__ status) {
  const uint32_t tiles_x = (w.cols + 7u) / 8u, tiles_y = (w.rows + 7u) / 8u;
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (tile >= tiles_x * tiles_y) return;
  const uint32_t u = (tile % tiles_x) * 8u + (lane & 7u), v = (tile / tiles_x) * 8u + (lane >> 3);
  if (u >= w.cols || v >= w.rows) return;
  const float x = ((float)u - w.cx) / w.fx, y = ((float)v - w.cy) / w.fy;
  const float dx = (w.R[0] * x + w.R[1] * y) + w.R[2];
  const float dy = (w.R[3] * x + w.R[4] * y) + w.R[5];
  const float dz = (w.R[6] * x + w.R[7] * y) + w.R[8];
  const RayEnd e = cast_ray(tb, q, w.t[0], w.t[1], w.t[2], dx, dy, dz);
  float4 row;
  row.x = row.y = row.z = __uint_as_float(0x7fc00000u);
  row.w = __uint_as_float(0u);
  if (e.status == RGBDFE_OCTOMAP_RAY_HIT) {
    const float q0 = e.c0 - w.t[0], q1 = e.c1 - w.t[1], q2 = e.c2 - w.t[2];
    row.x = (w.R[0] * q0 + w.R[3] * q1) + w.R[6] * q2;
    row.y = (w.R[1] * q0 + w.R[4] * q1) + w.R[7] * q2;
    row.z = (w.R[2] * q0 + w.R[5] * q1) + w.R[8] * q2;
    row.w = __uint_as_float(e.colour & 0x00ffffffu);
  }
  const size_t px = (size_t)v * w.cols + u;
  cloud[px] = row;
  if (status) status[px] = (uint8_t)e.status;
}

inline uint32_t blocks_of(uint32_t n) { return (uint32_t)(((uint64_t)n + 255u) / 256u); }

}  // namespace

void launch_octo_search(const OctoTable& tb, const float* points, uint32_t n, double inv_res, int32_t* found, uint4* leaves,
                        hipStream_t stream) {
  hipLaunchKernelGGL(octo_search_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, tb, points, n, inv_res, found, leaves);
}

void launch_octo_cast(const OctoTable& tb, const float* origins, const float* directions, uint32_t n, const OctoQuery& q,
                      rgbdfe_octomap_ray_hit* hits, hipStream_t stream) {
  hipLaunchKernelGGL(octo_cast_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, tb, origins, directions, n, q, hits);
}

void launch_octo_view(const OctoTable& tb, const OctoView& v, const OctoQuery& q, float4* cloud, uint8_t* status, hipStream_t stream) {
  const uint64_t tiles = (uint64_t)((v.cols + 7u) / 8u) * (uint64_t)((v.rows + 7u) / 8u);
  hipLaunchKernelGGL(octo_view_kernel, dim3((uint32_t)((tiles + 3u) / 4u)), dim3(256), 0, stream, tb, v, q, cloud, status);
}

}  // namespace rgbdfe
