// octomap_table.h -- the read-only side of the occupancy map's table (rgbdfe_internal.h: OctoTable), shared by octomap.hip
// (insertion) and octomap_query.hip (point lookups, ray casts, views): the key rule of include/rgbdfe.h ("occupancy map"),
// the packed key, the home slot and the lookup that claims nothing.  Device code only; every including translation unit
// gets its own copy (anonymous namespace).
#pragma once
#include "rgbdfe_internal.h"

namespace rgbdfe {

namespace {

constexpr uint32_t kNoSlot = 0xffffffffu;

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ bool octo_key1(double inv_res, float v, uint32_t& k) {
  const double f = floor(inv_res * (double)v) + 32768.0;
  if (!(f >= 0.0 && f < 65536.0)) return false;  // NaN too
  k = (uint32_t)f;
  return true;
}
__device__ __forceinline__ bool octo_key(double inv_res, float x, float y, float z, uint32_t& k0, uint32_t& k1, uint32_t& k2) {
  const bool a = octo_key1(inv_res, x, k0), b = octo_key1(inv_res, y, k1), c = octo_key1(inv_res, z, k2);
  return a && b && c;
}
__device__ __forceinline__ unsigned long long pack_key(uint32_t k0, uint32_t k1, uint32_t k2) {
  return (unsigned long long)k0 | ((unsigned long long)k1 << 16) | ((unsigned long long)k2 << 32);
}

__device__ __forceinline__ uint32_t home_slot(unsigned long long key, uint32_t cap) {
  unsigned long long h = key;  // the 64-bit finaliser of MurmurHash3
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return (uint32_t)(((h >> 32) * (unsigned long long)cap) >> 32);  // < cap
}

// the slot of `key` if it is there (no kernel claims keys while this runs)
__device__ __forceinline__ uint32_t find_slot(const OctoTable& tb, unsigned long long key) {
  uint32_t i = home_slot(key, tb.cap);
  for (uint32_t probe = 0; probe < tb.cap; ++probe) {
    const unsigned long long k = tb.key[i];
    if (k == key) return i;
    if (k == kOctoEmptyKey) return kNoSlot;
    i = i + 1u == tb.cap ? 0u : i + 1u;
  }
  return kNoSlot;
}

}  // namespace

}  // namespace rgbdfe
