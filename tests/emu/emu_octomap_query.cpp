// tests/emu/emu_octomap_query.cpp -- TEST INFRASTRUCTURE ONLY: csrc/octomap_query.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_octomap_query_kernels.py builds it: the kernel SOURCE of the product runs, one
// OS thread per HIP thread).  The vocabulary the shared header lacks is added here: the two bit casts.  The kernels use no
// wave-level operation and no atomics.  The table is filled on the host by the rule of the device's claim pass (the home
// slot, then linear probing with a wrap), entry after entry; an entry whose value word is kOctoNoLeaf is a key that was
// claimed and never became a leaf, which the public interface cannot produce.
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

static inline unsigned __float_as_uint(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
static inline float __uint_as_float(unsigned u) { float v; memcpy(&v, &u, 4); return v; }

#include "octomap_query.hip"

namespace {
struct Table {
  std::vector<unsigned long long> key;
  std::vector<uint32_t> value, colour;
  rgbdfe::OctoTable view() {
    rgbdfe::OctoTable t;
    t.key = key.data(); t.value = reinterpret_cast<float*>(value.data()); t.colour = colour.data(); t.mark = nullptr;
    t.cap = (uint32_t)key.size();
    return t;
  }
  // entries: n rows of (key, value bits, colour); false: the table has no free slot left
  Table(const unsigned long long* ekey, const uint32_t* evalue, const uint32_t* ecolour, uint32_t n, uint32_t cap, bool* ok)
      : key(cap, rgbdfe::kOctoEmptyKey), value(cap, rgbdfe::kOctoNoLeaf), colour(cap, 0xffffffffu) {
    *ok = true;
    for (uint32_t r = 0; r < n; ++r) {
      uint32_t i = rgbdfe::home_slot(ekey[r], cap), probe = 0;
      while (probe < cap && key[i] != rgbdfe::kOctoEmptyKey) { i = i + 1u == cap ? 0u : i + 1u; ++probe; }
      if (probe == cap) { *ok = false; return; }
      key[i] = ekey[r]; value[i] = evalue[r]; colour[i] = ecolour[r];
    }
  }
};

rgbdfe::OctoQuery query_of(const double* prm) {  // resolution, max_range, occupied log-odds, ignore_unknown
  rgbdfe::OctoQuery q{};
  q.res = prm[0]; q.inv_res = 1.0 / prm[0];
  q.max_range2 = prm[1] > 0.0 ? prm[1] * prm[1] : -1.0;
  q.occupied = (float)prm[2];
  q.ignore_unknown = prm[3] != 0.0 ? 1u : 0u;
  return q;
}
}  // namespace

extern "C" int emu_octo_search(const unsigned long long* ekey, const uint32_t* evalue, const uint32_t* ecolour, uint32_t n_entries,
                               uint32_t cap, double resolution, const float* points, uint32_t n, int32_t* found, void* leaves) {
  bool ok;
  Table tb(ekey, evalue, ecolour, n_entries, cap, &ok);
  if (!ok) return -1;
  if (n > 0) rgbdfe::launch_octo_search(tb.view(), points, n, 1.0 / resolution, found, static_cast<uint4*>(leaves), nullptr);
  return 0;
}

extern "C" int emu_octo_cast(const unsigned long long* ekey, const uint32_t* evalue, const uint32_t* ecolour, uint32_t n_entries,
                             uint32_t cap, const double* prm, const float* origins, const float* directions, uint32_t n, void* hits) {
  bool ok;
  Table tb(ekey, evalue, ecolour, n_entries, cap, &ok);
  if (!ok) return -1;
  if (n > 0) rgbdfe::launch_octo_cast(tb.view(), origins, directions, n, query_of(prm), static_cast<rgbdfe_octomap_ray_hit*>(hits), nullptr);
  return 0;
}

// T: column-major Matrix4f; intr: fx, fy, cx, cy (converted to float here, as the host code does)
extern "C" int emu_octo_view(const unsigned long long* ekey, const uint32_t* evalue, const uint32_t* ecolour, uint32_t n_entries,
                             uint32_t cap, const double* prm, const float* T, const double* intr, uint32_t rows, uint32_t cols,
                             float* cloud, uint8_t* status) {
  bool ok;
  Table tb(ekey, evalue, ecolour, n_entries, cap, &ok);
  if (!ok) return -1;
  rgbdfe::OctoView v{};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) v.R[r * 3 + c] = T[c * 4 + r];
    v.t[r] = T[12 + r];
  }
  v.fx = (float)intr[0]; v.fy = (float)intr[1]; v.cx = (float)intr[2]; v.cy = (float)intr[3];
  v.rows = rows; v.cols = cols;
  if (rows > 0 && cols > 0) rgbdfe::launch_octo_view(tb.view(), v, query_of(prm), reinterpret_cast<float4*>(cloud), status, nullptr);
  return 0;
}
