// Test-only program (built and run by tests/test_gpu_prescreen_split.py): the pre-screen count of a RANSAC hypothesis from
// prescreen_may_pass (every lane walks the 7-word records), from prescreen_may_pass_s4 (the transposed copy) and from
// prescreen_may_pass_s4_split (a partial wave's hypotheses spread over G lanes each) must be the same integer for every
// hypothesis.  One wave per block: lanes below `a` hold hypotheses of the pool, the other lanes hold junk (other pool
// entries and NaN) that must not reach any count.  Prints one line per case and ends with 0 only if every count agreed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "ransac_device.h"

using namespace rgbdfe;

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);  \
      return 2;                                                                    \
    }                                                                              \
  } while (0)

constexpr int kPool = 48;   // hypotheses per record set: the identity, random ones, planted ones

// block b, lane j < a: hypothesis b * a + j of the pool (past its end: none).  out[(b * 64 + lane) * 3 + {0, 1, 2}].
__global__ __launch_bounds__(64) void counts_kernel(const float* __restrict__ records, const float* __restrict__ pool, int n_pool,
                                                    int n_all, float pmax, RansacConst rc, int a, int log2_groups,
                                                    uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float M[RGBDFE_MAX_MATCHES * kRec];
  __shared__ __attribute__((aligned(16))) float S4[(RGBDFE_MAX_MATCHES / 4) * kS4Block];
  const int lane = threadIdx.x;
  for (int v = lane; v < RGBDFE_MAX_MATCHES * kRec; v += 64) M[v] = records[v];
  __syncthreads();
  transpose_records(M, S4, lane, 64);
  __syncthreads();
  float hypR[9], hypt[3];
  const int h = blockIdx.x * a + lane;
  if (lane < a && h < n_pool) {
    for (int i = 0; i < 9; ++i) hypR[i] = pool[h * 12 + i];
    for (int i = 0; i < 3; ++i) hypt[i] = pool[h * 12 + 9 + i];
  } else if (lane & 1) {  // junk: NaN in odd lanes, some other hypothesis scaled in even ones
    for (int i = 0; i < 9; ++i) hypR[i] = __int_as_float(0x7fc00000);
    for (int i = 0; i < 3; ++i) hypt[i] = __int_as_float(0x7fc00000);
  } else {
    const int o = (lane * 7 + blockIdx.x) % n_pool;
    for (int i = 0; i < 9; ++i) hypR[i] = 3.0f * pool[o * 12 + i];
    for (int i = 0; i < 3; ++i) hypt[i] = pool[o * 12 + 9 + i] + 1.0f;
  }
  uint32_t* o = out + ((size_t)blockIdx.x * 64 + lane) * 3;
  o[0] = prescreen_may_pass(hypR, hypt, M, n_all, pmax, rc);
  o[1] = prescreen_may_pass_s4(hypR, hypt, S4, n_all, pmax, rc);
  o[2] = prescreen_may_pass_s4_split(hypR, hypt, S4, n_all, pmax, rc, lane, log2_groups);
}

// ---- the host's restatement of the count's arithmetic, to plant records at the threshold
static float hi_of(const float* R, const float* t, float pmax, const RansacConst& rc) {
  const float u4 = 4.0f * 5.9604645e-8f;
  float es = 0.0f;
  for (int i = 0; i < 3; ++i)
    es += u4 * (((fabsf(R[3 * i]) + fabsf(R[3 * i + 1])) + fabsf(R[3 * i + 2]) + 1.0f) * pmax + fabsf(t[i]));
  const double smax = rc.raster_cov_x > rc.depth_cov ? rc.raster_cov_x : rc.depth_cov;
  const float S = (float)(2.0 * (smax + smax));
  const float E = 2.0f * ((2.0f * sqrtf(S) * 1.001f) * es + es * es + u4 * S) + 1e-30f;
  return S * 1.000001f + E;
}
static void moved(const float* R, const float* t, const float* p, float* w) {
  for (int i = 0; i < 3; ++i) w[i] = fmaf(R[3 * i], p[0], fmaf(R[3 * i + 1], p[1], fmaf(R[3 * i + 2], p[2], t[i])));
}
static float dsq_of(const float* R, const float* t, const float* rec) {
  float w[3];
  moved(R, t, rec, w);
  const float f0 = w[0] - rec[3], f1 = w[1] - rec[4], f2 = w[2] - rec[5];
  return fmaf(f0, f0, fmaf(f1, f1, f2 * f2));
}
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static void rotation(std::mt19937& g, float angle_max, float* R) {
  std::normal_distribution<float> nd;
  std::uniform_real_distribution<float> ud(-angle_max, angle_max);
  float ax[3] = {nd(g), nd(g), nd(g)};
  const float n = sqrtf(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-20f;
  for (float& v : ax) v /= n;
  const float th = ud(g), c = cosf(th), s = sinf(th), C = 1.0f - c;
  const float r[9] = {c + ax[0] * ax[0] * C, ax[0] * ax[1] * C - ax[2] * s, ax[0] * ax[2] * C + ax[1] * s,
                      ax[1] * ax[0] * C + ax[2] * s, c + ax[1] * ax[1] * C, ax[1] * ax[2] * C - ax[0] * s,
                      ax[2] * ax[0] * C - ax[1] * s, ax[2] * ax[1] * C + ax[0] * s, c + ax[2] * ax[2] * C};
  memcpy(R, r, sizeof r);
}

int main() {
  RansacConst rc;
  memset(&rc, 0, sizeof rc);
  rc.depth_cov = 1e-4;
  const double sx = 3 * tan(58.0 / 180.0 * M_PI / 640), sy = 3 * tan(45.0 / 180.0 * M_PI / 480);
  rc.raster_cov_x = sx * sx;
  rc.raster_cov_y = sy * sy;
  const float pmax = 8.0f;   // an input of the count like any other: at least every coordinate used below
  const int n_alls[] = {4, 5, 21, 63, 64, 65, 299, 300};
  const int lanes[] = {1, 7, 8, 9, 16, 17, 32};
  float *d_rec, *d_pool;
  uint32_t* d_out;
  CHECK(hipMalloc(&d_rec, RGBDFE_MAX_MATCHES * kRec * sizeof(float)));
  CHECK(hipMalloc(&d_pool, kPool * 12 * sizeof(float)));
  CHECK(hipMalloc(&d_out, (size_t)kPool * 64 * 3 * sizeof(uint32_t)));
  std::vector<uint32_t> out((size_t)kPool * 64 * 3);
  int bad = 0, cases = 0;
  for (int n_all : n_alls) {
    std::mt19937 g(1000 + n_all);
    std::uniform_real_distribution<float> xy(-3.0f, 3.0f), zd(0.5f, 4.0f), tr(-0.3f, 0.3f), un(0.0f, 1.0f);
    std::normal_distribution<float> nd;
    float Rt[9], tt[3];
    rotation(g, 0.3f, Rt);
    for (float& v : tt) v = tr(g);
    // every record of the buffer exists, as in PairPrep; two thirds follow the true motion with noise
    std::vector<float> rec(RGBDFE_MAX_MATCHES * kRec);
    for (int m = 0; m < RGBDFE_MAX_MATCHES; ++m) {
      float* r = &rec[m * kRec];
      r[0] = xy(g); r[1] = xy(g); r[2] = zd(g);
      moved(Rt, tt, r, r + 3);
      const bool outlier = un(g) < 0.33f;
      for (int i = 0; i < 3; ++i) r[3 + i] += outlier ? xy(g) : 0.01f * nd(g);
      r[6] = 1.0f;
    }
    const int m_nan = 1, m_zero = 2;   // below every n_all of the list
    rec[m_nan * kRec + 0] = NAN;
    rec[m_zero * kRec + 2] = 0.0f;
    // the pool: the identity, random motions (near the true one and anywhere), then the planted ones
    std::vector<float> pool(kPool * 12, 0.0f);
    pool[0] = pool[4] = pool[8] = 1.0f;
    const int first_planted = 32;
    for (int h = 1; h < kPool; ++h) {
      float* R = &pool[h * 12];
      if (h < 12) {
        rotation(g, 3.1f, R);
        for (int i = 0; i < 3; ++i) R[9 + i] = 4.0f * tr(g);
      } else {
        float dR[9];
        rotation(g, 0.01f, dR);
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) R[3 * i + j] = dR[3 * i] * Rt[j] + dR[3 * i + 1] * Rt[3 + j] + dR[3 * i + 2] * Rt[6 + j];
        for (int i = 0; i < 3; ++i) R[9 + i] = tt[i] + 0.02f * tr(g);
      }
    }
    // planted: hypothesis h takes two records (while there are any): their p.y is solved so that the moved point's y is
    // tiny -- q.y then has ulps far below the threshold's -- f0 is 0.98 sqrt(hi_f), f2 is 0, and q.y is bisected to the
    // two neighbouring floats at which dsq is the last value that still counts (<= hi_f) and the first that does not
    int next_rec = 3, planted = 0;
    for (int h = first_planted; h < kPool && next_rec + 2 <= n_all; ++h, next_rec += 2) {
      const float* R = &pool[h * 12];
      const float* t = R + 9;
      const float hi = hi_of(R, t, pmax, rc);
      uint32_t s_bits[2];
      float* r0 = &rec[next_rec * kRec];
      r0[1] = -(R[3] * r0[0] + R[5] * r0[2] + t[1]) / R[4];
      float w[3];
      moved(R, t, r0, w);
      r0[3] = w[0] - 0.98f * sqrtf(hi);
      r0[5] = w[2];
      uint32_t lo = 0, up = bits_of(sqrtf(hi));   // s = lo: counts, s = up: does not
      r0[4] = w[1] - from_bits(up);
      if (fabsf(r0[1]) > pmax || !(dsq_of(R, t, r0) > hi)) { fprintf(stderr, "planting failed (n_all %d, h %d)\n", n_all, h); return 2; }
      while (up - lo > 1) {
        const uint32_t mid = lo + (up - lo) / 2;
        r0[4] = w[1] - from_bits(mid);
        if (dsq_of(R, t, r0) > hi) up = mid; else lo = mid;
      }
      s_bits[0] = lo; s_bits[1] = up;
      for (int k = 0; k < 2; ++k) {
        float* r = &rec[(next_rec + k) * kRec];
        memmove(r, r0, kRec * sizeof(float));
        r[4] = w[1] - from_bits(s_bits[k]);
        const float d = dsq_of(R, t, r);
        const bool one_ulp = d >= nextafterf(hi, 0.0f) && d <= nextafterf(hi, INFINITY);
        if (!one_ulp || (k == 0) != !(d > hi)) { fprintf(stderr, "planted dsq %.9g not at hi_f %.9g (n_all %d, h %d)\n", d, hi, n_all, h); return 2; }
      }
      ++planted;
    }
    CHECK(hipMemcpy(d_rec, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_pool, pool.data(), pool.size() * sizeof(float), hipMemcpyHostToDevice));
    for (int log2_groups = 3; log2_groups >= 1; --log2_groups)
      for (int a : lanes) {
        if (a > (64 >> log2_groups)) continue;   // G lanes per hypothesis: at most 64 / G hypotheses
        const int blocks = (kPool + a - 1) / a;
        CHECK(hipMemset(d_out, 0xff, out.size() * sizeof(uint32_t)));
        hipLaunchKernelGGL(counts_kernel, dim3(blocks), dim3(64), 0, 0, d_rec, d_pool, kPool, n_all, pmax, rc, a, log2_groups, d_out);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(out.data(), d_out, (size_t)blocks * 64 * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        int mism = 0, seen = 0, host_differs = 0;
        uint32_t cmin = ~0u, cmax = 0;
        for (int b = 0; b < blocks; ++b)
          for (int j = 0; j < a && b * a + j < kPool; ++j, ++seen) {
            const uint32_t* o = &out[((size_t)b * 64 + j) * 3];
            if (o[0] != o[1] || o[0] != o[2]) {
              if (mism++ < 4) fprintf(stderr, "n_all %d a %d G %d hypothesis %d: records %u, s4 %u, split %u\n", n_all, a, 1 << log2_groups, b * a + j, o[0], o[1], o[2]);
            }
            // the host's restatement counts the same matches: the planted records sit at the device's threshold too
            const float* R = &pool[(b * a + j) * 12];
            const float hi = hi_of(R, R + 9, pmax, rc);
            uint32_t host = 0;
            for (int m = 0; m < ((n_all + 3) & ~3); ++m) host += !(dsq_of(R, R + 9, &rec[m * kRec]) > hi) ? 1u : 0u;
            host_differs += host != o[0];
            cmin = o[0] < cmin ? o[0] : cmin;
            cmax = o[0] > cmax ? o[0] : cmax;
          }
        printf("case n_all=%d a=%d G=%d hypotheses=%d planted=%d count_min=%u count_max=%u host_differs=%d mismatches=%d\n",
               n_all, a, 1 << log2_groups, seen, planted, cmin, cmax, host_differs, mism);
        bad += mism;
        ++cases;
      }
  }
  printf("cases=%d mismatches=%d\n", cases, bad);
  return bad ? 1 : 0;
}
