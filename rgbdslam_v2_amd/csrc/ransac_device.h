// ransac_device.h -- device-side arithmetic shared by the RANSAC kernels (select_ransac.hip: one wave per pair,
// result waves, g2o refinement; ransac_split.hip: the hypothesis and refinement kernels of the record / replay schedule).
// Every function follows the operation order of oracle/rgbd_oracle.c (which restates the reference and is pinned on
// the reference's own compiled code): with -ffp-contract=off the results are bit-identical to the CPU restatement.
#pragma once
#include <float.h>
#include <stddef.h>

#include <type_traits>

#include "rgbdfe_internal.h"
#include "tfc_device.h"

namespace rgbdfe {

constexpr int kWave = 64;
constexpr int kRounds = RGBDFE_MAX_MATCHES / kWave;  // 5

// RANSAC iterations refined side by side: the refits of a round share ONE recurrence loop (9 lanes per
// slot, 7 x 9 = 63 lanes) and ONE batched SVD (lane = slot).
constexpr int kSlots = 7;
constexpr int kFitUnroll = 4;   // recurrence steps per trip; loads run two trips ahead
// bytes per slot list: 320 entries + two trips of read-ahead, an odd number of words so that the
// slots' k-th entries sit in different LDS banks
constexpr int kOrdStride = RGBDFE_MAX_MATCHES + 2 * kFitUnroll + 4;
static_assert(kOrdStride % 4 == 0 && (kOrdStride / 4) % 2 == 1, "list rows: word aligned, odd word count");
static_assert(RGBDFE_MAX_MATCHES <= 512, "list entries keep the low 8 bits of a match index + one threshold");

// refit phase: the inlier set compacted in match order
struct FitBuf {
  // per slot: its participating matches in match order, low 8 bits of the match index (the lists ascend, so
  // "index >= 256" is one threshold position per list, kept in a register): 1/2 of the u16 footprint, which
  // is what lets 12 instead of 10 waves share a CU's LDS
  uint8_t ord[kSlots][kOrdStride];
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// D1: counter-based replacement of rand() (node.cpp:1033-1034); same integer function as
// the oracle's orc_rand31.
__device__ __forceinline__ uint32_t rand31(uint32_t seed_mixed_uid, uint32_t iter, uint32_t k) {
  uint32_t h = mix32(seed_mixed_uid ^ (iter * 0xC2B2AE35u + 0x165667B1u));
  h = mix32(h + k * 0x27D4EB2Fu);
  return h >> 1;
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {
  // number of set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ float bcast_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}


__device__ __forceinline__ bool has_nan12(const float* R, const float* t) {
  bool n = false;
#pragma unroll
  for (int i = 0; i < 9; ++i) n |= (R[i] != R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) n |= (t[i] != t[i]);
  return n;
}

// ---------------------------------------------------------------------------------
// d^T S^-1 d through the unblocked Cholesky factorisation and the two triangular solves of
// Eigen's llt().solve() (misc.cpp:763); S given by its lower triangle.  Same operation order as
// the oracle's orc_error_function2; `ok` = all pivots positive.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double mahal_llt_ieee(double S00, double S10, double S11, double S20, double S21,
                                                 double S22, const double* d, bool& ok) {
  ok = S00 > 0.0;
  const double l00 = sqrt(S00);
  const double l10 = S10 / l00;
  const double l20 = S20 / l00;
  const double x1 = S11 - l10 * l10;
  ok = ok && (x1 > 0.0);
  const double l11 = sqrt(x1);
  const double l21 = (S21 - l20 * l10) / l11;
  const double x2 = S22 - (l20 * l20 + l21 * l21);
  ok = ok && (x2 > 0.0);
  const double l22 = sqrt(x2);
  const double y0 = d[0] / l00;
  const double y1 = (d[1] - l10 * y0) / l11;
  const double y2 = (d[2] - (l20 * y0 + l21 * y1)) / l22;
  const double z2 = y2 / l22;
  const double z1 = (y1 - l21 * z2) / l11;
  const double z0 = (y0 - (l10 * z1 + l20 * z2)) / l00;
  return (d[0] * z0 + d[1] * z1) + d[2] * z2;
}

// The same arithmetic with the IEEE divisions and square roots spelled out as the gfx950 expansion of
// `/` and `sqrt` WITHOUT its range scaling (v_div_scale / v_div_fmas / v_div_fixup, v_ldexp), and with
// the refined reciprocal of a pivot shared by the 2-4 divisions that use it: 9 divisions cost
// 3 x 5 + 9 x 3 instructions instead of 9 x 11.  Bit-identical to the expansion whenever the scaling
// would have been the identity, i.e. every numerator and radicand is a normal number with a binary
// exponent within +-200 (no zero, denormal, inf, NaN).  `unsafe` reports a lane outside that window;
// the caller then recomputes with mahal_llt_ieee.
struct ExpWindow {
  uint32_t lo = 0x7FF00000u, hi = 0u;
  __device__ __forceinline__ void see(double v) {
    const uint32_t e = (uint32_t)__double2hiint(v) & 0x7FF00000u;
    lo = min(lo, e);
    hi = max(hi, e);
  }
  __device__ __forceinline__ bool outside() const {
    return lo < ((1023u - 200u) << 20) || hi > ((1023u + 200u) << 20);
  }
};
__device__ __forceinline__ double rcp_refined(double b) {
  double r = __builtin_amdgcn_rcp(b);
  double e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  return r;
}
__device__ __forceinline__ double div_by(double a, double b, double rb) {
  const double q = a * rb;
  const double res = __builtin_fma(-b, q, a);
  return __builtin_fma(res, rb, q);
}
__device__ __forceinline__ double sqrt_unscaled(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double t = __builtin_fma(-g, g, x);
  g = __builtin_fma(t, h, g);
  t = __builtin_fma(-g, g, x);
  g = __builtin_fma(t, h, g);
  return g;
}
__device__ __forceinline__ double mahal_llt_fast(double S00, double S10, double S11, double S20, double S21,
                                                 double S22, const double* d, bool& ok, bool& unsafe) {
  ExpWindow win;
  ok = S00 > 0.0;
  win.see(S00);
  const double l00 = sqrt_unscaled(S00);
  const double r00 = rcp_refined(l00);
  win.see(S10); win.see(S20); win.see(d[0]);
  const double l10 = div_by(S10, l00, r00);
  const double l20 = div_by(S20, l00, r00);
  const double y0 = div_by(d[0], l00, r00);
  const double x1 = S11 - l10 * l10;
  ok = ok && (x1 > 0.0);
  win.see(x1);
  const double l11 = sqrt_unscaled(x1);
  const double r11 = rcp_refined(l11);
  const double n21 = S21 - l20 * l10;
  const double ny1 = d[1] - l10 * y0;
  win.see(n21); win.see(ny1);
  const double l21 = div_by(n21, l11, r11);
  const double y1 = div_by(ny1, l11, r11);
  const double x2 = S22 - (l20 * l20 + l21 * l21);
  ok = ok && (x2 > 0.0);
  win.see(x2);
  const double l22 = sqrt_unscaled(x2);
  const double r22 = rcp_refined(l22);
  const double ny2 = d[2] - (l20 * y0 + l21 * y1);
  win.see(ny2);
  const double y2 = div_by(ny2, l22, r22);
  win.see(y2);
  const double z2 = div_by(y2, l22, r22);
  const double nz1 = y1 - l21 * z2;
  win.see(nz1);
  const double z1 = div_by(nz1, l11, r11);
  const double nz0 = y0 - (l10 * z1 + l20 * z2);
  win.see(nz0);
  const double z0 = div_by(nz0, l00, r00);
  unsafe = win.outside();
  return (d[0] * z0 + d[1] * z1) + d[2] * z2;
}

__device__ __forceinline__ double uniform_f64(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// ---------------------------------------------------------------------------------
// getTransformFromMatches for the active slots of a window round, all at once.
// The PCL recurrence (Tfc::add) is strictly sequential in its state, so one refit can keep only
// 9 lanes busy (lane l: C[i][j], mean2[i], mean1[j], i = l/3, j = l%3).  The refits of different
// slots are independent: slot s runs on lanes 9s .. 9s+8, each walking its own compacted inlier list.
//   fit_compact     (lane = match): k-th participating match of slot s -> ord[s][k]
//   fit_recurrence  (lane = slot x element): W += w; alpha = w / W; the 15 state elements advance
// Every float operation is the one the sequential code performs, in the same order on the same
// operands: bit-identical to Tfc::add over the same matches.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ int fit_compact(int s, const uint64_t* mask, const uint64_t* w_nonzero, FitBuf& fit,
                                           int& n_below_256, int lane) {
  uint32_t base = 0;
  n_below_256 = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    // tfc.add skips weight == 0; NaN depths never reach an inlier set (misc.cpp:712-717)
    const uint64_t pm = mask[r] & w_nonzero[r];  // wave-uniform: scalar ALU
    // lane's bit of the wave-uniform mask as the execution mask itself (s_and_saveexec), no per-lane shift
    if (__builtin_amdgcn_inverse_ballot_w64(pm)) fit.ord[s][base + lane_rank(pm)] = (uint8_t)(r * kWave + lane);
    base += (uint32_t)__popcll(pm);
    if (r == 256 / kWave - 1) n_below_256 = (int)base;
  }
  // the recurrence reads two trips past the end of a list: keep those entries valid match indices
  if (lane < 2 * kFitUnroll) fit.ord[s][base + lane] = 0;
  return (int)base;
}

// Keeps v in a register at this point: the compiler may not sink the computation of v into a
// conditionally executed block (which would serialise the LDS loads feeding it again).
__device__ __forceinline__ void pin(float& v) { asm volatile("" : "+v"(v)); }

// n_mine: list length of this lane's slot (0: nothing to do), n_min / n_max: the shortest / longest list among the
// slots that take part in the round.
// On return lane 9s+x holds C[x], lane 9s+j mean1[j], lane 9s+3i mean2[i] of slot s.
// Software pipeline per trip of kFitUnroll steps: list entries are read two trips ahead, the match
// records one trip ahead; every load is unconditional (lists are padded two trips past their end with a
// valid index) and a finished slot keeps its state through selects.
// FAST_DIV: alpha = w / W through the gfx950 expansion of the f32 division without its range scaling
// (v_div_scale / v_div_fmas / v_div_fixup): bit-identical when the scaling is the identity, which the
// caller guarantees by checking once per pair that every weight lies in [2^-40, 2^40] (W is a sum of at
// most 320 of them).
template <bool FAST_DIV>
__device__ __forceinline__ void fit_recurrence(int n_mine, int k256_mine, int n_min, int n_max, const FitBuf& fit,
                                               const float* __restrict__ M, float& C, float& m1, float& m2, int lane) {
  constexpr int U = kFitUnroll;
  const int sl = min(lane / 9, kSlots - 1);
  const int l9 = lane % 9;
  const int ci = l9 / 3, cj = l9 % 3;
  const uint8_t* __restrict__ ord = fit.ord[sl];
  // byte offset of the k-th list entry's record: (low 8 bits + 256 from position k256 on) * 28
  auto rec_off = [&](int k) {
    const uint32_t hi = (k >= k256_mine) ? 256u * kRecBytes : 0u;
    return (uint32_t)ord[k] * kRecBytes + hi;
  };
  const char* __restrict__ recs = reinterpret_cast<const char*>(M);
  const char* __restrict__ recP = recs + cj * 4;        // from[cj]
  const char* __restrict__ recQ = recs + 12 + ci * 4;   // to[ci]
  float W = 0.0f;
  C = 0.0f; m1 = 0.0f; m2 = 0.0f;
  uint32_t off[U];
  float wv[U], fv[U], tv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) off[u] = rec_off(u);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    wv[u] = *reinterpret_cast<const float*>(recs + off[u] + 24);
    fv[u] = *reinterpret_cast<const float*>(recP + off[u]);
    tv[u] = *reinterpret_cast<const float*>(recQ + off[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) off[u] = rec_off(U + u);
  auto trip = [&](int k0, auto with_select) {
    float wc[U], fc[U], tc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { wc[u] = wv[u]; fc[u] = fv[u]; tc[u] = tv[u]; }
    // records of the next trip, list entries of the trip after it
#pragma unroll
    for (int u = 0; u < U; ++u) {
      wv[u] = *reinterpret_cast<const float*>(recs + off[u] + 24);
      fv[u] = *reinterpret_cast<const float*>(recP + off[u]);
      tv[u] = *reinterpret_cast<const float*>(recQ + off[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) off[u] = rec_off(k0 + 2 * U + u);
    // W_k = W_{k-1} + w_k, alpha_k = w_k / W_k: off the state's dependence chain
    float al[U], om[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      W = W + wc[u];
      if (FAST_DIV) {
        float r = __builtin_amdgcn_rcpf(W);
        const float e = __builtin_fmaf(-W, r, 1.0f);
        r = __builtin_fmaf(e, r, r);
        float q = wc[u] * r;
        float res = __builtin_fmaf(-W, q, wc[u]);
        q = __builtin_fmaf(res, r, q);
        res = __builtin_fmaf(-W, q, wc[u]);
        al[u] = __builtin_fmaf(res, r, q);
      } else {
        al[u] = wc[u] / W;
      }
      om[u] = 1.0f - al[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool act = (k0 + u) < n_mine;
      const float d1 = fc[u] - m1;
      const float d2 = tc[u] - m2;
      const float outer = d2 * d1;
      const float scaled = al[u] * outer;
      const float sum = C + scaled;
      float Cn = om[u] * sum;
      float m1n = m1 + al[u] * d1;
      float m2n = m2 + al[u] * d2;
      if (decltype(with_select)::value) {  // a slot whose list has ended keeps its state
        pin(Cn); pin(m1n); pin(m2n);
        C = act ? Cn : C;
        m1 = act ? m1n : m1;
        m2 = act ? m2n : m2;
      } else {
        C = Cn; m1 = m1n; m2 = m2n;
      }
    }
  };
  // While every participating slot still has entries (k < n_min) no lane needs the selects; lanes of slots that
  // do not take part in this round (n_mine == 0) compute garbage that nobody reads.
  int k0 = 0;
  for (; k0 + U <= n_min; k0 += U) trip(k0, std::false_type());
  for (; k0 < n_max; k0 += U) trip(k0, std::true_type());
}

// Upper bound of the number of matches that can pass errorFunction2's shortcut test (misc.cpp:726-735) under THIS LANE's
// hypothesis (lane = hypothesis): the float evaluation of dsq with score_passes' error band -- a match counts unless its
// dsq_f is provably above the threshold, NaN counts.  Every lane walks all matches; the match record is the same LDS
// address for all lanes (a broadcast read).
__device__ __forceinline__ uint32_t prescreen_may_pass(const float* hypR, const float* hypt, const float* __restrict__ M,
                                                    int n_all, float pmax, const RansacConst& rc) {
  const float u4 = 4.0f * 5.9604645e-8f;
  float es = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    es += u4 * (((fabsf(hypR[3 * i]) + fabsf(hypR[3 * i + 1])) + fabsf(hypR[3 * i + 2]) + 1.0f) * pmax + fabsf(hypt[i]));
  const double smax = rc.raster_cov_x > rc.depth_cov ? rc.raster_cov_x : rc.depth_cov;
  const float S = (float)(2.0 * (smax + smax));
  const float E = 2.0f * ((2.0f * sqrtf(S) * 1.001f) * es + es * es + u4 * S) + 1e-30f;
  const float hi_f = S * 1.000001f + E;
  uint32_t may_pass = 0;
  // Four matches per trip (their 24 LDS reads are in flight together), evaluated two at a time with packed f32
  // arithmetic (v_pk_fma_f32 / v_pk_add_f32: the hypothesis' coefficients feed both halves).  No validity test per
  // match: the count is an UPPER bound, and a match without depth (zero or NaN z; none survive removeDepthless in
  // practice) or one of the up to three records behind n_all can only add to it -- the outcome of the iteration is the
  // scoring's either way, the pre-screen merely fails to skip it.  The records behind n_all exist: PairPrep holds
  // RGBDFE_MAX_MATCHES of them, a multiple of 4.
  typedef float v2f __attribute__((ext_vector_type(2)));
  v2f R2[9], t2[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R2[i] = v2f{hypR[i], hypR[i]};
#pragma unroll
  for (int i = 0; i < 3; ++i) t2[i] = v2f{hypt[i], hypt[i]};
#pragma unroll 1
  for (int m0 = 0; m0 < n_all; m0 += 4) {
    float rec[4][6];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < 6; ++c) rec[u][c] = M[(m0 + u) * kRec + c];
#pragma unroll
    for (int u = 0; u < 4; u += 2) {
      const v2f px = {rec[u][0], rec[u + 1][0]}, py = {rec[u][1], rec[u + 1][1]}, pz = {rec[u][2], rec[u + 1][2]};
      const v2f qx = {rec[u][3], rec[u + 1][3]}, qy = {rec[u][4], rec[u + 1][4]}, qz = {rec[u][5], rec[u + 1][5]};
      const v2f f0 = __builtin_elementwise_fma(R2[0], px, __builtin_elementwise_fma(R2[1], py, __builtin_elementwise_fma(R2[2], pz, t2[0]))) - qx;
      const v2f f1 = __builtin_elementwise_fma(R2[3], px, __builtin_elementwise_fma(R2[4], py, __builtin_elementwise_fma(R2[5], pz, t2[1]))) - qy;
      const v2f f2 = __builtin_elementwise_fma(R2[6], px, __builtin_elementwise_fma(R2[7], py, __builtin_elementwise_fma(R2[8], pz, t2[2]))) - qz;
      const v2f dsq = __builtin_elementwise_fma(f0, f0, __builtin_elementwise_fma(f1, f1, f2 * f2));
      may_pass += !(dsq.x > hi_f) ? 1u : 0u;
      may_pass += !(dsq.y > hi_f) ? 1u : 0u;
    }
  }
  return may_pass;
}

// The same count from a transposed copy of the records: blocks of four matches, component-major -- S4[block][component 0..5]
// [match 0..3] -- so that one 16-byte LDS read (the same address in every lane: a broadcast) brings one component of four
// matches, and the halves of its four registers ARE the operand pairs of the packed arithmetic: 6 reads and no register
// shuffling per four matches, against 24 reads and 19 moves from the 7-word records.  Same pairs, same operations, same
// count.  (The copy costs a workgroup 7 LDS writes per thread once.)
constexpr int kS4Block = 24;   // floats of a block of four matches
__device__ __forceinline__ void transpose_records(const float* __restrict__ M, float* __restrict__ S4, int tid, int n_threads) {
  for (int v = tid; v < (RGBDFE_MAX_MATCHES / 4) * kS4Block; v += n_threads) {
    const int blk = v / kS4Block, r = v - blk * kS4Block;
    S4[v] = M[(blk * 4 + (r & 3)) * kRec + (r >> 2)];
  }
}
// (first_block, block_step): the blocks this lane walks, first_block, first_block + block_step, ... -- (0, 1) is every block.
__device__ __forceinline__ uint32_t prescreen_count_s4(const float* hypR, const float* hypt, const float* __restrict__ S4,
                                                    int n_all, float pmax, const RansacConst& rc, int first_block,
                                                    int block_step) {
  const float u4 = 4.0f * 5.9604645e-8f;
  float es = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    es += u4 * (((fabsf(hypR[3 * i]) + fabsf(hypR[3 * i + 1])) + fabsf(hypR[3 * i + 2]) + 1.0f) * pmax + fabsf(hypt[i]));
  const double smax = rc.raster_cov_x > rc.depth_cov ? rc.raster_cov_x : rc.depth_cov;
  const float S = (float)(2.0 * (smax + smax));
  const float E = 2.0f * ((2.0f * sqrtf(S) * 1.001f) * es + es * es + u4 * S) + 1e-30f;
  const float hi_f = S * 1.000001f + E;
  uint32_t may_pass = 0;
  typedef float v2f __attribute__((ext_vector_type(2)));
  typedef float v4f __attribute__((ext_vector_type(4)));
  v2f R2[9], t2[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R2[i] = v2f{hypR[i], hypR[i]};
#pragma unroll
  for (int i = 0; i < 3; ++i) t2[i] = v2f{hypt[i], hypt[i]};
  const v4f* __restrict__ blocks = reinterpret_cast<const v4f*>(S4);
  const int n_blocks = (n_all + 3) >> 2;
#pragma unroll 1
  for (int blk = first_block; blk < n_blocks; blk += block_step) {
    const v4f* __restrict__ b = blocks + blk * 6;
    const v4f px = b[0], py = b[1], pz = b[2], qx = b[3], qy = b[4], qz = b[5];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const v2f x = h ? px.zw : px.xy, y = h ? py.zw : py.xy, z = h ? pz.zw : pz.xy;
      const v2f f0 = __builtin_elementwise_fma(R2[0], x, __builtin_elementwise_fma(R2[1], y, __builtin_elementwise_fma(R2[2], z, t2[0]))) - (h ? qx.zw : qx.xy);
      const v2f f1 = __builtin_elementwise_fma(R2[3], x, __builtin_elementwise_fma(R2[4], y, __builtin_elementwise_fma(R2[5], z, t2[1]))) - (h ? qy.zw : qy.xy);
      const v2f f2 = __builtin_elementwise_fma(R2[6], x, __builtin_elementwise_fma(R2[7], y, __builtin_elementwise_fma(R2[8], z, t2[2]))) - (h ? qz.zw : qz.xy);
      const v2f dsq = __builtin_elementwise_fma(f0, f0, __builtin_elementwise_fma(f1, f1, f2 * f2));
      may_pass += !(dsq.x > hi_f) ? 1u : 0u;
      may_pass += !(dsq.y > hi_f) ? 1u : 0u;
    }
  }
  return may_pass;
}
__device__ __forceinline__ uint32_t prescreen_may_pass_s4(const float* hypR, const float* hypt, const float* __restrict__ S4,
                                                       int n_all, float pmax, const RansacConst& rc) {
  return prescreen_count_s4(hypR, hypt, S4, n_all, pmax, rc, 0, 1);
}

// The same count for a wave that holds at most 64 / G hypotheses in its first lanes (G = 1 << log2_groups = 2, 4 or 8): the
// wave's lanes are regrouped as lane = g * (64 / G) + j, lane j's hypothesis goes to its G lanes through ds_bpermute (in
// place: lane j < 64 / G keeps its own twelve floats, the others' are dead by now), group g counts blocks g, g + G, g + 2G,
// ... of S4 and a butterfly over the groups leaves the sum in every lane of j -- the integer prescreen_may_pass_s4 gives
// lane j, from the same blocks and the same arithmetic per match, in a G-th of the trips.  All 64 lanes must be active.
// Interleaved blocks, not one contiguous share per group: the reads are no broadcast here, and a ds_read_b128 serves a
// 16-lane group in one cycle only if its distinct addresses fall on different 16-byte slots of the 256-byte bank row.  A
// block is six slots, so blocks b .. b + 7 start at slots 6b mod 16 = 0, 6, 12, 2, 8, 14, 4, 10 (rotated): any G <= 8
// consecutive blocks are conflict-free for every component, whichever lanes the hardware groups.  Contiguous shares
// (75 blocks over 8 groups: 10 blocks = 60 slots = 12 mod 16 apart) would put groups 0 and 4, 1 and 5, ... on one slot.
__device__ __forceinline__ uint32_t prescreen_may_pass_s4_split(float* hypR, float* hypt, const float* __restrict__ S4,
                                                             int n_all, float pmax, const RansacConst& rc, int lane,
                                                             int log2_groups) {
  const int per_group = kWave >> log2_groups;
  const int src = (lane & (per_group - 1)) << 2;
#pragma unroll
  for (int i = 0; i < 9; ++i) hypR[i] = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(hypR[i])));
#pragma unroll
  for (int i = 0; i < 3; ++i) hypt[i] = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(hypt[i])));
  uint32_t may_pass = prescreen_count_s4(hypR, hypt, S4, n_all, pmax, rc, lane >> (6 - log2_groups), 1 << log2_groups);
  for (int d = per_group; d < kWave; d <<= 1)
    may_pass += (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ d) << 2, (int)may_pass);
  return may_pass;
}

// ---------------------------------------------------------------------------------
// The reference's in-order bookkeeping (node.cpp:1130-1191: `it += 10 / 20`, the 80 % exit, best-so-far) over the recorded
// outcomes of iterations [w.real_iterations, recorded_end): one wave, 64 summaries fetched per step, the sequential decisions
// on wave-uniform values.  Stops when the loop ends (w.done) or the records run out.  listed(k): iteration k passed the
// pre-screen and has a summary (an iteration that did not counts as {1e6, 0} and leaves nothing in memory).
// COHERENT: the summaries were written by other waves of the SAME launch (the refinement kernel's walk between two windows
// of a pair): agent-scope loads that do not stop at this CU's vector cache.
// ---------------------------------------------------------------------------------
struct WalkRegs {
  int it, real_iterations, valid_iterations, best_idx, best_n;
  float rmse;
  bool done;
};
template <bool COHERENT, class Listed>
__device__ __forceinline__ void walk_records(WalkRegs& w, int recorded_end, int I, int n_all, uint32_t thr,
                                             const IterSum* __restrict__ sum_pair, Listed listed, int lane) {
  while (!w.done && w.it < I && w.real_iterations < recorded_end) {
    const int k0 = w.real_iterations;
    const int G = min(kWave, recorded_end - k0);
    int rn_l = 0;
    double rerr_l = 0.0;
    if (lane < G && listed(k0 + lane)) {
      if (COHERENT) {
        const unsigned long long* p = reinterpret_cast<const unsigned long long*>(sum_pair + (k0 + lane));
        const unsigned long long a = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rerr_l = __longlong_as_double((long long)a);
        rn_l = (int)(uint32_t)b;
      } else {
        const IterSum su = sum_pair[k0 + lane];
        rn_l = su.rn;
        rerr_l = su.rerr;
      }
    }
    // Iterations whose refinement left refined_matches empty (:1171 fails) only count: `if (!(it < I)) break;
    // real_iterations++; ++it` -- a run of them is taken in one step; only the others are looked at one by one.
    const uint64_t with_matches = __ballot(lane < G && rn_l > 0);
    for (int g = 0; g < G;) {
      const uint64_t rest = with_matches >> g;
      const int run = rest != 0ull ? (int)__builtin_ctzll(rest) : G - g;  // empty iterations before the next one with matches
      if (run > 0) {
        const int can = min(run, max(I - w.it, 0));  // (`it` may have jumped beyond ransac_iterations, :1186-1187)
        w.real_iterations += can;          // :1139
        w.it += can;
        if (can < run) { w.done = true; break; }  // the next check of `it < ransac_iterations` fails (:1130)
        g += run;
        if (g >= G) break;
      }
      if (!(w.it < I)) { w.done = true; break; }
      w.real_iterations++;  // :1139
      const int refined_n = __builtin_amdgcn_readlane(rn_l, g);
      const double refined_error = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(rerr_l), g),
                                                    __builtin_amdgcn_readlane(__double2loint(rerr_l), g));
      // refined_n > 0 (:1171)
      w.valid_iterations++;
      if (refined_error <= (double)w.rmse && refined_n >= w.best_n && (uint32_t)refined_n >= thr) {  // :1177
        w.rmse = (float)refined_error;  // :1182
        w.best_idx = k0 + g;
        w.best_n = refined_n;
        if ((double)refined_n > (double)n_all * 0.5) w.it += 10;   // :1186
        if ((double)refined_n > (double)n_all * 0.75) w.it += 10;  // :1187
        if ((double)refined_n > (double)n_all * 0.8) { w.done = true; break; }  // :1188
      }
      ++w.it;
      ++g;
    }
  }
}

// a pair is "junk-heavy" (class 2 of the record / replay plan) when at most kClass2Num / kClass2Den of the first phase's
// iterations produced a refined hypothesis
#ifndef RGBDFE_CLASS2_NUM
#define RGBDFE_CLASS2_NUM 9
#define RGBDFE_CLASS2_DEN 14
#endif
constexpr int kClass2Num = RGBDFE_CLASS2_NUM, kClass2Den = RGBDFE_CLASS2_DEN;

}  // namespace rgbdfe
