// tfc_device.h -- pcl::TransformationFromCorrespondences on the device: the float accumulator, the 3x3 two-sided Jacobi SVD
// (Eigen::JacobiSVD<Matrix3f> as published) and getTransformation.  Shared by the RANSAC kernels (ransac_device.h) and the ICP
// fallback (icp.hip); plain C++ apart from the __device__ markers, so the kernel emulation of tests/emu compiles it as it is.
// Every function follows the operation order of oracle/rgbd_oracle.c: with -ffp-contract=off the results are bit-identical.
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>

namespace rgbdfe {

// one match in LDS: from.xyz, to.xyz, weight (7 words: a lane = match access is bank-conflict free)
constexpr int kRec = 7;
constexpr uint32_t kRecBytes = kRec * 4;

// ---------------------------------------------------------------------------------
// pcl::TransformationFromCorrespondences accumulator (float, sequential recurrence)
// ---------------------------------------------------------------------------------
struct Tfc {
  float W;
  float m1[3], m2[3];
  float C[9];  // row-major C[i*3+j]
  __device__ __forceinline__ void reset() {
    W = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) m1[i] = m2[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = 0.0f;
  }
  // transformation_estimation_euclidean.cpp:20-25,56 + tfc.add()
  __device__ __forceinline__ void add(const float* __restrict__ M, int m) {
    float f[3] = {M[m * kRec + 0], M[m * kRec + 1], M[m * kRec + 2]};
    float t[3] = {M[m * kRec + 3], M[m * kRec + 4], M[m * kRec + 5]};
    if (__builtin_isnan(f[2]) || __builtin_isnan(t[2])) return;
    // weight = 1.0/(from(2)*to(2)): double divide rounded to float == float divide
    // (53 >= 2*24+2: double rounding is innocuous for division)
    float w = 1.0f / (f[2] * t[2]);
    if (w == 0.0f) return;
    W += w;
    float alpha = w / W;
    float d1[3], d2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) d1[j] = f[j] - m1[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) d2[i] = t[i] - m2[i];
    float oma = 1.0f - alpha;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float outer = d2[i] * d1[j];
        float scaled = alpha * outer;
        float sum = C[i * 3 + j] + scaled;
        C[i * 3 + j] = oma * sum;
      }
#pragma unroll
    for (int j = 0; j < 3; ++j) m1[j] = m1[j] + alpha * d1[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) m2[i] = m2[i] + alpha * d2[i];
  }
};

// ---------------------------------------------------------------------------------
// 3x3 two-sided Jacobi SVD (Eigen::JacobiSVD<Matrix3f> as published), row-major.
// Same operation order as the oracle's orc_svd3.
// ---------------------------------------------------------------------------------
template <int p, int q>
__device__ __forceinline__ bool jacobi_pair(float* W, float* U, float* V, float& max_diag) {
  const float precision = 2.0f * FLT_EPSILON;
  float threshold = precision * max_diag;
  if (FLT_MIN > threshold) threshold = FLT_MIN;
  if (!(fabsf(W[p * 3 + q]) > threshold || fabsf(W[q * 3 + p]) > threshold)) return false;
  float m00 = W[p * 3 + p], m01 = W[p * 3 + q], m10 = W[q * 3 + p], m11 = W[q * 3 + q];
  float t = m00 + m11;
  float d = m10 - m01;
  float c1, s1;
  if (fabsf(d) < FLT_MIN) {
    c1 = 1.0f; s1 = 0.0f;
  } else {
    float u = t / d;
    float tmp = sqrtf(1.0f + u * u);
    s1 = 1.0f / tmp;
    c1 = u / tmp;
  }
  float n00 = c1 * m00 + s1 * m10;
  float n01 = c1 * m01 + s1 * m11;
  float n11 = (-s1) * m01 + c1 * m11;
  float cr, sr;
  float deno = 2.0f * fabsf(n01);
  if (deno < FLT_MIN) {
    cr = 1.0f; sr = 0.0f;
  } else {
    float tau = (n00 - n11) / deno;
    float w = sqrtf(tau * tau + 1.0f);
    float tt = (tau > 0.0f) ? 1.0f / (tau + w) : 1.0f / (tau - w);
    float sign_t = (tt > 0.0f) ? 1.0f : -1.0f;
    float nn = 1.0f / sqrtf(tt * tt + 1.0f);
    sr = -sign_t * (n01 / fabsf(n01)) * fabsf(tt) * nn;
    cr = nn;
  }
  float cl = c1 * cr + s1 * sr;
  float sl = s1 * cr - c1 * sr;
  // Each rotation updates a pair (x, y) from its own old values.  Written so that the results can land in the registers
  // of x and y themselves (the lanes that skip this pair keep theirs): the four products first -- the last one into y --
  // then the two sums; as two assignments of full expressions the compiler computed into temporaries and copied.
  const float nsl = -sl;
  auto rot_l = [&](float& x, float& y) {   // x' = cl x + sl y, y' = (-sl) x + cl y
    const float a = cl * x, b = sl * y, c = nsl * x;
    y = cl * y;
    y = c + y;
    x = a + b;
  };
  auto rot_r = [&](float& x, float& y) {   // x' = cr x - sr y, y' = sr x + cr y
    const float a = cr * x, b = sr * y, c = sr * x;
    y = cr * y;
    y = c + y;
    x = a - b;
  };
#pragma unroll
  for (int k = 0; k < 3; ++k) rot_l(W[p * 3 + k], W[q * 3 + k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) rot_l(U[k * 3 + p], U[k * 3 + q]);
#pragma unroll
  for (int k = 0; k < 3; ++k) rot_r(W[k * 3 + p], W[k * 3 + q]);
#pragma unroll
  for (int k = 0; k < 3; ++k) rot_r(V[k * 3 + p], V[k * 3 + q]);
  float a = fabsf(W[p * 3 + p]), b = fabsf(W[q * 3 + q]);
  if (b > a) a = b;
  if (a > max_diag) max_diag = a;
  return true;
}

template <int a, int b>
__device__ __forceinline__ void swap_cols(float* S, float* U, float* V) {
  float ts = S[a]; S[a] = S[b]; S[b] = ts;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float tu = U[k * 3 + a]; U[k * 3 + a] = U[k * 3 + b]; U[k * 3 + b] = tu;
    float tv = V[k * 3 + a]; V[k * 3 + a] = V[k * 3 + b]; V[k * 3 + b] = tv;
  }
}

__device__ __forceinline__ float det3(const float* m) {
  float h0 = m[0] * (m[4] * m[8] - m[5] * m[7]);
  float h1 = m[1] * (m[3] * m[8] - m[5] * m[6]);
  float h2 = m[2] * (m[3] * m[7] - m[4] * m[6]);
  return h0 - h1 + h2;
}

// tfc.getTransformation(): R (row-major 9) and t (3)
__device__ __forceinline__ void tfc_get_transformation(const Tfc& s, float* R, float* tr) {
  float W[9], U[9], V[9], S[3];
  float scale = 0.0f;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    float a = fabsf(s.C[i]);
    if (a > scale) scale = a;
  }
  if (scale == 0.0f) scale = 1.0f;
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = s.C[i] / scale;
#pragma unroll
  for (int i = 0; i < 9; ++i) U[i] = V[i] = (i % 4 == 0) ? 1.0f : 0.0f;
  float max_diag = fabsf(W[0]);
  if (fabsf(W[4]) > max_diag) max_diag = fabsf(W[4]);
  if (fabsf(W[8]) > max_diag) max_diag = fabsf(W[8]);
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool any = false;
    any |= jacobi_pair<1, 0>(W, U, V, max_diag);
    any |= jacobi_pair<2, 0>(W, U, V, max_diag);
    any |= jacobi_pair<2, 1>(W, U, V, max_diag);
    if (!any) break;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float w = W[i * 3 + i];
    S[i] = fabsf(w);
    if (w < 0.0f) {
#pragma unroll
      for (int k = 0; k < 3; ++k) U[k * 3 + i] = -U[k * 3 + i];
    }
    S[i] = S[i] * scale;
  }
  // selection sort, descending, first maximum wins; stop at an all-zero tail
  {
    int pos = 0;
    float best = S[0];
    if (S[1] > best) { best = S[1]; pos = 1; }
    if (S[2] > best) { best = S[2]; pos = 2; }
    if (best != 0.0f) {
      if (pos == 1) swap_cols<0, 1>(S, U, V);
      if (pos == 2) swap_cols<0, 2>(S, U, V);
      if (S[2] > S[1]) {  // i = 1: best = S[2] != 0 here since S[2] > S[1] >= 0
        swap_cols<1, 2>(S, U, V);
      }
    }
  }
  float s22 = 1.0f;
  if (det3(U) * det3(V) < 0.0f) s22 = -1.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float us2 = U[i * 3 + 2] * s22;
      R[i * 3 + j] = (U[i * 3 + 0] * V[j * 3 + 0] + U[i * 3 + 1] * V[j * 3 + 1]) + us2 * V[j * 3 + 2];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float rm = (R[i * 3 + 0] * s.m1[0] + R[i * 3 + 1] * s.m1[1]) + R[i * 3 + 2] * s.m1[2];
    tr[i] = s.m2[i] - rm;
  }
}

}  // namespace rgbdfe
