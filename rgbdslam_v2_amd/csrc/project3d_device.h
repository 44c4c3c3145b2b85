// project3d_device.h -- the per-keypoint arithmetic of Node::projectTo3D / projectTo3DSiftGPU, getMinDepthInNeighborhood and
// squareroot_descriptor_space as device functions, shared by the single-frame kernels (project3d.hip) and the SIFTGPU node
// builder (sift_nodes.hip), so that both produce the same bits by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rgbdfe {

// Node::projectTo3DSiftGPU's lookup depth.at<float>(p2d.y, p2d.x) (node.cpp:733): float -> int by truncation
// (v_cvt_i32_f32 truncates, saturates and maps NaN to 0); the reference has no inside-the-image test, the indices are
// clamped to the image instead of read out of bounds
__device__ __forceinline__ size_t sift_depth_index(float px, float py, int rows, int cols) {
  int r = (int)py, c = (int)px;
  r = min(max(r, 0), rows - 1);
  c = min(max(c, 0), cols - 1);
  return (size_t)r * (size_t)cols + (size_t)c;
}

// depth * depth_scaling, in double as the reference's cast chain does
__device__ __forceinline__ float scaled_depth(float zraw, double depth_scaling) { return (float)((double)zraw * depth_scaling); }

// backProject (misc2.h:62-64): ((u - cx) * z) * fxinv in float; w = 1 (node.cpp:955)
__device__ __forceinline__ float4 back_project(float px, float py, float Z, float cx, float cy, float fxinv, float fyinv) {
  float4 o;
  o.x = (px - cx) * Z * fxinv;
  o.y = (py - cy) * Z * fyinv;
  o.z = Z;
  o.w = 1.0f;
  return o;
}

// getMinDepthInNeighborhood (misc.cpp:774-793) by one wave (lane = 0 .. 63, all lanes active): the smallest non-NaN depth of
// rows [int(y - r), int(y + r)) x cols [int(x - r), int(x + r)), r = int((size - 1) / 2), clamped to the image; no comparable
// value or a minimum of 0 gives NaN.  Lanes walk the window's columns; a minimum is order independent: exact.  Every lane
// returns the value.
__device__ __forceinline__ float min_depth_in_neighbourhood(float cx, float cy, float diameter, const float* __restrict__ depth,
                                                            int rows, int cols, int lane) {
  const int radius = (int)((diameter - 1) / 2);
  int top = (int)(cy - (float)radius); top = top < 0 ? 0 : top;
  int left = (int)(cx - (float)radius); left = left < 0 ? 0 : left;
  int bot = (int)(cy + (float)radius); bot = bot > rows ? rows : bot;
  int right = (int)(cx + (float)radius); right = right > cols ? cols : right;
  float mn = 3.402823466e+38f;
  bool found = false;
  for (int r = top; r < bot; ++r)
    for (int c = left + lane; c < right; c += 64) {
      const float v = depth[(size_t)r * (size_t)cols + (size_t)c];
      if (v < mn) { mn = v; found = true; }  // NaN never compares less: skipped, as in cv::minMaxLoc
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mn = fminf(mn, __shfl_xor(mn, d));  // no NaN among the partial minima
  found = __ballot(found) != 0ull;
  return (found && mn != 0.0f) ? mn : __builtin_nanf("");
}

// squareroot_descriptor_space (node.cpp:1557-1571, RootSIFT) of one 128-float row held by a whole wave, lane l holding
// columns 2l, 2l+1.  The L1 norm follows cv::reduce's float accumulation order (a0 over columns 0,2,..,124,126,127; a1 over
// 1,3,..,125; a0 + a1): a strictly sequential chain, fed by v_readlane so that the whole wave computes it uniformly.  A row
// that sums to 0 is not divided (:1565): it stays the abs() of the input.
__device__ __forceinline__ float2 root_sift_row(float2 v) {
  float2 o;
  o.x = fabsf(v.x);  // cv::abs (:1561)
  o.y = fabsf(v.y);
  auto lane_f = [](float f, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), l)); };
  float a0 = lane_f(o.x, 0), a1 = lane_f(o.y, 0);
#pragma unroll
  for (int l = 1; l < 63; ++l) {
    a0 = a0 + lane_f(o.x, l);
    a1 = a1 + lane_f(o.y, l);
  }
  a0 = a0 + lane_f(o.x, 63);
  a0 = a0 + lane_f(o.y, 63);
  const float sum = a0 + a1;
  if (sum != 0.0f) {  // :1565
    o.x = sqrtf(o.x / sum);  // :1569
    o.y = sqrtf(o.y / sum);
  }
  return o;
}

}  // namespace rgbdfe
