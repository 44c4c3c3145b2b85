// depth_convert.h -- depthToCV8UC1's per-pixel arithmetic (src/misc.cpp:414-430), written once for every kernel and host
// accessor that needs it (emm.hip's stand-alone depth kernels, ingest.hip, the sensor entry points' per-keypoint look-ups).
// cv::Mat::convertTo(CV_8UC1, a, b) is saturate_cast<uchar>(cvRound(v * a + b)) in float; convertTo(CV_32FC1, a) is
// v * a + 0 in float.  Compile with -ffp-contract=off: the product is rounded before the addition.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace rgbdfe {

// saturate_cast<uchar>(cvRound(t)): round half to even; NaN / out-of-int-range -> 0 (cvtss2si indefinite)
__host__ __device__ __forceinline__ uint8_t sat_u8_rne(float t) {
  if (!(t > -2147483648.0f && t < 2147483648.0f)) return 0;
  const int r = (int)rintf(t);
  return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// 32FC1 metres -> mask byte: depth_img.convertTo(mono8_img, CV_8UC1, 100, 0) (misc.cpp:419)
__host__ __device__ __forceinline__ uint8_t depth_f32_to_mono8(float d) { return sat_u8_rne(d * 100.0f + 0.0f); }
// 16UC1 millimetres (already converted to float) -> mask byte: convertTo(CV_8UC1, 0.05, -25) (misc.cpp:423)
__host__ __device__ __forceinline__ uint8_t depth_mm_to_mono8(float v) { return sat_u8_rne(v * 0.05f + -25.0f); }
// 16UC1 millimetres (already converted to float) -> metres: convertTo(CV_32FC1, 0.001, 0) (misc.cpp:424)
__host__ __device__ __forceinline__ float depth_mm_to_metres(float v) { return v * 0.001f + 0.0f; }

}  // namespace rgbdfe
