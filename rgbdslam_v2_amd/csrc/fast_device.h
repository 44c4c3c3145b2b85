// fast_device.h -- cv::FAST TYPE_9_16's corner score as a device function, shared by the ORB detection pass
// (orb_kernels.hip) and the FAST detector (fast_detect.hip): both score pixels with the same integers.
// fast_arc_score returns max(P, N) (orb_kernels.hip explains the arc form): a pixel is a corner at threshold t iff the value is
// > t, and its cornerScore<16> is the value - 1 whatever t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rgbdfe {

__device__ __forceinline__ int min3i(int a, int b, int c) { return min(min(a, b), c); }
__device__ __forceinline__ int max3i(int a, int b, int c) { return max(max(a, b), c); }

// ptr -> the centre pixel inside an LDS tile of row stride `stride`
__device__ __forceinline__ int fast_arc_score(const uint8_t* __restrict__ ptr, int stride) {
  const int v = ptr[0];
  int d[16];
  d[0] = v - ptr[3 * stride];       d[1] = v - ptr[1 + 3 * stride];   d[2] = v - ptr[2 + 2 * stride];
  d[3] = v - ptr[3 + stride];       d[4] = v - ptr[3];                d[5] = v - ptr[3 - stride];
  d[6] = v - ptr[2 - 2 * stride];   d[7] = v - ptr[1 - 3 * stride];   d[8] = v - ptr[-3 * stride];
  d[9] = v - ptr[-1 - 3 * stride];  d[10] = v - ptr[-2 - 2 * stride]; d[11] = v - ptr[-3 - stride];
  d[12] = v - ptr[-3];              d[13] = v - ptr[-3 + stride];     d[14] = v - ptr[-2 + 2 * stride];
  d[15] = v - ptr[-1 + 3 * stride];
  int lo3[16], hi3[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    lo3[k] = min3i(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
    hi3[k] = max3i(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
  }
  int P = -256, N = 256;
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
    const int p0 = min3i(lo3[k], lo3[(k + 3) & 15], lo3[(k + 6) & 15]);
    const int p1 = min3i(lo3[k + 1], lo3[(k + 4) & 15], lo3[(k + 7) & 15]);
    P = max3i(P, p0, p1);
    const int n0 = max3i(hi3[k], hi3[(k + 3) & 15], hi3[(k + 6) & 15]);
    const int n1 = max3i(hi3[k + 1], hi3[(k + 4) & 15], hi3[(k + 7) & 15]);
    N = min3i(N, n0, n1);
  }
  return max(P, -N);
}

__device__ __forceinline__ int reflect101_f(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// rBRIEF (computeOrbDescriptors, WTA_K = 2) of one level-0 keypoint by one wave, orb_brief_kernel's sampling on a frame of its
// own: (cx, cy) = cvRound of the keypoint's position, (a, b) = cos / sin of its angle, bl = the 7x7 sigma-2 blurred frame
// (orb_blur_kernel), raw = the frame itself.  Lane = (byte, half) evaluates 4 of the 256 tests; lanes 0..7 return dword
// `lane & 7` of the 32-byte descriptor (bytes 4d .. 4d + 3).  Shared by the FAST detector (fast_detect.hip) and the SiftGPU
// keypoints described by ORB (sift_orb.hip).
__device__ __forceinline__ uint32_t brief_level0_dword(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ bl, int rows,
                                                       int cols, int cx, int cy, float a, float b,
                                                       const int8_t* __restrict__ pattern, int lane) {
  const int byte = lane >> 1, half = lane & 1;
  int bits = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int test = byte * 8 + half * 4 + t;
    int v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float px = (float)pattern[(test * 2 + e) * 2], py = (float)pattern[(test * 2 + e) * 2 + 1];
      const float x = px * a - py * b;
      const float y = px * b + py * a;
      const int ix = cx + __float2int_rn(x), iy = cy + __float2int_rn(y);
      if (ix >= 0 && ix < cols && iy >= 0 && iy < rows)
        v[e] = bl[(size_t)iy * cols + ix];
      else  // the unblurred reflect-101 border copyMakeBorder wrote before the in-place blur
        v[e] = raw[(size_t)reflect101_f(iy, rows) * cols + reflect101_f(ix, cols)];
    }
    bits |= (v[0] < v[1]) << (half * 4 + t);
  }
  bits |= __shfl_xor(bits, 1);   // lane 2j: byte j
  const int d = lane & 7;        // lanes 0..7: dword d = bytes 4d .. 4d + 3
  return (uint32_t)(__shfl(bits, 8 * d) & 255) | ((uint32_t)(__shfl(bits, 8 * d + 2) & 255) << 8) |
         ((uint32_t)(__shfl(bits, 8 * d + 4) & 255) << 16) | ((uint32_t)(__shfl(bits, 8 * d + 6) & 255) << 24);
}

}  // namespace rgbdfe
