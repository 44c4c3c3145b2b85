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

}  // namespace rgbdfe
