// sift_orb.hip -- feature_detector_type "SIFTGPU" with feature_extractor_type "ORB" (node.cpp:149-152, 183-210): Node::Node's
// ORB-extractor steps behind SiftGPU's own detection, for a chunk of frames, on the device-resident keypoint lists the SIFT
// pipeline's keys-only mode leaves (gfx950):
//   sift_orb_keys   one workgroup of 256 lanes per frame, in the reference's order: the wrapper's conversions of size and
//                   angle (sift_gpu_wrapper.cpp:156-160), removeDepthless (node.cpp:186; :82 under "use_feature_min_depth")
//                   as an order-preserving compaction, the max_keypoints cut (retainBest + resize, :188-191: every response
//                   is 0, so the first max_keypoints survivors), cv::ORB::compute's 31-pixel border filter (level 0 only:
//                   every octave is 0), then projectTo3D (:210) into the node slab and / or the chunk's output rows.  The
//                   second removeDepthless (:206) sees the positions and sizes the first one passed: it keeps them all.
//   sift_orb_brief  rBRIEF at each keypoint's own angle on the 7x7 sigma-2 blurred frame (orb_blur_kernel), one wave per
//                   keypoint (brief_level0_dword, shared with the FAST detector)
// The depth arithmetic is project3d_device.h's, the compaction that of sift_keys_from_detector: the same bits as
// rgbdfe_project_to_3d(_min_depth) and rgbdfe_orb_compute by construction.
#include "sift_orb.h"
#include "fast_device.h"
#include "project3d_device.h"

namespace rgbdfe {

__global__ __launch_bounds__(256) void sift_orb_keys_kernel(SiftOrbChunk ch, int rows, int cols, float fxinv, float fyinv, float cx,
                                                            float cy, double depth_scaling, int max_keypoints, int min_depth) {
  __shared__ uint32_t cnt1[4], cnt2[4];
  __shared__ float zs[256];
  const int f = blockIdx.x;
  const SiftOrbFrame F = ch.frame[f];
  const int n_kp = F.n_keys;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t base1 = 0, base2 = 0;   // removeDepthless' survivors / the final keypoints so far
  for (int c0 = 0; c0 < n_kp && base1 < (uint32_t)max_keypoints; c0 += 256) {
    const int i = c0 + tid;
    if (min_depth) {  // node.cpp:82: getMinDepthInNeighborhood(depth, pt, size), a wave per keypoint
      const int k0 = c0 + wv * 64, kn = min(64, n_kp - k0);
      for (int k = 0; k < kn; ++k) {
        const SiftOrbKey q = F.keys[k0 + k];
        const float z = min_depth_in_neighbourhood(q.x, q.y, (float)(12.0 * (double)q.s), F.depth, rows, cols, lane);
        if (lane == 0) zs[wv * 64 + k] = z;
      }
      __syncthreads();
    }
    bool keep1 = false;
    SiftOrbKey q{};
    float z = 0.f;
    if (i < n_kp) {
      q = F.keys[i];
      // node.cpp:73-80
      const bool bad = q.x >= (float)cols || q.x < 0.f || q.y >= (float)rows || q.y < 0.f || __builtin_isnan(q.x) ||
                       __builtin_isnan(q.y);
      if (!bad) {
        // depth.at<float>(round(y), round(x)) (node.cpp:84), clamped to the last row / column as project3d.hip does
        int r = (int)roundf(q.y), c = (int)roundf(q.x);
        r = r >= rows ? rows - 1 : r;
        c = c >= cols ? cols - 1 : c;
        z = min_depth ? zs[tid] : F.depth[(size_t)r * (size_t)cols + (size_t)c];
        keep1 = !__builtin_isnan(z);  // node.cpp:87
      }
    }
    const uint64_t m1 = __ballot(keep1);
    const uint32_t rank1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
    if (lane == 0) cnt1[wv] = (uint32_t)__popcll(m1);
    __syncthreads();
    uint32_t pos1 = base1 + rank1, tot1 = 0;
    for (int v = 0; v < 4; ++v) {
      if (v < wv) pos1 += cnt1[v];
      tot1 += cnt1[v];
    }
    // the cut, ORB::compute's runByImageBorder(31) (orb_host.hip compute_enqueue), projectTo3D's NaN test on the scaled depth
    // (node.cpp:947; a removeDepthless survivor fails it only when depth_scaling turns a depth into NaN)
    const float Z = scaled_depth(z, depth_scaling);
    const bool keep2 = keep1 && pos1 < (uint32_t)max_keypoints && q.x >= 31.f && q.x < (float)(cols - 31) && q.y >= 31.f &&
                       q.y < (float)(rows - 31) && !__builtin_isnan(Z);
    const uint64_t m2 = __ballot(keep2);
    const uint32_t rank2 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0u));
    if (lane == 0) cnt2[wv] = (uint32_t)__popcll(m2);
    __syncthreads();
    uint32_t pos2 = base2 + rank2, tot2 = 0;
    for (int v = 0; v < 4; ++v) {
      if (v < wv) pos2 += cnt2[v];
      tot2 += cnt2[v];
    }
    if (keep2) {   // pos2 <= pos1 < max_keypoints
      F.list[pos2] = SiftOrbDescKp{__float2int_rn(q.x), __float2int_rn(q.y), q.cos_a, q.sin_a};   // cvRound
      const float4 xyz = back_project(q.x, q.y, Z, cx, cy, fxinv, fyinv);   // misc2.h:62-64, node.cpp:955
      if (F.node_xyz) F.node_xyz[pos2] = xyz;
      if (F.out_xyz) F.out_xyz[pos2] = xyz;
      // KeyPoint(x, y, 12.0 * s, o * 180.0 / 3.1415927): double arithmetic stored as float, response = octave = 0
      if (F.out_kp)
        F.out_kp[pos2] = rgbdfe_keypoint{q.x, q.y, (float)(12.0 * (double)q.s), (float)((double)q.o * 180.0 / 3.1415927), 0.f, 0};
    }
    __syncthreads();  // cnt1, cnt2 and zs are rewritten by the next chunk
    base1 += tot1;
    base2 += tot2;
  }
  if (tid == 0) ch.n_out[f] = (int32_t)base2;
}

__global__ __launch_bounds__(256) void sift_orb_brief_kernel(SiftOrbChunk ch, const uint8_t* __restrict__ gray,
                                                             const uint8_t* __restrict__ blur, uint32_t plane, int rows, int cols,
                                                             const int8_t* __restrict__ pattern) {
  const int f = blockIdx.y;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= ch.n_out[f]) return;
  const int lane = threadIdx.x & 63;
  const SiftOrbFrame& F = ch.frame[f];
  const SiftOrbDescKp kp = F.list[k];
  const uint32_t word = brief_level0_dword(gray + (size_t)f * plane, blur + (size_t)f * plane, rows, cols, kp.cx, kp.cy, kp.cos_a,
                                           kp.sin_a, pattern, lane);
  if (lane < 8) {
    if (F.node_desc) F.node_desc[(size_t)k * 8 + lane] = word;
    if (F.out_desc) reinterpret_cast<uint32_t*>(F.out_desc)[(size_t)k * 8 + lane] = word;
  }
}

void launch_sift_orb_keys(const SiftOrbChunk& ch, int rows, int cols, float fxinv, float fyinv, float cx, float cy,
                          double depth_scaling, int max_keypoints, bool min_depth, hipStream_t stream) {
  if (ch.n_frames > 0)
    hipLaunchKernelGGL(sift_orb_keys_kernel, dim3(ch.n_frames), dim3(256), 0, stream, ch, rows, cols, fxinv, fyinv, cx, cy,
                       depth_scaling, max_keypoints, min_depth ? 1 : 0);
}

void launch_sift_orb_brief(const SiftOrbChunk& ch, const uint8_t* gray, const uint8_t* blur, uint32_t plane, int rows, int cols,
                           int max_keypoints, const int8_t* pattern, hipStream_t stream) {
  if (ch.n_frames > 0 && max_keypoints > 0)
    hipLaunchKernelGGL(sift_orb_brief_kernel, dim3((max_keypoints + 3) / 4, ch.n_frames), dim3(256), 0, stream, ch, gray, blur,
                       plane, rows, cols, pattern);
}

}  // namespace rgbdfe
