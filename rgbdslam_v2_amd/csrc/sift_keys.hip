// sift_keys.hip -- feature_extractor_type "SIFTGPU" behind the ORB / FAST grid detector (node.cpp:165-176), the steps between
// the detector and the descriptor launch, for a chunk of frames in one launch (gfx950):
//   sift_keys_from_detector  one workgroup of 256 lanes per frame: projectTo3D's walk over the aggregate (node.cpp:900-965) as
//                            an order-preserving compaction -- the inside-the-image / NaN tests, depth(round(y), round(x)) or
//                            the neighbourhood minimum under "use_feature_min_depth" (project3d_device.h), a ballot / mbcnt
//                            rank per wave, a 4-entry wave-offset exchange in LDS, a running base across 256-keypoint
//                            chunks and the first-max_keypoints cut -- then SiftGPUWrapper::detect's conversions
//                            (sift_gpu_wrapper.cpp:135-165, in double, stored as float) for every kept keypoint
//   sift_rows_gather         the descriptor rows of a chunk from the descriptor launch's level order into the callers' order
// The arithmetic is that of rgbdfe_project_to_3d(_min_depth) and rgbdfe_sift_describe: the same bits by construction.
#include "rgbdfe_internal.h"
#include "project3d_device.h"

namespace rgbdfe {

__global__ __launch_bounds__(256) void sift_keys_from_detector_kernel(SiftKeysChunk ch, int rows, int cols, double depth_scaling,
                                                                      int max_keypoints, int min_depth) {
  __shared__ uint32_t wave_cnt[4];
  __shared__ float zs[256];
  const int f = blockIdx.x;
  const SiftKeysFrame F = ch.frame[f];
  const int n_kp = F.n_agg;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t base = 0;
  for (int c0 = 0; c0 < n_kp && base < (uint32_t)max_keypoints; c0 += 256) {
    const int i = c0 + tid;
    if (min_depth) {  // node.cpp:940: getMinDepthInNeighborhood(depth, pt, size), a wave per keypoint
      const int k0 = c0 + wv * 64, kn = min(64, n_kp - k0);
      for (int k = 0; k < kn; ++k) {
        const rgbdfe_keypoint q = F.agg[k0 + k];
        const float z = min_depth_in_neighbourhood(q.x, q.y, q.size, F.depth, rows, cols, lane);
        if (lane == 0) zs[wv * 64 + k] = z;
      }
      __syncthreads();
    }
    bool keep = false;
    rgbdfe_keypoint q{};
    if (i < n_kp) {
      q = F.agg[i];
      const float px = q.x, py = q.y;
      // node.cpp:931-937
      const bool bad = px >= (float)cols || px < 0.f || py >= (float)rows || py < 0.f || __builtin_isnan(px) || __builtin_isnan(py);
      if (!bad) {
        // depth.at<float>(round(y), round(x)) (node.cpp:942), clamped to the last row / column as project3d.hip does
        int r = (int)roundf(py), c = (int)roundf(px);
        r = r >= rows ? rows - 1 : r;
        c = c >= cols ? cols - 1 : c;
        const float zraw = min_depth ? zs[tid] : F.depth[(size_t)r * (size_t)cols + (size_t)c];
        keep = !__builtin_isnan(scaled_depth(zraw, depth_scaling));  // node.cpp:947
      }
    }
    const uint64_t m = __ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t pos = base + rank, total = 0;
    for (int v = 0; v < 4; ++v) {
      if (v < wv) pos += wave_cnt[v];
      total += wave_cnt[v];
    }
    if (keep && pos < (uint32_t)max_keypoints) {
      // SiftGPUWrapper::detect with the list: o = angle / 180 * 3.1415927, s = size / 12 in double, stored as float (:135-136),
      // and the keypoint rebuilt from them: size 12 * s, angle o * 180 / 3.1415927 (:161-164)
      const float s = (float)((double)q.size / 12.0);
      const float o = (float)((double)q.angle / 180.0 * 3.1415927);
      F.keys[pos] = make_float4(q.x, q.y, s, o);
      const float size = (float)(12.0 * (double)s);
      F.rebuilt[pos] = rgbdfe_keypoint{q.x, q.y, size, (float)((double)o * 180.0 / 3.1415927), 0.f, 0};
      F.node_keys[pos] = make_float4(q.x, q.y, size, 0.f);
    }
    __syncthreads();  // wave_cnt and zs are rewritten by the next chunk
    base += total;
  }
  if (tid == 0) ch.n_out[f] = (int32_t)min(base, (uint32_t)max_keypoints);
}

__global__ __launch_bounds__(32) void sift_rows_gather_kernel(const float4* __restrict__ src, const int32_t* __restrict__ map,
                                                             SiftGather g, size_t stride, float4* __restrict__ out) {
  const int r = blockIdx.x, f = blockIdx.y;
  if (r >= g.n[f]) return;
  const int32_t k = map[(size_t)f * stride + r];
  out[((size_t)f * stride + r) * 32 + threadIdx.x] = k >= 0 ? src[(size_t)k * 32 + threadIdx.x] : make_float4(0.f, 0.f, 0.f, 0.f);
}

void launch_sift_keys_from_detector(const SiftKeysChunk& ch, int rows, int cols, double depth_scaling, int max_keypoints,
                                    bool min_depth, hipStream_t stream) {
  if (ch.n_frames > 0)
    hipLaunchKernelGGL(sift_keys_from_detector_kernel, dim3(ch.n_frames), dim3(256), 0, stream, ch, rows, cols, depth_scaling,
                       max_keypoints, min_depth ? 1 : 0);
}

void launch_sift_rows_gather(const float* src, const int32_t* map, const SiftGather& g, size_t stride, float* out,
                             hipStream_t stream) {
  int mx = 0;
  for (int f = 0; f < g.n_frames; ++f) mx = g.n[f] > mx ? g.n[f] : mx;
  if (mx > 0)
    hipLaunchKernelGGL(sift_rows_gather_kernel, dim3(mx, g.n_frames), dim3(32), 0, stream, reinterpret_cast<const float4*>(src),
                       map, g, stride, reinterpret_cast<float4*>(out));
}

}  // namespace rgbdfe
