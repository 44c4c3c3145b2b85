// sift_nodes.hip -- Node::Node's SIFTGPU branch after the extraction, for a chunk of frames in one launch (gfx950):
// projectTo3DSiftGPU (src/node.cpp:695-769) + squareroot_descriptor_space (:1557-1571) straight into the node slabs
// (rgbdfe_sift_detect_batch_nodes, api_detect.hip).
//
// One workgroup of 256 lanes per frame.  Per 256-keypoint chunk of the frame's feature list:
//   1. the depth of every keypoint: depth(int(y), int(x)) clamped to the image, or -- under "use_feature_min_depth" -- the
//      neighbourhood minimum (each wave takes 64 keypoints one after the other, its lanes along the window's columns);
//   2. NaN depths drop out; the survivors are compacted in list order (ballot / mbcnt inside a wave, a 4-entry wave-offset
//      exchange in LDS, a running base across chunks) and cut at max_keypoints (:748);
//   3. a survivor's point is backProject'ed into its row of the node's xyz slab;
//   4. its descriptor row is read by the whole wave (lane l: columns 2l, 2l+1), RootSIFT-normalised when asked and written
//      into the node's float slab -- the wave walks its survivors one by one (a ballot mask), so no index list is needed.
// The per-keypoint arithmetic is project3d_device.h's, the same the single-frame kernels of project3d.hip use: bit-equal to
// rgbdfe_sift_node_features by construction.  Traffic: one depth load per keypoint (a window under min-depth), 512 bytes in
// and 512 out per kept row.
#include "rgbdfe_internal.h"
#include "project3d_device.h"

namespace rgbdfe {

__global__ __launch_bounds__(256) void sift_nodes_kernel(SiftNodeChunk ch, int rows, int cols, float fxinv, float fyinv, float cx,
                                                         float cy, double depth_scaling, int max_keypoints, int min_depth,
                                                         int root_sift) {
  __shared__ uint32_t wave_cnt[4];
  __shared__ float zs[256];
  const int f = blockIdx.x;
  const SiftNodeFrame F = ch.frame[f];
  const float4* __restrict__ keys = F.keys;
  const float2* __restrict__ desc = F.desc;
  const float* __restrict__ depth = F.depth;
  const int n_kp = F.n_keys;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  uint32_t base = 0;
  for (int c0 = 0; c0 < n_kp; c0 += 256) {
    const int i = c0 + tid;
    if (min_depth) {  // node.cpp:727-731: getMinDepthInNeighborhood(depth, pt, size)
      const int k0 = c0 + wv * 64;
      const int kn = min(64, n_kp - k0);
      for (int k = 0; k < kn; ++k) {
        const float4 kp = keys[k0 + k];
        const float z = min_depth_in_neighbourhood(kp.x, kp.y, kp.z, depth, rows, cols, lane);
        if (lane == 0) zs[wv * 64 + k] = z;
      }
      __syncthreads();
    }
    bool keep = false;
    float px = 0.f, py = 0.f, Z = 0.f;
    if (i < n_kp) {
      const float4 kp = keys[i];
      px = kp.x; py = kp.y;
      const float zraw = min_depth ? zs[tid] : depth[sift_depth_index(px, py, rows, cols)];  // :731 / :733
      Z = scaled_depth(zraw, depth_scaling);
      keep = !__builtin_isnan(Z);  // :736
    }
    const uint64_t m = __ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = base;
    for (int k = 0; k < wv; ++k) off += wave_cnt[k];
    const uint32_t chunk_total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    const uint32_t pos = off + rank;
    const bool used = keep && pos < (uint32_t)max_keypoints;  // :748
    if (used) {
      const float4 p = back_project(px, py, Z, cx, cy, fxinv, fyinv);
      if (F.xyz) F.xyz[pos] = p;
      if (F.xyz_out) F.xyz_out[pos] = p;
      if (F.kept_out) F.kept_out[pos] = i;
    }
    // the wave's used rows, in order: row pos <- descriptor i (:752-766), RootSIFT'ed (:1557-1571)
    uint64_t todo = __ballot(used);
    while (todo) {
      const int l = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int src = __shfl(i, l);
      const uint32_t dst = (uint32_t)__shfl((int)pos, l);
      const float2 v = desc[(size_t)src * 64 + lane];
      const float2 o = root_sift ? root_sift_row(v) : v;
      if (F.feat) F.feat[(size_t)dst * 64 + lane] = o;
      if (F.feat_out) F.feat_out[(size_t)dst * 64 + lane] = o;
    }
    base += chunk_total;
    __syncthreads();
    if (base >= (uint32_t)max_keypoints) break;  // :748
  }
  if (tid == 0) ch.n_out[f] = (int32_t)min(base, (uint32_t)max_keypoints);
}

void launch_sift_nodes(const SiftNodeChunk& ch, int rows, int cols, float fxinv, float fyinv, float cx, float cy,
                       double depth_scaling, int max_keypoints, bool min_depth, bool root_sift, hipStream_t stream) {
  if (ch.n_frames > 0)
    hipLaunchKernelGGL(sift_nodes_kernel, dim3(ch.n_frames), dim3(256), 0, stream, ch, rows, cols, fxinv, fyinv, cx, cy,
                       depth_scaling, max_keypoints, min_depth ? 1 : 0, root_sift ? 1 : 0);
}

}  // namespace rgbdfe
