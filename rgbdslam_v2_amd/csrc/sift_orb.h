// sift_orb.h -- shared by sift_orb.hip (kernels) and api_sift_orb.hip (host side): feature_detector_type "SIFTGPU" with
// feature_extractor_type "ORB" (node.cpp:149-152, 183-210)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rgbdfe_internal.h"

namespace rgbdfe {

// a SiftGPU feature as the SIFT pipeline's keys-only mode leaves it on the device (SiftExtractor::keys_only, 32 bytes):
// image coordinates, scale and orientation in radians as rgbdfe_sift_detect reports them, and cos / sin of the angle
// cv::ORB::compute derives from the keypoint the wrapper rebuilds (formed on the host, where the pipeline lists the features)
struct SiftOrbKey { float x, y, s, o, cos_a, sin_a, pad0, pad1; };
static_assert(sizeof(SiftOrbKey) == 32, "two float4 per feature");

// a keypoint handed to the rBRIEF launch: cvRound of its position and its rotation
struct SiftOrbDescKp { int32_t cx, cy; float cos_a, sin_a; };

// frame f of a chunk: its SiftGPU features and depth image in, the described keypoints and every output out (any output
// pointer may be null; node rows and output rows are device memory, max_keypoints rows each)
struct SiftOrbFrame {
  const SiftOrbKey* keys; int n_keys; const float* depth;
  SiftOrbDescKp* list;
  uint32_t* node_desc; float4* node_xyz;                // ORB node slab rows (8 dwords, 4 floats per row)
  rgbdfe_keypoint* out_kp; uint8_t* out_desc; float4* out_xyz;
};
struct SiftOrbChunk { int n_frames; int32_t* n_out; SiftOrbFrame frame[kSiftNodeFramesMax]; };

// sift_orb_keys: Node::Node's steps between the detection and the descriptors, one workgroup per frame, n_out[f] = the count
void launch_sift_orb_keys(const SiftOrbChunk& ch, int rows, int cols, float fxinv, float fyinv, float cx, float cy,
                          double depth_scaling, int max_keypoints, bool min_depth, hipStream_t stream);
// rBRIEF of every listed keypoint from the blurred frame: frame f's gray image at gray + f * plane, blurred at blur + f * plane
void launch_sift_orb_brief(const SiftOrbChunk& ch, const uint8_t* gray, const uint8_t* blur, uint32_t plane, int rows, int cols,
                           int max_keypoints, const int8_t* pattern, hipStream_t stream);

}  // namespace rgbdfe
