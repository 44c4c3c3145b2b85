// ingest.h -- sensor-frame ingest (ingest.hip): the launch description shared by the kernel and its callers.
// DESIGN.md section 4.16.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rgbdfe {

// One launch: n frames of one geometry, staged back to back.  Frame k's raw bytes start at raw + k * frame_bytes: the
// visual image with tightly packed rows (W * channels bytes each) at offset 0, the depth image with tightly packed rows
// (dW * 4 or dW * 2 bytes each) at depth_off.  frame_bytes and depth_off are multiples of 16.
// Outputs (each may be null) are W x H planes; frame k's plane starts at base + k * stride (elements).
struct IngestParams {
  const uint8_t* raw;
  size_t frame_bytes;
  size_t depth_off;
  int32_t W, H;          // visual size = output size
  int32_t dW, dH;        // depth image size
  int32_t channels;      // 1 (mono8) or 3 (rgb8 / bgr8: CV_RGB2GRAY on the channels as stored)
  int32_t depth_u16;     // 0: 32FC1 metres, 1: 16UC1 millimetres
  const int32_t* xmap;   // resampled depth (dW != W or dH != H): source column of output column x (W entries) ...
  const int32_t* ymap;   // ... and source row of output row y (H entries); both null otherwise
  uint8_t* gray;  size_t gray_stride;
  uint8_t* mask;  size_t mask_stride;
  float* depth_m; size_t depth_stride;
};

// grid (lanes of 16 pixels, frames); the vector instantiation when W % 16 == 0 and the depth image is not resampled
void launch_ingest(const IngestParams& p, int n_frames, hipStream_t stream);

}  // namespace rgbdfe
