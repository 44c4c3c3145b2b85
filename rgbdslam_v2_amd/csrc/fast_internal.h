// fast_internal.h -- shared by fast_detect.hip (kernels) and api_fast.hip (host side): feature_detector_type "FAST"
// 
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rgbdfe_internal.h"

namespace rgbdfe {

constexpr int kFastMaxCells = 64;  // grid_resolution <= 8

// One grid cell of a frame (VideoGridAdaptedFeatureDetector's rectangle, feature_adjuster.cpp:285-317) as the kernels see
// it: frame coordinates of its sub-image, the pass kernel's 64 x 16 tiles over it, and its regions of the per-frame
// keep-bit and score buffers.  Keep bits: h rows of tiles_x 64-bit words (word w of a row = columns 64w .. 64w + 63).
struct FastCellGeom {
  int32_t x0, y0, w, h;
  int32_t tiles_x, tile_begin;   // tiles of the cell: [tile_begin, tile_begin + tiles_x * ceil(h / 16)) of the frame's
  uint32_t keep_off, score_off;  // in 64-bit words / bytes from the frame's first
};
struct FastGeom {  // a kernel argument (~2 KB)
  int32_t n_cells, tiles_per_frame, rows, cols;
  uint32_t plane;        // bytes of one frame's gray (and mask) image: rows x cols
  uint32_t keep_words;   // keep-bit words per frame
  uint32_t score_bytes;  // score-plane bytes per frame
  int32_t pad;
  FastCellGeom cell[kFastMaxCells];
};

// The adjuster kernel's result per (frame, cell): the cell keeps its survivors with score > cut, and the first `ties` of
// those with score == cut in raster order; `n` of them in all; `thr` = the FAST threshold of the cell's last detect()
struct FastCut { int32_t cut, ties, n, thr; };

struct FastAdjust {
  int32_t n_cells, cell_min, cell_max, max_iters, max_per_cell;
  int32_t fixed_thr;  // >= 0: no adaptation, every survivor at this threshold (rgbdfe_fast_detect)
};

// a keypoint between the kernels: integer position, FAST score, depth (12 bytes)
struct FastKp {
  uint16_t x, y, s, pad;
  float z;
};

// cv::KeyPoint as rgbdfe_keypoint lays it out
struct FastKpOut {
  float x, y, size, angle, response;
  int32_t octave;
};
static_assert(sizeof(FastKpOut) == sizeof(rgbdfe_keypoint), "rgbdfe_keypoint layout");

// where frame f's outputs go (any pointer may be null): node slab rows and the chunk's output rows, all device memory (the
// output rows go to the host behind the chunk, one copy per array)
struct FastFrameOut {
  uint32_t* node_desc;   // 8 dwords per row
  float4* node_xyz;
  FastKpOut* out_kp;
  uint8_t* out_desc;     // 32 bytes per row
  float4* out_xyz;
};

struct FastSelect {
  int32_t n_cells, list_cap, max_kp, min_depth;
  int32_t describe;  // 0: the aggregated keypoint list only (rgbdfe_fast_detect, the cloud path); 1: Node::Node's steps
  int32_t rows, cols, pad;
  float fxinv, fyinv, cx, cy;
  double depth_scaling;
};

void launch_fast_pass(const uint8_t* gray, const uint8_t* mask, const int32_t* has_mask, const FastGeom& g, int n_frames,
                      int floor_thr, uint64_t* keep, uint8_t* score, int32_t* hist, int32_t* mask_nz, hipStream_t s);
void launch_fast_adjust(const int32_t* hist, const int32_t* mask_nz, const int32_t* has_mask, int n_frames,
                        const FastAdjust& a, double* thresh, FastCut* cut, hipStream_t s);
void launch_fast_select(const FastGeom& g, int n_frames, const uint64_t* keep, const uint8_t* score, const FastCut* cut,
                        const float* depth, const FastSelect& p, FastKp* list, const FastFrameOut* outs, int32_t* n_out,
                        hipStream_t s);
void launch_fast_brief(const uint8_t* gray, const uint8_t* blur, uint32_t plane, int rows, int cols, int n_frames, int max_kp,
                       const FastKp* list, int list_cap, const int32_t* n_out, const FastFrameOut* outs,
                       const int8_t* pattern, float cos_a, float sin_a, hipStream_t s);

}  // namespace rgbdfe
