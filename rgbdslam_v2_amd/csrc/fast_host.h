// fast_host.h -- the per-context workspace of feature_detector_type "FAST" (api_fast.hip): no pyramids, no per-frame host
// work between the upload of a chunk of frames and its outputs
#pragma once
#include <string>
#include <vector>

#include "fast_internal.h"
#include "orb_internal.h"

namespace rgbdfe {

struct FastWorkspace {
  static constexpr int kSlots = 3;  // chunks in flight: staged / uploaded / computed
  // geometry of the current buffers (a call with another one rebuilds them)
  int W = 0, H = 0, grid = 0, list_cap = 0, out_rows = 0;
  bool use_grid = false, describe = false;
  FastGeom geom{};
  int version = 0;
  uint32_t plane = 0;
  int blur_units_per_frame = 0;
  // one chunk of up to `cap` frames: device buffers, page-locked staging and host-output rows
  struct Slot {
    int cap = 0;
    int version = -1;            // the geometry its buffers are laid out for
    void* dev = nullptr;
    void* pin = nullptr;
    size_t dev_bytes = 0, pin_bytes = 0;   // allocations only grow: a new geometry is laid out in the old ones if it fits
    uint8_t* d_img = nullptr;    // gray images of the chunk, then their masks (cap x plane each)
    uint8_t* d_blur = nullptr;
    float* d_depth = nullptr;
    int32_t* d_has_mask = nullptr;
    uint64_t* d_keep = nullptr;
    uint8_t* d_score = nullptr;
    int32_t* d_hist = nullptr;   // cap x cells x 256 survivor-score histograms, then cap x cells hasNonZero flags
    int32_t* d_mask_nz = nullptr;
    size_t hist_bytes = 0;       // both
    FastCut* d_cut = nullptr;
    FastKp* d_list = nullptr;
    int32_t* d_n = nullptr;
    FastFrameOut* d_outs = nullptr;
    FastKpOut* d_kp = nullptr; uint8_t* d_desc = nullptr; float4* d_xyz = nullptr;  // output rows: out_rows per frame
    ImgDesc* d_frame_imgs = nullptr;
    TileUnit* d_blur_units = nullptr;
    uint8_t* h_img = nullptr; float* h_depth = nullptr; int32_t* h_has_mask = nullptr;  // staging
    FastFrameOut* h_outs = nullptr;
    int32_t* h_n = nullptr;
    FastKpOut* h_kp = nullptr; uint8_t* h_desc = nullptr; float4* h_xyz = nullptr;      // their host copies
    FastKp* h_list = nullptr;                                                           // list_cap (detect-only calls)
    hipEvent_t uploaded = nullptr, done = nullptr;
  } slot[kSlots];
  hipStream_t st = nullptr, up = nullptr;  // kernels / uploads (+ the blur, which needs nothing else)
  double* d_thresh = nullptr; double* h_thresh = nullptr;
  int8_t* d_pattern = nullptr;
  ~FastWorkspace();
  void release_slot(Slot& s);
  void release();
  // (re)builds the geometry for a frame size and cell layout (ensure_slot then lays the slots out again)
  int prepare(int cols, int rows, int grid_res, bool grid, int max_total, int max_kp, bool describe, std::string& err);
  int ensure_slot(int i, int frames, std::string& err);
  int ensure_common(std::string& err);
};

}  // namespace rgbdfe
