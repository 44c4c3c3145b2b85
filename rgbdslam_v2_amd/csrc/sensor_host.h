// sensor_host.h -- the host side of sensor-frame ingest (api_sensor.hip): a validated run of sensor frames as the detect /
// describe pipelines see it in place of the three prepared planes.  The pipelines stage the frames' RAW bytes (rows
// re-packed tightly, nothing else) into page-locked memory, upload them and run ingest.hip's kernel in front of their chain;
// what they look up on the host -- one depth pixel per keypoint (removeDepthless, projectTo3D), the mask's hasNonZero per
// detector cell -- goes through the accessors below, which apply steps 1-2 of include/rgbdfe.h's sensor section to the
// caller's raw depth at the pixel they visit.  No full-frame conversion on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "depth_convert.h"
#include "ingest.h"
#include "rgbdfe.h"

namespace rgbdfe_host {

struct SensorRun {
  const rgbdfe_sensor_frame* frames = nullptr;
  int n = 0;
  int W = 0, H = 0, dW = 0, dH = 0, channels = 1;
  bool u16 = false, resample = false;
  size_t vis_bytes = 0, dep_bytes = 0, depth_off = 0, frame_bytes = 0;  // a staged frame: [visual | pad to 16 | depth | pad to 16]
  std::vector<int32_t> xmap, ymap;     // resample: source column / row of an output column / row (OpenCV 3.3 resizeNN)
  const int32_t* d_maps = nullptr;     // resample: the two tables on the device, xmap (W) then ymap (H)

  // sizes of a staged frame and, for a depth image of another size, the two index tables -- OpenCV 3.3 resizeNN:
  // x_ofs[x] = min(cvFloor(x * ifx), src.cols - 1) with ifx = 1 / ((double)dst.cols / src.cols), rows alike
  void layout() {
    resample = W != dW || H != dH;
    vis_bytes = (size_t)W * H * channels;
    dep_bytes = (size_t)dW * dH * (u16 ? 2 : 4);
    depth_off = (vis_bytes + 15) & ~(size_t)15;
    frame_bytes = depth_off + ((dep_bytes + 15) & ~(size_t)15);
    xmap.clear(); ymap.clear();
    if (!resample) return;
    const double ifx = 1.0 / ((double)W / dW), ify = 1.0 / ((double)H / dH);
    xmap.resize((size_t)W);
    ymap.resize((size_t)H);
    for (int x = 0; x < W; ++x) { const int sx = (int)std::floor(x * ifx); xmap[(size_t)x] = sx < dW - 1 ? sx : dW - 1; }
    for (int y = 0; y < H; ++y) { const int sy = (int)std::floor(y * ify); ymap[(size_t)y] = sy < dH - 1 ? sy : dH - 1; }
  }
  // the depth image every later step sees, in metres, at (r, c) of the visual raster
  float depth_at(int f, int r, int c) const {
    const rgbdfe_sensor_frame& fr = frames[f];
    const int sr = resample ? ymap[(size_t)r] : r, sc = resample ? xmap[(size_t)c] : c;
    const char* row = (const char*)fr.depth + (size_t)sr * (size_t)fr.depth_step;
    if (u16) {
      uint16_t v;
      memcpy(&v, row + (size_t)sc * 2, 2);
      return rgbdfe::depth_mm_to_metres((float)v);
    }
    float v;
    memcpy(&v, row + (size_t)sc * 4, 4);
    return v;
  }
  uint8_t mono8_at(int f, int r, int c) const {
    const rgbdfe_sensor_frame& fr = frames[f];
    const int sr = resample ? ymap[(size_t)r] : r, sc = resample ? xmap[(size_t)c] : c;
    const char* row = (const char*)fr.depth + (size_t)sr * (size_t)fr.depth_step;
    if (u16) {
      uint16_t v;
      memcpy(&v, row + (size_t)sc * 2, 2);
      return rgbdfe::depth_mm_to_mono8((float)v);
    }
    float v;
    memcpy(&v, row + (size_t)sc * 4, 4);
    return rgbdfe::depth_f32_to_mono8(v);
  }
  // hasNonZero(mask(cell)) (feature_adjuster.cpp:175-183)
  bool mask_nonzero(int f, int x0, int y0, int w, int h) const {
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        if (mono8_at(f, y0 + y, x0 + x)) return true;
    return false;
  }
  // frame f's raw bytes into a staging buffer of frame_bytes (any thread; the only thing staging does)
  void stage(int f, uint8_t* dst) const {
    const rgbdfe_sensor_frame& fr = frames[f];
    const size_t vrow = (size_t)W * (size_t)channels, drow = (size_t)dW * (u16 ? 2 : 4);
    if ((size_t)fr.visual_step == vrow) memcpy(dst, fr.visual, vrow * (size_t)H);
    else
      for (int y = 0; y < H; ++y) memcpy(dst + (size_t)y * vrow, fr.visual + (size_t)y * (size_t)fr.visual_step, vrow);
    uint8_t* d = dst + depth_off;
    if ((size_t)fr.depth_step == drow) memcpy(d, fr.depth, drow * (size_t)dH);
    else
      for (int y = 0; y < dH; ++y) memcpy(d + (size_t)y * drow, (const char*)fr.depth + (size_t)y * (size_t)fr.depth_step, drow);
  }
  // the launch description of n_frames staged frames at d_raw; the callers fill in the outputs
  rgbdfe::IngestParams params(const uint8_t* d_raw) const {
    rgbdfe::IngestParams p{};
    p.raw = d_raw; p.frame_bytes = frame_bytes; p.depth_off = depth_off;
    p.W = W; p.H = H; p.dW = dW; p.dH = dH; p.channels = channels; p.depth_u16 = u16 ? 1 : 0;
    p.xmap = resample ? d_maps : nullptr;
    p.ymap = resample ? d_maps + W : nullptr;
    return p;
  }
};

}  // namespace rgbdfe_host
