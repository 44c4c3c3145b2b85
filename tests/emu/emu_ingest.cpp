// tests/emu/emu_ingest.cpp -- TEST INFRASTRUCTURE ONLY: csrc/ingest.hip compiled as host C++ over tests/emu/hip/hip_runtime.h
// (tests/test_oracle_ingest.py builds it: the kernel SOURCE of the product runs, one OS thread per HIP thread; the kernel
// has no wave-level operation and no barrier).  Staging and the index tables are the product's too (csrc/sensor_host.h).
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include "ingest.hip"
#include "sensor_host.h"

namespace {
template <class T>
T* aligned(size_t n) { return static_cast<T*>(aligned_alloc(64, ((n * sizeof(T) + 63) / 64) * 64)); }
}  // namespace

// One sensor frame through SensorRun::stage -> launch_ingest; outputs rows x cols, each may be null.  misalign != 0 shifts the
// output planes off 16-byte alignment (the launcher must then take the scalar instantiation).  Returns the number of frames run.
extern "C" int emu_ingest(const rgbdfe_sensor_frame* frame, uint8_t* gray, uint8_t* mono8, float* depth_m, int misalign) {
  rgbdfe_host::SensorRun run;
  run.frames = frame; run.n = 1;
  run.W = frame->visual_cols; run.H = frame->visual_rows; run.dW = frame->depth_cols; run.dH = frame->depth_rows;
  run.channels = frame->visual_encoding == RGBDFE_VISUAL_MONO8 ? 1 : 3;
  run.u16 = frame->depth_encoding == RGBDFE_DEPTH_16UC1;
  run.layout();
  const size_t plane = (size_t)run.W * run.H;
  uint8_t* raw = aligned<uint8_t>(run.frame_bytes);
  uint8_t* g = aligned<uint8_t>(plane + 64);
  uint8_t* m = aligned<uint8_t>(plane + 64);
  float* d = aligned<float>(plane + 64);
  memset(raw, 0, run.frame_bytes);
  run.stage(0, raw);
  std::vector<int32_t> maps;
  if (run.resample) {
    maps.insert(maps.end(), run.xmap.begin(), run.xmap.end());
    maps.insert(maps.end(), run.ymap.begin(), run.ymap.end());
    run.d_maps = maps.data();
  }
  const int sh = misalign ? 1 : 0;
  rgbdfe::IngestParams p = run.params(raw);
  p.gray = gray ? g + sh : nullptr;
  p.mask = mono8 ? m + sh : nullptr;
  p.depth_m = depth_m ? d + sh : nullptr;
  rgbdfe::launch_ingest(p, 1, nullptr);
  if (gray) memcpy(gray, g + sh, plane);
  if (mono8) memcpy(mono8, m + sh, plane);
  if (depth_m) memcpy(depth_m, d + sh, plane * 4);
  free(raw); free(g); free(m); free(d);
  return 1;
}
