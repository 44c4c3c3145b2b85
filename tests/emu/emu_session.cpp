// tests/emu/emu_session.cpp -- TEST INFRASTRUCTURE ONLY: csrc/session.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_session_pack_kernel.py builds it: the kernel SOURCE of the product runs, one
// OS thread per HIP thread).
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include "session.hip"

// table: n x {slot, rows, first_row, has_kp}.  A NULL slab reads as zeros, a NULL output is left out.  Returns the launches.
extern "C" int emu_node_pack(const uint32_t* table, uint32_t n, uint32_t max_rows, const void* desc, uint32_t desc_units,
                             const void* xyz, const void* kp, const uint8_t* stats, uint32_t max_kp, uint32_t stats_stride,
                             void* out_desc, void* out_xyz, void* out_kp, uint8_t* out_stats) {
  rgbdfe::NodePackArgs a{};
  a.desc = static_cast<const uint4*>(desc); a.desc_units = desc_units;
  a.xyz = static_cast<const uint4*>(xyz); a.kp = static_cast<const float2*>(kp); a.stats = stats;
  a.max_kp = max_kp; a.stats_stride = stats_stride;
  a.out_desc = static_cast<uint4*>(out_desc); a.out_xyz = static_cast<uint4*>(out_xyz);
  a.out_kp = static_cast<float2*>(out_kp); a.out_stats = out_stats;
  return rgbdfe::launch_node_pack(reinterpret_cast<const rgbdfe::NodePackEntry*>(table), n, max_rows, a, nullptr);
}
