// tests/emu/emu_map_files.cpp -- TEST INFRASTRUCTURE ONLY: csrc/map_files.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_ply_pack_kernel.py builds it: the kernel SOURCE of the product runs, one
// OS thread per HIP thread).
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include "map_files.hip"

// rows: carry_in (n_carry rows of 16 bytes) then body (n rows); returns the rows packed (see map_files.h)
extern "C" unsigned emu_cloud_pack_ply(const void* carry_in, unsigned n_carry, const void* body, unsigned n, int final, void* out,
                                       void* carry_out) {
  return rgbdfe::launch_cloud_pack_ply(static_cast<const float4*>(carry_in), n_carry, static_cast<const float4*>(body), n, final != 0,
                                       static_cast<uint32_t*>(out), static_cast<float4*>(carry_out), nullptr);
}

extern "C" unsigned emu_ply_pack_tile() { return rgbdfe::kPlyPackTile; }
