// map_files.h -- what map_files.hip (the PLY pack kernel) and api_map_files.hip (host side) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbdfe {

constexpr uint32_t kPlyPackTile = 1024;                      // points of one workgroup: 256 quads
constexpr uint32_t kPlyPackTileWords = kPlyPackTile / 4 * 15;  // the 32-bit words they become

// The rows of one group as PLY vertices.  The sequence is `n_carry` (0..3) rows of carry_in followed by the n rows of `body`.
// Of its T = n_carry + n rows, P = T (final) or the largest multiple of four below or equal to T are packed: ceil(15 P / 4)
// whole words go to `out` (4-byte aligned; the bytes of the last word behind 15 P are zero), and the T - P rows that are
// left go to carry_out[0 ..] for the next group.  carry_in and carry_out are different buffers of three rows.
// Returns P.  n_carry + n < 2^32.  No launch when T == 0.
uint32_t launch_cloud_pack_ply(const float4* carry_in, uint32_t n_carry, const float4* body, uint32_t n, bool final, uint32_t* out,
                               float4* carry_out, hipStream_t stream);

}  // namespace rgbdfe
