// map_files.hip -- the byte repacking of a map file's PLY vertices (rgbdfe_save_map), gfx950.
//
// cloud_pack_ply_kernel: cloud rows of 16 bytes (x, y, z, rgb word) -> vertex records of 15 bytes (x, y, z, then bits
// 23-16, 15-8, 7-0 of the rgb word as three bytes).  Four rows are fifteen 32-bit words, so the output is written as whole
// aligned words and never as bytes: a workgroup takes kPlyPackTile rows (256 quads), every lane loads four rows as 16-byte
// units into LDS with the colour bytes already in file order, and after one barrier every lane assembles fifteen output
// words, word t + 256 r in round r, from the two LDS words its four bytes straddle.  Consecutive lanes load consecutive rows
// and store consecutive words.  Rows behind the packed ones read as zeros, so the bytes of the last word behind 15 P are zero.
//
// The rows come as a short carry (0..3 rows the previous group left over) followed by the group's own rows, and the rows that
// do not fill a quad go out as the next carry: every group's vertices then start on a word of the page-locked slot they are
// stored into, whatever the number of points the groups in front kept.
// No atomics, no wave-level operation, 16 KiB of LDS: every output word has exactly one writer.
#include "map_files.h"

namespace rgbdfe {

namespace {

__global__ __launch_bounds__(256) void cloud_pack_ply_kernel(const uint4* __restrict__ carry_in, uint32_t n_carry,
                                                            const uint4* __restrict__ body, uint32_t total, uint32_t packed,
                                                            uint32_t* __restrict__ out, uint4* __restrict__ carry_out) {
  __shared__ uint4 rec[kPlyPackTile];   // a row as the first 15 bytes of its record: x, y, z, then r | g << 8 | b << 16
  const uint32_t t = threadIdx.x;
  const uint32_t row0 = blockIdx.x * kPlyPackTile;
#pragma unroll
  for (uint32_t j = 0; j < kPlyPackTile / 256u; ++j) {
    const uint32_t i = row0 + t + j * 256u;
    uint4 p = make_uint4(0u, 0u, 0u, 0u);
    if (i < total) p = i < n_carry ? carry_in[i] : body[i - n_carry];
    if (i >= packed && i < total) carry_out[i - packed] = p;   // at most three rows of the last workgroup
    if (i >= packed) p = make_uint4(0u, 0u, 0u, 0u);
    p.w = ((p.w >> 16) & 0xffu) | (p.w & 0xff00u) | ((p.w & 0xffu) << 16);
    rec[t + j * 256u] = p;
  }
  __syncthreads();
  const uint32_t* words = reinterpret_cast<const uint32_t*>(rec);
  const uint64_t n_words = ((uint64_t)packed * 15u + 3u) / 4u;
  const uint64_t word0 = (uint64_t)blockIdx.x * kPlyPackTileWords;
#pragma unroll
  for (uint32_t r = 0; r < kPlyPackTileWords / 256u; ++r) {
    const uint32_t g = t + r * 256u;        // output word of the tile: bytes 4 g .. 4 g + 3 of its vertex stream
    if (word0 + g >= n_words) break;
    const uint32_t pk = (4u * g) / 15u;     // the row its first byte belongs to
    const uint32_t o = 4u * g - 15u * pk;   // ... and that byte's place in the record: 0..14
    const uint32_t w = o >> 2, s = (o & 3u) * 8u;
    uint32_t a = words[4u * pk + w], b;
    if (w == 3u) {   // bytes 12..14 of this record, then the next row's x (pk is not the last row of its quad here)
      const uint32_t nx = words[4u * pk + 4u];
      a = (a & 0xffffffu) | (nx << 24);
      b = nx >> 8;
    } else {
      b = words[4u * pk + w + 1u];
    }
    out[word0 + g] = s ? (a >> s) | (b << (32u - s)) : a;
  }
}

}  // namespace

uint32_t launch_cloud_pack_ply(const float4* carry_in, uint32_t n_carry, const float4* body, uint32_t n, bool final, uint32_t* out,
                               float4* carry_out, hipStream_t stream) {
  const uint32_t total = n_carry + n;
  const uint32_t packed = final ? total : (total & ~3u);
  if (total == 0) return 0;
  const uint32_t blocks = (total + kPlyPackTile - 1) / kPlyPackTile;
  hipLaunchKernelGGL(cloud_pack_ply_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const uint4*>(carry_in), n_carry,
                     reinterpret_cast<const uint4*>(body), total, packed, out, reinterpret_cast<uint4*>(carry_out));
  return packed;
}

}  // namespace rgbdfe
