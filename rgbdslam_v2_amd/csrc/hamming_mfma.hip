// hamming_mfma.hip -- the 256-bit Hamming distance matrix as an exact fp4 contraction on the gfx950 matrix cores.
//
// Same contract as hamming_nn.hip (the popcount kernel): for every query row of the newer node the nearest train row
// of the older node under bruteForceSearchORB's rules (features.cpp:163-182: rows [0, nt-1) only, strict <, first
// minimum wins), delivered as (hd << 16 | row) keys.  The arithmetic is different:
//
//   * every descriptor bit becomes one fp4 (E2M1) operand nibble: +1.0 (0x2) for a 0 bit, -1.0 (0xA) for a 1 bit
//     (hamming_expand_kernel, once per node upload; 128 bytes per descriptor, stored in MFMA fragment order);
//     the query side flips the sign bit of every nibble on load, so one product is -1 for equal bits and +1 for
//     different bits and the 256-term dot product is  2*hd - 256  -- small integers, exact in the f32 accumulator;
//   * v_mfma_f32_32x32x64_f8f6f4 (cbsz = blgp = 4: both operands fp4) does 32 train rows x 32 queries x 64 bits per
//     instruction, four of them per 32x32 tile: 2*32*32*256 FLOP at the fp4 rate (4x the bf16 rate) instead of
//     16 VALU instructions per 64 compares;
//   * the accumulator is initialised with  256 + row_in_tile / 2^14, so an accumulator element is the complete sort key
//     2*hd + row/2^14  (24 significant bits at most: exact in f32), non-negative, hence ordered like its bit pattern:
//     "first minimum wins" is an unsigned integer minimum; train rows run along the accumulator registers of a lane,
//     queries along the lanes, so the running minimum is ONE register per 32-query tile and the epilogue is a
//     v_min3_u32 tree: 10 VALU instructions per 16 matrix elements;
//   * a 256-thread block holds 256 queries (two 32-query operand tiles per wave) and streams the train tiles of the
//     pair through LDS (16 KB stages, double buffered, one barrier per stage); the four waves share every tile.
//
// MODE 1 adds the row term inside the MFMA (C operand); MODE 2 starts from C = 0 and adds it with v_add_f32 (kept as
// the conservative variant: it does not rely on the matrix core adding a 2^-14-granular C to the integer sum exactly);
// MODE 3 (hamming_mfma_pipe_kernel below, the default since round 4) is mode 1's arithmetic as a software pipeline inside
// every wave: reductions and LDS reads between the MFMAs, train tiles by global_load_lds through three LDS buffers;
// hamming_mfma_x16_kernel (further below, what mode 3 runs for large batches) is its 512-query block on 16x16x128 tiles.
// Keys are identical to the popcount kernel's, bit for bit (tests/test_gpu_hamming.py runs every mode against the
// golden vectors of the reference function).  Usable while max_keypoints <= 32768 (15 index bits next to 9 distance
// bits in a 24-bit significand); the host falls back to the popcount kernel above that.
#include "rgbdfe_internal.h"

namespace rgbdfe {

// The train tiles of ONE block of hamming_mfma_pipe_kernel (mode 3) as slots of four-tile stages: the block's full tiles
// first, then phantoms, the pair's ragged tile -- if it is this block's -- in the LAST slot of the last stage.  Host and
// device (rgbdfe_debug_hamming_slots, tests/test_hamming_slots.py check the enumeration without a GPU).
constexpr uint32_t kHammingPhantomTile = 0x7FFFFFFFu;
struct HammingSlots {
  uint32_t nt_search, n_ttiles, tile0, tile1, n_full, n_stages, last_slot;
  bool has_ragged;
  __host__ __device__ static HammingSlots make(uint32_t nt, uint32_t tsplit, uint32_t split, uint32_t tiles_per_stage) {
    HammingSlots s;
    s.nt_search = nt > 0 ? nt - 1u : 0u;   // features.cpp:174 (and D4): the node's last row is never a candidate
    s.n_ttiles = (s.nt_search + 31u) >> 5;
    s.tile0 = 0; s.tile1 = s.n_ttiles;
    if (tsplit > 1u) {
      const uint32_t chunk = (s.n_ttiles + tsplit - 1u) / tsplit;
      s.tile0 = split * chunk < s.n_ttiles ? split * chunk : s.n_ttiles;
      s.tile1 = s.tile0 + chunk < s.n_ttiles ? s.tile0 + chunk : s.n_ttiles;
    }
    const uint32_t full_tiles = s.nt_search >> 5;
    const uint32_t fend = s.tile1 < full_tiles ? s.tile1 : full_tiles;
    s.n_full = fend > s.tile0 ? fend - s.tile0 : 0u;
    s.has_ragged = (s.nt_search & 31u) != 0u && s.tile1 == s.n_ttiles && s.tile1 > s.tile0;
    s.n_stages = (s.n_full + (s.has_ragged ? 1u : 0u) + tiles_per_stage - 1u) / tiles_per_stage;
    s.last_slot = s.n_stages * tiles_per_stage - 1u;
    return s;
  }
  __host__ __device__ uint32_t tile(uint32_t slot) const {
    const uint32_t behind = (has_ragged & (slot == last_slot)) ? n_ttiles - 1u : kHammingPhantomTile;   // (selects, no branches)
    return slot < n_full ? tile0 + slot : behind;
  }
};

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
#ifndef RGBDFE_HAMMING_QT
#define RGBDFE_HAMMING_QT 2
#endif
#ifndef RGBDFE_HAMMING_STAGE
#define RGBDFE_HAMMING_STAGE 4
#endif
constexpr int kQT = RGBDFE_HAMMING_QT;          // 32-query operand tiles per wave
constexpr int kQueriesPerBlock = 4 * kQT * 32;  // 256
constexpr int kStage = RGBDFE_HAMMING_STAGE;    // train tiles (of 32 rows, 4 KB each) per LDS stage
constexpr float kNone = 3.0e38f;
constexpr float kRowUnit = 1.0f / 16384.0f;  // 2^-14
constexpr float kBias = 256.0f;  // element = 2*hd + row / 2^14 >= 0 (24 significant bits at most: 2*hd <= 512, row < 2^15)

// 8 descriptor bits -> 8 fp4 nibbles (0x2 = +1.0 for a 0 bit, 0xA = -1.0 for a 1 bit)
__device__ __forceinline__ uint32_t spread8(uint32_t x) {
  uint32_t t = (x | (x << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  t = (t | (t << 3)) & 0x11111111u;
  return 0x22222222u | (t << 3);
}

// One thread per (row of a 32-row tile, descriptor dword): writes the 16 bytes lane (half*32 + row) feeds to k-step s,
// with dword = 2*s + half.  Rows >= n of a touched tile are written as zeros (0.0 operands).
__global__ __launch_bounds__(256) void hamming_expand_kernel(const uint32_t* __restrict__ rows, uint4* __restrict__ tiles,
                                                             uint32_t n) {
  const uint32_t gid = blockIdx.x * 256u + threadIdx.x;  // tile*256 + s*64 + half*32 + row
  const uint32_t tile = gid >> 8, s = (gid >> 6) & 3u, half = (gid >> 5) & 1u, r = gid & 31u;
  const uint32_t row = tile * 32u + r;
  if (tile * 32u >= n) return;
  uint4 o = make_uint4(0u, 0u, 0u, 0u);
  if (row < n) {
    const uint32_t w = rows[(size_t)row * 8u + 2u * s + half];
    o.x = spread8(w & 0xFFu);
    o.y = spread8((w >> 8) & 0xFFu);
    o.z = spread8((w >> 16) & 0xFFu);
    o.w = spread8(w >> 24);
  }
  tiles[gid] = o;
}

__device__ __forceinline__ v8i as_operand(uint4 v) {
  v8i o;
  o[0] = (int)v.x; o[1] = (int)v.y; o[2] = (int)v.z; o[3] = (int)v.w;
  o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;
  return o;
}

__device__ __forceinline__ v8i op8(v4i v) {
  v8i o;
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;
  return o;
}

// Accumulator elements are non-negative (the C operand carries a +256 bias next to the row term), and non-negative
// floats order like their bit patterns: the minimum is an INTEGER min3 tree -- fminf would add a canonicalising v_max
// in front of every v_min3_f32 (44 of ~190 VALU instructions per four tiles).
__device__ __forceinline__ uint32_t min16(const v16f& a) {
  uint32_t x[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) x[r] = __float_as_uint(a[r]);
  const uint32_t m0 = min(min(x[0], x[1]), x[2]);
  const uint32_t m1 = min(min(x[3], x[4]), x[5]);
  const uint32_t m2 = min(min(x[6], x[7]), x[8]);
  const uint32_t m3 = min(min(x[9], x[10]), x[11]);
  const uint32_t m4 = min(min(x[12], x[13]), x[14]);
  const uint32_t m5 = min(min(m0, m1), x[15]);
  const uint32_t m6 = min(min(m2, m3), m4);
  return min(m5, m6);
}

template <int MODE, bool SPLIT>
__global__ __launch_bounds__(kThreads) void hamming_mfma_kernel(const uint4* __restrict__ slab,
                                                                const PairWork* __restrict__ work,
                                                                uint32_t* __restrict__ keys, uint32_t max_kp,
                                                                uint32_t tiles_per_slot, uint32_t n_pairs,
                                                                uint32_t qblocks, uint32_t tsplit) {
  __shared__ uint4 lds[2][kStage * 256];
  // whole pairs per XCD (block b runs on XCD b % 8), as in hamming_nn_kernel
  const uint32_t L = blockIdx.x;
  const uint32_t xcd = L & 7u;
  const uint32_t j = L >> 3;
  const uint32_t subs = qblocks * tsplit;
  const uint32_t pair = (j / subs) * 8u + xcd;
  if (pair >= n_pairs) return;
  const uint32_t sub = j % subs;
  const uint32_t qblock = sub / tsplit;
  const uint32_t split = sub % tsplit;

  const PairWork w = work[pair];
  const uint32_t nq = w.nq;
  if (qblock * kQueriesPerBlock >= nq) return;
  const uint32_t nt_search = w.nt > 0 ? w.nt - 1u : 0u;  // features.cpp:174 (and D4)
  const uint32_t n_ttiles = (nt_search + 31u) >> 5;
  uint32_t tile0 = 0, tile1 = n_ttiles;
  if (SPLIT) {
    const uint32_t chunk = (n_ttiles + tsplit - 1u) / tsplit;
    tile0 = min(split * chunk, n_ttiles);
    tile1 = min(tile0 + chunk, n_ttiles);
  }

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t half = lane >> 5;

  // query operands: kQT tiles x 4 k-steps, sign-flipped
  v8i bq[kQT][4];
#pragma unroll
  for (int t = 0; t < kQT; ++t) {
    uint32_t qt = qblock * (kQueriesPerBlock / 32) + wave * kQT + t;
    qt = min(qt, tiles_per_slot - 1u);  // tiles beyond the node's rows: results are discarded
    const uint4* __restrict__ qs = slab + ((size_t)w.q_slot * tiles_per_slot + qt) * 256u;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint4 v = qs[s * 64 + lane];
      v.x ^= 0x88888888u; v.y ^= 0x88888888u; v.z ^= 0x88888888u; v.w ^= 0x88888888u;
      bq[t][s] = as_operand(v);
    }
  }

  // accumulator register r of this lane belongs to train row (r & 3) + 8 * (r >> 2) + 4 * half of the tile
  v16f crow;
#pragma unroll
  for (int r = 0; r < 16; ++r) crow[r] = kBias + (float)((r & 3) + 8 * (r >> 2) + 4 * (int)half) * kRowUnit;
  v16f czero;
#pragma unroll
  for (int r = 0; r < 16; ++r) czero[r] = 0.f;
  // The pair's last tile is ragged (rows >= nt_search do not take part: at least the node's last row, features.cpp:174):
  // its row term is kNone for those rows, so their accumulator elements can never be a minimum -- the exclusion costs
  // nothing in the epilogue, the ragged tile just starts from another C vector (3e38 + a dot product of at most 256 in
  // magnitude stays 3e38).
  v16f crow_ragged;
  {
    const uint32_t rag0 = (nt_search >> 5) << 5;  // first row of the ragged tile (no ragged tile when nt_search % 32 == 0)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t row = rag0 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * half;
      crow_ragged[r] = row < nt_search ? crow[r] : kNone;
    }
  }

  uint32_t best[kQT];  // float bit patterns
#pragma unroll
  for (int t = 0; t < kQT; ++t) best[t] = __float_as_uint(kNone);

  const uint4* __restrict__ ts = slab + (size_t)w.t_slot * tiles_per_slot * 256u;
  const uint32_t n_tiles = tile1 - tile0;
  const uint32_t n_stages = (n_tiles + kStage - 1u) / kStage;
  const uint32_t last_tile = tiles_per_slot - 1u;

  // stage 0 -> LDS
  {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const uint32_t tl = min(tile0 + (uint32_t)i, last_tile);
      lds[0][i * 256 + threadIdx.x] = ts[(size_t)tl * 256u + threadIdx.x];
    }
  }
  __syncthreads();

  for (uint32_t st = 0; st < n_stages; ++st) {
    // the next stage's tiles travel through registers while this stage is computed (behind the last stage the
    // clamped addresses are simply read again: no branch around the loads, nothing is done with them)
    uint4 nxt[kStage];
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const uint32_t tl = min(tile0 + (st + 1u) * kStage + (uint32_t)i, last_tile);
      nxt[i] = ts[(size_t)tl * 256u + threadIdx.x];
    }
    const uint4* __restrict__ buf = lds[st & 1u];
    // one train tile against this wave's query tiles; CROW = the row term (C operand in mode 1, added after in mode 2)
    auto do_tile = [&](int i, uint32_t tile, const v16f& CROW) {
      v8i a[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) a[s] = as_operand(buf[i * 256 + s * 64 + lane]);
      const float base = (float)(tile * 32u) * kRowUnit;
      // both query tiles' MFMA chains are issued before the first epilogue: the matrix pipe works on tile 1 while
      // the VALU reduces tile 0
      v16f acc[kQT];
#pragma unroll
      for (int t = 0; t < kQT; ++t) {
        acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[0], bq[t][0], MODE == 1 ? CROW : czero, 4, 4, 0, 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[1], bq[t][1], acc[t], 4, 4, 0, 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[2], bq[t][2], acc[t], 4, 4, 0, 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[3], bq[t][3], acc[t], 4, 4, 0, 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < kQT; ++t) {
        if (MODE != 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] += CROW[r];
        }
        const float m = __uint_as_float(min16(acc[t]));
        best[t] = min(best[t], __float_as_uint(m + base));  // kNone + base stays huge
      }
    };
    const uint32_t stage_tile0 = tile0 + st * kStage;
    if (stage_tile0 + kStage <= tile1 && (stage_tile0 + kStage) * 32u <= nt_search) {
      // a full stage without the ragged tile: ONE basic block, so the LDS reads of tile i + 1 can be scheduled beside
      // the MFMAs of tile i
#pragma unroll
      for (int i = 0; i < kStage; ++i) do_tile(i, stage_tile0 + (uint32_t)i, crow);
    } else {
#pragma unroll
      for (int i = 0; i < kStage; ++i) {
        const uint32_t tile = stage_tile0 + (uint32_t)i;
        if (tile < tile1) {  // block-uniform
          if (tile * 32u + 32u > nt_search) do_tile(i, tile, crow_ragged);  // block-uniform: the pair's last tile only
          else do_tile(i, tile, crow);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kStage; ++i) lds[(st + 1u) & 1u][i * 256 + threadIdx.x] = nxt[i];
    __syncthreads();
  }

  uint32_t* kout = keys + ((size_t)pair * tsplit + split) * max_kp;
#pragma unroll
  for (int t = 0; t < kQT; ++t) {
    uint32_t bb = best[t];
    bb = min(bb, (uint32_t)__shfl_xor((int)bb, 32));  // the two row halves of the tiles
    const float b = __uint_as_float(bb);
    const uint32_t qi = qblock * kQueriesPerBlock + (wave * kQT + (uint32_t)t) * 32u + (lane & 31u);
    if (half == 0 && qi < nq) {
      uint32_t key = kNoMatchKey;
      if (b < 1.0e30f) {
        // 2*hd + row / 2^14  ->  hd * 2^15 + row   (exact: < 2^24)
        const uint32_t k = (uint32_t)(b * 16384.0f);
        key = ((k >> 15) << 16) | (k & 32767u);
      }
      kout[qi] = key;
    }
  }
}


// ------------------------------------------------------------------------------------------------
// MODE 3: the same contraction as a software pipeline inside every wave (round 4).
//
// In the kernel above a wave issues the eight MFMAs of a train tile in one burst and reduces the two accumulators
// afterwards: the matrix pipe only stays busy while ANOTHER wave of the SIMD happens to be in its burst, and bursts of
// co-resident waves drift into step (measured: matrix pipe 0.61 + VALU 0.40 of the kernel time, i.e. no overlap).  Here the
// overlap is built into the instruction stream of each wave:
//   * the unit of work is one chain of four MFMAs (one train tile x one of the wave's two query tiles); the v_min3 tree of
//     unit u - 1 and the LDS reads of the next train tile are placed in the gaps between the MFMAs of unit u
//     (sched_group_barrier pins the order): ~3.3 single-issue instructions per 32-cycle MFMA;
//   * the two accumulators alternate (unit u writes acc[u & 1] while acc[(u - 1) & 1] is reduced): no more registers than
//     the burst form;
//   * train tiles come in stages of four through THREE LDS buffers filled by global_load_lds (no staging registers, no
//     ds_write); the one barrier per stage sits in the MIDDLE of the stage's instruction stream -- it publishes the NEXT
//     stage (loaded a whole stage ago) and frees the buffer of the previous one -- so the stream of MFMAs does not drain at
//     a stage boundary;
//   * every stage is the same straight-line code: the pair's ragged tile is moved to the last slot of the last stage
//     (the minimum does not care about the order of the tiles) where the C operand is `c3` (= the row term with 3e38 for
//     the excluded rows in that one stage), missing tiles are phantoms: they read some valid tile and add a base of
//     2^22, which no real key reaches (real keys are < 1024).
// Keys are those of the other kernels, bit for bit (tests/test_gpu_hamming.py runs all four).
//
// The kernel is a template over QT, the 32-query operand tiles a wave holds.  QT = 2 (256 queries per block) is the stream
// described above.  QT = 4 (512 queries per block, "wide") walks the same stages with FOUR units per train tile: per MFMA it
// needs half the LDS reads, half the L2 -> LDS traffic, half the block prologues and half the barriers.  The two
// accumulators still alternate unit by unit and there are four running minima.  Its 64 query-operand registers leave room,
// at three waves per SIMD (168 VGPRs), for neither a second A operand set nor `c3`: the one A operand set is refilled in
// place by the last unit of every tile, and the ragged tile's rows that do not take part are overwritten in LDS (see the
// QT = 4 stream below).  hamming_mfma_geometry picks QT per batch.
// ------------------------------------------------------------------------------------------------
#ifndef RGBDFE_HAMMING_PIPE_QT
#define RGBDFE_HAMMING_PIPE_QT 0             // 0: both forms, chosen per batch; 2 / 4: the automatic choice always takes that one
#endif                                       // (diagnostics, tools/build_hamming_pipe_variants.sh; modes 3 and 4 still force theirs)
#ifndef RGBDFE_HAMMING_PIPE_BURST
#define RGBDFE_HAMMING_PIPE_BURST 0
#endif
#ifndef RGBDFE_HAMMING_PIPE_ALT4
#define RGBDFE_HAMMING_PIPE_ALT4 0
#endif
#ifndef RGBDFE_HAMMING_PIPE_WAVES
#define RGBDFE_HAMMING_PIPE_WAVES 3          // waves per SIMD the register allocation aims at (48 KB of LDS: three blocks per CU)
#endif
#ifndef RGBDFE_HAMMING_PIPE_VALU_GROUPS
#define RGBDFE_HAMMING_PIPE_VALU_GROUPS 334  // reduction instructions behind the 2nd / 3rd / 4th MFMA of a unit (diagnostics)
#endif
#ifndef RGBDFE_HAMMING_PIPE_DIAG
#define RGBDFE_HAMMING_PIPE_DIAG 0   // TIMING-ONLY builds (keys are forced to "no match"): 1 no reductions, 2 no LDS reads in the
#endif                               // loop, 4 no global_load_lds / barriers in the loop; tools/build_hamming_pipe_variants.sh
constexpr int kPipeStage = 4;  // train tiles per stage (the unrolled stream below is written for four)
constexpr float kRowUnitPerTile = 32.0f / 16384.0f;  // the tile's first row, in key units

#define HP_MFMA(ACC, A, B, C) ACC = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, C, 4, 4, 0, 0, 0, 0);
#define HP_SGB(MASK, N) __builtin_amdgcn_sched_group_barrier(MASK, N, 0);
#define HP_FENCE() __builtin_amdgcn_sched_barrier(0);

template <int QT, bool SPLIT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(RGBDFE_HAMMING_PIPE_WAVES, RGBDFE_HAMMING_PIPE_WAVES)))
void hamming_mfma_pipe_kernel(const uint4* __restrict__ slab,
                                                                     const PairWork* __restrict__ work,
                                                                     uint32_t* __restrict__ keys, uint32_t max_kp,
                                                                     uint32_t tiles_per_slot, uint32_t n_pairs,
                                                                     uint32_t qblocks, uint32_t tsplit) {
  // three stage buffers [slot][fragment order of a tile] as three VARIABLES: the compiler tells LDS objects apart by
  // variable, and only then does it let the LDS reads of one buffer pass the global_load_lds towards another
  __shared__ uint4 lds0[kPipeStage][256], lds1[kPipeStage][256], lds2[kPipeStage][256];
  static_assert((QT == 2 || QT == 4) && kPipeStage == 4, "the unrolled streams are written for two or four query tiles and four-tile stages");
  constexpr uint32_t kQPB = 4u * QT * 32u;  // queries per block
  const uint32_t L = blockIdx.x;
  const uint32_t xcd = L & 7u;
  const uint32_t j = L >> 3;
  const uint32_t subs = qblocks * tsplit;
  const uint32_t pair = (j / subs) * 8u + xcd;
  if (pair >= n_pairs) return;
  const uint32_t sub = j % subs;
  const uint32_t qblock = sub / tsplit;
  const uint32_t split = sub % tsplit;

  const PairWork w = work[pair];
  const uint32_t nq = w.nq;
  if (qblock * kQPB >= nq) return;
  // this block's tiles as slots: the full tiles first, phantoms, the ragged tile (if it is this block's) in the last slot
  const HammingSlots slots = HammingSlots::make(w.nt, SPLIT ? tsplit : 1u, SPLIT ? split : 0u, kPipeStage);
  const uint32_t nt_search = slots.nt_search, n_stages = slots.n_stages;
  const bool has_ragged = slots.has_ragged;
  auto slot_tile = [&](uint32_t s) -> uint32_t { return slots.tile(s); };  // block-uniform

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t half = lane >> 5;

  v8i bq[QT][4];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    uint32_t qt = qblock * (kQPB / 32u) + wave * QT + t;
    qt = min(qt, tiles_per_slot - 1u);
    const uint4* __restrict__ qs = slab + ((size_t)w.q_slot * tiles_per_slot + qt) * 256u;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint4 v = qs[s * 64 + lane];
      v.x ^= 0x88888888u; v.y ^= 0x88888888u; v.z ^= 0x88888888u; v.w ^= 0x88888888u;
      bq[t][s] = as_operand(v);
    }
  }

  v16f crow, c3;   // (c3: QT = 2 only)
#pragma unroll
  for (int r = 0; r < 16; ++r) crow[r] = kBias + (float)((r & 3) + 8 * (r >> 2) + 4 * (int)half) * kRowUnit;
  c3 = crow;
  auto set_c3_ragged = [&]() {
    uint32_t nts = nt_search;
    asm volatile("" : "+v"(nts));  // formed where it is needed (once per block), not kept in 16 registers from the start
    const uint32_t rag0 = (nts >> 5) << 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t row = rag0 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * half;
      c3[r] = row < nts ? crow[r] : kNone;
    }
  };
  uint32_t best0 = __float_as_uint(kNone), best1 = __float_as_uint(kNone);
  uint32_t best2 = __float_as_uint(kNone), best3 = __float_as_uint(kNone);   // (QT = 4)

  const uint32_t last_tile = tiles_per_slot - 1u;
  const char* __restrict__ ts = reinterpret_cast<const char*>(slab + (size_t)w.t_slot * tiles_per_slot * 256u);
  const uint64_t ts_u = reinterpret_cast<uint64_t>(ts);
  const uint32_t ts_lo = __builtin_amdgcn_readfirstlane((uint32_t)ts_u);
  const uint32_t ts_hi = __builtin_amdgcn_readfirstlane((uint32_t)(ts_u >> 32));
  const uint32_t vo16 = threadIdx.x * 16u;

  // stage `st` of this block -> LDS buffer `b` (this wave's quarter of each of the four tiles)
  auto load_stage = [&](uint32_t st, uint4 (*buf)[256]) {
#pragma unroll
    for (int i = 0; i < kPipeStage; ++i) {
      const uint32_t tl = min(slot_tile(st * kPipeStage + (uint32_t)i), last_tile);
      const char* tb = reinterpret_cast<const char*>((((uint64_t)ts_hi << 32) | ts_lo) + (uint64_t)tl * 4096u);
      uint32_t vo = vo16;
      asm volatile("" : "+v"(vo));
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(tb + vo),
                                       (__attribute__((address_space(3))) void*)&buf[i][wave * 64],
                                       16, 0, 0);
    }
  };

  if (n_stages > 0) {
    load_stage(0, lds0);
    if (n_stages > 1) load_stage(1, lds1);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();

    v8i aA[4], aB[4];  // A operands of the even / odd slots of a stage
    // (BUF = 0, 1, 2 is a literal everywhere: the compiler must SEE that a stage's LDS reads and the global_load_lds of the
    // stage after the next one touch different buffers, or it waits for the loads in front of the next LDS read)
#if RGBDFE_HAMMING_PIPE_DIAG & 2
#define HP_READ(DST, BUF, SLOT, S) asm volatile("" : "+v"(DST[S]));
#else
#define HP_READ(DST, BUF, SLOT, S) DST[S] = as_operand(lds##BUF[SLOT][(S) * 64 + lane]);
#endif
#define HP_BASE(SLOT) ((float)slot_tile(st * kPipeStage + (SLOT)) * kRowUnitPerTile)
    // reduction of one accumulator into the running minimum of its query tile
#if RGBDFE_HAMMING_PIPE_DIAG & 1
#define HP_EPI(ACC, BEST, BASE) asm volatile("" : : "v"(ACC));
#else
#define HP_EPI(ACC, BEST, BASE)                                                 \
    BEST = min(BEST, __float_as_uint(__uint_as_float(min16(ACC)) + (BASE))); \
    asm volatile("" : "+v"(BEST));   /* the reduction is finished HERE, not merged into a later one */
#endif
    // one unit: four MFMAs with the previous unit's reduction (10 VALU) and two LDS reads in their gaps
#if RGBDFE_HAMMING_PIPE_BURST   /* diagnostics: the chain back to back, everything else behind it */
#define HP_UNIT_SCHED() HP_SGB(0x008, 4) HP_SGB(0x100, 2) HP_SGB(0x002, 12)
#else
#define HP_UNIT_SCHED()                                                                             \
    HP_SGB(0x008, 1) HP_SGB(0x100, 2)                                                               \
    HP_SGB(0x008, 1) HP_SGB(0x002, RGBDFE_HAMMING_PIPE_VALU_GROUPS / 100)                            \
    HP_SGB(0x008, 1) HP_SGB(0x002, RGBDFE_HAMMING_PIPE_VALU_GROUPS / 10 % 10)                        \
    HP_SGB(0x008, 1) HP_SGB(0x002, RGBDFE_HAMMING_PIPE_VALU_GROUPS % 10)
#endif
    // (a unit without LDS reads, QT = 4: the same order without the read group)
#if RGBDFE_HAMMING_PIPE_BURST
#define HP_UNIT_SCHED0() HP_SGB(0x008, 4) HP_SGB(0x002, 12)
#else
#define HP_UNIT_SCHED0()                                                                            \
    HP_SGB(0x008, 1)                                                                                \
    HP_SGB(0x008, 1) HP_SGB(0x002, RGBDFE_HAMMING_PIPE_VALU_GROUPS / 100)                            \
    HP_SGB(0x008, 1) HP_SGB(0x002, RGBDFE_HAMMING_PIPE_VALU_GROUPS / 10 % 10)                        \
    HP_SGB(0x008, 1) HP_SGB(0x002, RGBDFE_HAMMING_PIPE_VALU_GROUPS % 10)
#endif
#define HP_UNIT_X(ACC, A, Q, C, PACC, PBEST, PBASE, READS, SCHED)                                   \
    HP_MFMA(ACC, A[0], bq[Q][0], C)                                                                 \
    READS                                                                                           \
    HP_MFMA(ACC, A[1], bq[Q][1], ACC)                                                               \
    HP_EPI(PACC, PBEST, PBASE)                                                                      \
    HP_MFMA(ACC, A[2], bq[Q][2], ACC)                                                               \
    HP_MFMA(ACC, A[3], bq[Q][3], ACC)                                                               \
    SCHED()                                                                                         \
    HP_FENCE()
#define HP_UNIT(ACC, A, Q, C, PACC, PBEST, PBASE, R0, R1) HP_UNIT_X(ACC, A, Q, C, PACC, PBEST, PBASE, R0 R1, HP_UNIT_SCHED)
    // A stage out of buffer CUR in two halves; the barrier between them publishes the NEXT stage (this wave's
    // global_load_lds of it was issued a whole stage ago) and frees the buffer of the PREVIOUS one for the stage after the
    // next.  The loop below turns at that barrier, where nothing is in flight (the compiler's bookkeeping of what an LDS
    // read may have to wait for is exact in straight-line code only).
#if RGBDFE_HAMMING_PIPE_DIAG & 4
#define HP_TURN()
#define HP_LOADS false
#else
    /* vmcnt(0): this wave's share of the next stage has landed */
#define HP_TURN() __builtin_amdgcn_s_waitcnt(0x0F70); __syncthreads();
#define HP_LOADS true
#endif
#if RGBDFE_HAMMING_PIPE_ALT4
    // Diagnostics (2 waves per SIMD: four accumulators): a unit is a whole train tile, the chains of the two query tiles
    // ALTERNATE (no instruction ever sits between two MFMAs on the same accumulator without an MFMA on another one), the
    // previous tile's two reductions fill the gaps.
#define HP_TILE(X0, X1, A, C, P0, P1, PBASE, R0, R1, R2, R3)                                         \
    HP_MFMA(X0, A[0], bq[0][0], C) HP_MFMA(X1, A[0], bq[1][0], C)                                    \
    R0 R1 R2 R3                                                                                      \
    HP_MFMA(X0, A[1], bq[0][1], X0) HP_MFMA(X1, A[1], bq[1][1], X1)                                  \
    HP_EPI(P0, best0, PBASE)                                                                         \
    HP_MFMA(X0, A[2], bq[0][2], X0) HP_MFMA(X1, A[2], bq[1][2], X1)                                  \
    HP_EPI(P1, best1, PBASE)                                                                         \
    HP_MFMA(X0, A[3], bq[0][3], X0) HP_MFMA(X1, A[3], bq[1][3], X1)                                  \
    HP_SGB(0x008, 1) HP_SGB(0x100, 1) HP_SGB(0x008, 1) HP_SGB(0x100, 1)                              \
    HP_SGB(0x008, 1) HP_SGB(0x100, 1) HP_SGB(0x002, 2) HP_SGB(0x008, 1) HP_SGB(0x100, 1) HP_SGB(0x002, 3) \
    HP_SGB(0x008, 1) HP_SGB(0x002, 4) HP_SGB(0x008, 1) HP_SGB(0x002, 4)                              \
    HP_SGB(0x008, 1) HP_SGB(0x002, 4) HP_SGB(0x008, 1) HP_SGB(0x002, 4)                              \
    HP_FENCE()
#define HP_HALF_A(CUR)                                                                                               \
    {                                                                                                                \
      b0 = HP_BASE(0); b1 = HP_BASE(1);                                                                              \
      HP_FENCE()                                                                                                     \
      HP_TILE(acc0, acc1, aA, crow, acc2, acc3, pend, HP_READ(aB, CUR, 1, 0), HP_READ(aB, CUR, 1, 1),                \
              HP_READ(aB, CUR, 1, 2), HP_READ(aB, CUR, 1, 3))                                                        \
      HP_TILE(acc2, acc3, aB, crow, acc0, acc1, b0, HP_READ(aA, CUR, 2, 0), HP_READ(aA, CUR, 2, 1),                  \
              HP_READ(aA, CUR, 2, 2), HP_READ(aA, CUR, 2, 3))                                                        \
      HP_TURN()                                                                                                      \
    }
#define HP_HALF_B(CUR, NXT, NN)                                                                                      \
    {                                                                                                                \
      if (HP_LOADS && st + 2u < n_stages) load_stage(st + 2u, lds##NN);                                              \
      const float b2 = HP_BASE(2), b3 = HP_BASE(3);                                                                  \
      if (has_ragged && st + 1u == n_stages) {                                                                       \
        set_c3_ragged();                                                                                             \
        asm volatile("" : "+v"(c3));                                                                                 \
      }                                                                                                              \
      HP_FENCE()                                                                                                     \
      HP_TILE(acc0, acc1, aA, crow, acc2, acc3, b1, HP_READ(aB, CUR, 3, 0), HP_READ(aB, CUR, 3, 1),                  \
              HP_READ(aB, CUR, 3, 2), HP_READ(aB, CUR, 3, 3))                                                        \
      HP_TILE(acc2, acc3, aB, c3, acc0, acc1, b2, HP_READ(aA, NXT, 0, 0), HP_READ(aA, NXT, 0, 1),                    \
              HP_READ(aA, NXT, 0, 2), HP_READ(aA, NXT, 0, 3))                                                        \
      pend = b3;                                                                                                     \
    }
#else
#define HP_HALF_A(CUR)                                                                                               \
    {                                                                                                                \
      b0 = HP_BASE(0); b1 = HP_BASE(1);                                                                              \
      HP_FENCE()                                                                                                     \
      HP_UNIT(acc0, aA, 0, crow, acc1, best1, pend, HP_READ(aB, CUR, 1, 0), HP_READ(aB, CUR, 1, 1))                  \
      HP_UNIT(acc1, aA, 1, crow, acc0, best0, b0, HP_READ(aB, CUR, 1, 2), HP_READ(aB, CUR, 1, 3))                    \
      HP_UNIT(acc0, aB, 0, crow, acc1, best1, b0, HP_READ(aA, CUR, 2, 0), HP_READ(aA, CUR, 2, 1))                    \
      HP_UNIT(acc1, aB, 1, crow, acc0, best0, b1, HP_READ(aA, CUR, 2, 2), HP_READ(aA, CUR, 2, 3))                    \
      HP_TURN()                                                                                                      \
    }
#define HP_HALF_B(CUR, NXT, NN)                                                                                      \
    {                                                                                                                \
      if (HP_LOADS && st + 2u < n_stages) load_stage(st + 2u, lds##NN); /* (nothing may be in flight at the end) */   \
      const float b2 = HP_BASE(2), b3 = HP_BASE(3);                                                                  \
      if (has_ragged && st + 1u == n_stages) {                                                                       \
        set_c3_ragged();                                                                                             \
        asm volatile("" : "+v"(c3)); /* a real (block-uniform) branch: not sixteen selects in every stage */        \
      }                                                                                                              \
      HP_FENCE()                                                                                                     \
      HP_UNIT(acc0, aA, 0, crow, acc1, best1, b1, HP_READ(aB, CUR, 3, 0), HP_READ(aB, CUR, 3, 1))                    \
      HP_UNIT(acc1, aA, 1, crow, acc0, best0, b2, HP_READ(aB, CUR, 3, 2), HP_READ(aB, CUR, 3, 3))                    \
      HP_UNIT(acc0, aB, 0, c3, acc1, best1, b2, HP_READ(aA, NXT, 0, 0), HP_READ(aA, NXT, 0, 1))                      \
      HP_UNIT(acc1, aB, 1, c3, acc0, best0, b3, HP_READ(aA, NXT, 0, 2), HP_READ(aA, NXT, 0, 3))                      \
      pend = b3;                                                                                                     \
    }

#endif
    // QT = 4: four units per train tile (query tiles 0..3 of the wave), the accumulators alternate as above.  64 registers
    // of query operands leave room for ONE A operand set, and only if the next tile's operand lands in the registers of
    // the current one -- which the register allocator does not do by itself (it scatters the new values and spills the
    // query operands).  So this stream reads LDS with its own ds_read_b128 (`a4[s]` is input and output of the statement:
    // the same four registers) and counts its own waits:
    //   * the tile's last unit reads the next tile's k-step s right behind its own MFMA of k-step s; the other three units
    //     carry no read;
    //   * LDS reads return in order, so the next tile's first unit waits for lgkmcnt(3 - s) in front of its MFMA of k-step
    //     s -- nothing else in the loop counts on lgkmcnt (the stage loads are LDS-DMA: vmcnt); a fence behind every wait
    //     keeps the MFMA behind it, and one between an MFMA and the read that replaces its operand keeps that order.
    //     (The compiler folds neighbouring waits into the stricter one: lgkmcnt(2) and lgkmcnt(0) per tile in the ISA.)
    // Unit q reduces unit q - 1 (q = 0: the previous tile's unit 3).
    // There is no second C operand either (`c3` above; a changed `crow` would have to live beside the unchanged one).  The
    // ragged tile is excluded in LDS instead: once its stage has been published, every row of it that does not take part
    // is overwritten with the tile's FIRST row, which always takes part.  A copy has that row's distance and a larger row
    // index, so its key is larger than the original's and it can never be the minimum.  One LDS read and one LDS write per
    // thread and block, between the barrier that publishes the last stage and the next one (which comes before the last
    // slot of any stage is read).
#if RGBDFE_HAMMING_PIPE_DIAG & 2
#define HP4_READ(BUF, SLOT, S) asm volatile("" : "+v"(a4[S]));
#else
#define HP4_READ(BUF, SLOT, S)                                                                                       \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(a4[S]) : "v"(rd##BUF), "n"((SLOT) * 4096 + (S) * 1024) : "memory");
#endif
#define HP4_WAIT(N) __builtin_amdgcn_s_waitcnt(0xC07F | ((N) << 8)); HP_FENCE()   /* lgkmcnt(N) alone */
#define HP4_A(S) op8(a4[S])
    // (the tile bases are block-uniform: kept in scalar registers here, five vector registers less)
#define HP4_BASE(SLOT) __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(HP_BASE(SLOT))))
#define HP4_UNIT0(ACC, Q, C, PACC, PBEST, PBASE)                                                                     \
      HP_MFMA(ACC, HP4_A(0), bq[Q][0], C)                                                                            \
      HP_MFMA(ACC, HP4_A(1), bq[Q][1], ACC)                                                                          \
      HP_EPI(PACC, PBEST, PBASE)                                                                                     \
      HP_MFMA(ACC, HP4_A(2), bq[Q][2], ACC)                                                                          \
      HP_MFMA(ACC, HP4_A(3), bq[Q][3], ACC)                                                                          \
      HP_UNIT_SCHED0()                                                                                               \
      HP_FENCE()
#define HP4_TILE(C, PB, B, RSLOT, RBUF)                                                                              \
      HP4_WAIT(3) HP_MFMA(acc0, HP4_A(0), bq[0][0], C)                                                               \
      HP4_WAIT(2) HP_MFMA(acc0, HP4_A(1), bq[0][1], acc0)                                                            \
      HP_EPI(acc1, best3, PB)                                                                                        \
      HP4_WAIT(1) HP_MFMA(acc0, HP4_A(2), bq[0][2], acc0)                                                            \
      HP4_WAIT(0) HP_MFMA(acc0, HP4_A(3), bq[0][3], acc0)                                                            \
      HP_FENCE()                                                                                                     \
      HP4_UNIT0(acc1, 1, C, acc0, best0, B)                                                                          \
      HP4_UNIT0(acc0, 2, C, acc1, best1, B)                                                                          \
      HP_MFMA(acc1, HP4_A(0), bq[3][0], C)                                                                           \
      HP_FENCE() HP4_READ(RBUF, RSLOT, 0)                                                                            \
      HP_MFMA(acc1, HP4_A(1), bq[3][1], acc1)                                                                        \
      HP_FENCE() HP4_READ(RBUF, RSLOT, 1)                                                                            \
      HP_EPI(acc0, best2, B)                                                                                         \
      HP_MFMA(acc1, HP4_A(2), bq[3][2], acc1)                                                                        \
      HP_FENCE() HP4_READ(RBUF, RSLOT, 2)                                                                            \
      HP_MFMA(acc1, HP4_A(3), bq[3][3], acc1)                                                                        \
      HP_FENCE() HP4_READ(RBUF, RSLOT, 3)                                                                            \
      HP_FENCE()
#define HP4_HALF_A(CUR, NXT)                                                                                         \
    {                                                                                                                \
      b0 = HP4_BASE(0); b1 = HP4_BASE(1);                                                                            \
      HP_FENCE()                                                                                                     \
      HP4_TILE(crow, pend, b0, 1, CUR)                                                                               \
      HP4_TILE(crow, b0, b1, 2, CUR)                                                                                 \
      HP_TURN()                                                                                                      \
      if (has_ragged && st + 2u == n_stages) patch_ragged(lds##NXT);   /* the next stage is the last one */           \
    }
#define HP4_HALF_B(CUR, NXT, NN)                                                                                     \
    {                                                                                                                \
      if (HP_LOADS && st + 2u < n_stages) load_stage(st + 2u, lds##NN);                                              \
      const float b2 = HP4_BASE(2), b3 = HP4_BASE(3);                                                                \
      HP_FENCE()                                                                                                     \
      HP4_TILE(crow, b1, b2, 3, CUR)                                                                                 \
      HP_FENCE()                                                                                                     \
      HP4_TILE(crow, b2, b3, 0, NXT)                                                                                 \
      pend = b3;                                                                                                     \
    }
    if constexpr (QT == 2) {
      HP_READ(aA, 0, 0, 0) HP_READ(aA, 0, 0, 1) HP_READ(aA, 0, 0, 2) HP_READ(aA, 0, 0, 3)
#if RGBDFE_HAMMING_PIPE_ALT4
      v16f acc0, acc1, acc2 = crow, acc3 = crow;
#else
      v16f acc0, acc1 = crow;
#endif
      float pend = 4.0e6f;  // acc1 = the row terms (>= 256), + 4e6: a phantom for the first unit's reduction slot
      float b0, b1;
      uint32_t st = 0;
      HP_HALF_A(0)
      for (;;) {
        HP_HALF_B(0, 1, 2)
        if (++st == n_stages) break;
        HP_HALF_A(1)
        HP_HALF_B(1, 2, 0)
        if (++st == n_stages) break;
        HP_HALF_A(2)
        HP_HALF_B(2, 0, 1)
        if (++st == n_stages) break;
        HP_HALF_A(0)
      }
#if RGBDFE_HAMMING_PIPE_ALT4
      HP_EPI(acc2, best0, pend)
      HP_EPI(acc3, best1, pend)
#else
      HP_EPI(acc1, best1, pend)
#endif
    } else {
      // this lane's 16 bytes of (slot 0, k-step 0) in each stage buffer, as LDS addresses
      const uint32_t rd0 = (uint32_t)(size_t)(__attribute__((address_space(3))) char*)&lds0[0][0] + lane * 16u;
      const uint32_t rd1 = (uint32_t)(size_t)(__attribute__((address_space(3))) char*)&lds1[0][0] + lane * 16u;
      const uint32_t rd2 = (uint32_t)(size_t)(__attribute__((address_space(3))) char*)&lds2[0][0] + lane * 16u;
      v4i a4[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
      auto patch_ragged = [&](uint4 (*buf)[256]) {   // (thread = one 16-byte piece of the tile: k-step, row half, row)
        const uint32_t t = threadIdx.x;
        if ((t & 31u) >= (nt_search & 31u)) buf[kPipeStage - 1][t] = buf[kPipeStage - 1][t & ~31u];
      };
      if (has_ragged && n_stages <= 2u) patch_ragged(n_stages == 1u ? lds0 : lds1);   // published by the barrier above
      HP4_READ(0, 0, 0) HP4_READ(0, 0, 1) HP4_READ(0, 0, 2) HP4_READ(0, 0, 3)
      v16f acc0, acc1 = crow;
      float pend = 4.0e6f;  // (as above: the first unit reduces a phantom)
      float b0, b1;
      uint32_t st = 0;
      HP4_HALF_A(0, 1)
      for (;;) {
        HP4_HALF_B(0, 1, 2)
        if (++st == n_stages) break;
        HP4_HALF_A(1, 2)
        HP4_HALF_B(1, 2, 0)
        if (++st == n_stages) break;
        HP4_HALF_A(2, 0)
        HP4_HALF_B(2, 0, 1)
        if (++st == n_stages) break;
        HP4_HALF_A(0, 1)
      }
      HP_EPI(acc1, best3, pend)
    }
#undef HP4_TILE
#undef HP4_UNIT0
#undef HP4_BASE
#undef HP4_A
#undef HP4_WAIT
#undef HP4_READ
#undef HP4_HALF_A
#undef HP4_HALF_B
#undef HP_HALF_A
#undef HP_HALF_B
#undef HP_TURN
#undef HP_LOADS
#undef HP_UNIT
#undef HP_UNIT_X
#undef HP_EPI
#undef HP_BASE
#undef HP_READ
  }

  uint32_t* kout = keys + ((size_t)pair * tsplit + split) * max_kp;
  const uint32_t bests[4] = {best0, best1, best2, best3};
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    uint32_t bb = bests[t];
    bb = min(bb, (uint32_t)__shfl_xor((int)bb, 32));
    const float b = __uint_as_float(bb);
    const uint32_t qi = qblock * kQPB + (wave * QT + (uint32_t)t) * 32u + (lane & 31u);
    if (half == 0 && qi < nq) {
      uint32_t key = kNoMatchKey;
      if (RGBDFE_HAMMING_PIPE_DIAG ? b < -1.0f : b < 1024.0f) {  // real keys: 2*hd + row / 2^14 < 514; phantoms and excluded rows are >= 2^22
        const uint32_t k = (uint32_t)(b * 16384.0f);
        key = ((k >> 15) << 16) | (k & 32767u);
      }
      kout[qi] = key;
    }
  }
}
#undef HP_MFMA

// ------------------------------------------------------------------------------------------------
// The 512-query block on 16x16x128 tiles (v_mfma_f32_16x16x128_f8f6f4): the same blocks, stages, slots and keys as the
// QT = 4 form above, out of the small shape of the instruction.
//   * No other slab format: a dot product does not care which k a bit sits at as long as both operands agree.  The small
//     MFMA takes, from lane g*16 + r, 32 nibbles of row r for k-group g; k-step S (of two) and k-group g together are
//     descriptor dword 4S + g, so the lane reads the 16-byte piece (2S + (g >> 1))*64 + (g & 1)*32 + 16u + r of the 32-row
//     tile image for the 16-row sub-tile u -- the query side from global memory, the train side from LDS.  The four lane
//     groups of a ds_read_b128 each touch sixteen different 16-byte slots of the 256-byte bank row: no conflicts.
//   * A wave holds 128 queries as EIGHT 16-query operand tiles (64 registers, as the four 32-query tiles above).  A unit is
//     one 16-row sub-tile x one query tile: a chain of TWO MFMAs into a 4-register accumulator, reduced by two v_min3_u32
//     straight into the running minimum (one register per query tile).  Nothing is added behind the MFMA: the C operand
//     carries 256 + (absolute row) / 2^14, one 4-register C per sub-tile, moved on from train tile to train tile in place by
//     the block-uniform distance between them (8 v_add_f32 per 32 MFMAs; multiples of 2^-14 below 2^10: exact).
//   * The stream is a rotation over four accumulators: step n issues the first MFMA of unit n, the second MFMA of unit
//     n - 1 and the reduction of unit n - 3, so no MFMA waits for the one in front of it and a reduction reads a result that
//     is three MFMAs old.  A 16-cycle MFMA leaves room for about two single-issue instructions: a step carries two or three
//     VALU instructions and at most one ds_read_b128, pinned by sched_group_barrier as above.
//   * Two A operand sets (16 registers each) alternate tile by tile, the next tile's four reads ride in steps 1..4; the
//     registers are there because the accumulators take 16, not 32.  The ragged tile is excluded in LDS as in the QT = 4 form.
//   * The stage is ONE loop body with one way out (the buffers rotate as addresses, see below): written as three copies like
//     the forms above, the copies' accumulators and operand sets met at the joins in different registers and were spilled.
//   148 VGPRs, no scratch (tests/test_hamming_x16_build.py); measured against the QT = 4 form in DESIGN 4.1c.
// ------------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));
#define HX_MFMA(ACC, A, B, C) ACC = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(op8(A), op8(B), C, 4, 4, 0, 0, 0, 0);

template <bool SPLIT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(RGBDFE_HAMMING_PIPE_WAVES, RGBDFE_HAMMING_PIPE_WAVES)))
void hamming_mfma_x16_kernel(const uint4* __restrict__ slab, const PairWork* __restrict__ work, uint32_t* __restrict__ keys,
                             uint32_t max_kp, uint32_t tiles_per_slot, uint32_t n_pairs, uint32_t qblocks, uint32_t tsplit) {
  __shared__ uint4 lds0[kPipeStage][256], lds1[kPipeStage][256], lds2[kPipeStage][256];   // the three stage buffers
  constexpr uint32_t kQPB = 512u;
  const uint32_t L = blockIdx.x;
  const uint32_t xcd = L & 7u;
  const uint32_t j = L >> 3;
  const uint32_t subs = qblocks * tsplit;
  const uint32_t pair = (j / subs) * 8u + xcd;
  if (pair >= n_pairs) return;
  const uint32_t sub = j % subs;
  const uint32_t qblock = sub / tsplit;
  const uint32_t split = sub % tsplit;

  const PairWork w = work[pair];
  const uint32_t nq = w.nq;
  if (qblock * kQPB >= nq) return;
  const HammingSlots slots = HammingSlots::make(w.nt, SPLIT ? tsplit : 1u, SPLIT ? split : 0u, kPipeStage);
  const uint32_t nt_search = slots.nt_search, n_stages = slots.n_stages;
  const bool has_ragged = slots.has_ragged;
  // A slot without a tile of its own repeats one of the block's tiles (a minimum does not mind seeing a row twice): the
  // block's first full tile, or -- in a block that has the ragged tile alone -- the ragged tile.  So every slot has a real
  // base and the C operands below stay exact sums of small multiples of 2^-14.
  const uint32_t dup_tile = slots.n_full > 0u ? slots.tile0 : slots.n_ttiles - 1u;
  auto slot_tile = [&](uint32_t s) -> uint32_t {   // block-uniform
    const uint32_t t = slots.tile(s);
    return t == kHammingPhantomTile ? dup_tile : t;
  };

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t grp = lane >> 4;   // k-group of the operands, row group of the accumulator
  // this lane's 16-byte piece of (k-step 0, sub-tile 0) in a tile image; k-step S adds 128 pieces, sub-tile u adds 16
  const uint32_t lpiece = (grp >> 1) * 64u + (grp & 1u) * 32u + (lane & 15u);

  v4i bq[8][2];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    uint32_t qt = qblock * (kQPB / 32u) + wave * 4u + (uint32_t)(q >> 1);
    qt = min(qt, tiles_per_slot - 1u);
    const uint4* __restrict__ qs = slab + ((size_t)w.q_slot * tiles_per_slot + qt) * 256u;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint4 v = qs[s * 128 + (q & 1) * 16 + lpiece];
      bq[q][s][0] = (int)v.x; bq[q][s][1] = (int)v.y; bq[q][s][2] = (int)v.z; bq[q][s][3] = (int)v.w;
    }
  }

  // (the sign flip after all sixteen loads, each operand in the registers it arrived in)
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bq[q][s] ^= (int)0x88888888u;
      asm volatile("" : "+v"(bq[q][s]));
    }

  // accumulator register i of this lane belongs to train row 16u + 4*grp + i of the tile
  v4f c[2];   // the C operands of the two sub-tiles: 256 + (absolute row) / 2^14, moved from tile to tile by the stream
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int i = 0; i < 4; ++i) c[u][i] = kBias + (float)(16 * u + 4 * (int)grp + i) * kRowUnit;
  uint32_t best[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) best[q] = __float_as_uint(kNone);

  const uint32_t last_tile = tiles_per_slot - 1u;
  const char* __restrict__ ts = reinterpret_cast<const char*>(slab + (size_t)w.t_slot * tiles_per_slot * 256u);
  const uint64_t ts_u = reinterpret_cast<uint64_t>(ts);
  const uint32_t ts_lo = __builtin_amdgcn_readfirstlane((uint32_t)ts_u);
  const uint32_t ts_hi = __builtin_amdgcn_readfirstlane((uint32_t)(ts_u >> 32));
  const uint32_t vo16 = threadIdx.x * 16u;
  // The three stage buffers take turns as CUR / NXT / the one being filled; the stream below is ONE loop body, so they are
  // LDS byte addresses in scalar registers that rotate once per stage (the reads are the stream's own ds_read_b128 and the
  // fills are LDS-DMA: neither needs the compiler to tell the buffers apart).
  typedef __attribute__((address_space(3))) char lds_char;
  const uint32_t o0 = (uint32_t)(size_t)(lds_char*)&lds0[0][0];
  const uint32_t o1 = (uint32_t)(size_t)(lds_char*)&lds1[0][0];
  const uint32_t o2 = (uint32_t)(size_t)(lds_char*)&lds2[0][0];
  auto load_stage = [&](uint32_t st, uint32_t buf) {
#pragma unroll
    for (int i = 0; i < kPipeStage; ++i) {
      const uint32_t tl = min(slot_tile(st * kPipeStage + (uint32_t)i), last_tile);
      const char* tb = reinterpret_cast<const char*>((((uint64_t)ts_hi << 32) | ts_lo) + (uint64_t)tl * 4096u);
      uint32_t vo = vo16;
      asm volatile("" : "+v"(vo));
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(tb + vo),
                                       (__attribute__((address_space(3))) void*)(lds_char*)(size_t)(buf + (uint32_t)i * 4096u + wave * 1024u),
                                       16, 0, 0);
    }
  };

  if (n_stages > 0) {
    load_stage(0, o0);
    if (n_stages > 1) load_stage(1, o1);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();
    // as in the QT = 4 form: the rows of the ragged tile that do not take part become copies of its row 0 (slot `slot` of `buf`)
    auto patch_ragged = [&](uint32_t buf, uint32_t slot) {
      const uint32_t t = threadIdx.x;
      __attribute__((address_space(3))) v4i* tile = (__attribute__((address_space(3))) v4i*)(lds_char*)(size_t)(buf + slot * 4096u);
      if ((t & 31u) >= (nt_search & 31u)) tile[t] = tile[t & ~31u];
    };
    if (has_ragged && slots.n_full == 0u) {   // one stage, the ragged tile in all four slots
#pragma unroll
      for (int i = 0; i < kPipeStage; ++i) patch_ragged(o0, (uint32_t)i);
      __syncthreads();
    } else if (has_ragged && n_stages == 1u) {   // (a later last stage is patched in the loop, once it is published)
      patch_ragged(o0, kPipeStage - 1u);
    }

    v4i aA[2][2], aB[2][2];   // [sub-tile][k-step] of the even / odd slots of a stage
    // LDS reads are this stream's own ds_read_b128, as in the QT = 4 form and for its reason: the operand lands in the
    // registers it replaces (input and output of the statement), so the two sets stay the same 32 registers round the loop.
    // The stream counts its own waits: a tile's four reads are issued in its steps 1..4 and the next tile starts with
    // lgkmcnt(0), eleven steps later.
    const uint32_t lp16 = lpiece * 16u;
    uint32_t cur = o0, nxt = o1, fill = o2;   // block-uniform
    uint32_t rdc, rdn;                        // this lane's piece of (slot 0, k-step 0, sub-tile 0) in CUR / NXT
#define HX_RD(DST, RD, SLOT, U, S)                                                                                    \
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(DST[U][S]) : "v"(RD), "n"((SLOT) * 4096 + (S) * 2048 + (U) * 256) : "memory");
#define HX_WAIT() __builtin_amdgcn_s_waitcnt(0xC07F); HP_FENCE()   /* lgkmcnt(0) alone */
#define HX_NORD
    // the way from the tile of slot SLOT - 1 to the tile of slot SLOT of this stage, in key units (block-uniform, exact)
#define HX_DELTA(SLOT) __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(                                \
      (float)((int)slot_tile(st * kPipeStage + (SLOT)) - (int)slot_tile(st * kPipeStage + (SLOT) - 1u)) * kRowUnitPerTile)))
    // the C operand of sub-tile U moves on by D, one register per step, in place
#define HX_C(U, I, D) c[U][I] += (D); asm volatile("" : "+v"(c[U][I]));
#define HX_EPI(ACC, BEST) {                                                                                             \
      const uint32_t m_ = min(min(__float_as_uint(ACC[0]), __float_as_uint(ACC[1])), __float_as_uint(ACC[2]));          \
      BEST = min(min(m_, __float_as_uint(ACC[3])), BEST);                                                               \
      asm volatile("" : "+v"(BEST)); }
    // step N of a tile (N = 8u + q): first MFMA of this unit, second MFMA of the previous unit (operand set P, sub-tile PU,
    // query tile PQ), reduction of the unit three back (query tile RQ); EXTRA = one ds_read_b128 and / or one v_add_f32
#define HX_STEP(N, X, P, PU, PQ, RQ, EXTRA, SCHED)                                       \
      HX_MFMA(acc[(N) & 3], X[(N) >> 3][0], bq[(N) & 7][0], c[(N) >> 3])                 \
      EXTRA                                                                              \
      HX_MFMA(acc[((N) + 3) & 3], P[PU][1], bq[PQ][1], acc[((N) + 3) & 3])               \
      HX_EPI(acc[((N) + 1) & 3], best[RQ])                                               \
      SCHED                                                                              \
      HP_FENCE()
#define HX_SCHED_V  HP_SGB(0x008, 1) HP_SGB(0x002, 1) HP_SGB(0x008, 1) HP_SGB(0x002, 1)
#define HX_SCHED_VV HP_SGB(0x008, 1) HP_SGB(0x002, 2) HP_SGB(0x008, 1) HP_SGB(0x002, 1)
#define HX_SCHED_DV HP_SGB(0x008, 1) HP_SGB(0x100, 1) HP_SGB(0x002, 1) HP_SGB(0x008, 1) HP_SGB(0x002, 1)
#define HX_SCHED_DVV HP_SGB(0x008, 1) HP_SGB(0x100, 1) HP_SGB(0x002, 2) HP_SGB(0x008, 1) HP_SGB(0x002, 1)
    // one train tile out of operand set X; Y is refilled with slot RSLOT behind RD; B = the way from the previous tile to
    // this one (sub-tile 1 follows in steps 0..3), BN = from this one to the next (sub-tile 0 goes ahead in steps 8..11)
#define HX_TILE(X, Y, RD, RSLOT, B, BN)                                                                   \
      HX_WAIT()                                                                                           \
      HX_STEP(0, X, Y, 1, 7, 5, HX_C(1, 0, B), HX_SCHED_VV)                                               \
      HX_STEP(1, X, X, 0, 0, 6, HX_RD(Y, RD, RSLOT, 0, 0) HX_C(1, 1, B), HX_SCHED_DVV)                    \
      HX_STEP(2, X, X, 0, 1, 7, HX_RD(Y, RD, RSLOT, 0, 1) HX_C(1, 2, B), HX_SCHED_DVV)                    \
      HX_STEP(3, X, X, 0, 2, 0, HX_RD(Y, RD, RSLOT, 1, 0) HX_C(1, 3, B), HX_SCHED_DVV)                    \
      HX_STEP(4, X, X, 0, 3, 1, HX_RD(Y, RD, RSLOT, 1, 1), HX_SCHED_DV)                                   \
      HX_STEP(5, X, X, 0, 4, 2, HX_NORD, HX_SCHED_V)                                                      \
      HX_STEP(6, X, X, 0, 5, 3, HX_NORD, HX_SCHED_V)                                                      \
      HX_STEP(7, X, X, 0, 6, 4, HX_NORD, HX_SCHED_V)                                                      \
      HX_STEP(8, X, X, 0, 7, 5, HX_C(0, 0, BN), HX_SCHED_VV)                                              \
      HX_STEP(9, X, X, 1, 0, 6, HX_C(0, 1, BN), HX_SCHED_VV)                                              \
      HX_STEP(10, X, X, 1, 1, 7, HX_C(0, 2, BN), HX_SCHED_VV)                                             \
      HX_STEP(11, X, X, 1, 2, 0, HX_C(0, 3, BN), HX_SCHED_VV)                                             \
      HX_STEP(12, X, X, 1, 3, 1, HX_NORD, HX_SCHED_V)                                                     \
      HX_STEP(13, X, X, 1, 4, 2, HX_NORD, HX_SCHED_V)                                                     \
      HX_STEP(14, X, X, 1, 5, 3, HX_NORD, HX_SCHED_V)                                                     \
      HX_STEP(15, X, X, 1, 6, 4, HX_NORD, HX_SCHED_V)
    // A stage out of buffer CUR in two halves.  The barrier between them publishes the NEXT stage (this wave's LDS-DMA of it
    // was issued a whole stage ago) and frees the buffer of the PREVIOUS one for the stage after the next, as in the forms above.
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int s = 0; s < 2; ++s) { aA[u][s] = v4i{0, 0, 0, 0}; aB[u][s] = v4i{0, 0, 0, 0}; }
    rdc = cur + lp16;
    HX_RD(aA, rdc, 0, 0, 0) HX_RD(aA, rdc, 0, 0, 1) HX_RD(aA, rdc, 0, 1, 0) HX_RD(aA, rdc, 0, 1, 1)
    // the first three steps finish and reduce units that do not exist: their accumulators are kNone and stay it
    v4f acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = v4f{kNone, kNone, kNone, kNone};
    {
      const float b0 = (float)slot_tile(0) * kRowUnitPerTile;
#pragma unroll
      for (int i = 0; i < 4; ++i) { c[0][i] += b0; c[1][i] += b0; }
    }
    for (uint32_t st = 0;;) {
      {
        const float b0 = st > 0u ? HX_DELTA(0) : 0.f, b1 = HX_DELTA(1), b2 = HX_DELTA(2);
        rdc = cur + lp16;
        HP_FENCE()
        HX_TILE(aA, aB, rdc, 1, b0, b1)
        HX_TILE(aB, aA, rdc, 2, b1, b2)
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's share of the next stage has landed
        __syncthreads();
        if (has_ragged && st + 2u == n_stages) patch_ragged(nxt, kPipeStage - 1u);   // the next stage is the last one
      }
      {
        if (st + 2u < n_stages) load_stage(st + 2u, fill);
        const float b2 = HX_DELTA(2), b3 = HX_DELTA(3), b4 = HX_DELTA(4);   // (slot 4 = the next stage's slot 0)
        rdn = nxt + lp16;
        HP_FENCE()
        HX_TILE(aA, aB, rdc, 3, b2, b3)
        HX_TILE(aB, aA, rdn, 0, b3, b4)
      }
      if (++st == n_stages) break;
      const uint32_t t_ = cur; cur = nxt; nxt = fill; fill = t_;
    }
    // the last unit's second MFMA and the last three reductions (behind the last tile's reads, which nobody uses: their
    // registers are free for others only once they have landed)
    HX_WAIT()
    HX_MFMA(acc[3], aB[1][1], bq[7][1], acc[3])
    HX_EPI(acc[1], best[5])
    HX_EPI(acc[2], best[6])
    HX_EPI(acc[3], best[7])
#undef HX_TILE
#undef HX_SCHED_V
#undef HX_SCHED_VV
#undef HX_SCHED_DV
#undef HX_SCHED_DVV
#undef HX_STEP
#undef HX_EPI
#undef HX_C
#undef HX_DELTA
#undef HX_NORD
#undef HX_WAIT
#undef HX_RD
  }

  // a query's minimum is spread over the four row groups of its column: lanes q, q + 16, q + 32, q + 48
  uint32_t* kout = keys + ((size_t)pair * tsplit + split) * max_kp;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    uint32_t bb = best[q];
    bb = min(bb, (uint32_t)__shfl_xor((int)bb, 16));
    bb = min(bb, (uint32_t)__shfl_xor((int)bb, 32));
    const float b = __uint_as_float(bb);
    const uint32_t qi = qblock * kQPB + (wave * 4u + (uint32_t)(q >> 1)) * 32u + (uint32_t)(q & 1) * 16u + (lane & 15u);
    if (grp == 0 && qi < nq) {
      uint32_t key = kNoMatchKey;
      if (b < 1024.0f) {  // real keys: 2*hd + row / 2^14 < 516; phantoms are >= 2^22
        const uint32_t k = (uint32_t)(b * 16384.0f);
        key = ((k >> 15) << 16) | (k & 32767u);
      }
      kout[qi] = key;
    }
  }
}
#undef HX_MFMA
#undef HP_SGB
#undef HP_FENCE

}  // namespace

}  // namespace rgbdfe

// tests: the slot enumeration of one block of the pipelined kernel (host only; tiles_out[s] = train tile of slot s or
// 0x7FFFFFFF for a phantom); returns the number of slots (4 x stages) or -1 when they do not fit
extern "C" int rgbdfe_debug_hamming_slots(uint32_t nt, uint32_t tsplit, uint32_t split, uint32_t* tiles_out, int capacity,
                                          int* has_ragged, uint32_t* n_ttiles) {
  const rgbdfe::HammingSlots s = rgbdfe::HammingSlots::make(nt, tsplit, split, 4u);
  if (has_ragged) *has_ragged = s.has_ragged ? 1 : 0;
  if (n_ttiles) *n_ttiles = s.n_ttiles;
  const int n = (int)(s.n_stages * 4u);
  if (n > capacity) return -1;
  for (int i = 0; i < n; ++i) tiles_out[i] = s.tile((uint32_t)i);
  return n;
}

namespace rgbdfe {

uint32_t hamming_mfma_tiles_per_slot(uint32_t max_kp) { return (max_kp + 31u) / 32u; }

size_t hamming_mfma_slab_bytes(uint32_t max_nodes, uint32_t max_kp) {
  return ((size_t)max_nodes * hamming_mfma_tiles_per_slot(max_kp) + 1u) * 4096u;
}

void launch_hamming_expand(const uint32_t* node_rows, uint32_t* slab, uint32_t slot, uint32_t max_kp, uint32_t n,
                           hipStream_t stream) {
  if (n == 0) return;
  const uint32_t tiles = (n + 31u) / 32u;
  uint4* dst = reinterpret_cast<uint4*>(slab) + (size_t)slot * hamming_mfma_tiles_per_slot(max_kp) * 256u;
  hipLaunchKernelGGL(hamming_expand_kernel, dim3(tiles), dim3(256), 0, stream, node_rows, dst, n);
}

// The wide (512-query) form of the pipelined kernel halves the blocks of a batch and doubles their length.  The automatic
// choice takes it only where that costs nothing: the train rows are not split (a batch that needs splits to fill the chip has
// no blocks to spare: live SLAM, ~20 pairs), and the batch is still at least kWideMinBlocksPerSlot blocks deep on every one of
// the chip's block slots (256 CUs x 3 blocks of 48 KB LDS).  A launch ends with a partly idle chip for about one block's
// length; a wide block is two narrow ones long, so the wide form adds one narrow block's length of tail to a launch that is
// 2 x depth of them long: 1 / (2 x 10) = 5 % at the threshold in the worst case (a last round of one block), about half of
// that on average and less for deeper batches -- against the 3-4 % the wide form gains where it was measured, at 8000 blocks
// of equal length.  Below the threshold nothing is known to be gained, so nothing changes there.
constexpr uint32_t kHammingBlockSlots = 256u * 3u;
constexpr uint32_t kWideMinBlocksPerSlot = 10u;

// The MFMA tile the automatic choice gives 512-query blocks: what was measured faster at both batch sizes.
// (A variant build that fixes RGBDFE_HAMMING_PIPE_QT is there to time the 32x32x64 kernels: it keeps their tile.)
#ifndef RGBDFE_HAMMING_WIDE_SHAPE
#if RGBDFE_HAMMING_PIPE_QT == 0
#define RGBDFE_HAMMING_WIDE_SHAPE 16
#else
#define RGBDFE_HAMMING_WIDE_SHAPE 32
#endif
#endif

// pipe_wide: -1 = choose (the pipelined kernel only), 0 = 256-query blocks, 1 = 512-query blocks;
// wide_shape: 0 = choose, 16 / 32 = the MFMA tile of 512-query blocks
HammingGeometry hamming_mfma_geometry(uint32_t n_pairs, uint32_t max_nq, uint32_t max_nt, uint32_t key_planes_capacity,
                                      int pipe_wide, int wide_shape) {
  HammingGeometry g{0, 1, 0, 32};
  if (n_pairs == 0 || max_nq == 0) return g;
  const uint32_t ttiles = (max_nt + 31u) / 32u;
  auto shape = [&](uint32_t queries_per_block) {
    HammingGeometry h{(max_nq + queries_per_block - 1u) / queries_per_block, 1, 0, 32};
    // small batches (live SLAM: ~20 pairs per frame) split the train tiles over several blocks, one key plane each
    const uint32_t blocks1 = n_pairs * h.qblocks;
    if (blocks1 < 1024 && ttiles > kStage) {
      uint32_t tsplit = (1024 + blocks1 - 1) / blocks1;
      const uint32_t max_split = (ttiles + kStage - 1) / kStage;  // at least one LDS stage per block
      if (tsplit > max_split) tsplit = max_split;
      if (tsplit > 32) tsplit = 32;
      const uint32_t fit = key_planes_capacity / n_pairs;
      if (tsplit > fit) tsplit = fit;
      if (tsplit < 1) tsplit = 1;
      h.tsplit = tsplit;
    }
    return h;
  };
  g = shape(kQueriesPerBlock);
  if (pipe_wide < 0) {
#if RGBDFE_HAMMING_PIPE_QT == 4
    pipe_wide = 1;
#elif RGBDFE_HAMMING_PIPE_QT == 2
    pipe_wide = 0;
#else
    const uint64_t wide_blocks = (uint64_t)n_pairs * ((max_nq + 2u * kQueriesPerBlock - 1u) / (2u * kQueriesPerBlock));
    pipe_wide = g.tsplit == 1u && wide_blocks >= (uint64_t)kHammingBlockSlots * kWideMinBlocksPerSlot ? 1 : 0;
#endif
  }
  if (pipe_wide > 0) {
    g = shape(2u * kQueriesPerBlock);
    g.wide = 1;
    g.shape = wide_shape == 16 || wide_shape == 32 ? (uint32_t)wide_shape : (uint32_t)RGBDFE_HAMMING_WIDE_SHAPE;
  }
  return g;
}

uint32_t launch_hamming_mfma(const uint32_t* slab, const PairWork* work, uint32_t* keys, uint32_t max_kp,
                             uint32_t n_pairs, HammingGeometry geom, int mode, hipStream_t stream) {
  if (n_pairs == 0 || geom.qblocks == 0) return 1;
  const uint32_t qblocks = geom.qblocks, tsplit = geom.tsplit;
  const uint32_t tiles_per_slot = hamming_mfma_tiles_per_slot(max_kp);
  const uint32_t pairs8 = (n_pairs + 7u) / 8u * 8u;
  const uint32_t grid = pairs8 * qblocks * tsplit;
  const uint4* s4 = reinterpret_cast<const uint4*>(slab);
#define RGBDFE_LAUNCH_HM(M, S)                                                                                   \
  hipLaunchKernelGGL((hamming_mfma_kernel<M, S>), dim3(grid), dim3(kThreads), 0, stream, s4, work, keys, max_kp, \
                     tiles_per_slot, n_pairs, qblocks, tsplit)
#define RGBDFE_LAUNCH_HP(QT, S)                                                                                        \
  hipLaunchKernelGGL((hamming_mfma_pipe_kernel<QT, S>), dim3(grid), dim3(kThreads), 0, stream, s4, work, keys, max_kp, \
                     tiles_per_slot, n_pairs, qblocks, tsplit)
#define RGBDFE_LAUNCH_HX(S)                                                                                        \
  hipLaunchKernelGGL((hamming_mfma_x16_kernel<S>), dim3(grid), dim3(kThreads), 0, stream, s4, work, keys, max_kp, \
                     tiles_per_slot, n_pairs, qblocks, tsplit)
  if (mode == 3 || mode == 4) {   // the geometry says which form (mode 4's is always wide, an explicit mode 3's never)
    if (geom.wide && geom.shape == 16) {
      if (tsplit > 1) RGBDFE_LAUNCH_HX(true); else RGBDFE_LAUNCH_HX(false);
    } else if (geom.wide) {
      if (tsplit > 1) RGBDFE_LAUNCH_HP(4, true); else RGBDFE_LAUNCH_HP(4, false);
    } else {
      if (tsplit > 1) RGBDFE_LAUNCH_HP(2, true); else RGBDFE_LAUNCH_HP(2, false);
    }
  } else if (mode == 2) {
    if (tsplit > 1) RGBDFE_LAUNCH_HM(2, true); else RGBDFE_LAUNCH_HM(2, false);
  } else {
    if (tsplit > 1) RGBDFE_LAUNCH_HM(1, true); else RGBDFE_LAUNCH_HM(1, false);
  }
#undef RGBDFE_LAUNCH_HX
#undef RGBDFE_LAUNCH_HP
#undef RGBDFE_LAUNCH_HM
  return tsplit;
}

}  // namespace rgbdfe
