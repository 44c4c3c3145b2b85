// octomap_tree.hip -- the whole octree of an occupancy map from its leaves, on the device, gfx950: inner nodes
// (updateInnerOccupancy), the pre-order node records of an .ot file, and the nodes of one depth.  The contract is the
// "occupancy map: the tree of a leaf set" block of include/rgbdfe.h.
//
// A leaf's path code is its key with the bits of the three coordinates interleaved (bit b of key[a] -> bit 3 b + a): the child
// index of depth d is the three bits at 3 (16 - d), so ascending path code is depth-first pre-order with the children in
// ascending index.  Every stage is count -> scan -> write over tiles of kTreeTile elements (`tree_count_kernel`,
// `tree_scan_kernel`, `tree_write_kernel`, instantiated per stage); a position comes from the element's index alone.
//
//   gather   a lane per table slot: the leaves, compacted in slot order: (path code, slot), sort key = the low 24 bits
//   sort     launch_vox_sort (voxel_filter.hip, unchanged) twice, three 8-bit passes each: by the low 24 bits, then
//            (tree_rekey_kernel) by the high 24 bits; the sort is stable, so the result is ascending path code
//   arrange  a lane per sorted leaf: code / value / colour of depth 16 in tree order, and top[j] = the shallowest depth
//            whose node has leaf j as its first leaf = 16 - hb / 3 with hb the highest bit in which the code differs from
//            its predecessor's (0, the root, for the first leaf).  Leaf j opens the 17 - top[j] nodes of depths top[j] .. 16.
//   chain    the exclusive scan of 17 - top[j]: off[j] = the pre-order position of the node of depth top[j]; the node of
//            depth d whose first leaf is j stands at off[j] + (d - top[j]).  The total is the node count (the one value the
//            host reads before the capacity check).
//   levels   depth 15 down to 0.  The nodes of depth d + 1 are in tree order in one of two level buffers (value, colour |
//            mask << 24, first leaf); node i starts a parent iff top[first[i]] <= d.  A lane per such head walks the
//            <= 8 nodes up to the next head: float maximum from -FLT_MAX, integer colour sums over the children that are
//            not white, child mask; it writes the parent into the other buffer at its rank and, when a tree is wanted,
//            its 8-byte record.  The count of each depth stays on the device (TreeHdr::cnt); a grid is sized by the
//            bound min(leaves, 8^depth) and the surplus workgroups leave at once.
//   leaves   a lane per leaf: its record at off[j] + (16 - top[j]).
//   filter   the nodes of one depth with value >= the threshold, compacted, as rgbdfe_octomap_leaf records.
//
// No atomics at all, no workgroup waits for another, plain vector stores; the bytes are a function of the leaf set.
#include "rgbdfe_internal.h"

#include <cfloat>

namespace rgbdfe {

namespace {

__device__ __forceinline__ unsigned long long spread3(uint32_t v) {  // bit b -> bit 3 b, 16 bits
  unsigned long long x = v & 0xffffu;
  x = (x | (x << 16)) & 0x0000ff0000ffull;
  x = (x | (x << 8)) & 0x00f00f00f00full;
  x = (x | (x << 4)) & 0x0c30c30c30c3ull;
  x = (x | (x << 2)) & 0x249249249249ull;
  return x;
}
__device__ __forceinline__ uint32_t gather3(unsigned long long x) {  // the inverse
  x &= 0x249249249249ull;
  x = (x | (x >> 2)) & 0x0c30c30c30c3ull;
  x = (x | (x >> 4)) & 0x00f00f00f00full;
  x = (x | (x >> 8)) & 0x0000ff0000ffull;
  x = (x | (x >> 16)) & 0xffffull;
  return (uint32_t)x;
}
// the second word of a node record: the bytes r, g, b, child mask from col = r << 16 | g << 8 | b
__device__ __forceinline__ uint32_t tree_record_word(uint32_t col, uint32_t mask) {
  return ((col >> 16) & 255u) | (col & 0xff00u) | ((col & 255u) << 16) | (mask << 24);
}
__device__ __forceinline__ unsigned long long code_of_key(unsigned long long key) {
  return spread3((uint32_t)key) | (spread3((uint32_t)(key >> 16)) << 1) | (spread3((uint32_t)(key >> 32)) << 2);
}

// the exclusive prefix of v over the 256 threads of the workgroup; *total = the sum (to every thread)
__device__ __forceinline__ uint32_t block_excl_256(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= (uint32_t)d) incl += o;
  }
  __syncthreads();  // the previous use of wave_tot is over
  if (lane == 63) wave_tot[wv] = incl;
  __syncthreads();
  uint32_t off = 0, sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t t = wave_tot[w];
    if (w < wv) off += t;
    sum += t;
  }
  *total = sum;
  return off + incl - v;
}

// A stage S: n() elements, value(i) of element i < n(), emit(i, value, position) with position = the sum of the values
// in front of i.  Thread t of tile b owns the elements b * kTreeTile + 4 t .. + 3.
template <class S>
__global__ __launch_bounds__(256) void tree_count_kernel(S s, uint32_t* __restrict__ tile_count) {
  const uint32_t n = s.n();
  const uint64_t i0 = (uint64_t)blockIdx.x * kTreeTile + 4u * threadIdx.x;
  if ((uint64_t)blockIdx.x * kTreeTile >= n) return;  // the whole workgroup
  uint32_t v = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    if (i0 + j < n) v += s.value((uint32_t)(i0 + j));
  uint32_t total;
  (void)block_excl_256(v, &total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// one workgroup: tile_first = the exclusive scan of tile_count over the tiles of *n_ptr (or n_imm) elements; *total_out
__global__ __launch_bounds__(1024) void tree_scan_kernel(const uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ n_ptr,
                                                         uint32_t n_imm, uint32_t* __restrict__ tile_first,
                                                         uint32_t* __restrict__ total_out) {
  __shared__ uint32_t wave_tot[16];
  __shared__ uint32_t base;
  const uint32_t n_elem = n_ptr ? *n_ptr : n_imm;
  const uint32_t n = (uint32_t)(((uint64_t)n_elem + kTreeTile - 1) / kTreeTile);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < n; t0 += 1024u) {
    const uint32_t t = t0 + tid;
    const uint32_t c = t < n ? tile_count[t] : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t w = 0; w < wv; ++w) off += wave_tot[w];
    if (t < n) tile_first[t] = base + off + incl - c;
    __syncthreads();
    if (tid == 0) {
      uint32_t s = 0;
      for (int w = 0; w < 16; ++w) s += wave_tot[w];
      base += s;
    }
    __syncthreads();
  }
  if (tid == 0) *total_out = base;
}

template <class S>
__global__ __launch_bounds__(256) void tree_write_kernel(S s, const uint32_t* __restrict__ tile_first) {
  const uint32_t n = s.n();
  const uint64_t i0 = (uint64_t)blockIdx.x * kTreeTile + 4u * threadIdx.x;
  if ((uint64_t)blockIdx.x * kTreeTile >= n) return;
  uint32_t v[4], sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    v[j] = i0 + j < n ? s.value((uint32_t)(i0 + j)) : 0u;
    sum += v[j];
  }
  uint32_t total;
  uint32_t at = tile_first[blockIdx.x] + block_excl_256(sum, &total);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    if (i0 + j < n) s.emit((uint32_t)(i0 + j), v[j], at);
    at += v[j];
  }
}

struct GatherStage {
  OctoTable tb;
  unsigned long long* code;  // of the compacted leaves
  uint32_t *slot, *key, *idx;
  uint32_t limit;            // the rows the arrays have (= the leaves the host counts)
  __device__ uint32_t n() const { return tb.cap; }
  __device__ uint32_t value(uint32_t i) const {
    return tb.key[i] != kOctoEmptyKey && __float_as_uint(tb.value[i]) != kOctoNoLeaf ? 1u : 0u;
  }
  __device__ void emit(uint32_t i, uint32_t v, uint32_t at) const {
    if (!v || at >= limit) return;  // (a table with more leaves than the host counts is reported by the caller)
    const unsigned long long c = code_of_key(tb.key[i]);
    code[at] = c;
    slot[at] = i;
    key[at] = (uint32_t)c & 0xffffffu;
    idx[at] = at;
  }
};

struct ChainStage {
  const TreeHdr* hdr;
  const uint32_t* top;
  uint32_t* off;
  __device__ uint32_t n() const { return hdr->cnt[16]; }
  __device__ uint32_t value(uint32_t i) const { return 17u - top[i]; }
  __device__ void emit(uint32_t i, uint32_t, uint32_t at) const { off[i] = at; }
};

// depth d from depth d + 1
struct LevelStage {
  const TreeHdr* hdr;
  TreeLevel child, parent;
  const unsigned long long* code;  // of the sorted leaves
  const uint32_t *top, *off;
  uint2* out;                      // the records, or NULL
  uint32_t d;
  __device__ uint32_t n() const { return hdr->cnt[d + 1u]; }
  __device__ uint32_t value(uint32_t i) const { return top[child.first[i]] <= d ? 1u : 0u; }
  __device__ void emit(uint32_t i, uint32_t v, uint32_t at) const {
    if (!v) return;
    const uint32_t nc = n(), j = child.first[i], shift = 3u * (15u - d);
    float mx = -FLT_MAX;
    uint32_t r = 0, g = 0, b = 0, c = 0, mask = 0;
    for (uint32_t k = 0; k < 8u; ++k) {  // (a parent has at most 8 children: the bound only guards the loop)
      const uint32_t m = i + k;
      if (m >= nc) break;
      const uint32_t f = child.first[m];
      if (k > 0 && top[f] <= d) break;  // the next parent
      const float val = child.value[m];
      if (val > mx) mx = val;
      const uint32_t col = child.colour[m] & 0xffffffu;
      if (col != 0xffffffu) {
        r += (col >> 16) & 255u; g += (col >> 8) & 255u; b += col & 255u;
        ++c;
      }
      mask |= 1u << ((uint32_t)(code[f] >> shift) & 7u);
    }
    uint32_t col = 0xffffffu;
    if (c > 0) col = ((r / c) << 16) | ((g / c) << 8) | (b / c);
    parent.value[at] = mx;
    parent.colour[at] = col | (mask << 24);
    parent.first[at] = j;
    if (out) out[(size_t)off[j] + (d - top[j])] = make_uint2(__float_as_uint(mx), tree_record_word(col, mask));
  }
};

struct FilterStage {
  const TreeHdr* hdr;
  TreeLevel lv;
  const unsigned long long* code;
  uint4* out;
  float thr;
  uint32_t d;
  __device__ uint32_t n() const { return hdr->cnt[d]; }
  __device__ uint32_t value(uint32_t i) const { return lv.value[i] >= thr ? 1u : 0u; }
  __device__ void emit(uint32_t i, uint32_t v, uint32_t at) const {
    if (!v) return;
    const unsigned long long c = code[lv.first[i]];
    const uint32_t keep = (0xffffu << (16u - d)) & 0xffffu;
    const uint32_t k0 = gather3(c) & keep, k1 = gather3(c >> 1) & keep, k2 = gather3(c >> 2) & keep;
    const uint32_t col = lv.colour[i];
    out[at] = make_uint4(k0 | (k1 << 16), k2, __float_as_uint(lv.value[i]),
                         ((col >> 16) & 255u) | (col & 0xff00u) | ((col & 255u) << 16));
  }
};

// the keys of the second sort: the high 24 bits of the code of the leaf each row stands for
__global__ __launch_bounds__(256) void tree_rekey_kernel(const unsigned long long* __restrict__ code, const uint32_t* __restrict__ idx,
                                                        uint32_t n, uint32_t* __restrict__ key) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) key[i] = (uint32_t)(code[idx[i]] >> 24);
}

__global__ __launch_bounds__(256) void tree_arrange_kernel(OctoTable tb, const unsigned long long* __restrict__ code,
                                                          const uint32_t* __restrict__ slot, const uint32_t* __restrict__ idx,
                                                          uint32_t n, unsigned long long* __restrict__ scode, TreeLevel lv,
                                                          uint32_t* __restrict__ top) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t r = idx[j];
  const unsigned long long c = code[r];
  const uint32_t s = slot[r];
  scode[j] = c;
  lv.value[j] = tb.value[s];
  lv.colour[j] = tb.colour[s] & 0xffffffu;
  lv.first[j] = j;
  uint32_t t = 0;
  if (j > 0) {
    const unsigned long long x = c ^ code[idx[j - 1]];  // the keys are distinct; a zero would give depth 16 + 1 below
    const uint32_t hb = x ? 63u - (uint32_t)__clzll((long long)x) : 0u;
    t = 16u - hb / 3u;
  }
  top[j] = t;
}

__global__ __launch_bounds__(256) void tree_leaf_records_kernel(const TreeHdr* __restrict__ hdr, TreeLevel lv,
                                                               const uint32_t* __restrict__ top, const uint32_t* __restrict__ off,
                                                               uint2* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= hdr->cnt[16]) return;
  out[(size_t)off[j] + (16u - top[j])] = make_uint2(__float_as_uint(lv.value[j]), tree_record_word(lv.colour[j] & 0xffffffu, 0u));
}

inline uint32_t blocks_of(uint32_t n, uint32_t per) { return (uint32_t)(((uint64_t)n + per - 1) / per); }

template <class S>
void run_stage(const S& s, uint32_t bound, const uint32_t* n_ptr, uint32_t n_imm, const TreeScratch& t, uint32_t* total_out,
               hipStream_t stream) {
  const uint32_t tiles = blocks_of(bound, kTreeTile);
  if (tiles > 0) hipLaunchKernelGGL(tree_count_kernel<S>, dim3(tiles), dim3(256), 0, stream, s, t.tile_count);
  hipLaunchKernelGGL(tree_scan_kernel, dim3(1), dim3(1024), 0, stream, t.tile_count, n_ptr, n_imm, t.tile_first, total_out);
  if (tiles > 0) hipLaunchKernelGGL(tree_write_kernel<S>, dim3(tiles), dim3(256), 0, stream, s, t.tile_first);
}

// the nodes of depth d are at most min(n_leaves, 8^d)
inline uint32_t level_bound(uint32_t n_leaves, uint32_t d) {
  return d >= 11u ? n_leaves : (uint32_t)std::min<uint64_t>(n_leaves, (uint64_t)1 << (3u * d));
}

}  // namespace

int launch_tree_leaves(const OctoTable& tb, uint32_t n_leaves, const TreeScratch& t, hipStream_t stream) {
  int launches = 0;
  GatherStage g{tb, t.code, t.slot, t.keys[0], t.idx[0], n_leaves};
  run_stage(g, tb.cap, nullptr, tb.cap, t, &t.hdr->cnt[16], stream);
  launches += 3;
  if (n_leaves == 0) return launches;
  uint32_t* keys[2] = {t.keys[0], t.keys[1]};
  uint32_t* idx[2] = {t.idx[0], t.idx[1]};
  int cur = launch_vox_sort(n_leaves, 3, keys, idx, t.hist, t.digits, stream);
  hipLaunchKernelGGL(tree_rekey_kernel, dim3(blocks_of(n_leaves, 256u)), dim3(256), 0, stream, t.code, idx[cur], n_leaves, keys[cur]);
  uint32_t* keys2[2] = {keys[cur], keys[cur ^ 1]};
  uint32_t* idx2[2] = {idx[cur], idx[cur ^ 1]};
  cur = launch_vox_sort(n_leaves, 3, keys2, idx2, t.hist, t.digits, stream);
  hipLaunchKernelGGL(tree_arrange_kernel, dim3(blocks_of(n_leaves, 256u)), dim3(256), 0, stream, tb, t.code, t.slot, idx2[cur], n_leaves,
                     t.scode, t.level[0], t.top);
  return launches + 9 + 1 + 9 + 1;
}

int launch_tree_chain(uint32_t n_leaves, const TreeScratch& t, hipStream_t stream) {
  ChainStage c{t.hdr, t.top, t.off};
  run_stage(c, n_leaves, &t.hdr->cnt[16], 0u, t, &t.hdr->n_nodes, stream);
  return 3;
}

int launch_tree_levels(uint32_t n_leaves, uint32_t down_to, const TreeScratch& t, void* d_records, hipStream_t stream) {
  int launches = 0;
  if (d_records) {
    hipLaunchKernelGGL(tree_leaf_records_kernel, dim3(blocks_of(n_leaves, 256u)), dim3(256), 0, stream, t.hdr, t.level[0], t.top,
                       t.off, (uint2*)d_records);
    ++launches;
  }
  for (uint32_t d = 15u; d + 1u > down_to; --d) {  // the level of depth d lands in t.level[(16 - d) & 1]
    LevelStage l{t.hdr, t.level[(15u - d) & 1u], t.level[(16u - d) & 1u], t.scode, t.top, t.off, (uint2*)d_records, d};
    run_stage(l, level_bound(n_leaves, d + 1u), &t.hdr->cnt[d + 1u], 0u, t, &t.hdr->cnt[d], stream);
    launches += 3;
    if (d == 0u) break;
  }
  return launches;
}

int launch_tree_filter(uint32_t n_leaves, uint32_t depth, float min_log_odds, const TreeScratch& t, void* d_out, hipStream_t stream) {
  FilterStage f{t.hdr, t.level[(16u - depth) & 1u], t.scode, (uint4*)d_out, min_log_odds, depth};
  run_stage(f, level_bound(n_leaves, depth), &t.hdr->cnt[depth], 0u, t, &t.hdr->n_out, stream);
  return 3;
}

}  // namespace rgbdfe
