// fast_detect.hip -- feature_detector_type "FAST" on gfx950: the grid of threshold-adaptive cv::FAST detectors
// (features.cpp:71-72, 100-112; feature_adjuster.cpp:88-91, 185-317) and Node::Node's ORB-extractor steps after it
// (node.cpp:183-210), for a chunk of frames in four launches and no host round trip.
//
// FAST's survivors at a threshold t >= 2 are exactly its survivors at threshold 2 whose score is >= t (a corner at t is a pixel
// whose cornerScore is >= t, and the 3x3 suppression only compares corners), so one threshold-free pass per frame answers
// every threshold the adjuster can ask for (it never goes below 2):
//   fast_pass_kernel    per (frame, cell) 64 x 16 tile: FAST-9/16 scores at floor 2 with the cell's own 3-pixel border, the
//                       3x3 suppression inside the cell, the mask; keep bits, survivor scores, a 256-bin survivor-score
//                       histogram per (frame, cell) and hasNonZero(sub_mask)
//   fast_adjust_kernel  one wave per cell walks the chunk's frames in order: the reference's adjuster loop on suffix sums of the
//                       histogram (the count at threshold t), then keepStrongest's cut as (score, ties taken in raster order)
//   fast_select_kernel  one workgroup per frame: the cells' survivors above the cut in raster order, aggregated in row-major
//                       cell order; removeDepthless; the max_keypoints cut; ORB::compute's 31-pixel border filter;
//                       projectTo3D into the node slab and / or the chunk's output rows
//   fast_brief_kernel   rBRIEF at angle -1 on the 7x7 sigma-2 blurred frame (orb_blur_kernel), one wave per keypoint
#include "fast_internal.h"
#include "fast_device.h"
#include "project3d_device.h"

namespace rgbdfe {

typedef uint32_t __attribute__((aligned(1))) u32_unaligned_f;

__device__ __forceinline__ int wave_excl_scan(int v, int lane, int* total) {
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  *total = __shfl(incl, 63);
  return incl - v;
}

// ------------------------------------------------------------------------------------------------
// pass: one workgroup per 64 x 16 tile of one (frame, cell) sub-image (the ORB pass's tiling, orb_fast_nms_kernel)
// ------------------------------------------------------------------------------------------------
constexpr int kFTW = 64, kFTH = 16, kFSrcStride = 76, kFScStride = 68;
__global__ __launch_bounds__(256) void fast_pass_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ mask,
                                                        const int32_t* __restrict__ has_mask, const FastGeom g, int floor_thr,
                                                        uint64_t* __restrict__ keep, uint8_t* __restrict__ score,
                                                        int32_t* __restrict__ hist, int32_t* __restrict__ mask_nz) {
  __shared__ __attribute__((aligned(4))) uint8_t src[(kFTH + 8) * kFSrcStride];
  __shared__ uint8_t sc[(kFTH + 2) * kFScStride];
  __shared__ uint16_t cand[(kFTH + 2) * 66];
  __shared__ int lhist[256];
  __shared__ int n_cand, any_mask;
  const int f = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  int c = 0;
  while (c + 1 < g.n_cells && t >= g.cell[c + 1].tile_begin) ++c;
  const FastCellGeom ce = g.cell[c];
  const int tl = t - ce.tile_begin;
  const int by = tl / ce.tiles_x, bx = tl - by * ce.tiles_x;
  const int x0 = bx * kFTW, y0 = by * kFTH, w = ce.w, h = ce.h, cols = g.cols;
  const size_t org = (size_t)f * g.plane + (size_t)ce.y0 * cols + ce.x0;
  const uint8_t* __restrict__ img = gray + org;
  const bool hm = has_mask[f] != 0;
  lhist[tid] = 0;
  if (tid == 0) { n_cand = 0; any_mask = 0; }
  // sub-image rows y0 - 4 .. y0 + 19 (clamped into the cell), columns x0 - 4 .. x0 + 67.  Bytes outside the cell -- a dword
  // reaching past its right edge, a clamped row -- feed only pixels of the cell's 3-pixel border, whose score is 0 by
  // definition (cv::FAST looks only inside the sub-image).  The pools have slack behind the last frame for the last dword.
  for (int i = tid; i < (kFTH + 8) * 18; i += 256) {
    const int r = (i * 3641) >> 16, j = i - r * 18;   // i / 18 for i < 432
    const int gy = min(max(y0 - 4 + r, 0), h - 1), gx = x0 - 4 + 4 * j;
    uint32_t v = 0;
    if (gx >= 0 && gx < w) v = *reinterpret_cast<const u32_unaligned_f*>(img + (size_t)gy * cols + gx);
    *reinterpret_cast<uint32_t*>(src + r * kFSrcStride + 4 * j) = v;
  }
  if (hm) {  // hasNonZero(sub_mask) (feature_adjuster.cpp:175-183): any pixel of the cell, border included
    const uint8_t* __restrict__ mk = mask + org;
    bool nz = false;
    for (int i = tid; i < kFTW * kFTH; i += 256) {
      const int x = x0 + (i & 63), y = y0 + (i >> 6);
      if (x < w && y < h && mk[(size_t)y * cols + x]) nz = true;
    }
    if (nz) any_mask = 1;
  }
  __syncthreads();
  // the four-pixel screen (a necessary condition for a score above the floor, orb_fast_nms_kernel), then the arc score of the
  // pixels that pass; the score of a corner is independent of the floor
  for (int i0 = 0; i0 < (kFTH + 2) * 66; i0 += 256) {
    const int i = i0 + tid;
    bool pass = false;
    if (i < (kFTH + 2) * 66) {
      const int ty = (i * 993) >> 16, tx = i - ty * 66;   // i / 66 for i < 1188
      const int x = x0 - 1 + tx, y = y0 - 1 + ty;
      sc[ty * kFScStride + tx] = 0;
      if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
        const uint8_t* ptr = src + (ty + 3) * kFSrcStride + (tx + 3);
        const int v = ptr[0];
        const int d0 = v - ptr[3 * kFSrcStride], d8 = v - ptr[-3 * kFSrcStride], d4 = v - ptr[3], d12 = v - ptr[-3];
        pass = (max(d0, d8) > floor_thr && max(d4, d12) > floor_thr) || (min(d0, d8) < -floor_thr && min(d4, d12) < -floor_thr);
      }
    }
    const uint64_t m = __ballot(pass);
    if (m) {
      const int lane = tid & 63;
      int base = 0;
      if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(&n_cand, (int)__popcll(m));
      base = __shfl(base, (int)__builtin_ctzll(m));
      if (pass) cand[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)i;
    }
  }
  __syncthreads();
  for (int q = tid; q < n_cand; q += 256) {
    const int i = cand[q];
    const int ty = (i * 993) >> 16, tx = i - ty * 66;
    const int mm = fast_arc_score(src + (ty + 3) * kFSrcStride + (tx + 3), kFSrcStride);
    if (mm > floor_thr) sc[ty * kFScStride + tx] = (uint8_t)(mm - 1);
  }
  __syncthreads();
  // 3x3 suppression (strict >, neighbours outside the cell's [3, w - 4] x [3, h - 4] score 0) + runByPixelsMask;
  // wave v: rows 4v .. 4v + 3 of the tile, lane = column
  const int lane = tid & 63, wv = tid >> 6;
  const size_t fc = (size_t)f * g.n_cells + c;
  uint64_t* __restrict__ keep_c = keep + (size_t)f * g.keep_words + ce.keep_off;
  uint8_t* __restrict__ score_c = score + (size_t)f * g.score_bytes + ce.score_off;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int ty = wv * 4 + rr, y = y0 + ty, x = x0 + lane;
    if (y >= h) break;
    const uint8_t* p = sc + (ty + 1) * kFScStride + (lane + 1);
    const int s = p[0];
    bool k = false;
    if (s && x < w) {
      k = s > p[1] && s > p[-1] && s > p[-kFScStride - 1] && s > p[-kFScStride] && s > p[-kFScStride + 1] &&
          s > p[kFScStride - 1] && s > p[kFScStride] && s > p[kFScStride + 1];
      if (k && hm && mask[org + (size_t)y * cols + x] == 0) k = false;
    }
    if (k) {
      score_c[(size_t)y * w + x] = (uint8_t)s;   // read back only where a keep bit is set
      atomicAdd(&lhist[s], 1);
    }
    const uint64_t m = __ballot(k);
    if (lane == 0) keep_c[(size_t)y * ce.tiles_x + bx] = m;
  }
  __syncthreads();
  const int v = lhist[tid];
  if (v) atomicAdd(&hist[fc * 256 + tid], v);   // one global add per non-empty bin
  if (tid == 0 && any_mask) mask_nz[fc] = 1;
}

// ------------------------------------------------------------------------------------------------
// adjuster: one wave per cell, the chunk's frames in order (a cell's threshold chain depends on its own history only)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void fast_adjust_kernel(const int32_t* __restrict__ hist, const int32_t* __restrict__ mask_nz,
                                                         const int32_t* __restrict__ has_mask, int n_frames, const FastAdjust a,
                                                         double* __restrict__ thresh, FastCut* __restrict__ cut) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double thr = a.fixed_thr >= 0 ? 0.0 : thresh[c];
  auto load = [&](int f) -> int4 {
    return f < n_frames ? *reinterpret_cast<const int4*>(hist + ((size_t)f * a.n_cells + c) * 256 + 4 * lane)
                        : make_int4(0, 0, 0, 0);
  };
  int4 hv = load(0);
  for (int f = 0; f < n_frames; ++f) {
    const int4 nxt = load(f + 1);  // (independent of the threshold chain: in flight while this frame is decided)
    // suf_k = survivors with score >= 4 lane + k
    const int s3 = hv.w, s2 = hv.z + s3, s1 = hv.y + s2, s0 = hv.x + s1;
    int incl = s0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_down(incl, d);
      if (lane + d < 64) incl += o;
    }
    const int above = incl - s0;
    const int suf[4] = {s0 + above, s1 + above, s2 + above, s3 + above};
    auto count_at = [&](int b) -> int {  // survivors with score >= b (b uniform)
      if (b >= 256) return 0;
      const int k = b & 3;
      const int v = k == 0 ? suf[0] : k == 1 ? suf[1] : k == 2 ? suf[2] : suf[3];
      return __shfl(v, b >> 2);
    };
    int t, n;
    if (a.fixed_thr >= 0) {
      t = a.fixed_thr;
      n = count_at(t);
    } else {
      // VideoDynamicAdaptedFeatureDetector::detect (feature_adjuster.cpp:185-224) with DetectorAdjuster's tooFew / tooMany /
      // good (:102-136) in double, as orb_grid_detect restates it; cv::FAST clamps the threshold to [0, 255]
      int iter = a.max_iters;
      bool checked = false;
      do {
        t = min(max((int)thr, 0), 255);
        n = count_at(t);
        if (n < a.cell_min) {
          thr = thr * 0.7;
          if (thr < 2) thr = 2;
          if (n == 0 && !checked) {
            checked = true;
            if (!(has_mask[f] && mask_nz[(size_t)f * a.n_cells + c])) break;  // hasNonZero(mask): an absent mask has none
          }
        } else if (n > a.cell_max) {
          thr = thr * 1.3;
          if (thr > 10000) thr = 10000;
          break;
        } else {
          break;
        }
        --iter;
      } while (iter > 0 && thr > 2 && thr < 10000);
    }
    // keepStrongest(maxPerCell) (:247-255) with the oracle's tie rule: the N largest scores, ties in raster order
    FastCut o{t, INT32_MAX, n, t};
    const int N = a.max_per_cell;
    if (n > N) {
      o.n = N;
      if (N <= 0) {
        o.cut = 256; o.ties = 0; o.n = 0;
      } else {
        int best = -1;  // the largest score b >= t with count_at(b) >= N
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * lane + k >= t && suf[k] >= N) best = 4 * lane + k;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d));
        o.cut = best;
        o.ties = N - count_at(best + 1);
      }
    }
    if (lane == 0) cut[(size_t)f * a.n_cells + c] = o;
    hv = nxt;
  }
  if (lane == 0 && a.fixed_thr < 0) thresh[c] = thr;
}

// ------------------------------------------------------------------------------------------------
// select: one workgroup of four waves per frame
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fast_select_kernel(const FastGeom g, const uint64_t* __restrict__ keep,
                                                          const uint8_t* __restrict__ score, const FastCut* __restrict__ cut,
                                                          const float* __restrict__ depth, const FastSelect p,
                                                          FastKp* __restrict__ list, const FastFrameOut* __restrict__ outs,
                                                          int32_t* __restrict__ n_out) {
  __shared__ int cell_off[kFastMaxCells + 1];
  __shared__ int lhist[256];
  __shared__ int wave_cnt[4], wave_cnt2[4];
  __shared__ float zs[256];
  __shared__ int cut_s, cut_k;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n_cells = p.n_cells;
  FastKp* __restrict__ L = list + (size_t)f * p.list_cap;
  const FastCut* __restrict__ C = cut + (size_t)f * n_cells;
  lhist[tid] = 0;
  if (wv == 0) {  // the cells' first rows in the aggregate (aggregateKeypointsPerGridCell: row-major cell order)
    int tot;
    const int ex = wave_excl_scan(lane < n_cells ? C[lane].n : 0, lane, &tot);
    cell_off[lane] = ex;
    if (lane == 0) cell_off[kFastMaxCells] = tot;
  }
  __syncthreads();
  // 1. each cell's kept survivors in raster order (a wave per cell; lane = one keep word = 64 pixels of a row)
  for (int c = wv; c < n_cells; c += 4) {
    const FastCut ct = C[c];
    if (ct.n == 0) continue;
    const FastCellGeom ce = g.cell[c];
    const uint64_t* __restrict__ K = keep + (size_t)f * g.keep_words + ce.keep_off;
    const uint8_t* __restrict__ S = score + (size_t)f * g.score_bytes + ce.score_off;
    const int room = p.list_cap - cell_off[c];
    FastKp* __restrict__ out = L + cell_off[c];
    const int wpr = ce.tiles_x, total = ce.h * wpr;
    int eq_seen = 0, emitted = 0;
    for (int i0 = 0; i0 < total && emitted < ct.n; i0 += 64) {
      const int i = i0 + lane;
      const uint64_t m = i < total ? K[i] : 0ull;
      const int y = i / wpr, xb = (i - y * wpr) * 64;
      const uint8_t* __restrict__ Srow = S + (size_t)y * ce.w + xb;
      int gt = 0, eq = 0;
      for (uint64_t b = m; b; b &= b - 1) {
        const int s = Srow[__builtin_ctzll(b)];
        gt += s > ct.cut;
        eq += s == ct.cut;
      }
      int eq_tot, sel_tot;
      const int eq0 = eq_seen + wave_excl_scan(eq, lane, &eq_tot);   // rank of this lane's first tie
      const int sel = gt + min(max(ct.ties - eq0, 0), eq);
      int pos = emitted + wave_excl_scan(sel, lane, &sel_tot);
      int r = eq0;
      for (uint64_t b = m; b; b &= b - 1) {
        const int x = __builtin_ctzll(b);
        const int s = Srow[x];
        const bool take = s > ct.cut || (s == ct.cut && r < ct.ties);
        r += s == ct.cut;
        if (take) {
          if (pos < room) out[pos] = FastKp{(uint16_t)(ce.x0 + xb + x), (uint16_t)(ce.y0 + y), (uint16_t)s, 0, 0.f};
          ++pos;
        }
      }
      eq_seen += eq_tot;
      emitted += sel_tot;
    }
  }
  __syncthreads();
  const int n0 = min(cell_off[kFastMaxCells], p.list_cap);
  if (!p.describe) {
    if (tid == 0) n_out[f] = n0;
    return;
  }
  const int rows = p.rows, cols = p.cols;
  const float* __restrict__ D = depth + (size_t)f * rows * cols;
  // 2. removeDepthless (node.cpp:186; node.cpp:82 under "use_feature_min_depth": the neighbourhood minimum over the keypoint's
  //    size, 7), in place and in order -- every read of a 256-keypoint chunk happens before the barrier, every write after it
  //    (to a position <= the one read); the survivors' score histogram for the max_keypoints cut
  int n1 = 0;
  for (int c0 = 0; c0 < n0; c0 += 256) {
    const int i = c0 + tid;
    if (p.min_depth) {
      const int k0 = c0 + wv * 64, kn = min(64, n0 - k0);
      for (int k = 0; k < kn; ++k) {
        const FastKp q = L[k0 + k];
        const float z = min_depth_in_neighbourhood((float)q.x, (float)q.y, 7.f, D, rows, cols, lane);
        if (lane == 0) zs[wv * 64 + k] = z;
      }
      __syncthreads();
    }
    FastKp q{};
    bool k = false;
    if (i < n0) {
      q = L[i];
      q.z = p.min_depth ? zs[tid] : D[(size_t)q.y * cols + q.x];   // depth(round(y), round(x)) of an integer position
      k = !__builtin_isnan(q.z);
    }
    const uint64_t m = __ballot(k);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) wave_cnt[wv] = (int)__popcll(m);
    __syncthreads();
    int off = n1;
    for (int v = 0; v < wv; ++v) off += wave_cnt[v];
    if (k) {
      L[off + rank] = q;
      atomicAdd(&lhist[q.s], 1);
    }
    n1 += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  // 3. retainBest(max_keypoints) + resize (node.cpp:188-191): the max_keypoints largest scores, ties in list order -- a cut
  //    score and the number of its ties to take
  if (tid < 64) {
    int cs = -1, ck = INT32_MAX;
    if (n1 > p.max_kp) {
      const int4 hv = make_int4(lhist[4 * lane], lhist[4 * lane + 1], lhist[4 * lane + 2], lhist[4 * lane + 3]);
      const int s3 = hv.w, s2 = hv.z + s3, s1 = hv.y + s2, s0 = hv.x + s1;
      int incl = s0;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(incl, d);
        if (lane + d < 64) incl += o;
      }
      const int above = incl - s0;
      const int suf[4] = {s0 + above, s1 + above, s2 + above, s3 + above};
      int best = -1;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (suf[k] >= p.max_kp) best = 4 * lane + k;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d));
      const int nb = best + 1;   // survivors with score >= best + 1
      const int v = (nb & 3) == 0 ? suf[0] : (nb & 3) == 1 ? suf[1] : (nb & 3) == 2 ? suf[2] : suf[3];
      const int above_best = nb >= 256 ? 0 : __shfl(v, nb >> 2);
      cs = best;
      ck = p.max_kp - above_best;
    }
    if (tid == 0) { cut_s = cs; cut_k = ck; }
  }
  __syncthreads();
  const int cs = cut_s, ck = cut_k;
  // 4. ORB::compute's runByImageBorder(31) (orb.cpp; one level: no regrouping), then projectTo3D (node.cpp:900-965) of the
  //    final list -- written where the caller wants it; the list itself stays for the descriptor launch
  const FastFrameOut o = outs[f];
  int eq_seen = 0, n2 = 0;
  for (int c0 = 0; c0 < n1; c0 += 256) {
    const int i = c0 + tid;
    const bool in = i < n1;
    FastKp q{};
    if (in) q = L[i];
    const bool eq = in && (int)q.s == cs;
    const uint64_t me = __ballot(eq);
    const int rank_e = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(me >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)me, 0u));
    if (lane == 0) wave_cnt[wv] = (int)__popcll(me);
    __syncthreads();
    int r = eq_seen + rank_e;
    for (int v = 0; v < wv; ++v) r += wave_cnt[v];
    const bool sel = in && ((int)q.s > cs || (eq && r < ck));
    const bool k = sel && q.x >= 31 && q.x < cols - 31 && q.y >= 31 && q.y < rows - 31;
    const uint64_t mk = __ballot(k);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
    if (lane == 0) wave_cnt2[wv] = (int)__popcll(mk);
    __syncthreads();
    int pos = n2 + rank;
    for (int v = 0; v < wv; ++v) pos += wave_cnt2[v];
    if (k) {
      L[pos] = q;
      const float4 xyz = back_project((float)q.x, (float)q.y, scaled_depth(q.z, p.depth_scaling), p.cx, p.cy, p.fxinv, p.fyinv);
      if (o.node_xyz) o.node_xyz[pos] = xyz;
      if (o.out_xyz) o.out_xyz[pos] = xyz;
      if (o.out_kp) o.out_kp[pos] = FastKpOut{(float)q.x, (float)q.y, 7.f, -1.f, (float)q.s, 0};
    }
    eq_seen += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    n2 += wave_cnt2[0] + wave_cnt2[1] + wave_cnt2[2] + wave_cnt2[3];
    __syncthreads();
  }
  if (tid == 0) n_out[f] = n2;
}

// ------------------------------------------------------------------------------------------------
// rBRIEF (computeOrbDescriptors, WTA_K = 2) of level-0 keypoints at angle -1 degree: orb_brief_kernel's sampling for a
// frame-indexed list (brief_level0_dword, fast_device.h); a wave per keypoint, the 32 bytes leave as eight dwords
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fast_brief_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ blur,
                                                         uint32_t plane, int rows, int cols, const FastKp* __restrict__ list,
                                                         int list_cap, const int32_t* __restrict__ n_out,
                                                         const FastFrameOut* __restrict__ outs, const int8_t* __restrict__ pattern,
                                                         float a, float b) {
  const int f = blockIdx.y;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_out[f]) return;
  const int lane = threadIdx.x & 63;
  const FastKp kp = list[(size_t)f * list_cap + k];
  const uint32_t word = brief_level0_dword(gray + (size_t)f * plane, blur + (size_t)f * plane, rows, cols, (int)kp.x, (int)kp.y,
                                           a, b, pattern, lane);
  const int d = lane & 7;
  if (lane < 8) {
    const FastFrameOut o = outs[f];
    if (o.node_desc) o.node_desc[(size_t)k * 8 + d] = word;
    if (o.out_desc) reinterpret_cast<uint32_t*>(o.out_desc)[(size_t)k * 8 + d] = word;
  }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
void launch_fast_pass(const uint8_t* gray, const uint8_t* mask, const int32_t* has_mask, const FastGeom& g, int n_frames,
                      int floor_thr, uint64_t* keep, uint8_t* score, int32_t* hist, int32_t* mask_nz, hipStream_t s) {
  if (n_frames > 0 && g.tiles_per_frame > 0)
    hipLaunchKernelGGL(fast_pass_kernel, dim3(g.tiles_per_frame, n_frames), dim3(256), 0, s, gray, mask, has_mask, g, floor_thr,
                       keep, score, hist, mask_nz);
}
void launch_fast_adjust(const int32_t* hist, const int32_t* mask_nz, const int32_t* has_mask, int n_frames,
                        const FastAdjust& a, double* thresh, FastCut* cut, hipStream_t s) {
  if (n_frames > 0)
    hipLaunchKernelGGL(fast_adjust_kernel, dim3(a.n_cells), dim3(64), 0, s, hist, mask_nz, has_mask, n_frames, a, thresh, cut);
}
void launch_fast_select(const FastGeom& g, int n_frames, const uint64_t* keep, const uint8_t* score, const FastCut* cut,
                        const float* depth, const FastSelect& p, FastKp* list, const FastFrameOut* outs, int32_t* n_out,
                        hipStream_t s) {
  if (n_frames > 0)
    hipLaunchKernelGGL(fast_select_kernel, dim3(n_frames), dim3(256), 0, s, g, keep, score, cut, depth, p, list, outs, n_out);
}
void launch_fast_brief(const uint8_t* gray, const uint8_t* blur, uint32_t plane, int rows, int cols, int n_frames, int max_kp,
                       const FastKp* list, int list_cap, const int32_t* n_out, const FastFrameOut* outs,
                       const int8_t* pattern, float cos_a, float sin_a, hipStream_t s) {
  if (n_frames > 0 && max_kp > 0)
    hipLaunchKernelGGL(fast_brief_kernel, dim3((max_kp + 3) / 4, n_frames), dim3(256), 0, s, gray, blur, plane, rows, cols, list,
                       list_cap, n_out, outs, pattern, cos_a, sin_a);
}

}  // namespace rgbdfe
