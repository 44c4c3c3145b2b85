// orb_replay.h -- the host half of the grid detector, each of the reference's rules once: the adjuster step of
// VideoDynamicAdaptedFeatureDetector::detect (feature_adjuster.cpp:185-224), the per-level selections of orb.cpp
// computeKeyPoints over a pass's scored corners, the cell merge of VideoGridAdaptedFeatureDetector::detect (:247-317), the
// replay of a covered super-frame from counts, and Node::Node's removeDepthless / retainBest / depth look-ups
// (node.cpp:67-97, :186-191, :942).  Pure host code without a HIP runtime call: orb_host.hip and api_detect.hip drive it
// with device passes, tests/emu/orb_replay_main.cpp with planted ones.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "orb_internal.h"  // RawKp

namespace rgbdfe {

constexpr int kOrbLevels = 8;            // ORB nlevels
constexpr int kDetectFeatures = 10000;   // ORB::create(10000, 1.2, 8, 15, ...)   feature_adjuster.cpp:94

struct KpOut {  // cv::KeyPoint fields in use
  float x, y, size, angle, response;
  int octave;
};
struct GridCell { int x0, y0, w, h; };
// the read-back of one detection pass: per-image counts, their prefix, the scored corners ((cell, level) image c * 8 + l)
struct PassView { const int* totals = nullptr; const int* base = nullptr; const RawKp* raw = nullptr; };
// what the host half knows of a detector: cells per frame, the adjuster's bounds, the (frame, cell) rectangles and their
// hasNonZero(sub_mask) flags
struct GridDetector {
  int pc = 0, cell_min = 0, cell_max = 0, max_total = 0, adjuster_iters = 0;
  const GridCell* cells = nullptr;
  const char* mask_nonzero = nullptr;
};

inline double orb_now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline int cv_round_f(float v) { return (int)lrintf(v); }

inline void level_geometry(int cols, int rows, int nlevels, float* scale, int* lw, int* lh) {
  const double scaleFactor = (double)1.2f;
  for (int l = 0; l < nlevels; ++l) {
    scale[l] = (float)std::pow(scaleFactor, (double)l);
    lw[l] = cv_round_f((float)cols / scale[l]);
    lh[l] = cv_round_f((float)rows / scale[l]);
  }
}

inline void per_level_caps(int* per_level) {  // nfeaturesPerLevel (orb.cpp computeKeyPoints)
  const float factor = (float)(1.0 / (double)1.2f);
  float nd = kDetectFeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)kOrbLevels));
  int sum = 0;
  for (int l = 0; l < kOrbLevels - 1; ++l) { per_level[l] = cv_round_f(nd); sum += per_level[l]; nd *= factor; }
  per_level[kOrbLevels - 1] = std::max(kDetectFeatures - sum, 0);
}

struct KP {  // a corner inside computeKeyPoints
  float x, y, size, angle, response;
  int octave;
  float score;  // FAST score (first retainBest)
};

// KeyPointsFilter::retainBest: keep everything >= the n-th largest response; survivors keep their order
template <typename F>
void retain_best(std::vector<KP>& v, int n_points, F key) {
  if (n_points < 0 || (int)v.size() <= n_points) return;
  if (n_points == 0) { v.clear(); return; }
  static thread_local std::vector<float> r;  // scratch: 144 selections per detection pass
  r.resize(v.size());
  for (size_t i = 0; i < v.size(); ++i) r[i] = key(v[i]);
  std::nth_element(r.begin(), r.begin() + (n_points - 1), r.end(), [](float a, float b) { return a > b; });
  const float ambiguous = r[n_points - 1];
  size_t m = 0;
  for (size_t i = 0; i < v.size(); ++i)
    if (key(v[i]) >= ambiguous) v[m++] = v[i];
  v.resize(m);
}

// exactly the N first of the order (key descending, position ascending); survivors keep their order, and `side` (one value
// per element, optional) is compacted with them.  The N-th element of that order is the cut: a selection, not a sort.
template <typename T, typename F>
void strongest_n(std::vector<T>& v, int N, F key, std::vector<float>* side = nullptr) {
  if ((int)v.size() <= N) return;
  if (N <= 0) { v.clear(); if (side) side->clear(); return; }
  static thread_local std::vector<std::pair<float, int>> r;
  r.resize(v.size());
  for (size_t i = 0; i < v.size(); ++i) r[i] = std::make_pair(key(v[i]), (int)i);
  auto before = [](const std::pair<float, int>& a, const std::pair<float, int>& b) {
    return a.first > b.first || (a.first == b.first && a.second < b.second);
  };
  std::nth_element(r.begin(), r.begin() + (N - 1), r.end(), before);
  const std::pair<float, int> cut = r[(size_t)N - 1];
  size_t m = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    if (before(cut, std::make_pair(key(v[i]), (int)i))) continue;  // behind the cut
    if (side) (*side)[m] = (*side)[i];
    v[m++] = v[i];
  }
  v.resize(m);
  if (side) side->resize(m);
}
inline void keep_strongest(std::vector<KpOut>& v, int N) {  // keepStrongest(N) (feature_adjuster.cpp:247-255)
  strongest_n(v, N, [](const KpOut& k) { return std::fabs(k.response); });
}

// One iteration of VideoDynamicAdaptedFeatureDetector::detect (feature_adjuster.cpp:185-224) for a cell whose detection at
// static_cast<int>(thresh) has found `found` keypoints: moves the threshold and says whether the cell detects again.
inline bool adjust_cell(double& thresh, int found, int& iter_left, bool& checked, bool mask_nonzero, int cell_min, int cell_max) {
  if (found < cell_min) {
    thresh *= 0.7;                       // tooFew (:131-136)
    if (thresh < 2) thresh = 2;
    if (found == 0 && !checked) {
      checked = true;
      if (!mask_nonzero) return false;   // hasNonZero(mask) (:205-209)
    }
    iter_left--;
    return iter_left > 0 && (thresh > 2 && thresh < 10000);  // good() (:147-150)
  }
  if (found > cell_max) {
    thresh *= 1.3;                       // tooMany (:138-143)
    if (thresh > 10000) thresh = 10000;
  }
  return false;
}

// The keypoints of (frame, cell) c at threshold thr_c (level coordinates scaled to the cell image, cell-local) after orb.cpp
// computeKeyPoints' per-level selection: retainBest(2*featuresNum) by FAST score, Harris responses, retainBest(featuresNum).
// thr_c may be HIGHER than the threshold the pass ran the cell with: cv::FAST at threshold t keeps the pixels whose best arc
// has min |difference| m > t that are strict 3x3 maxima of the score m - 1 (non-corners count as 0).  A corner kept at t
// therefore has score >= t and beats every neighbour whose own score is < t whether that neighbour counts as a corner (floor
// f <= its score) or as 0; and a pixel that loses against a neighbour at the floor loses against the same neighbour at t when
// its own score is >= t (the neighbour's is larger still).  So { corners at t } = { corners at f with score >= t }, in the
// same raster order; Harris response and angle do not depend on the threshold.
inline void select_cell(const GridCell& cell, const PassView& pv, int c, int thr_c, std::vector<KpOut>& out) {
  int per_level[kOrbLevels];
  per_level_caps(per_level);
  out.clear();
  const int t = std::min(std::max(thr_c, 0), 255);  // the kernel's clamp
  float sc[kOrbLevels]; int lw[kOrbLevels], lh[kOrbLevels];
  level_geometry(cell.w, cell.h, kOrbLevels, sc, lw, lh);
  for (int l = 0; l < kOrbLevels; ++l) {
    const int img = c * kOrbLevels + l;
    static thread_local std::vector<KP> v;  // scratch: 72 (cell, level) images per pass
    v.clear();
    v.reserve((size_t)pv.totals[img]);
    for (int k = 0; k < pv.totals[img]; ++k) {
      const RawKp& r = pv.raw[(size_t)pv.base[img] + k];
      if ((int)r.score < t) continue;
      v.push_back(KP{(float)r.x, (float)r.y, 31 * sc[l], r.angle, r.harris, l, (float)r.score});
    }
    retain_best(v, 2 * per_level[l], [](const KP& k) { return k.score; });
    retain_best(v, per_level[l], [](const KP& k) { return k.response; });
    for (const KP& k : v) out.push_back(KpOut{k.x * sc[l], k.y * sc[l], k.size, k.angle, k.response, l});
  }
}

// How many keypoints select_cell(c, t) would return, without building them: per level the corners with score >= t -- exact as
// long as no level reaches its retainBest cap (n <= nfeaturesPerLevel: neither retainBest(2n) nor retainBest(n) cuts, ties
// included); *capped is set otherwise and the caller runs the selection itself.
inline int count_cell(const PassView& pv, int c, int thr_c, bool* capped) {
  int per_level[kOrbLevels];
  per_level_caps(per_level);
  const int t = std::min(std::max(thr_c, 0), 255);
  int found = 0;
  for (int l = 0; l < kOrbLevels; ++l) {
    const int img = c * kOrbLevels + l;
    const RawKp* r = pv.raw + pv.base[img];
    int n = 0;
    for (int k = 0; k < pv.totals[img]; ++k) n += (int)r[k].score >= t ? 1 : 0;
    if (n > per_level[l]) { *capped = true; return 0; }
    found += n;
  }
  return found;
}

// A cell's share of VideoGridAdaptedFeatureDetector::detect's output: keepStrongest(maxPerCell) (:247-255, :292) of the
// cell's keypoints (cut in place), cell offsets added, appended to the frame's aggregate (aggregateKeypointsPerGridCell,
// :259-282)
inline void merge_cell(std::vector<KpOut>& cell_kps, const GridCell& cell, int max_per_cell, std::vector<KpOut>& kps) {
  keep_strongest(cell_kps, max_per_cell);
  for (const KpOut& k : cell_kps) kps.push_back(KpOut{k.x + cell.x0, k.y + cell.y0, k.size, k.angle, k.response, k.octave});
}

// The adjuster over the frames [0, nf) of a super-frame whose one pass at `floors` covers every frame, from counts alone: per
// grid cell the chain "threshold -> keypoints found -> again, or on to the next frame" needs `found` only (count_cell; a
// level at its retainBest cap falls back to the real selection), and the chains of the grid's cells do not interact.
// thr_final[c] = the threshold of the LAST detection of (frame, cell) c, the one whose keypoints the reference keeps.
// Returns 0 -- thresh untouched -- when a threshold falls below its floor: the pass does not hold that detection's corners.
inline int replay_counts(const GridDetector& g, int nf, const int* floors, const PassView& pv, double* thresh,
                         std::vector<int>& thr_final) {
  thr_final.assign((size_t)nf * g.pc, 0);
  std::vector<double> th_end((size_t)g.pc);
  std::vector<KpOut> scratch;
  for (int c9 = 0; c9 < g.pc; ++c9) {
    double th = thresh[c9];
    for (int f = 0; f < nf; ++f) {
      const int c = f * g.pc + c9;
      int iter_left = g.adjuster_iters;
      bool checked = false, again = true;
      while (again) {
        const int t = (int)th;  // static_cast<int>(thresh_)
        if (t < floors[c]) return 0;
        thr_final[(size_t)c] = t;
        bool capped = false;
        int found = count_cell(pv, c, t, &capped);
        if (capped) { select_cell(g.cells[c], pv, c, t, scratch); found = (int)scratch.size(); }
        again = adjust_cell(th, found, iter_left, checked, g.mask_nonzero[c] != 0, g.cell_min, g.cell_max);
      }
    }
    th_end[(size_t)c9] = th;
  }
  for (int c9 = 0; c9 < g.pc; ++c9) thresh[c9] = th_end[(size_t)c9];
  return 1;
}

// VideoGridAdaptedFeatureDetector::detect's output for one frame of a super-frame, given each cell's final threshold
// (replay_counts): select_cell at that threshold, then the merge.  Reads the pass view only: runs on any thread.
inline void select_frame(const GridDetector& g, const PassView& pv, int frame, const int* thr_final, std::vector<KpOut>& kps) {
  kps.clear();
  std::vector<KpOut> cell;
  for (int c = frame * g.pc; c < (frame + 1) * g.pc; ++c) {
    select_cell(g.cells[c], pv, c, thr_final[c], cell);
    merge_cell(cell, g.cells[c], g.max_total / g.pc, kps);
  }
}

// what the sequential loop below knows of the device passes read back so far: the latest one's view, the (frame, cell)
// detectors it ran and the thresholds it ran them at
struct PassCover {
  PassView pv;
  std::vector<char> covered;
  std::vector<int> floors;
};

// VideoGridAdaptedFeatureDetector::detect (feature_adjuster.cpp:286-317) for the frames [0, nf) IN ORDER: frame f + 1 starts
// from the per-cell thresholds frame f leaves behind.  A cell detects from the corners of the latest pass while that pass
// covers it at or below the cell's threshold (select_cell); otherwise pass(f, active, cover) -- active: which cells of frame
// f are still detecting -- runs another device pass over frame f onwards, updates `cover` and returns 0, or an error that
// ends the loop.  Results do not depend on which passes ran at which floors.  select_us (optional): the selections' time.
template <typename Pass>
int detect_frames(const GridDetector& g, int nf, double* thresh, PassCover& cover, Pass&& pass,
                  std::vector<std::vector<KpOut>>& kps_per_frame, double* select_us = nullptr) {
  struct CellRun { int iter_left; bool checked, active; };
  std::vector<std::vector<KpOut>> cellkp((size_t)g.pc);
  std::vector<CellRun> run((size_t)g.pc);
  std::vector<char> active((size_t)g.pc);
  kps_per_frame.assign((size_t)nf, std::vector<KpOut>());
  for (int f = 0; f < nf; ++f) {
    for (CellRun& r : run) r = CellRun{g.adjuster_iters, false, true};
    for (bool any = true; any;) {
      bool need_pass = false;
      for (int c9 = 0; c9 < g.pc; ++c9) {
        const int c = f * g.pc + c9;
        active[(size_t)c9] = run[(size_t)c9].active;
        if (run[(size_t)c9].active && (!cover.covered[(size_t)c] || (int)thresh[c9] < cover.floors[(size_t)c])) need_pass = true;
      }
      if (need_pass) {
        const int rc = pass(f, active, cover);
        if (rc != 0) return rc;
      }
      const double t0 = select_us ? orb_now_us() : 0;
      for (int c9 = 0; c9 < g.pc; ++c9)
        if (run[(size_t)c9].active)
          select_cell(g.cells[f * g.pc + c9], cover.pv, f * g.pc + c9, (int)thresh[c9], cellkp[(size_t)c9]);  // static_cast<int>(thresh_)
      if (select_us) *select_us += orb_now_us() - t0;
      any = false;
      for (int c9 = 0; c9 < g.pc; ++c9) {
        CellRun& r = run[(size_t)c9];
        if (!r.active) continue;
        r.active = adjust_cell(thresh[c9], (int)cellkp[(size_t)c9].size(), r.iter_left, r.checked,
                               g.mask_nonzero[f * g.pc + c9] != 0, g.cell_min, g.cell_max);
        any |= r.active;
      }
    }
    for (int c9 = 0; c9 < g.pc; ++c9)
      merge_cell(cellkp[(size_t)c9], g.cells[f * g.pc + c9], g.max_total / g.pc, kps_per_frame[(size_t)f]);
  }
  return 0;
}

// hasNonZero(sub_mask) per cell (feature_adjuster.cpp:175-183); nonzero(cell) answers for one rectangle
inline bool mask_nonzero(const uint8_t* mask, int cols, const GridCell& ce) {
  for (int y = 0; y < ce.h; ++y) {
    const uint8_t* r = mask + (size_t)(ce.y0 + y) * cols + ce.x0;
    for (int x = 0; x < ce.w; ++x)
      if (r[x]) return true;
  }
  return false;
}
template <typename NonZero>
void cell_mask_flags(const GridCell* cells, int n, char* flags, NonZero nonzero) {
  for (int c = 0; c < n; ++c) flags[c] = nonzero(cells[c]) ? 1 : 0;
}

// the depth pixel of a keypoint: depth.at<float>(round(y), round(x)), clamped as node.cpp:88-91 / :942 clamp it
inline void depth_pixel(const KpOut& k, int rows, int cols, int& r, int& c) {
  r = (int)roundf(k.y); c = (int)roundf(k.x);
  r = r >= rows ? rows - 1 : r;
  c = c >= cols ? cols - 1 : c;
}

// removeDepthless (node.cpp:67-97, :186) -- zmin given: with each keypoint's neighbourhood depth (:82), compacted alongside;
// otherwise with depth_px(r, c) of its pixel -- then retainBest(max_kp) + resize (:188-191): the max_kp first of the order
// (response descending, position ascending), in their original order
template <typename DepthPx>
void remove_depthless_and_cut(std::vector<KpOut>& kps, std::vector<float>* zmin, DepthPx depth_px, int rows, int cols, int max_kp) {
  size_t m = 0;
  for (size_t i = 0; i < kps.size(); ++i) {
    const KpOut k = kps[i];
    if (k.x >= (float)cols || k.x < 0 || k.y >= (float)rows || k.y < 0 || std::isnan(k.x) || std::isnan(k.y)) continue;
    if (zmin) {
      if (std::isnan((*zmin)[i])) continue;
      (*zmin)[m] = (*zmin)[i];
    } else {
      int r, c;
      depth_pixel(k, rows, cols, r, c);
      if (std::isnan(depth_px(r, c))) continue;
    }
    kps[m++] = k;
  }
  kps.resize(m);
  if (zmin) zmin->resize(m);
  strongest_n(kps, max_kp, [](const KpOut& k) { return k.response; }, zmin);
}

// projectTo3D's inputs for the n keypoints that cv::ORB::compute kept (kps; order[i] = keypoint i's position in the list
// remove_depthless_and_cut left): xyz_in = n (x, y) pairs, then n depths -- depth.at<float>(round(y), round(x)) (node.cpp:942)
// or, zmin given, the neighbourhood depth removeDepthless saw (:940-941)
template <typename DepthPx>
void depth_lookups(const std::vector<KpOut>& kps, const std::vector<float>* zmin, const std::vector<int>& order, DepthPx depth_px,
                   int rows, int cols, float* xyz_in) {
  const size_t n = kps.size();
  for (size_t i = 0; i < n; ++i) {
    xyz_in[2 * i] = kps[i].x;
    xyz_in[2 * i + 1] = kps[i].y;
    if (zmin) { xyz_in[2 * n + i] = (*zmin)[(size_t)order[i]]; continue; }
    int r, c;
    depth_pixel(kps[i], rows, cols, r, c);
    xyz_in[2 * n + i] = depth_px(r, c);
  }
}

}  // namespace rgbdfe
