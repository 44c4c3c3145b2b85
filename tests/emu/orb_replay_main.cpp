// tests/test_orb_replay_host.py: csrc/orb_replay.h -- the host half of the grid detector -- as a stand-alone program over
// planted detection passes, built with the address and undefined-behaviour sanitizers.
//
//   orb_replay_main replay CASE MASKS
//     CASE (text): pc nf cell_min cell_max max_total iters rows cols | pc thresholds | nf*pc floors | nf*pc cells (x0 y0 w h) |
//     per (frame, cell, level) image: n, then n corners (x y score harris-bits angle-bits).  MASKS: nf masks of rows x cols bytes.
//     Prints, once for replay_counts + select_frame and once for the sequential loop (detect_frames; a threshold below its
//     floor asks for a pass, which here lowers every floor to 0): "<name> done=<0|1> passes=<n>", the thresholds, and per
//     frame its keypoints (x y size angle response as bit patterns, octave).
//   orb_replay_main cut CASE DEPTH
//     CASE (text): rows cols max_kp use_zmin n | n keypoints (x-bits y-bits response-bits zmin-bits).  DEPTH: rows x cols floats.
//     Prints the input positions remove_depthless_and_cut keeps, then depth_lookups' depth (bit pattern) of each.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "orb_replay.h"

using namespace rgbdfe;

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static std::vector<char> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void print_run(const char* name, int done, int passes, const std::vector<double>& thresh,
                      const std::vector<std::vector<KpOut>>& frames) {
  printf("%s done=%d passes=%d\n", name, done, passes);
  for (double t : thresh) printf("%.17g ", t);
  printf("\n");
  for (const std::vector<KpOut>& kps : frames) {
    printf("%zu", kps.size());
    for (const KpOut& k : kps) printf(" %08x %08x %08x %08x %08x %d", bits(k.x), bits(k.y), bits(k.size), bits(k.angle), bits(k.response), k.octave);
    printf("\n");
  }
}

static int replay(const char* case_path, const char* mask_path) {
  std::ifstream in(case_path);
  GridDetector g;
  int nf = 0, rows = 0, cols = 0;
  in >> g.pc >> nf >> g.cell_min >> g.cell_max >> g.max_total >> g.adjuster_iters >> rows >> cols;
  const int n_cells = nf * g.pc;
  std::vector<double> thresh0((size_t)g.pc);
  for (double& t : thresh0) in >> t;
  std::vector<int> floors((size_t)n_cells);
  for (int& f : floors) in >> f;
  std::vector<GridCell> cells((size_t)n_cells);
  for (GridCell& c : cells) in >> c.x0 >> c.y0 >> c.w >> c.h;
  std::vector<int> totals((size_t)n_cells * kOrbLevels), base((size_t)n_cells * kOrbLevels);
  std::vector<RawKp> raw;
  for (size_t img = 0; img < totals.size(); ++img) {
    in >> totals[img];
    base[img] = (int)raw.size();
    for (int k = 0; k < totals[img]; ++k) {
      int x, y, score;
      uint32_t harris, angle;
      in >> x >> y >> score >> harris >> angle;
      raw.push_back(RawKp{(uint16_t)x, (uint16_t)y, (uint16_t)img, (uint16_t)score, from_bits(harris), from_bits(angle)});
    }
  }
  if (!in) { fprintf(stderr, "bad case file\n"); return 2; }
  const std::vector<char> masks = read_file(mask_path);
  if (masks.size() != (size_t)nf * rows * cols) { fprintf(stderr, "bad mask file\n"); return 2; }
  std::vector<char> flags((size_t)n_cells);
  for (int f = 0; f < nf; ++f) {
    const uint8_t* m = reinterpret_cast<const uint8_t*>(masks.data()) + (size_t)f * rows * cols;
    cell_mask_flags(cells.data() + (size_t)f * g.pc, g.pc, flags.data() + (size_t)f * g.pc,
                    [&](const GridCell& ce) { return mask_nonzero(m, cols, ce); });
  }
  g.cells = cells.data();
  g.mask_nonzero = flags.data();
  PassView pv;
  pv.totals = totals.data(); pv.base = base.data(); pv.raw = raw.data();

  {  // from counts, the selections afterwards
    std::vector<double> thresh = thresh0;
    std::vector<int> thr_final;
    const int done = replay_counts(g, nf, floors.data(), pv, thresh.data(), thr_final);
    std::vector<std::vector<KpOut>> frames((size_t)(done ? nf : 0));
    for (int f = 0; f < nf && done; ++f) select_frame(g, pv, f, thr_final.data(), frames[(size_t)f]);
    print_run("counts", done, 0, thresh, frames);
  }
  {  // the sequential loop, every frame covered by the one pass
    std::vector<double> thresh = thresh0;
    PassCover cover;
    cover.pv = pv;
    cover.covered.assign((size_t)n_cells, 1);
    cover.floors = floors;
    int passes = 0;
    auto pass = [&](int f, const std::vector<char>& active, PassCover& cv) -> int {
      bool any = false;
      for (char a : active) any |= a != 0;
      if (!any || f < 0 || f >= nf) return 7;   // never asked for without a cell that needs it
      ++passes;
      std::fill(cv.floors.begin(), cv.floors.end(), 0);   // the planted corners are those of floor 0 already
      return 0;
    };
    std::vector<std::vector<KpOut>> frames;
    const int rc = detect_frames(g, nf, thresh.data(), cover, pass, frames);
    if (rc != 0) { fprintf(stderr, "detect_frames: %d\n", rc); return 3; }
    print_run("loop", passes == 0, passes, thresh, frames);
  }
  return 0;
}

static int cut(const char* case_path, const char* depth_path) {
  std::ifstream in(case_path);
  int rows = 0, cols = 0, max_kp = 0, use_zmin = 0, n = 0;
  in >> rows >> cols >> max_kp >> use_zmin >> n;
  std::vector<KpOut> kps((size_t)n);
  std::vector<float> zmin((size_t)n);
  for (int i = 0; i < n; ++i) {
    uint32_t x, y, r, z;
    in >> x >> y >> r >> z;
    kps[(size_t)i] = KpOut{from_bits(x), from_bits(y), 31.f, 0.f, from_bits(r), i};   // octave: the input position
    zmin[(size_t)i] = from_bits(z);
  }
  if (!in) { fprintf(stderr, "bad case file\n"); return 2; }
  const std::vector<char> d = read_file(depth_path);
  if (d.size() != (size_t)rows * cols * 4) { fprintf(stderr, "bad depth file\n"); return 2; }
  const float* depth = reinterpret_cast<const float*>(d.data());
  auto depth_px = [&](int r, int c) { return depth[(size_t)r * cols + c]; };
  remove_depthless_and_cut(kps, use_zmin ? &zmin : nullptr, depth_px, rows, cols, max_kp);
  if (use_zmin && zmin.size() != kps.size()) { fprintf(stderr, "zmin not compacted\n"); return 3; }
  std::vector<int> order(kps.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::vector<float> xyz_in(kps.size() * 3 + 1);
  depth_lookups(kps, use_zmin ? &zmin : nullptr, order, depth_px, rows, cols, xyz_in.data());
  for (const KpOut& k : kps) printf("%d ", k.octave);
  printf("\n");
  for (size_t i = 0; i < kps.size(); ++i) printf("%08x ", bits(xyz_in[2 * kps.size() + i]));
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "replay")) return replay(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "cut")) return cut(argv[2], argv[3]);
  fprintf(stderr, "usage: orb_replay_main replay|cut CASE DATA\n");
  return 2;
}
