// header_host_main.cpp -- TEST INFRASTRUCTURE: the parts of include/rgbdfe.hpp that need no device, as a stand-alone program
// for tests/test_cpp_header_host.py (built plain and with the address and undefined-behaviour sanitizers; it links nothing
// of librgbdfe.so).
//   header_host_main inverse <in> <out>   n x 16 float32 column-major matrices -> inverse4 of each, n x 16 float32
//   header_host_main records              toMatchingResult on hand-made rgbdfe_match_result records, one JSON line each
//   header_host_main display              displayTypeFromParameter of the four parameter values, one line
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "rgbdfe.hpp"

using namespace rgbdslam;

static void printResult(const char* name, const MatchingResult& mr) {
  std::printf("{\"name\": \"%s\", \"id1\": %d, \"id2\": %d, \"rmse\": %.9g, \"info\": %.17g, \"all\": [", name, mr.edge.id1, mr.edge.id2,
              mr.rmse, mr.edge.informationScale);
  for (size_t i = 0; i < mr.all_matches.size(); ++i)
    std::printf("%s[%d, %d, %d, %.9g]", i ? ", " : "", mr.all_matches[i].queryIdx, mr.all_matches[i].trainIdx, mr.all_matches[i].imgIdx,
                mr.all_matches[i].distance);
  std::printf("], \"inliers\": [");
  for (size_t i = 0; i < mr.inlier_matches.size(); ++i)
    std::printf("%s[%d, %d, %.9g]", i ? ", " : "", mr.inlier_matches[i].queryIdx, mr.inlier_matches[i].trainIdx,
                mr.inlier_matches[i].distance);
  std::printf("], \"ransac\": [");
  for (int i = 0; i < 16; ++i) std::printf("%s%.9g", i ? ", " : "", mr.ransac_trafo[i]);
  std::printf("], \"final\": [");
  for (int i = 0; i < 16; ++i) std::printf("%s%.9g", i ? ", " : "", mr.final_trafo[i]);
  std::printf("], \"icp\": [");
  for (int i = 0; i < 16; ++i) std::printf("%s%.9g", i ? ", " : "", mr.icp_trafo[i]);
  std::printf("], \"edge\": [");
  for (int i = 0; i < 16; ++i) std::printf("%s%.17g", i ? ", " : "", mr.edge.transform[i]);
  std::printf("], \"points\": [%u, %u, %u, %u]}\n", mr.inlier_points, mr.outlier_points, mr.occluded_points, mr.all_points);
}

static int records() {
  std::unique_ptr<rgbdfe_match_result> r(new rgbdfe_match_result);
  // no edge: three matches, the first and the last inliers; the transform is kept, the edge stays as constructed
  std::memset(r.get(), 0, sizeof(*r));
  r->id1 = r->id2 = -1;
  r->n_all = 3;
  r->n_inl = 2;
  r->rmse = 0.5f;
  for (int i = 0; i < 16; ++i) r->trafo[i] = (float)(i + 1);
  r->info_scale = 77.0;
  const uint16_t q[3] = {5, 6, 7}, t[3] = {1, 2, 3};
  const uint8_t hd[3] = {0, 128, 255};
  for (int m = 0; m < 3; ++m) { r->all_q[m] = q[m]; r->all_t[m] = t[m]; r->all_hd[m] = hd[m]; }
  r->inlier_mask[0] = 0x5ull;
  printResult("no edge", toMatchingResult(*r));
  // an edge: 70 matches, inliers either side of the first mask word's end
  std::memset(r.get(), 0, sizeof(*r));
  r->id1 = 3;
  r->id2 = 9;
  r->n_all = 70;
  r->n_inl = 3;
  r->rmse = 0.25f;
  for (int i = 0; i < 16; ++i) r->trafo[i] = 0.1f * (float)(i + 1);
  r->info_scale = 123.5;
  for (int m = 0; m < 70; ++m) { r->all_q[m] = (uint16_t)(1000 + m); r->all_t[m] = (uint16_t)(2000 - m); r->all_hd[m] = (uint8_t)m; }
  r->inlier_mask[0] = 1ull << 63;
  r->inlier_mask[1] = 0x21ull;
  printResult("edge", toMatchingResult(*r));
  // the float-distance overload: the distances given replace hd / 256
  std::vector<float> dist(70);
  for (int m = 0; m < 70; ++m) dist[(size_t)m] = 0.5f + 0.25f * (float)m;
  printResult("float distances", toMatchingResult(*r, dist.data()));
  // n_all at RGBDFE_MAX_MATCHES, every match an inlier: the last bit of the last mask word is read, nothing behind it
  std::memset(r.get(), 0, sizeof(*r));
  r->id1 = 0;
  r->id2 = 1;
  r->n_all = r->n_inl = RGBDFE_MAX_MATCHES;
  for (int m = 0; m < RGBDFE_MAX_MATCHES; ++m) { r->all_q[m] = (uint16_t)m; r->all_t[m] = (uint16_t)(65535 - m); r->all_hd[m] = (uint8_t)(m & 255); }
  for (int w = 0; w < RGBDFE_MASK_WORDS; ++w) r->inlier_mask[w] = ~0ull;
  printResult("full", toMatchingResult(*r));
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "inverse" && argc == 4) {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::perror("open"); return 2; }
    std::vector<std::array<float, 16>> in;
    std::array<float, 16> T;
    while (std::fread(T.data(), 4, 16, f) == 16) in.push_back(T);
    std::fclose(f);
    std::FILE* g = std::fopen(argv[3], "wb");
    if (!g) { std::perror("open"); return 2; }
    for (const std::array<float, 16>& m : in) {
      const std::array<float, 16> inv = inverse4(m);
      if (std::fwrite(inv.data(), 4, 16, g) != 16) return 2;
    }
    return std::fclose(g) == 0 ? 0 : 2;
  }
  if (mode == "records") return records();
  if (mode == "display") {
    std::printf("%d %d %d %d\n", displayTypeFromParameter("POINTS"), displayTypeFromParameter("TRIANGLES"),
                displayTypeFromParameter("TRIANGLE_STRIP"), displayTypeFromParameter("anything"));
    return 0;
  }
  std::fprintf(stderr, "usage: header_host_main inverse <in> <out> | records | display\n");
  return 2;
}
