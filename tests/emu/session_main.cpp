// tests/emu/session_main.cpp -- TEST INFRASTRUCTURE ONLY: csrc/session_format.h as a stand-alone host program
// (tests/test_session_format_host.py builds it with the address and undefined-behaviour sanitizers, together with
// csrc/candidates.cpp).  Per file named on the command line, one line:
//   ok <nodes> <rows> <clouds> <graph: 0 | 1> <slam: 0 | 1>     the validator accepted it; a GRPH / SLAM chunk was also turned
//                                                               into a graph / a machine and serialised back to its bytes
//   bad <cause>                                                 the validator refused it
// The file's bytes are handed over in a heap block of exactly their length, so that a read past the end is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "session_format.h"

namespace sf = rgbdfe_session;

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> bytes;
    if (!read_file(argv[a], bytes)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes.size() ? bytes.size() : 1]);
    if (!bytes.empty()) memcpy(exact.get(), bytes.data(), bytes.size());
    sf::SessionView v;
    const std::string err = sf::session_parse(exact.get(), bytes.size(), v);
    if (!err.empty()) { printf("bad %s\n", err.c_str()); continue; }
    uint64_t rows = 0, sum = 0;
    for (int k = 0; k < 3; ++k) {   // every byte the views name is read
      const sf::NodeGroup& g = v.group[k];
      rows += g.total;
      const uint64_t widths[4] = {k == 0 ? 32ull : 512ull, 16, 8, 1};
      const uint8_t* arrays[4] = {g.desc, g.xyz, g.kp, g.stats};
      for (int i = 0; i < 4; ++i)
        for (uint64_t b = 0; b < g.total * widths[i]; ++b) sum += arrays[i][b];
    }
    for (const sf::CloudView& c : v.clouds)
      for (uint64_t b = 0; b < 16ull * (uint64_t)c.ch * (uint64_t)c.cw; ++b) sum += c.points[b];
    if (v.chunk[sf::kGrph].present) {
      sf::GraphImage img;
      rgbdfe_pose_graph g;
      std::vector<uint8_t> back;
      std::string e = sf::graph_parse(v.chunk[sf::kGrph].p, v.chunk[sf::kGrph].n, img);
      if (e.empty()) { sf::graph_commit(g, img); sf::graph_serialize(g, back, e); }
      if (!e.empty() || back.size() != v.chunk[sf::kGrph].n || memcmp(back.data(), v.chunk[sf::kGrph].p, back.size()) != 0) {
        printf("bad the GRPH chunk does not serialise back to its bytes\n");
        continue;
      }
    }
    if (v.chunk[sf::kSlam].present) {
      sf::SlamImage img;
      rgbdfe_slam_machine::Machine m;
      std::vector<uint8_t> back;
      const std::string e = sf::slam_parse(v.chunk[sf::kSlam].p, v.chunk[sf::kSlam].n, img);
      if (e.empty()) { m.prm = img.prm; sf::slam_commit(m, img); sf::slam_serialize(m, back); }
      if (!e.empty() || back.size() != v.chunk[sf::kSlam].n || memcmp(back.data(), v.chunk[sf::kSlam].p, back.size()) != 0) {
        printf("bad the SLAM chunk does not serialise back to its bytes\n");
        continue;
      }
    }
    printf("ok %zu %llu %zu %d %d\n", v.ids.size(), (unsigned long long)rows, v.clouds.size(), v.chunk[sf::kGrph].present ? 1 : 0,
           v.chunk[sf::kSlam].present ? 1 : 0);
    if (sum == 0xFFFFFFFFFFFFFFFFull) printf("\n");   // (keeps the byte walk alive)
  }
  return 0;
}
