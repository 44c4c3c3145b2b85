// tests/cpp/session_resume.cpp -- TEST INFRASTRUCTURE ONLY: rgbdslam::GraphManager::saveSession / loadSession and
// rgbdslam::FrontEnd::downloadNodes of include/rgbdfe.hpp (tests/test_gpu_session.py builds it with plain g++ against the
// header and librgbdfe.so): the frames of tests/cpp/slam_session.cpp's frames.bin through addNode, with the front end, the
// graph manager and the machine saved after `cut` frames, destroyed, created again and loaded.
//   session_resume frames.bin strategy optimizer_skip_step clear_non_keyframes predecessor_candidates neighbor_candidates
//                  min_sampled_candidates cut session_path
// Output: per frame "status id keyframe_added cleared_first optimized lm_iterations chi2(hex)", then "K" keyframes, "T" slots,
// "D" the rows and the byte sum of a read-back of every resident node in ascending id.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rgbdfe.hpp"

struct Run {
  rgbdslam::FrontEnd fe;
  rgbdslam::GraphManager gm;
  std::vector<std::unique_ptr<rgbdslam::Node>> nodes;
  Run(const rgbdfe_config& cfg, char** argv) : fe(cfg), gm(fe) {
    gm.setPoseRelativeTo(atoi(argv[2]));
    rgbdfe_slam_params& sp = gm.slamParams();
    sp.optimizer_skip_step = atoi(argv[3]);
    sp.clear_non_keyframes = atoi(argv[4]);
    sp.predecessor_candidates = atoi(argv[5]);
    sp.neighbor_candidates = atoi(argv[6]);
    sp.min_sampled_candidates = atoi(argv[7]);
  }
};

int main(int argc, char** argv) {
  if (argc != 10) { fprintf(stderr, "usage: session_resume frames.bin strategy skip clear pc nc sc cut session_path\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  const int32_t cut = atoi(argv[8]);
  rgbdfe_config cfg = rgbdslam::FrontEnd::defaultConfig();
  cfg.max_nodes = 24; cfg.max_keypoints = 130; cfg.max_pairs_per_batch = 16;
  std::unique_ptr<Run> run(new Run(cfg, argv));
  for (int32_t k = 0; k < n; ++k) {
    if (k == cut) {
      if (!run->gm.saveSession(argv[9])) { fprintf(stderr, "save: %s\n", rgbdfe_last_error(run->fe.get())); return 7; }
      run.reset();   // nodes, machine, graph and context go
      run.reset(new Run(cfg, argv));
      if (!run->gm.loadSession(argv[9])) { fprintf(stderr, "load: %s\n", rgbdfe_last_error(run->fe.get())); return 8; }
    }
    int32_t rows = 0, nsec = 0;
    int64_t sec = 0;
    if (fread(&rows, 4, 1, f) != 1 || fread(&sec, 8, 1, f) != 1 || fread(&nsec, 4, 1, f) != 1) return 2;
    std::vector<uint8_t> desc((size_t)rows * 32);
    std::vector<float> xyz((size_t)rows * 4);
    if (rows > 0 && (fread(desc.data(), 32, (size_t)rows, f) != (size_t)rows || fread(xyz.data(), 16, (size_t)rows, f) != (size_t)rows)) return 2;
    run->nodes.emplace_back(new rgbdslam::Node(run->fe, k, desc.data(), xyz.data(), rows));   // uploads into slot k
    rgbdfe_slam_step st;
    run->gm.addNode(run->nodes.back().get(), sec, nsec, &st);
    if (run->gm.lastAddNodeStatus() != RGBDFE_OK) return 6;
    uint64_t chi2;
    memcpy(&chi2, &st.chi2, 8);
    printf("%d %d %d %d %d %d %016" PRIx64 "\n", st.status, st.id, st.keyframe_added, st.cleared_first, st.optimized, st.lm_iterations, chi2);
  }
  fclose(f);
  printf("K");
  for (int32_t id : run->gm.keyframeIds()) printf(" %d", id);
  printf("\nT");
  for (int id = 0; run->gm.slotOf(id) >= -1; ++id) printf(" %d", run->gm.slotOf(id));
  printf("\nD");
  std::vector<int32_t> resident;
  for (int32_t id = 0; id < cfg.max_nodes; ++id)
    if (rgbdfe_node_count(run->fe.get(), id) >= 0) resident.push_back(id);
  const rgbdslam::FrontEnd::NodeRows rows = run->fe.downloadNodes(resident);
  uint64_t sum = 0;
  for (uint8_t b : rows.desc) sum += b;
  for (uint8_t b : rows.stats) sum += b;
  printf(" %zu %lld %" PRIu64 "\n", resident.size(), (long long)rows.row_offsets.back(), sum);
  return 0;
}
