// tests/cpp/slam_session.cpp -- TEST INFRASTRUCTURE ONLY: rgbdslam::GraphManager::addNode of include/rgbdfe.hpp over a run of
// frames the test writes (tests/test_gpu_cpp_slam.py builds it with plain g++ against the header and librgbdfe.so and
// compares what it prints with the binding's step records, text for text).
//   slam_session frames.bin strategy optimizer_skip_step clear_non_keyframes predecessor_candidates neighbor_candidates
//                min_sampled_candidates
// frames.bin: int32 n, then per frame int32 rows, int64 sec, int32 nsec, rows x 32 descriptor bytes, rows x 4 floats.
// Output: one line per frame -- the step record without its times, as tests/slam_cases.step_line prints it -- then K
// keyframes, T slots, V valid_tf.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rgbdfe.hpp"

static void print_hex(const double* v, int n) {
  for (int k = 0; k < n; ++k) {
    uint64_t u;
    memcpy(&u, v + k, 8);
    printf("%s%016" PRIx64, k ? " " : "", u);
  }
}

int main(int argc, char** argv) {
  if (argc != 8) { fprintf(stderr, "usage: slam_session frames.bin strategy skip clear pc nc sc\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  rgbdfe_config cfg = rgbdslam::FrontEnd::defaultConfig();
  cfg.max_nodes = 24; cfg.max_keypoints = 130; cfg.max_pairs_per_batch = 16;
  rgbdslam::FrontEnd fe(cfg);
  rgbdslam::GraphManager gm(fe);
  if (!gm.setPoseRelativeTo(atoi(argv[2]))) return 3;
  rgbdfe_slam_params& sp = gm.slamParams();
  sp.optimizer_skip_step = atoi(argv[3]);
  sp.clear_non_keyframes = atoi(argv[4]);
  sp.predecessor_candidates = atoi(argv[5]);
  sp.neighbor_candidates = atoi(argv[6]);
  sp.min_sampled_candidates = atoi(argv[7]);
  std::vector<std::unique_ptr<rgbdslam::Node>> nodes;
  int added = 0;
  for (int32_t k = 0; k < n; ++k) {
    int32_t rows = 0, nsec = 0;
    int64_t sec = 0;
    if (fread(&rows, 4, 1, f) != 1 || fread(&sec, 8, 1, f) != 1 || fread(&nsec, 4, 1, f) != 1) return 2;
    std::vector<uint8_t> desc((size_t)rows * 32);
    std::vector<float> xyz((size_t)rows * 4);
    if (rows > 0 && (fread(desc.data(), 32, (size_t)rows, f) != (size_t)rows || fread(xyz.data(), 16, (size_t)rows, f) != (size_t)rows)) return 2;
    nodes.emplace_back(new rgbdslam::Node(fe, k, desc.data(), xyz.data(), rows));   // uploads into slot k
    rgbdfe_slam_step st;
    const bool ok = gm.addNode(nodes.back().get(), sec, nsec, &st);
    if (ok != (st.status == RGBDFE_SLAM_FIRST || st.status == RGBDFE_SLAM_ADDED || st.status == RGBDFE_SLAM_REPLACED_FIRST)) return 4;
    if (gm.lastAddNodeStatus() != RGBDFE_OK) return 6;   // a dropped frame is no failed call
    added += ok ? 1 : 0;
    printf("%d %d %d %d %d %d", st.status, st.id, st.found, st.initial_id, st.initial_verdict, st.n_candidates);
    for (int c = 0; c < st.n_candidates; ++c) printf(" %d", st.candidates[c]);
    for (int c = 0; c < st.n_candidates; ++c) printf(" %d", (int)st.verdicts[c]);
    printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | ", st.best_id1, st.best_id2, st.best_n_inl, st.predecessor_matched,
           st.edge_to_keyframe, st.keyframe_added, st.cleared_first, st.cleared_last, st.released_slot, st.constant_position,
           st.cloud_released, st.has_broadcast_pose, st.optimize_due, st.sequential_edges, st.loop_closure_edges);
    print_hex(st.motion_estimate, 16);
    printf(" | ");
    print_hex(st.broadcast_pose, 16);
    printf("\n");
  }
  fclose(f);
  printf("K");
  for (int32_t id : gm.keyframeIds()) printf(" %d", id);
  printf("\nT");
  for (int id = 0; gm.slotOf(id) >= -1; ++id) printf(" %d", gm.slotOf(id));
  printf("\nV");
  for (int id = 0; gm.slotOf(id) >= -1; ++id) printf(" %d", gm.validTfEstimate(id) ? 1 : 0);
  printf("\n");
  return added > 0 ? 0 : 5;
}
