// tests/emu/slam_machine_main.cpp -- TEST INFRASTRUCTURE ONLY: the decision machine of csrc/slam_machine.h in a stand-alone
// program over the scripts of tests/slam_cases.py (tests/test_slam_machine_host.py builds it together with
// csrc/candidates.cpp, with the address and undefined-behaviour sanitizers, and compares what it prints).
//   slam_machine_main script.txt
// Script lines: S strategy / P name value(hex of the double) / F slot rows sec nsec n_results, followed by its
// R id edge n_inl info(hex) flags T(16 hex floats) lines.  Output: one line per frame (the step record without its times, as
// slam_cases.step_line prints it), then the final state (K keyframes, T slots, V valid_tf, X fixed, E edges, N estimates).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "slam_machine.h"

namespace {

double double_of_hex(const char* s) {
  const uint64_t u = strtoull(s, nullptr, 16);
  double d;
  memcpy(&d, &u, 8);
  return d;
}
void print_hex(const double* v, int n) {
  for (int k = 0; k < n; ++k) {
    uint64_t u;
    memcpy(&u, v + k, 8);
    printf("%s%016" PRIx64, k ? " " : "", u);
  }
}
struct Result { int edge, n_inl, flags; double info; float T[16]; };

bool set_param(rgbdfe_slam_params& p, const std::string& name, double v) {
#define INT_PARAM(f) if (name == #f) { p.f = (int32_t)v; return true; }
#define DBL_PARAM(f) if (name == #f) { p.f = v; return true; }
  INT_PARAM(min_matches) INT_PARAM(predecessor_candidates) INT_PARAM(neighbor_candidates) INT_PARAM(min_sampled_candidates)
  INT_PARAM(geodesic_depth) INT_PARAM(keep_all_nodes) INT_PARAM(keep_good_nodes) INT_PARAM(clear_non_keyframes)
  INT_PARAM(create_cloud_every_nth_node) INT_PARAM(optimizer_skip_step) INT_PARAM(have_odometry_frame)
  DBL_PARAM(min_translation_meter) DBL_PARAM(min_rotation_degree) DBL_PARAM(max_translation_meter) DBL_PARAM(max_rotation_degree)
  if (name == "seed") { p.seed = (uint32_t)v; return true; }
  return false;
}

void print_step(const rgbdfe_slam_step& st) {
  printf("%d %d %d %d %d %d", st.status, st.id, st.found, st.initial_id, st.initial_verdict, st.n_candidates);
  for (int k = 0; k < st.n_candidates; ++k) printf(" %d", st.candidates[k]);
  for (int k = 0; k < st.n_candidates; ++k) printf(" %d", (int)st.verdicts[k]);
  printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | ", st.best_id1, st.best_id2, st.best_n_inl, st.predecessor_matched,
         st.edge_to_keyframe, st.keyframe_added, st.cleared_first, st.cleared_last, st.released_slot, st.constant_position,
         st.cloud_released, st.has_broadcast_pose, st.optimize_due, st.sequential_edges, st.loop_closure_edges);
  print_hex(st.motion_estimate, 16);
  printf(" | ");
  print_hex(st.broadcast_pose, 16);
  printf("\n");
}

}  // namespace

// the parameter defaults of rgbdfe_slam_default_params (csrc/api_slam.hip is not part of this program)
static void default_params(rgbdfe_slam_params* p) {
  *p = rgbdfe_slam_params{};
  p->min_matches = 20; p->predecessor_candidates = 4; p->neighbor_candidates = 4; p->min_sampled_candidates = 4;
  p->geodesic_depth = 3; p->create_cloud_every_nth_node = 1; p->optimizer_skip_step = 1; p->emm__skip_step = 8;
  p->max_translation_meter = 1e10; p->max_rotation_degree = 360; p->optimizer_iterations = 0.01; p->observability_threshold = -0.6;
  for (int k = 0; k < 16; ++k) p->init_base_pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: slam_machine_main script.txt\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  rgbdfe_pose_graph* g = rgbdfe_pose_graph_create();
  rgbdfe_slam_machine::Machine m;
  default_params(&m.prm);
  m.g = g;
  char line[1024];
  int status = 0;
  while (status == 0 && fgets(line, sizeof(line), f)) {
    char name[64], hex[32];
    int a, b, c2, n_res;
    long long sec;
    if (sscanf(line, "S %d", &a) == 1) {
      if (rgbdfe_pose_graph_set_strategy(g, a) != RGBDFE_OK) status = 3;
    } else if (sscanf(line, "P %63s %31s", name, hex) == 2) {
      if (!set_param(m.prm, name, double_of_hex(hex))) { fprintf(stderr, "unknown parameter %s\n", name); status = 3; }
    } else if (sscanf(line, "F %d %d %lld %d %d", &a, &b, &sec, &c2, &n_res) == 5) {
      std::map<int, Result> res;
      for (int r = 0; r < n_res && status == 0; ++r) {
        if (!fgets(line, sizeof(line), f)) { status = 3; break; }
        Result R{};
        int id, used = 0;
        if (sscanf(line, "R %d %d %d %31s %d%n", &id, &R.edge, &R.n_inl, hex, &R.flags, &used) != 5) { status = 3; break; }
        R.info = double_of_hex(hex);
        const char* at = line + used;
        for (int k = 0; k < 16; ++k) {
          char* end = nullptr;
          const uint32_t u = (uint32_t)strtoul(at, &end, 16);
          if (end == at) { status = 3; break; }
          memcpy(&R.T[k], &u, 4);
          at = end;
        }
        res[id] = R;
      }
      if (status) break;
      int32_t ids[RGBDFE_SLAM_MAX_CANDIDATES], n = 0;
      rgbdfe_slam_step st;
      int rc = m.begin(a, b, (int64_t)sec, c2, ids, RGBDFE_SLAM_MAX_CANDIDATES, &n, &st);
      while (rc == RGBDFE_OK && n > 0) {
        rgbdfe_compact_result rec[RGBDFE_SLAM_MAX_CANDIDATES];
        uint8_t flags[RGBDFE_SLAM_MAX_CANDIDATES];
        memset(rec, 0, sizeof(rec));
        for (int k = 0; k < n; ++k) {
          const auto it = res.find(ids[k]);
          rec[k].id1 = -1; rec[k].id2 = -1;
          flags[k] = 0;
          if (it == res.end()) continue;
          if (it->second.edge) { rec[k].id1 = 900 + ids[k]; rec[k].id2 = 999; }
          rec[k].n_inl = it->second.n_inl;
          rec[k].info_scale = it->second.info;
          memcpy(rec[k].trafo, it->second.T, sizeof(rec[k].trafo));
          flags[k] = (uint8_t)it->second.flags;
        }
        rc = m.feed(rec, flags, n, ids, RGBDFE_SLAM_MAX_CANDIDATES, &n, &st);
      }
      if (rc != RGBDFE_OK) { fprintf(stderr, "the machine returned %d\n", rc); status = 4; break; }
      print_step(st);
    } else if (line[0] != '\n') {
      fprintf(stderr, "bad line: %s", line);
      status = 3;
    }
  }
  fclose(f);
  if (status == 0) {
    printf("K");
    for (int32_t k : m.keyframes) printf(" %d", k);
    printf("\nT");
    for (int32_t s : m.slot_of) printf(" %d", s);
    printf("\nV");
    for (uint8_t v : m.valid_tf) printf(" %d", (int)v);
    printf("\nX");
    for (size_t i = 0; i < m.slot_of.size(); ++i) {
      int32_t fx = -1;
      rgbdfe_pose_graph_get_fixed(g, (int32_t)i, &fx);
      printf(" %d", fx);
    }
    printf("\nE");
    for (int e = 0;; ++e) {
      int32_t i1, i2;
      double info[36];
      if (rgbdfe_pose_graph_get_edge(g, e, &i1, &i2, nullptr, info, nullptr) != RGBDFE_OK) break;
      printf(" %d-%d:", i1, i2);
      print_hex(info, 1);
    }
    printf("\n");
    for (size_t i = 0; i < m.slot_of.size(); ++i) {
      double X[16];
      rgbdfe_pose_graph_get_estimate(g, (int32_t)i, X);
      printf("N %d ", (int)i);
      print_hex(X, 16);
      printf("\n");
    }
  }
  rgbdfe_pose_graph_destroy(g);
  return status;
}
