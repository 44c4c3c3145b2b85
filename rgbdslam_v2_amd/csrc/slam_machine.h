// slam_machine.h -- the decision machine of the SLAM step (include/rgbdfe.h, "the SLAM step"): GraphManager::addNode,
// nodeComparisons, firstNode, addKeyframe and addEdgeToG2O (graph_manager.cpp:360-898) with isBigTrafo / isSmallTrafo
// (misc.cpp:272-315), over the pose-graph object's C functions -- and two members of its struct (pose_graph_host.h) that
// have no function: earliest_loop_closure_node is written and read, camera_vertices is counted.  Plain C++: no HIP, no
// globals; everything that needs the device (the comparisons, the optimiser, releasing slots and clouds) stays with the
// caller, which reads what is due from the step record.  Build with -ffp-contract=off: the transformation tests are part of the contract.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rgbdfe.h"
#include "pose_graph_host.h"

namespace rgbdfe_slam_machine {

// trafoSize (misc.cpp:272-276) on the double cast of a column-major Matrix4f
inline void trafo_size(const float* T, double* angle, double* dist) {
  const double trace = ((double)T[0] + (double)T[5]) + (double)T[10];
  *angle = std::acos((trace - 1) / 2) * 180.0 / 3.14159265358979323846;
  const double tx = (double)T[12], ty = (double)T[13], tz = (double)T[14];
  *dist = std::sqrt((tx * tx + ty * ty) + tz * tz);
}
inline bool is_big_trafo(const rgbdfe_slam_params& p, const float* T) {
  double angle, dist;
  trafo_size(T, &angle, &dist);
  return dist > p.min_translation_meter || angle > p.min_rotation_degree;
}
inline bool is_small_trafo(const rgbdfe_slam_params& p, const float* T, double seconds) {
  if (seconds <= 0.0) return true;
  double angle, dist;
  trafo_size(T, &angle, &dist);
  return dist / seconds < p.max_translation_meter && angle / seconds < p.max_rotation_degree;
}
// (ros::Time a - ros::Time b).toSec(): integer seconds and nanoseconds, normalised to nsec in [0, 1e9)
inline double stamp_diff(int64_t a_sec, int32_t a_nsec, int64_t b_sec, int32_t b_nsec) {
  int64_t sec = a_sec - b_sec, nsec = (int64_t)a_nsec - (int64_t)b_nsec;
  while (nsec >= 1000000000LL) { nsec -= 1000000000LL; ++sec; }
  while (nsec < 0) { nsec += 1000000000LL; --sec; }
  return (double)sec + 1e-9 * (double)nsec;
}

struct Machine {
  enum Phase { kIdle = 0, kInitial = 1, kMain = 2 };
  rgbdfe_slam_params prm{};
  rgbdfe_pose_graph* g = nullptr;
  rgbdfe_rand_fn rand_fn = nullptr;
  void* rand_state = nullptr;
  // graph_: everything indexed by graph id
  std::vector<int32_t> slot_of, rows;
  std::vector<int64_t> stamp_sec;
  std::vector<int32_t> stamp_nsec;
  std::vector<uint8_t> valid_tf;
  std::vector<int32_t> keyframes;     // keyframe_ids_
  int32_t next_seq_id = 0;
  uint32_t calls = 0;                 // begin calls so far
  int32_t sequential_edges = 0, loop_closure_edges = 0;
  int32_t best_id1 = -1, best_id2 = -1, best_n_inl = 0;   // curr_best_result_
  // the step in flight
  Phase phase = kIdle;
  int32_t new_slot = -1, new_rows = 0, new_id = -1, new_nsec = 0, prev_id = -1;
  int64_t new_sec = 0;
  bool has_vertex = false, predecessor_matched = false, edge_to_keyframe = false;
  int32_t edges_added = 0;
  std::vector<int32_t> pending;       // the ids handed out
  std::vector<int32_t> to_release;    // slots the step gave up (cleared non-keyframes, a replaced first node): the caller's
  rgbdfe_slam_step st{};

  static void identity(double* m) {
    for (int k = 0; k < 16; ++k) m[k] = (k % 5 == 0) ? 1.0 : 0.0;
  }
  void clear_step() {
    std::memset(&st, 0, sizeof(st));
    st.id = -1; st.initial_id = -1; st.best_id1 = -1; st.best_id2 = -1; st.keyframe_added = -1;
    st.cleared_first = -1; st.cleared_last = -1; st.released_slot = -1;
    identity(st.motion_estimate);
    identity(st.broadcast_pose);
  }
  void reset() {   // resetGraph
    slot_of.clear(); rows.clear(); stamp_sec.clear(); stamp_nsec.clear(); valid_tf.clear(); keyframes.clear();
    next_seq_id = 0; sequential_edges = 0; loop_closure_edges = 0;
    best_id1 = -1; best_id2 = -1; best_n_inl = 0;
    phase = kIdle;
    pending.clear();
    rgbdfe_pose_graph_clear(g);
  }
  bool is_keyframe(int32_t id) const {
    for (int32_t k : keyframes) if (k == id) return true;
    return false;
  }
  void push_node(int32_t slot, int32_t n_rows, int64_t sec, int32_t nsec) {
    slot_of.push_back(slot); rows.push_back(n_rows); stamp_sec.push_back(sec); stamp_nsec.push_back(nsec);
    valid_tf.push_back(1);
  }
  int finish(rgbdfe_slam_step* out, int32_t* n_ids) {
    st.best_id1 = best_id1; st.best_id2 = best_id2; st.best_n_inl = best_n_inl;
    st.predecessor_matched = predecessor_matched; st.edge_to_keyframe = edge_to_keyframe;
    st.sequential_edges = sequential_edges; st.loop_closure_edges = loop_closure_edges;
    phase = kIdle;
    pending.clear();
    *n_ids = 0;
    if (out) *out = st;
    return RGBDFE_OK;
  }

  // addKeyframe (:784-809)
  int add_keyframe(int32_t id) {
    if (prm.clear_non_keyframes && keyframes.size() >= 2) {
      const int32_t most_recent = keyframes.back(), second = keyframes[keyframes.size() - 2];
      if (second + 1 <= most_recent - 1) { st.cleared_first = second + 1; st.cleared_last = most_recent - 1; }
      for (int32_t k = second + 1; k < most_recent; ++k) {
        if (k < 0 || k >= (int32_t)slot_of.size()) continue;
        rgbdfe_pose_graph_set_matchable(g, k, 0);
      }
    }
    keyframes.push_back(id);
    return rgbdfe_pose_graph_add_keyframe(g, id);
  }

  // firstNode (:360-402)
  int first_node(int32_t slot, int32_t n_rows, int64_t sec, int32_t nsec) {
    const int32_t id = (int32_t)slot_of.size();   // 0
    ++next_seq_id;
    int rc = rgbdfe_pose_graph_add_node(g, id, id, 1, 0);
    if (rc != RGBDFE_OK) return rc;
    rc = rgbdfe_pose_graph_set_estimate(g, id, prm.init_base_pose);
    if (rc != RGBDFE_OK) return rc;
    rc = rgbdfe_pose_graph_set_fixed(g, id, 1);
    if (rc != RGBDFE_OK) return rc;
    push_node(slot, n_rows, sec, nsec);
    st.id = id;
    std::memcpy(st.motion_estimate, prm.init_base_pose, sizeof(st.motion_estimate));
    return add_keyframe(id);
  }

  // addEdgeToG2O (:811-898) for an edge id1 -> the new node.  *added = 0: refused.
  int add_edge(int32_t id1, const double* Z, const double* info, bool large_edge, bool set_estimate, bool* added) {
    *added = false;
    if (!has_vertex && !large_edge) return RGBDFE_OK;   // "Edge to new vertex is too short"
    const bool create = !has_vertex;
    if (create) {
      const int rc = rgbdfe_pose_graph_add_node(g, new_id, new_id, 1, 0);
      if (rc != RGBDFE_OK) return rc;
      // (add_node sets earliest_loop_closure_node = new_id under a strategy: the value it has already)
      has_vertex = true;
      push_node(new_slot, new_rows, new_sec, new_nsec);   // graph_[new_node->id_] = new_node
    }
    const int rc = rgbdfe_pose_graph_add_edge_se3(g, id1, new_id, Z, info, (create || set_estimate) ? 1 : 0);
    if (rc != RGBDFE_OK) return rc;
    if (create || set_estimate) rgbdfe_pose_graph_get_estimate(g, new_id, st.motion_estimate);
    const int32_t d = id1 > new_id ? id1 - new_id : new_id - id1;
    if (d > prm.predecessor_candidates) ++loop_closure_edges; else ++sequential_edges;
    ++edges_added;
    *added = true;
    return RGBDFE_OK;
  }

  static void edge_of_result(const rgbdfe_compact_result& r, bool icp, double* Z, double* info) {
    for (int k = 0; k < 16; ++k) Z[k] = (double)r.trafo[k];
    for (int k = 0; k < 36; ++k) info[k] = (k % 7 == 0) ? (icp ? 1e-2 : r.info_scale) : 0.0;
  }

  int select_candidates(int32_t* ids, int32_t capacity, int32_t* n_ids) {
    const int32_t cap = capacity < RGBDFE_SLAM_MAX_CANDIDATES ? capacity : RGBDFE_SLAM_MAX_CANDIDATES;
    int32_t n = 0;
    int32_t tmp[RGBDFE_SLAM_MAX_CANDIDATES];
    const int rc = rgbdfe_potential_edge_targets(g, prm.predecessor_candidates - 1, prm.neighbor_candidates, prm.min_sampled_candidates,
                                                 prm.geodesic_depth, predecessor_matched ? best_id1 : prev_id,
                                                 predecessor_matched ? 0 : 1, rand_fn, rand_state, prm.seed + (calls - 1u), tmp,
                                                 cap, &n);
    if (rc != RGBDFE_OK) return rc;
    pending.assign(tmp, tmp + n);
    st.n_candidates = n;
    for (int32_t k = 0; k < n; ++k) { st.candidates[k] = tmp[k]; ids[k] = tmp[k]; }
    *n_ids = n;
    return RGBDFE_OK;
  }

  int begin(int32_t slot, int32_t n_rows, int64_t sec, int32_t nsec, int32_t* ids, int32_t capacity, int32_t* n_ids,
            rgbdfe_slam_step* out) {
    if (!g || !ids || !n_ids || capacity < 1 || n_rows < 0 || phase != kIdle) return RGBDFE_ERR_INVALID_ARG;
    clear_step();
    to_release.clear();
    ++calls;
    has_vertex = false; predecessor_matched = false; edge_to_keyframe = false; edges_added = 0;
    if (n_rows < prm.min_matches) {   // addNode :687
      st.status = RGBDFE_SLAM_TOO_FEW_FEATURES;
      return finish(out, n_ids);
    }
    if (slot_of.empty()) {
      const int rc = first_node(slot, n_rows, sec, nsec);
      if (rc != RGBDFE_OK) return rc;
      st.status = RGBDFE_SLAM_FIRST;
      return finish(out, n_ids);
    }
    // nodeComparisons :440-455
    new_slot = slot; new_rows = n_rows; new_sec = sec; new_nsec = nsec;
    new_id = (int32_t)slot_of.size();
    ++next_seq_id;
    g->earliest_loop_closure_node = new_id;   // :444, whatever the strategy: the keyframe rule reads it
    prev_id = new_id - 1;   // graph_.rbegin()->second->id_
    best_id1 = -1; best_id2 = -1; best_n_inl = 0;   // curr_best_result_ = mr
    if (prm.min_translation_meter > 0.0 || prm.min_rotation_degree > 0.0) {
      phase = kInitial;
      pending.assign(1, prev_id);
      st.initial_id = prev_id;
      ids[0] = prev_id;
      *n_ids = 1;
      return RGBDFE_OK;
    }
    phase = kMain;
    const int rc = select_candidates(ids, capacity, n_ids);
    if (rc != RGBDFE_OK) { phase = kIdle; return rc; }
    if (*n_ids == 0) return conclude(out, n_ids);
    return RGBDFE_OK;
  }

  int feed(const rgbdfe_compact_result* results, const uint8_t* flags, int32_t n, int32_t* ids, int32_t capacity, int32_t* n_ids,
           rgbdfe_slam_step* out) {
    if (!g || !ids || !n_ids || capacity < 1 || phase == kIdle || n != (int32_t)pending.size() || (n > 0 && !results))
      return RGBDFE_ERR_INVALID_ARG;
    double Z[16], info[36];
    bool added = false;
    if (phase == kInitial) {   // :456-512
      const rgbdfe_compact_result& r = results[0];
      const uint8_t f = flags ? flags[0] : 0;
      const bool icp = (f & RGBDFE_SLAM_RESULT_ICP) != 0;
      st.initial_verdict = RGBDFE_SLAM_VERDICT_NO_EDGE;
      if (f & RGBDFE_SLAM_RESULT_WITHDRAWN) st.initial_verdict = RGBDFE_SLAM_VERDICT_WITHDRAWN;
      else if (r.id1 >= 0 && r.id2 >= 0) {
        const double dt = stamp_diff(new_sec, new_nsec, stamp_sec[(size_t)prev_id], stamp_nsec[(size_t)prev_id]);
        edge_of_result(r, icp, Z, info);
        if (!is_big_trafo(prm, r.trafo) || !is_small_trafo(prm, r.trafo, dt)) {
          st.status = RGBDFE_SLAM_MOTION_OUT_OF_BOUNDS;
          st.initial_verdict = RGBDFE_SLAM_VERDICT_OUT_OF_BOUNDS | (icp ? RGBDFE_SLAM_VERDICT_ICP : 0);
          double X[16];
          rgbdfe_pose_graph_get_estimate(g, prev_id, X);
          for (int c = 0; c < 4; ++c)   // previous * incremental, sums of three products as (a0 b0 + a1 b1) + a2 b2
            for (int r_ = 0; r_ < 3; ++r_)
              st.broadcast_pose[4 * c + r_] = ((X[r_] * Z[4 * c] + X[4 + r_] * Z[4 * c + 1]) + X[8 + r_] * Z[4 * c + 2]) + (c == 3 ? X[12 + r_] : 0.0);
          st.has_broadcast_pose = 1;
          best_id1 = prev_id; best_id2 = new_id; best_n_inl = icp ? 0 : r.n_inl;   // curr_best_result_ = mr
          return finish(out, n_ids);
        }
        const int rc = add_edge(prev_id, Z, info, true, true, &added);
        if (rc != RGBDFE_OK) { phase = kIdle; return rc; }
        if (!added) {   // (cannot happen with largeEdge: kept for the reference's shape)
          st.status = RGBDFE_SLAM_NO_MATCH;
          return finish(out, n_ids);
        }
        st.initial_verdict = RGBDFE_SLAM_VERDICT_ACCEPTED | (icp ? RGBDFE_SLAM_VERDICT_ICP : 0);
        if (is_keyframe(prev_id)) edge_to_keyframe = true;
        valid_tf[(size_t)prev_id] = 1;
        best_id1 = prev_id; best_id2 = new_id; best_n_inl = icp ? 0 : r.n_inl;
        predecessor_matched = true;
      }
      phase = kMain;
      const int rc = select_candidates(ids, capacity, n_ids);
      if (rc != RGBDFE_OK) { phase = kIdle; return rc; }
      if (*n_ids == 0) return conclude(out, n_ids);
      return RGBDFE_OK;
    }
    // the main loop :550-583
    for (int32_t k = 0; k < n; ++k) {
      const rgbdfe_compact_result& r = results[k];
      const uint8_t f = flags ? flags[k] : 0;
      const bool icp = (f & RGBDFE_SLAM_RESULT_ICP) != 0;
      const uint8_t src = icp ? RGBDFE_SLAM_VERDICT_ICP : 0;
      const int32_t id1 = pending[(size_t)k];
      st.verdicts[k] = RGBDFE_SLAM_VERDICT_NO_EDGE;
      if (f & RGBDFE_SLAM_RESULT_WITHDRAWN) { st.verdicts[k] = RGBDFE_SLAM_VERDICT_WITHDRAWN; continue; }
      if (r.id1 < 0) continue;
      const int32_t n_inl = icp ? 0 : r.n_inl;
      const double dt = stamp_diff(new_sec, new_nsec, stamp_sec[(size_t)id1], stamp_nsec[(size_t)id1]);
      if (!is_small_trafo(prm, r.trafo, dt)) { st.verdicts[k] = RGBDFE_SLAM_VERDICT_NOT_SMALL | src; continue; }
      edge_of_result(r, icp, Z, info);
      const int rc = add_edge(id1, Z, info, is_big_trafo(prm, r.trafo), n_inl > best_n_inl, &added);
      if (rc != RGBDFE_OK) { phase = kIdle; return rc; }
      if (!added) { st.verdicts[k] = RGBDFE_SLAM_VERDICT_TOO_SHORT | src; continue; }
      st.verdicts[k] = RGBDFE_SLAM_VERDICT_ACCEPTED | src;
      if (id1 == new_id - 1) predecessor_matched = true;
      valid_tf[(size_t)id1] = 1;
      if (n_inl > best_n_inl) { best_id1 = id1; best_id2 = new_id; best_n_inl = n_inl; }
      if (is_keyframe(id1)) edge_to_keyframe = true;
    }
    return conclude(out, n_ids);
  }

  // nodeComparisons :624-657, then addNode :704-773
  int conclude(rgbdfe_slam_step* out, int32_t* n_ids) {
    const bool found_trafo = edges_added > 0;
    const bool keep_anyway = prm.keep_all_nodes || (new_rows > prm.min_matches && prm.keep_good_nodes);
    const float time_delta_sec = (float)std::fabs(stamp_diff(new_sec, new_nsec, stamp_sec[(size_t)prev_id], stamp_nsec[(size_t)prev_id]));
    if ((!found_trafo && prm.have_odometry_frame) || ((!found_trafo && keep_anyway) || (!predecessor_matched && time_delta_sec < 0.1))) {
      if (time_delta_sec == 0.0f) {
        st.constant_position = RGBDFE_SLAM_CONSTANT_SKIPPED;   // I / 0: not handed to the optimiser
      } else {
        double Z[16], info[36];
        identity(Z);
        identity(st.motion_estimate);
        for (int k = 0; k < 36; ++k) info[k] = (k % 7 == 0) ? 1.0 / time_delta_sec : 0.0 / time_delta_sec;
        bool added = false;
        const int rc = add_edge(prev_id, Z, info, true, true, &added);
        if (rc != RGBDFE_OK) { phase = kIdle; return rc; }
        st.constant_position = RGBDFE_SLAM_CONSTANT_ADDED;
        valid_tf[(size_t)new_id] = 0;
        best_id1 = prev_id; best_id2 = new_id; best_n_inl = 0;   // an empty result carrying this edge
      }
    }
    st.found = edges_added > 0 ? 1 : 0;
    if (st.found) {
      st.status = RGBDFE_SLAM_ADDED;
      st.id = new_id;
      if (prm.create_cloud_every_nth_node != 0 && new_id % prm.create_cloud_every_nth_node != 0) st.cloud_released = 1;
      if (!edge_to_keyframe && g->earliest_loop_closure_node > keyframes.back()) {
        const int rc = add_keyframe(new_id - 1);
        if (rc != RGBDFE_OK) { phase = kIdle; return rc; }
        st.keyframe_added = new_id - 1;
        for (int32_t k = st.cleared_first; k >= 0 && k <= st.cleared_last; ++k) {
          if (slot_of[(size_t)k] >= 0) to_release.push_back(slot_of[(size_t)k]);
          slot_of[(size_t)k] = -1;
        }
      }
      if (prm.optimizer_skip_step > 0 && (int32_t)g->camera_vertices.size() % prm.optimizer_skip_step == 0) st.optimize_due = 1;
    } else if (slot_of.size() == 1 && new_rows > rows[0]) {   // :762-769
      const int32_t old_slot = slot_of[0];
      reset();
      const int rc = first_node(new_slot, new_rows, new_sec, new_nsec);
      if (rc != RGBDFE_OK) return rc;
      st.status = RGBDFE_SLAM_REPLACED_FIRST;
      st.released_slot = old_slot;
      to_release.push_back(old_slot);
    } else {
      st.status = RGBDFE_SLAM_NO_MATCH;
    }
    return finish(out, n_ids);
  }
};

}  // namespace rgbdfe_slam_machine
