// pose_graph_host.h -- the pose-graph object (include/rgbdfe.h): what candidate selection reads (candidates.cpp) and what
// the optimiser reads and writes (api_pose_graph.hip).  Plain C++: candidates.cpp is built without the HIP headers, so the
// optimiser's device buffers hang on an opaque pointer with the function that frees them.
#pragma once
#include <cstdint>
#include <deque>
#include <map>
#include <set>
#include <vector>

struct rgbdfe_pose_graph {
  struct NodeInfo {
    int32_t vertex_id;
    bool matchable;
    bool fixed = false;
    double est[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};  // VertexSE3 estimate: rotation row-major, then translation
  };
  struct MeasuredEdge {      // g2o::EdgeSE3: vertices (node ids), measurement (as est), information row-major
    int32_t id1, id2;
    double z[12];
    double info[36];
    bool active = true;      // false once pruned with verdict REMOVED: the slot stays, the edge contributes nothing
  };
  std::map<int32_t, NodeInfo> nodes;                 // node id -> node (graph_)
  std::set<int32_t> camera_vertices;                 // vertex ids
  std::map<int32_t, std::set<int32_t>> adjacency;    // vertex id -> vertex ids joined by an edge
  std::deque<int32_t> keyframes;
  std::vector<MeasuredEdge> edges;                   // in insertion order; edges without a measurement are not here
  int32_t strategy = 0;                              // RGBDFE_POSE_RELATIVE_TO_*
  int32_t earliest_loop_closure_node = 0;            // graph_manager.cpp:444, :893-896 (kept while a strategy is set)
  void* device = nullptr;                            // the optimiser's buffers (api_pose_graph.hip)
  void (*device_free)(void*) = nullptr;
};

namespace rgbdfe_host {
// the trajectory writer's matrix -> quaternion conversion (candidates.cpp): R row-major, q = (x, y, z, w)
void quat_from_rot_xyzw(const double* R, double* q);
}  // namespace rgbdfe_host
