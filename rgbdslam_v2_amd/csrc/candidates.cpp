// Candidate selection for loop closure: which earlier nodes a new node is compared with
// (GraphManager::getPotentialEdgeTargetsWithDijkstra, graph_manager.cpp:204-324) -- the step in front of the pair
// path; its output is the `tids` list of rgbdfe_match_node_pairs.  Host code only (no device work): the pose-graph
// topology it reads is a few integers per node.
//
// What the reference reads, and what stands for it here:
//   graph_ (std::map<int, Node*>: id_, vertex_id_, matchable_)      PoseGraph::nodes
//   camera_vertices (g2o::HyperGraph::VertexSet)                   PoseGraph::camera_vertices (vertex ids)
//   optimizer_ edges between camera vertices                       PoseGraph::adjacency
//   keyframe_ids_ (QList<int>)                                     PoseGraph::keyframes
//   g2o::HyperDijkstra::shortestPaths(v, UniformCostFunction, geodesic_depth)   bounded_neighbourhood()
//   rand()                                                         the caller's generator (NULL: a counter-based one)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <limits>
#include <map>
#include <new>
#include <queue>
#include <set>
#include <utility>
#include <vector>

#include <string>

#include "rgbdfe.h"
#include "pose_graph_host.h"
#include "session_format.h"

namespace {

// g2o::HyperDijkstra::shortestPaths with UniformCostFunction (every edge costs 1) and maxDistance: a vertex is
// relaxed only while its distance stays BELOW maxDistance (g2o/core/hyper_dijkstra.cpp: `zDistance < maxDistance`),
// visited() = the start vertex and every vertex that was relaxed.  (g2o is a third-party dependency that is not part
// of the reference tree: restated.)
std::set<int32_t> bounded_neighbourhood(const rgbdfe_pose_graph& g, int32_t start, double max_distance) {
  std::map<int32_t, double> dist;
  std::set<int32_t> visited;
  typedef std::pair<double, int32_t> Entry;
  std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> frontier;
  dist[start] = 0.0;
  frontier.push(Entry(0.0, start));
  while (!frontier.empty()) {
    const Entry e = frontier.top();
    frontier.pop();
    const int32_t u = e.second;
    const double du = dist[u];
    visited.insert(u);
    const auto at = g.adjacency.find(u);
    if (at == g.adjacency.end()) continue;
    for (int32_t z : at->second) {
      const double dz = du + 1.0;
      const auto zt = dist.find(z);
      const double old = zt == dist.end() ? std::numeric_limits<double>::max() : zt->second;
      if (dz < old && dz < max_distance) {
        dist[z] = dz;
        frontier.push(Entry(dz, z));
      }
    }
  }
  return visited;
}

struct CounterRand {  // stand-in for rand() when the caller brings no generator: same integer mixer as the RANSAC sampler
  uint32_t seed, k = 0;
  static uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
  }
  int next() { return (int)(mix(mix(seed ^ 0x9E3779B9u) + (k++) * 0x85EBCA6Bu) >> 1); }
};

}  // namespace

std::string& rgbdfe_session::contextless_error() {
  static thread_local std::string msg;
  return msg;
}

extern "C" {

rgbdfe_pose_graph* rgbdfe_pose_graph_create(void) { return new (std::nothrow) rgbdfe_pose_graph(); }

void rgbdfe_pose_graph_destroy(rgbdfe_pose_graph* g) {
  if (g && g->device && g->device_free) g->device_free(g->device);  // the optimiser's device buffers
  delete g;
}

int rgbdfe_pose_graph_add_node(rgbdfe_pose_graph* g, int32_t node_id, int32_t vertex_id, int32_t matchable,
                               int32_t keyframe) try {
  if (!g || node_id < 0 || vertex_id < 0) return RGBDFE_ERR_INVALID_ARG;
  rgbdfe_pose_graph::NodeInfo& nd = g->nodes[node_id];  // a node added again keeps its estimate and its fixed flag
  nd.vertex_id = vertex_id;
  nd.matchable = matchable != 0;
  if (g->strategy != RGBDFE_POSE_RELATIVE_TO_NONE) g->earliest_loop_closure_node = node_id;  // graph_manager.cpp:444
  g->camera_vertices.insert(vertex_id);
  g->adjacency[vertex_id];
  if (keyframe) g->keyframes.push_back(node_id);
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_add_edge(rgbdfe_pose_graph* g, int32_t node_id1, int32_t node_id2) try {
  if (!g) return RGBDFE_ERR_INVALID_ARG;
  const auto a = g->nodes.find(node_id1), b = g->nodes.find(node_id2);
  if (a == g->nodes.end() || b == g->nodes.end() || node_id1 == node_id2) return RGBDFE_ERR_INVALID_ARG;
  g->adjacency[a->second.vertex_id].insert(b->second.vertex_id);
  g->adjacency[b->second.vertex_id].insert(a->second.vertex_id);
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_set_matchable(rgbdfe_pose_graph* g, int32_t node_id, int32_t matchable) try {
  if (!g) return RGBDFE_ERR_INVALID_ARG;
  const auto a = g->nodes.find(node_id);
  if (a == g->nodes.end()) return RGBDFE_ERR_INVALID_ARG;
  a->second.matchable = matchable != 0;
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

// GraphManager::addKeyframe's keyframe_ids_.push_back (graph_manager.cpp:804): the reference promotes id - 1 after the fact
int rgbdfe_pose_graph_add_keyframe(rgbdfe_pose_graph* g, int32_t node_id) try {
  if (!g) return RGBDFE_ERR_INVALID_ARG;
  if (g->nodes.find(node_id) == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;
  g->keyframes.push_back(node_id);
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

// resetGraph: nodes, edges and keyframes go; the strategy stays, and so do the optimiser's device buffers (they are sized
// again by the next plan)
int rgbdfe_pose_graph_clear(rgbdfe_pose_graph* g) {
  if (!g) return RGBDFE_ERR_INVALID_ARG;
  g->nodes.clear();
  g->camera_vertices.clear();
  g->adjacency.clear();
  g->keyframes.clear();
  g->edges.clear();
  g->earliest_loop_closure_node = 0;
  return RGBDFE_OK;
}

// ---- the graph as a byte string (session_format.h) ---------------------------------------------------------------------
namespace {
int graph_fail(int code, const std::string& msg) {
  rgbdfe_session::contextless_error() = msg;
  return code;
}
}  // namespace

int rgbdfe_pose_graph_serialize(const rgbdfe_pose_graph* g, uint8_t* out, int64_t capacity, int64_t* bytes) try {
  if (!g || !bytes || capacity < 0 || (capacity > 0 && !out)) return graph_fail(RGBDFE_ERR_INVALID_ARG, "pose graph: bad arguments");
  std::vector<uint8_t> b;
  std::string err;
  const int rc = rgbdfe_session::graph_serialize(*g, b, err);
  if (rc != RGBDFE_OK) return graph_fail(rc, err);
  *bytes = (int64_t)b.size();
  if ((int64_t)b.size() > capacity) return graph_fail(RGBDFE_ERR_CAPACITY, "pose graph: capacity below the string's length (*bytes holds it)");
  std::copy(b.begin(), b.end(), out);
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_deserialize(rgbdfe_pose_graph* g, const uint8_t* in, int64_t bytes) try {
  if (!g || !in || bytes < 0) return graph_fail(RGBDFE_ERR_INVALID_ARG, "pose graph: bad arguments");
  if (!rgbdfe_session::graph_is_empty(*g))
    return graph_fail(RGBDFE_ERR_INVALID_ARG, "pose graph: the target of a deserialise must be empty (rgbdfe_pose_graph_clear)");
  rgbdfe_session::GraphImage img;
  const std::string err = rgbdfe_session::graph_parse(in, (size_t)bytes, img);
  if (!err.empty()) return graph_fail(RGBDFE_ERR_INVALID_ARG, err);
  rgbdfe_session::graph_commit(*g, img);
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_node_ids(const rgbdfe_pose_graph* g, int32_t* ids, int32_t capacity, int32_t* n_out) {
  if (!g || !n_out || capacity < 0 || (capacity > 0 && !ids)) return RGBDFE_ERR_INVALID_ARG;
  *n_out = (int32_t)g->nodes.size();
  if (*n_out > capacity) return RGBDFE_ERR_CAPACITY;
  int32_t k = 0;
  for (const auto& kv : g->nodes) ids[k++] = kv.first;
  return RGBDFE_OK;
}

int rgbdfe_potential_edge_targets(const rgbdfe_pose_graph* g, int32_t sequential_targets, int32_t geodesic_targets,
                                  int32_t sampled_targets, int32_t geodesic_depth, int32_t predecessor_id,
                                  int32_t include_predecessor, rgbdfe_rand_fn rand_fn, void* rand_state, uint32_t seed,
                                  int32_t* ids_out, int32_t capacity, int32_t* n_out) try {
  if (!g || !ids_out || !n_out || capacity < 0) return RGBDFE_ERR_INVALID_ARG;
  CounterRand own{seed};
  auto draw = [&]() { return rand_fn ? rand_fn(rand_state) : own.next(); };
  const int graph_size = (int)g->nodes.size();
  std::deque<int32_t> ids;  // QList<int> ids_to_link_to: sampled ids go to the front, sequential ones to the back
  if (predecessor_id < 0) predecessor_id = graph_size - 1;  // :207

  // fewer previous nodes than targets requested: just use all of them (:212-219)
  if ((int)g->camera_vertices.size() <= sequential_targets + geodesic_targets + sampled_targets ||
      g->camera_vertices.size() <= 1) {
    sequential_targets = sequential_targets + geodesic_targets + sampled_targets;
    geodesic_targets = 0;
    sampled_targets = 0;
    predecessor_id = graph_size - 1;
  }

  if (sequential_targets > 0)  // :221-227
    for (int i = 1; i < sequential_targets + 1 && predecessor_id - i >= 0; i++) ids.push_back(predecessor_id - i);

  if (geodesic_targets > 0) {  // :229-295
    const auto pred = g->nodes.find(predecessor_id);
    if (pred == g->nodes.end()) return RGBDFE_ERR_INVALID_ARG;
    const std::set<int32_t> vs = bounded_neighbourhood(*g, pred->second.vertex_id, (double)geodesic_depth);
    std::map<int32_t, int32_t> vertex_id_to_node_id;
    for (const auto& kv : g->nodes) vertex_id_to_node_id[kv.second.vertex_id] = kv.first;
    // geodesic neighbours except the sequential ones, weighted by their distance in time (:246-270)
    std::map<int32_t, int32_t> neighbour_weights;
    int sum_of_weights = 0;
    for (int32_t vid : vs) {
      const auto it = vertex_id_to_node_id.find(vid);
      const int32_t id = it == vertex_id_to_node_id.end() ? 0 : it->second;  // the reference falls back to id 0 (:250-265)
      const auto nd = g->nodes.find(id);
      if (nd == g->nodes.end() || !nd->second.matchable) continue;
      if (id < predecessor_id - sequential_targets || (id > predecessor_id && id <= graph_size - 1)) {
        const int weight = id > predecessor_id ? id - predecessor_id : predecessor_id - id;
        neighbour_weights[id] = weight;
        sum_of_weights += weight;
      }
    }
    // weighted sampling without replacement (:273-294)
    while ((int)ids.size() < sequential_targets + geodesic_targets && !neighbour_weights.empty()) {
      if (sum_of_weights <= 0) return RGBDFE_ERR_INVALID_ARG;  // rand() % 0 in the reference
      const int random_pick = draw() % sum_of_weights;
      int weight_so_far = 0;
      for (auto mit = neighbour_weights.begin(); mit != neighbour_weights.end(); ++mit) {
        weight_so_far += mit->second;
        if (weight_so_far > random_pick) {
          ids.push_front(mit->first);
          sum_of_weights -= mit->second;
          neighbour_weights.erase(mit);
          break;
        }
      }
    }
  }

  if (sampled_targets > 0) {  // :297-317: uniform sampling among the keyframes not yet chosen
    std::vector<int32_t> pool;
    pool.reserve(g->nodes.size());
    for (int32_t kf : g->keyframes) {
      bool chosen = false;
      for (int32_t v : ids) chosen |= (v == kf);
      const auto nd = g->nodes.find(kf);
      if (!chosen && nd != g->nodes.end() && nd->second.matchable) pool.push_back(kf);
    }
    while ((int)ids.size() < geodesic_targets + sampled_targets + sequential_targets && !pool.empty()) {
      const size_t k = (size_t)draw() % pool.size();
      const int32_t sampled = pool[k];
      pool[k] = pool.back();
      pool.pop_back();
      ids.push_front(sampled);
    }
  }

  if (include_predecessor) ids.push_back(predecessor_id);  // :319-322
  *n_out = (int32_t)ids.size();
  if ((int32_t)ids.size() > capacity) return RGBDFE_ERR_CAPACITY;
  for (size_t i = 0; i < ids.size(); ++i) ids_out[i] = ids[i];
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

// ---- the optimiser's vertices and edges (the device work: api_pose_graph.hip) ----------------------------------------
namespace {
bool all_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!(v[i] - v[i] == 0.0)) return false;
  return true;
}
void pose_from_matrix(const double* m, double* est) {  // column-major 4x4 -> rotation row-major, translation
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) est[3 * r + c] = m[4 * c + r];
    est[9 + r] = m[12 + r];
  }
}
double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
}  // namespace

int rgbdfe_pose_graph_set_estimate(rgbdfe_pose_graph* g, int32_t node_id, const double* transform) try {
  if (!g || !transform || !all_finite(transform, 16)) return RGBDFE_ERR_INVALID_ARG;
  const auto a = g->nodes.find(node_id);
  if (a == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;
  pose_from_matrix(transform, a->second.est);
  return RGBDFE_OK;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_get_estimate(const rgbdfe_pose_graph* g, int32_t node_id, double* transform) try {
  if (!g || !transform) return RGBDFE_ERR_INVALID_ARG;
  const auto a = g->nodes.find(node_id);
  if (a == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;
  const double* est = a->second.est;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) transform[4 * c + r] = est[3 * r + c];
    transform[12 + r] = est[9 + r];
    transform[4 * r + 3] = 0.0;
  }
  transform[15] = 1.0;
  return RGBDFE_OK;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_set_fixed(rgbdfe_pose_graph* g, int32_t node_id, int32_t fixed) try {
  if (!g) return RGBDFE_ERR_INVALID_ARG;
  const auto a = g->nodes.find(node_id);
  if (a == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;
  a->second.fixed = fixed != 0;
  return RGBDFE_OK;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_add_edge_se3(rgbdfe_pose_graph* g, int32_t node_id1, int32_t node_id2, const double* transform,
                                   const double* information, int32_t set_estimate) try {
  if (!g || !transform || !information || node_id1 == node_id2 || !all_finite(transform, 16) || !all_finite(information, 36))
    return RGBDFE_ERR_INVALID_ARG;
  const auto a = g->nodes.find(node_id1), b = g->nodes.find(node_id2);
  if (a == g->nodes.end() || b == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;
  rgbdfe_pose_graph::MeasuredEdge m;
  m.id1 = node_id1;
  m.id2 = node_id2;
  pose_from_matrix(transform, m.z);
  for (int k = 0; k < 36; ++k) m.info[k] = information[k];
  g->edges.push_back(m);
  g->adjacency[a->second.vertex_id].insert(b->second.vertex_id);
  g->adjacency[b->second.vertex_id].insert(a->second.vertex_id);
  if (g->strategy == RGBDFE_POSE_RELATIVE_TO_INAFFECTED) {  // :889-892
    a->second.fixed = false;
    b->second.fixed = false;
  } else if (g->strategy == RGBDFE_POSE_RELATIVE_TO_LARGEST_LOOP) {  // :893-896
    g->earliest_loop_closure_node = std::min(g->earliest_loop_closure_node, std::min(node_id1, node_id2));
  }
  if (set_estimate) {  // X2 = X1 * Z (addEdgeToG2O, graph_manager.cpp:858,864)
    const double* x = a->second.est;
    double* y = b->second.est;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) y[3 * r + c] = dot3(x[3 * r], x[3 * r + 1], x[3 * r + 2], m.z[c], m.z[3 + c], m.z[6 + c]);
      y[9 + r] = dot3(x[3 * r], x[3 * r + 1], x[3 * r + 2], m.z[9], m.z[10], m.z[11]) + x[9 + r];
    }
  }
  return RGBDFE_OK;
} catch (const std::bad_alloc&) {
  return RGBDFE_ERR_OUT_OF_MEMORY;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_transforms(const rgbdfe_pose_graph* g, int32_t n, const int32_t* node_ids, float* out) try {
  if (!g || n < 0 || (n > 0 && (!node_ids || !out))) return RGBDFE_ERR_INVALID_ARG;
  for (int32_t i = 0; i < n; ++i)
    if (g->nodes.find(node_ids[i]) == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;  // before anything is written
  for (int32_t i = 0; i < n; ++i) {
    const double* est = g->nodes.find(node_ids[i])->second.est;
    float* m = out + 16 * (size_t)i;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) m[4 * c + r] = (float)est[3 * r + c];
      m[12 + r] = (float)est[9 + r];
      m[4 * r + 3] = 0.0f;
    }
    m[15] = 1.0f;
  }
  return RGBDFE_OK;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

// ---- fixation strategies, pruning helpers and the trajectory file (include/rgbdfe.h; the device work: api_pose_graph.hip) ---
int rgbdfe_pose_graph_set_strategy(rgbdfe_pose_graph* g, int32_t strategy) {
  if (!g || strategy < RGBDFE_POSE_RELATIVE_TO_NONE || strategy > RGBDFE_POSE_RELATIVE_TO_INAFFECTED) return RGBDFE_ERR_INVALID_ARG;
  g->strategy = strategy;
  return RGBDFE_OK;
}

int rgbdfe_pose_graph_get_fixed(const rgbdfe_pose_graph* g, int32_t node_id, int32_t* fixed) try {
  if (!g || !fixed) return RGBDFE_ERR_INVALID_ARG;
  const auto a = g->nodes.find(node_id);
  if (a == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;
  *fixed = a->second.fixed ? 1 : 0;
  return RGBDFE_OK;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

int rgbdfe_pose_graph_get_edge(const rgbdfe_pose_graph* g, int32_t index, int32_t* node_id1, int32_t* node_id2, double* transform,
                               double* information, int32_t* active) {
  if (!g || index < 0 || (size_t)index >= g->edges.size()) return RGBDFE_ERR_INVALID_ARG;
  const rgbdfe_pose_graph::MeasuredEdge& m = g->edges[(size_t)index];
  if (node_id1) *node_id1 = m.id1;
  if (node_id2) *node_id2 = m.id2;
  if (transform) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) transform[4 * c + r] = m.z[3 * r + c];
      transform[12 + r] = m.z[9 + r];
      transform[4 * r + 3] = 0.0;
    }
    transform[15] = 1.0;
  }
  if (information)
    for (int k = 0; k < 36; ++k) information[k] = m.info[k];
  if (active) *active = m.active ? 1 : 0;
  return RGBDFE_OK;
}

int rgbdfe_pose_graph_sanity_check(rgbdfe_pose_graph* g, float thresh) {
  if (!g || thresh != thresh) return RGBDFE_ERR_INVALID_ARG;
  thresh *= thresh;  // in float, as the reference's (graph_manager.cpp:1348)
  int changed = 0;
  for (rgbdfe_pose_graph::MeasuredEdge& m : g->edges) {
    if (!m.active) continue;
    const double sq = (m.z[9] * m.z[9] + m.z[10] * m.z[10]) + m.z[11] * m.z[11];
    if (sq > (double)thresh) {
      for (int k = 0; k < 36; ++k) m.info[k] = (k % 7 == 0) ? 0.000001 : 0.0;
      ++changed;
    }
  }
  return changed;
}

namespace {
// poses as est: rotation row-major [0..8], translation [9..11]
void pose_mul(const double* a, const double* b, double* out) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[3 * r + c] = dot3(a[3 * r], a[3 * r + 1], a[3 * r + 2], b[c], b[3 + c], b[6 + c]);
    out[9 + r] = dot3(a[3 * r], a[3 * r + 1], a[3 * r + 2], b[9], b[10], b[11]) + a[9 + r];
  }
}
// (x, y, z, w): the contract's matrix -> quaternion conversion (csrc/pose_graph.hip quat_from_rot)
void quat_from_rot(const double* R, double* q) {
  const double tr = (R[0] + R[4]) + R[8];
  double x, y, z, w;
  if (tr > 0.0) {
    double s = std::sqrt(tr + 1.0);
    w = 0.5 * s;
    s = 0.5 / s;
    x = (R[7] - R[5]) * s;
    y = (R[2] - R[6]) * s;
    z = (R[3] - R[1]) * s;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = std::sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0);
    double v[3];
    v[i] = 0.5 * s;
    s = 0.5 / s;
    w = (R[3 * k + j] - R[3 * j + k]) * s;
    v[j] = (R[3 * j + i] + R[3 * i + j]) * s;
    v[k] = (R[3 * k + i] + R[3 * i + k]) * s;
    x = v[0]; y = v[1]; z = v[2];
  }
  const double n = std::sqrt(((x * x + y * y) + z * z) + w * w);
  x = x / n; y = y / n; z = z / n; w = w / n;
  if (w < 0.0) { x = -x; y = -y; z = -z; w = -w; }
  q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}
}  // namespace

}  // extern "C"
void rgbdfe_host::quat_from_rot_xyzw(const double* R, double* q) { quat_from_rot(R, q); }   // the node cloud files' viewpoint
extern "C" {

int rgbdfe_pose_graph_write_trajectory(const rgbdfe_pose_graph* g, const char* path, int32_t n, const int32_t* node_ids,
                                       const double* timestamps, const double* base2points, const double* init_base_pose,
                                       const char* frame_id, const char* child_frame_id) try {
  if (!g || !path || n < 0 || (n > 0 && (!node_ids || !timestamps))) return RGBDFE_ERR_INVALID_ARG;
  if ((base2points && !all_finite(base2points, 16)) || (init_base_pose && !all_finite(init_base_pose, 16)))
    return RGBDFE_ERR_INVALID_ARG;
  for (int32_t i = 0; i < n; ++i)
    if (g->nodes.find(node_ids[i]) == g->nodes.end()) return RGBDFE_ERR_UNKNOWN_NODE;  // before anything is written
  const double ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  double b2p[12], init[12], inv[12], left[12];
  std::copy(ident, ident + 12, b2p);
  std::copy(ident, ident + 12, init);
  if (base2points) pose_from_matrix(base2points, b2p);
  if (init_base_pose) pose_from_matrix(init_base_pose, init);
  for (int r = 0; r < 3; ++r) {  // the rigid inverse: R', -R't
    for (int c = 0; c < 3; ++c) inv[3 * r + c] = b2p[3 * c + r];
    inv[9 + r] = -dot3(b2p[r], b2p[3 + r], b2p[6 + r], b2p[9], b2p[10], b2p[11]);
  }
  pose_mul(init, b2p, left);
  FILE* f = fopen(path, "w");
  if (!f) return RGBDFE_ERR_INVALID_ARG;
  bool ok = true;
  if (frame_id) ok = fprintf(f, "# TF Coordinate Frame ID: %s(data: %s)\n", frame_id, child_frame_id ? child_frame_id : "") >= 0;
  for (int32_t i = 0; i < n && ok; ++i) {
    double lx[12], w2b[12], q[4];
    pose_mul(left, g->nodes.find(node_ids[i])->second.est, lx);
    pose_mul(lx, inv, w2b);
    quat_from_rot(w2b, q);
    ok = fprintf(f, "%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n", timestamps[i], w2b[9], w2b[10], w2b[11], q[0], q[1], q[2], q[3]) >= 0;
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? RGBDFE_OK : RGBDFE_ERR_INTERNAL;
} catch (...) {
  return RGBDFE_ERR_INTERNAL;  // no exception crosses the C ABI
}

}  // extern "C"
