// session_format.h -- the bytes of a saved session (include/rgbdfe.h, "session files"): the pose graph's and the decision
// machine's byte strings, and the validation of a whole session file into a table of views.  Plain C++: no HIP headers, no
// device -- candidates.cpp, api_slam.hip, api_session.hip and tests/emu/session_main.cpp (under the sanitizers) include it.
// Everything is little-endian and is read and written through memcpy: no alignment is assumed of a caller's buffer, and
// doubles travel as their 8 bytes (NaN payloads, -0.0 and denormals survive).
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "rgbdfe.h"
#include "pose_graph_host.h"
#include "slam_machine.h"

namespace rgbdfe_session {

// the message of the latest failed call that has no context to leave it with, per calling thread: rgbdfe_last_error(NULL)
// (candidates.cpp holds the string)
std::string& contextless_error();

static_assert(sizeof(double) == 8 && sizeof(float) == 4, "IEEE-754 binary64 / binary32");

// ---- CRC-32 with zlib's polynomial (reflected 0xEDB88320, initial value and final xor 0xFFFFFFFF): zlib.crc32's value
inline uint32_t crc32(const uint8_t* p, size_t n) {
  static const struct Table {
    uint32_t t[256];
    Table() {
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
        t[i] = c;
      }
    }
  } table;
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = table.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

struct Writer {
  std::vector<uint8_t> b;
  template <class T> void put(T v) { const size_t at = b.size(); b.resize(at + sizeof(T)); std::memcpy(b.data() + at, &v, sizeof(T)); }
  void bytes(const void* p, size_t n) { if (n) { const size_t at = b.size(); b.resize(at + n); std::memcpy(b.data() + at, p, n); } }
  void zeros(size_t n) { b.resize(b.size() + n, 0); }
  void pad8() { zeros((8 - b.size() % 8) % 8); }
  template <class T> void set(size_t at, T v) { std::memcpy(b.data() + at, &v, sizeof(T)); }
};

// a bounds-checked cursor: every get past the end sets `ok` to false and yields zeros
struct Reader {
  const uint8_t* p;
  size_t n, at = 0;
  bool ok = true;
  Reader(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
  size_t left() const { return n - at; }
  template <class T> T get() {
    T v{};
    if (!ok || left() < sizeof(T)) { ok = false; return v; }
    std::memcpy(&v, p + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  const uint8_t* take(size_t bytes) {   // NULL when the bytes are not there
    if (!ok || left() < bytes) { ok = false; return nullptr; }
    const uint8_t* r = p + at;
    at += bytes;
    return r;
  }
  bool skip_pad8() {   // the padding is zeros
    while (ok && at % 8 != 0) if (get<uint8_t>() != 0) ok = false;
    return ok;
  }
};

// ---- the envelope of the two byte strings: 8 bytes magic, u32 version 1, u32 CRC-32 of the bytes [16, length),
// u64 length of the whole string (a multiple of 8), then the body
constexpr uint32_t kStringVersion = 1;
constexpr size_t kEnvelope = 24;
inline void begin_string(Writer& w, const char magic[8]) { w.bytes(magic, 8); w.put<uint32_t>(kStringVersion); w.put<uint32_t>(0); w.put<uint64_t>(0); }
inline void end_string(Writer& w) {
  w.pad8();
  w.set<uint64_t>(16, (uint64_t)w.b.size());
  w.set<uint32_t>(12, crc32(w.b.data() + 16, w.b.size() - 16));
}
// "" when [p, p + n) is one whole string with this magic, else what is wrong with it
inline std::string check_string(const uint8_t* p, size_t n, const char magic[8], const char* what) {
  const std::string w(what);
  if (!p || n < kEnvelope) return w + ": shorter than its header";
  if (std::memcmp(p, magic, 8) != 0) return w + ": wrong magic";
  uint32_t version, crc;
  uint64_t length;
  std::memcpy(&version, p + 8, 4); std::memcpy(&crc, p + 12, 4); std::memcpy(&length, p + 16, 8);
  if (version != kStringVersion) return w + ": unknown version";
  if (length != (uint64_t)n || n % 8 != 0) return w + ": the length field differs from the bytes given";
  if (crc32(p + 16, n - 16) != crc) return w + ": CRC mismatch";
  return "";
}

// ---- the pose graph ----------------------------------------------------------------------------------------------------
// body: i32 strategy, i32 earliest_loop_closure_node, u32 n_nodes, u32 n_edges, u32 n_keyframes, u32 n_links,
//       u32 n_extra_vertices, u32 0
//   nodes (ascending id), 112 bytes each: i32 node id, i32 vertex id, u8 matchable, u8 fixed, 6 x u8 0, 12 x f64 estimate
//     (rotation row-major, then translation)
//   edges (insertion order), 400 bytes each: i32 id1, i32 id2, u8 active, 7 x u8 0, 12 x f64 z, 36 x f64 information
//   keyframes: n x i32;  links: n x (i32 u, i32 v), u < v ascending: the topology-only edges (rgbdfe_pose_graph_add_edge)
//     as vertex ids;  extra vertices: n x i32 ascending: camera vertices that are no node's vertex id;  zeros to 8 bytes.
// camera_vertices and adjacency are not stored: they are rebuilt from the nodes' vertex ids, the measured edges, the links and
// the extra vertices.
constexpr char kGraphMagic[9] = "RGBDFEPG";
constexpr size_t kGraphNodeBytes = 112, kGraphEdgeBytes = 400;

typedef std::set<std::pair<int32_t, int32_t>> LinkSet;
inline void implied_topology(const rgbdfe_pose_graph& g, std::set<int32_t>& vertices, LinkSet& links) {
  for (const auto& kv : g.nodes) vertices.insert(kv.second.vertex_id);
  for (const auto& m : g.edges) {
    const auto a = g.nodes.find(m.id1), b = g.nodes.find(m.id2);
    if (a == g.nodes.end() || b == g.nodes.end()) continue;
    const int32_t u = a->second.vertex_id, v = b->second.vertex_id;
    links.insert(u < v ? std::make_pair(u, v) : std::make_pair(v, u));
  }
}

// RGBDFE_ERR_INVALID_ARG (with `err`): the graph's topology is not what its nodes and edges imply plus additions, which
// happens only when a node was added again under another vertex id after edges had been added
inline int graph_serialize(const rgbdfe_pose_graph& g, std::vector<uint8_t>& out, std::string& err) {
  std::set<int32_t> vertices;
  LinkSet implied, actual;
  implied_topology(g, vertices, implied);
  for (const auto& kv : g.adjacency)
    for (int32_t v : kv.second)
      if (kv.first < v) actual.insert(std::make_pair(kv.first, v));
  std::vector<std::pair<int32_t, int32_t>> links;
  for (const auto& l : actual) if (!implied.count(l)) links.push_back(l);
  std::vector<int32_t> extra;
  for (int32_t v : g.camera_vertices) if (!vertices.count(v)) extra.push_back(v);
  bool rebuildable = true;
  for (const auto& l : implied) rebuildable &= actual.count(l) != 0;
  for (int32_t v : vertices) rebuildable &= g.camera_vertices.count(v) != 0 && g.adjacency.count(v) != 0;
  for (const auto& kv : g.adjacency) {
    rebuildable &= g.camera_vertices.count(kv.first) != 0;
    for (int32_t v : kv.second) rebuildable &= g.adjacency.count(v) != 0 && g.adjacency.find(v)->second.count(kv.first) != 0;
  }
  if (!rebuildable) { err = "pose graph: a node's vertex id changed after edges were added: not serialisable"; return RGBDFE_ERR_INVALID_ARG; }
  Writer w;
  begin_string(w, kGraphMagic);
  w.put<int32_t>(g.strategy); w.put<int32_t>(g.earliest_loop_closure_node);
  w.put<uint32_t>((uint32_t)g.nodes.size()); w.put<uint32_t>((uint32_t)g.edges.size()); w.put<uint32_t>((uint32_t)g.keyframes.size());
  w.put<uint32_t>((uint32_t)links.size()); w.put<uint32_t>((uint32_t)extra.size()); w.put<uint32_t>(0);
  for (const auto& kv : g.nodes) {
    w.put<int32_t>(kv.first); w.put<int32_t>(kv.second.vertex_id);
    w.put<uint8_t>(kv.second.matchable ? 1 : 0); w.put<uint8_t>(kv.second.fixed ? 1 : 0); w.zeros(6);
    w.bytes(kv.second.est, sizeof(kv.second.est));
  }
  for (const auto& m : g.edges) {
    w.put<int32_t>(m.id1); w.put<int32_t>(m.id2); w.put<uint8_t>(m.active ? 1 : 0); w.zeros(7);
    w.bytes(m.z, sizeof(m.z)); w.bytes(m.info, sizeof(m.info));
  }
  for (int32_t k : g.keyframes) w.put<int32_t>(k);
  for (const auto& l : links) { w.put<int32_t>(l.first); w.put<int32_t>(l.second); }
  for (int32_t v : extra) w.put<int32_t>(v);
  end_string(w);
  out.swap(w.b);
  return RGBDFE_OK;
}

struct GraphImage {   // a byte string parsed and checked, not yet anybody's graph
  int32_t strategy = 0, earliest = 0;
  std::map<int32_t, rgbdfe_pose_graph::NodeInfo> nodes;
  std::vector<rgbdfe_pose_graph::MeasuredEdge> edges;
  std::vector<int32_t> keyframes, extra;
  std::vector<std::pair<int32_t, int32_t>> links;
};

// "" or what is wrong; the whole string is checked before `img` means anything
inline std::string graph_parse(const uint8_t* p, size_t n, GraphImage& img) {
  const std::string e = check_string(p, n, kGraphMagic, "pose graph");
  if (!e.empty()) return e;
  Reader r(p + kEnvelope, n - kEnvelope);
  img.strategy = r.get<int32_t>(); img.earliest = r.get<int32_t>();
  const uint32_t n_nodes = r.get<uint32_t>(), n_edges = r.get<uint32_t>(), n_kf = r.get<uint32_t>(), n_links = r.get<uint32_t>(),
                 n_extra = r.get<uint32_t>(), zero = r.get<uint32_t>();
  if (!r.ok || zero != 0) return "pose graph: bad counts";
  const uint64_t need = (uint64_t)n_nodes * kGraphNodeBytes + (uint64_t)n_edges * kGraphEdgeBytes + 4ull * n_kf + 8ull * n_links + 4ull * n_extra;
  if (need > r.left() || r.left() - need >= 8) return "pose graph: the counts do not fit the length";
  if (img.strategy < RGBDFE_POSE_RELATIVE_TO_NONE || img.strategy > RGBDFE_POSE_RELATIVE_TO_INAFFECTED) return "pose graph: unknown strategy";
  int64_t last = -1;
  for (uint32_t i = 0; i < n_nodes; ++i) {
    const int32_t id = r.get<int32_t>();
    rgbdfe_pose_graph::NodeInfo nd;
    nd.vertex_id = r.get<int32_t>();
    const uint8_t matchable = r.get<uint8_t>(), fixed = r.get<uint8_t>();
    uint8_t pad = 0;
    for (int k = 0; k < 6; ++k) pad |= r.get<uint8_t>();
    if (id <= last || nd.vertex_id < 0 || matchable > 1 || fixed > 1 || pad) return "pose graph: bad node record";
    last = id;
    nd.matchable = matchable != 0; nd.fixed = fixed != 0;
    for (double& v : nd.est) v = r.get<double>();
    img.nodes[id] = nd;
  }
  img.edges.resize(n_edges);
  for (auto& m : img.edges) {
    m.id1 = r.get<int32_t>(); m.id2 = r.get<int32_t>();
    const uint8_t active = r.get<uint8_t>();
    uint8_t pad = 0;
    for (int k = 0; k < 7; ++k) pad |= r.get<uint8_t>();
    if (m.id1 == m.id2 || !img.nodes.count(m.id1) || !img.nodes.count(m.id2) || active > 1 || pad) return "pose graph: bad edge record";
    m.active = active != 0;
    for (double& v : m.z) v = r.get<double>();
    for (double& v : m.info) v = r.get<double>();
  }
  for (uint32_t i = 0; i < n_kf; ++i) {
    img.keyframes.push_back(r.get<int32_t>());
    if (!img.nodes.count(img.keyframes.back())) return "pose graph: a keyframe that is no node";
  }
  for (uint32_t i = 0; i < n_links; ++i) {
    const int32_t u = r.get<int32_t>(), v = r.get<int32_t>();
    if (u < 0 || u >= v || (!img.links.empty() && !(img.links.back() < std::make_pair(u, v)))) return "pose graph: bad link";
    img.links.push_back(std::make_pair(u, v));
  }
  for (uint32_t i = 0; i < n_extra; ++i) {
    const int32_t v = r.get<int32_t>();
    if (v < 0 || (!img.extra.empty() && img.extra.back() >= v)) return "pose graph: bad extra vertex";
    img.extra.push_back(v);
  }
  if (!r.skip_pad8() || r.left() != 0) return "pose graph: trailing bytes";
  return "";
}

inline bool graph_is_empty(const rgbdfe_pose_graph& g) {
  return g.nodes.empty() && g.edges.empty() && g.keyframes.empty() && g.camera_vertices.empty() && g.adjacency.empty();
}

// the image becomes the (empty) graph's content; the optimiser's device buffers go, so that no stale plan survives
inline void graph_commit(rgbdfe_pose_graph& g, GraphImage& img) {
  if (g.device && g.device_free) g.device_free(g.device);
  g.device = nullptr;
  g.strategy = img.strategy;
  g.earliest_loop_closure_node = img.earliest;
  g.nodes.swap(img.nodes);
  g.edges.swap(img.edges);
  g.keyframes.assign(img.keyframes.begin(), img.keyframes.end());
  std::set<int32_t> vertices;
  LinkSet links;
  implied_topology(g, vertices, links);
  links.insert(img.links.begin(), img.links.end());
  vertices.insert(img.extra.begin(), img.extra.end());
  for (const auto& l : links) { vertices.insert(l.first); vertices.insert(l.second); }
  for (int32_t v : vertices) { g.camera_vertices.insert(v); g.adjacency[v]; }
  for (const auto& l : links) { g.adjacency[l.first].insert(l.second); g.adjacency[l.second].insert(l.first); }
}

// ---- the decision machine ----------------------------------------------------------------------------------------------
// body: the parameters in the order of rgbdfe_slam_params (14 x i32 with the u32 seed last of them, 6 x f64, 16 x f64
//   init_base_pose), u32 n_nodes, u32 n_keyframes, i32 next_seq_id, u32 calls, i32 sequential_edges, i32 loop_closure_edges,
//   i32 best_id1, i32 best_id2, i32 best_n_inl, u32 0, then per graph id: n x i32 slot_of, n x i32 rows, n x i64 stamp_sec,
//   n x i32 stamp_nsec, n x u8 valid_tf, zeros to 4 bytes, keyframes n x i32, zeros to 8 bytes.
// A caller's generator (rgbdfe_slam_set_rand) and its state are the caller's: not part of the string.
constexpr char kSlamMagic[9] = "RGBDFESM";

#define RGBDFE_SLAM_PARAM_I32(X) \
  X(min_matches) X(predecessor_candidates) X(neighbor_candidates) X(min_sampled_candidates) X(geodesic_depth) \
  X(keep_all_nodes) X(keep_good_nodes) X(clear_non_keyframes) X(create_cloud_every_nth_node) X(optimizer_skip_step) \
  X(use_icp) X(emm__skip_step) X(have_odometry_frame)
#define RGBDFE_SLAM_PARAM_F64(X) \
  X(min_translation_meter) X(min_rotation_degree) X(max_translation_meter) X(max_rotation_degree) X(optimizer_iterations) \
  X(observability_threshold)

inline void slam_put_params(Writer& w, const rgbdfe_slam_params& p) {
#define X(f) w.put<int32_t>(p.f);
  RGBDFE_SLAM_PARAM_I32(X)
#undef X
  w.put<uint32_t>(p.seed);
#define X(f) w.put<double>(p.f);
  RGBDFE_SLAM_PARAM_F64(X)
#undef X
  w.bytes(p.init_base_pose, sizeof(p.init_base_pose));
}
inline void slam_get_params(Reader& r, rgbdfe_slam_params& p) {
#define X(f) p.f = r.get<int32_t>();
  RGBDFE_SLAM_PARAM_I32(X)
#undef X
  p.seed = r.get<uint32_t>();
#define X(f) p.f = r.get<double>();
  RGBDFE_SLAM_PARAM_F64(X)
#undef X
  for (double& v : p.init_base_pose) v = r.get<double>();
}
// the first field in which two parameter sets differ (doubles by their bytes), or NULL
inline const char* slam_params_differ(const rgbdfe_slam_params& a, const rgbdfe_slam_params& b) {
#define X(f) if (a.f != b.f) return #f;
  RGBDFE_SLAM_PARAM_I32(X)
#undef X
  if (a.seed != b.seed) return "seed";
#define X(f) if (std::memcmp(&a.f, &b.f, 8) != 0) return #f;
  RGBDFE_SLAM_PARAM_F64(X)
#undef X
  if (std::memcmp(a.init_base_pose, b.init_base_pose, sizeof(a.init_base_pose)) != 0) return "init_base_pose";
  return nullptr;
}

// a machine between two steps (the caller refuses phase != kIdle)
inline void slam_serialize(const rgbdfe_slam_machine::Machine& m, std::vector<uint8_t>& out) {
  Writer w;
  begin_string(w, kSlamMagic);
  slam_put_params(w, m.prm);
  w.put<uint32_t>((uint32_t)m.slot_of.size()); w.put<uint32_t>((uint32_t)m.keyframes.size());
  w.put<int32_t>(m.next_seq_id); w.put<uint32_t>(m.calls); w.put<int32_t>(m.sequential_edges); w.put<int32_t>(m.loop_closure_edges);
  w.put<int32_t>(m.best_id1); w.put<int32_t>(m.best_id2); w.put<int32_t>(m.best_n_inl); w.put<uint32_t>(0);
  for (int32_t v : m.slot_of) w.put<int32_t>(v);
  for (int32_t v : m.rows) w.put<int32_t>(v);
  for (int64_t v : m.stamp_sec) w.put<int64_t>(v);
  for (int32_t v : m.stamp_nsec) w.put<int32_t>(v);
  for (uint8_t v : m.valid_tf) w.put<uint8_t>(v);
  w.zeros((4 - w.b.size() % 4) % 4);
  for (int32_t v : m.keyframes) w.put<int32_t>(v);
  end_string(w);
  out.swap(w.b);
}

struct SlamImage {
  rgbdfe_slam_params prm{};
  std::vector<int32_t> slot_of, rows, stamp_nsec, keyframes;
  std::vector<int64_t> stamp_sec;
  std::vector<uint8_t> valid_tf;
  int32_t next_seq_id = 0, sequential_edges = 0, loop_closure_edges = 0, best_id1 = -1, best_id2 = -1, best_n_inl = 0;
  uint32_t calls = 0;
};

inline std::string slam_parse(const uint8_t* p, size_t n, SlamImage& img) {
  const std::string e = check_string(p, n, kSlamMagic, "slam state");
  if (!e.empty()) return e;
  Reader r(p + kEnvelope, n - kEnvelope);
  slam_get_params(r, img.prm);
  const uint32_t n_nodes = r.get<uint32_t>(), n_kf = r.get<uint32_t>();
  img.next_seq_id = r.get<int32_t>(); img.calls = r.get<uint32_t>();
  img.sequential_edges = r.get<int32_t>(); img.loop_closure_edges = r.get<int32_t>();
  img.best_id1 = r.get<int32_t>(); img.best_id2 = r.get<int32_t>(); img.best_n_inl = r.get<int32_t>();
  const uint32_t zero = r.get<uint32_t>();
  if (!r.ok || zero != 0) return "slam state: bad counts";
  const uint64_t arrays = 21ull * n_nodes, need = (arrays + 3) / 4 * 4 + 4ull * n_kf;
  if (need > r.left() || r.left() - need >= 8) return "slam state: the counts do not fit the length";
  img.slot_of.resize(n_nodes); img.rows.resize(n_nodes); img.stamp_sec.resize(n_nodes); img.stamp_nsec.resize(n_nodes);
  img.valid_tf.resize(n_nodes); img.keyframes.resize(n_kf);
  for (auto& v : img.slot_of) v = r.get<int32_t>();
  for (auto& v : img.rows) v = r.get<int32_t>();
  for (auto& v : img.stamp_sec) v = r.get<int64_t>();
  for (auto& v : img.stamp_nsec) v = r.get<int32_t>();
  for (auto& v : img.valid_tf) { v = r.get<uint8_t>(); if (v > 1) return "slam state: bad valid_tf"; }
  while (r.ok && r.at % 4 != 0) if (r.get<uint8_t>() != 0) return "slam state: bad padding";
  for (auto& v : img.keyframes) { v = r.get<int32_t>(); if (v < 0 || (uint32_t)v >= n_nodes) return "slam state: a keyframe that is no node"; }
  for (int32_t v : img.rows) if (v < 0) return "slam state: negative rows";
  if (!r.skip_pad8() || r.left() != 0) return "slam state: trailing bytes";
  if (n_nodes > 0 && n_kf == 0) return "slam state: nodes without a keyframe";   // firstNode declares one; conclude reads keyframes.back()
  return "";
}

inline bool slam_is_fresh(const rgbdfe_slam_machine::Machine& m) {
  return m.phase == rgbdfe_slam_machine::Machine::kIdle && m.slot_of.empty() && m.keyframes.empty();
}

inline void slam_commit(rgbdfe_slam_machine::Machine& m, SlamImage& img) {
  m.slot_of.swap(img.slot_of); m.rows.swap(img.rows); m.stamp_sec.swap(img.stamp_sec); m.stamp_nsec.swap(img.stamp_nsec);
  m.valid_tf.swap(img.valid_tf); m.keyframes.swap(img.keyframes);
  m.next_seq_id = img.next_seq_id; m.calls = img.calls;
  m.sequential_edges = img.sequential_edges; m.loop_closure_edges = img.loop_closure_edges;
  m.best_id1 = img.best_id1; m.best_id2 = img.best_id2; m.best_n_inl = img.best_n_inl;
  m.phase = rgbdfe_slam_machine::Machine::kIdle;
  m.pending.clear();
  m.to_release.clear();
}

// ---- the session file --------------------------------------------------------------------------------------------------
// header (32 bytes): "RGBDFESS", u32 version 1, u32 flags, u64 file length, u64 0
// chunks: 4-byte tag, u32 CRC-32 of the payload (padding excluded), u64 payload length, payload, zeros to 8 bytes;
//   order CONF, DETE, NODE, [CLOU], [GRPH], [SLAM], "END " (empty); the payloads: include/rgbdfe.h
constexpr char kFileMagic[9] = "RGBDFESS";
constexpr uint32_t kFileVersion = 1;
constexpr size_t kFileHeader = 32, kChunkHeader = 16;
constexpr int kChunks = 7;
constexpr const char* kChunkTags[kChunks] = {"CONF", "DETE", "NODE", "CLOU", "GRPH", "SLAM", "END "};
enum { kConf = 0, kDete = 1, kNode = 2, kClou = 3, kGrph = 4, kSlam = 5, kEnd = 6 };

inline void begin_file(Writer& w, uint32_t flags) {
  w.bytes(kFileMagic, 8); w.put<uint32_t>(kFileVersion); w.put<uint32_t>(flags); w.put<uint64_t>(0); w.put<uint64_t>(0);
}
inline void put_chunk(Writer& w, int which, const std::vector<uint8_t>& payload) {
  w.bytes(kChunkTags[which], 4);
  w.put<uint32_t>(crc32(payload.data(), payload.size()));
  w.put<uint64_t>((uint64_t)payload.size());
  w.bytes(payload.data(), payload.size());
  w.pad8();
}
inline void end_file(Writer& w) {
  put_chunk(w, kEnd, std::vector<uint8_t>());
  w.set<uint64_t>(16, (uint64_t)w.b.size());
}

struct View { const uint8_t* p = nullptr; size_t n = 0; bool present = false; };

struct NodeGroup {            // the nodes of one kind, ascending id, and their packed arrays
  std::vector<int32_t> ids, rows, has_kp;
  const uint8_t* desc = nullptr; const uint8_t* xyz = nullptr; const uint8_t* kp = nullptr; const uint8_t* stats = nullptr;
  uint64_t total = 0;
};
struct CloudView { int32_t id, ch, cw, cloud_skip; float fx, fy, cx, cy; const uint8_t* points; };

struct SessionView {
  uint32_t flags = 0;
  View chunk[kChunks];
  // CONF
  int32_t max_keypoints = 0, abi_version = 0;
  uint32_t kinds_present = 0;
  // DETE
  int32_t detector_type = 0, detector_max_keypoints = 0, grid = 0, adjuster_iters = 0, feature_min_depth = 0, n_cells = 0;
  double thresholds[64] = {};
  // NODE
  std::vector<int32_t> ids, kinds, rows, has_kp;   // ascending id
  NodeGroup group[3];
  int32_t max_rows = 0;
  // CLOU
  std::vector<CloudView> clouds;
};

// The whole file is checked -- magic, version, length, the chunk table, every CRC, every count against its chunk's length,
// the two byte strings -- before `v` means anything.  "" or the cause.  The views point into [p, p + n).
inline std::string session_parse(const uint8_t* p, size_t n, SessionView& v) {
  if (!p || n < kFileHeader) return "session file: shorter than its header";
  if (std::memcmp(p, kFileMagic, 8) != 0) return "session file: wrong magic";
  Reader h(p + 8, kFileHeader - 8);
  const uint32_t version = h.get<uint32_t>();
  v.flags = h.get<uint32_t>();
  const uint64_t length = h.get<uint64_t>(), zero = h.get<uint64_t>();
  if (version != kFileVersion) return "session file: unknown version";
  if (length != (uint64_t)n) return "session file: the length field differs from the file's length";
  if (zero != 0 || (v.flags & ~(uint32_t)RGBDFE_SESSION_CLOUDS)) return "session file: bad header";
  size_t at = kFileHeader;
  int next = 0;
  bool ended = false;
  while (!ended) {
    if (n - at < kChunkHeader) return "session file: truncated chunk table";
    int which = -1;
    for (int k = next; k < kChunks; ++k) if (std::memcmp(p + at, kChunkTags[k], 4) == 0) { which = k; break; }
    if (which < 0) return "session file: unknown chunk tag or chunks out of order";
    uint32_t crc;
    uint64_t bytes;
    std::memcpy(&crc, p + at + 4, 4); std::memcpy(&bytes, p + at + 8, 8);
    at += kChunkHeader;
    if (bytes > n - at) return std::string("session file: chunk ") + kChunkTags[which] + " is longer than the file";
    if (crc32(p + at, (size_t)bytes) != crc) return std::string("session file: CRC mismatch in chunk ") + kChunkTags[which];
    v.chunk[which].p = p + at; v.chunk[which].n = (size_t)bytes; v.chunk[which].present = true;
    at += (size_t)bytes;
    while (at % 8 != 0) { if (at >= n || p[at] != 0) return "session file: bad chunk padding"; ++at; }
    next = which + 1;
    ended = which == kEnd;
  }
  if (at != n) return "session file: bytes behind the END chunk";
  if (v.chunk[kEnd].n != 0) return "session file: the END chunk is not empty";
  if (!v.chunk[kConf].present || !v.chunk[kDete].present || !v.chunk[kNode].present) return "session file: a mandatory chunk is missing";
  if (v.chunk[kClou].present != ((v.flags & RGBDFE_SESSION_CLOUDS) != 0)) return "session file: the CLOU chunk and the flags disagree";
  {
    Reader r(v.chunk[kConf].p, v.chunk[kConf].n);
    v.max_keypoints = r.get<int32_t>(); v.abi_version = r.get<int32_t>(); v.kinds_present = r.get<uint32_t>();
    const uint32_t z = r.get<uint32_t>();
    if (!r.ok || r.left() != 0 || z != 0 || v.max_keypoints < 1 || v.kinds_present > 7u) return "session file: bad CONF chunk";
  }
  {
    Reader r(v.chunk[kDete].p, v.chunk[kDete].n);
    v.detector_type = r.get<int32_t>(); v.detector_max_keypoints = r.get<int32_t>(); v.grid = r.get<int32_t>();
    v.adjuster_iters = r.get<int32_t>(); v.feature_min_depth = r.get<int32_t>(); v.n_cells = r.get<int32_t>();
    if (!r.ok || v.grid < 1 || v.grid > 8 || v.n_cells != v.grid * v.grid || v.detector_max_keypoints < 1 || v.adjuster_iters < 1 ||
        (v.detector_type != RGBDFE_DETECTOR_ORB && v.detector_type != RGBDFE_DETECTOR_FAST) || (v.feature_min_depth & ~1) ||
        r.left() != 8u * (size_t)v.n_cells)
      return "session file: bad DETE chunk";
    for (int i = 0; i < v.n_cells; ++i) {
      v.thresholds[i] = r.get<double>();
      if (!(v.thresholds[i] - v.thresholds[i] == 0.0)) return "session file: a detector threshold is not finite";
    }
  }
  {
    Reader r(v.chunk[kNode].p, v.chunk[kNode].n);
    const uint32_t count = r.get<uint32_t>(), z = r.get<uint32_t>();
    if (!r.ok || z != 0 || 16ull * count > r.left()) return "session file: bad NODE chunk (count)";
    v.ids.resize(count); v.kinds.resize(count); v.rows.resize(count); v.has_kp.resize(count);
    for (auto& x : v.ids) x = r.get<int32_t>();
    for (auto& x : v.kinds) x = r.get<int32_t>();
    for (auto& x : v.rows) x = r.get<int32_t>();
    for (auto& x : v.has_kp) x = r.get<int32_t>();
    uint32_t kinds_seen = 0;
    for (uint32_t i = 0; i < count; ++i) {
      if ((i > 0 && v.ids[i] <= v.ids[i - 1]) || v.kinds[i] < 0 || v.kinds[i] > 2 || v.rows[i] < 0 || (v.has_kp[i] & ~1))
        return "session file: bad NODE chunk (a node's record)";
      if (v.rows[i] > v.max_keypoints) return "session file: a node has more rows than the CONF chunk's max_keypoints";
      kinds_seen |= 1u << v.kinds[i];
      NodeGroup& g = v.group[v.kinds[i]];
      g.ids.push_back(v.ids[i]); g.rows.push_back(v.rows[i]); g.has_kp.push_back(v.has_kp[i]);
      g.total += (uint64_t)v.rows[i];
      v.max_rows = v.rows[i] > v.max_rows ? v.rows[i] : v.max_rows;
    }
    if (kinds_seen != v.kinds_present) return "session file: the CONF chunk's node kinds differ from the NODE chunk's";
    for (int k = 0; k < 3; ++k) {
      NodeGroup& g = v.group[k];
      if (g.ids.empty()) continue;
      const uint64_t widths[4] = {k == 0 ? 32ull : 512ull, 16, 8, 1};
      const uint8_t** dst[4] = {&g.desc, &g.xyz, &g.kp, &g.stats};
      for (int a = 0; a < 4; ++a) {
        if (g.total * widths[a] > r.left()) return "session file: bad NODE chunk (the arrays are shorter than the rows)";
        *dst[a] = r.take((size_t)(g.total * widths[a]));
        if (!r.skip_pad8()) return "session file: bad NODE chunk (padding)";
      }
    }
    if (!r.ok || r.left() != 0) return "session file: bad NODE chunk (length)";
  }
  if (v.chunk[kClou].present) {
    Reader r(v.chunk[kClou].p, v.chunk[kClou].n);
    const uint32_t count = r.get<uint32_t>(), z = r.get<uint32_t>();
    if (!r.ok || z != 0 || 32ull * count > r.left()) return "session file: bad CLOU chunk (count)";
    for (uint32_t i = 0; i < count; ++i) {
      CloudView c{};
      c.id = r.get<int32_t>(); c.ch = r.get<int32_t>(); c.cw = r.get<int32_t>(); c.cloud_skip = r.get<int32_t>();
      c.fx = r.get<float>(); c.fy = r.get<float>(); c.cx = r.get<float>(); c.cy = r.get<float>();
      if (!r.ok || c.ch < 1 || c.cw < 0 || c.cloud_skip < 1 || (!v.clouds.empty() && v.clouds.back().id >= c.id))
        return "session file: bad CLOU chunk (a cloud's record)";
      const uint64_t bytes = 16ull * (uint64_t)c.ch * (uint64_t)c.cw;
      if (bytes > r.left()) return "session file: bad CLOU chunk (the points are shorter than rows x cols)";
      c.points = r.take((size_t)bytes);
      v.clouds.push_back(c);
    }
    if (!r.ok || r.left() != 0) return "session file: bad CLOU chunk (length)";
  }
  if (v.chunk[kGrph].present) {
    GraphImage img;
    const std::string e = graph_parse(v.chunk[kGrph].p, v.chunk[kGrph].n, img);
    if (!e.empty()) return "session file: GRPH chunk: " + e;
  }
  if (v.chunk[kSlam].present) {
    SlamImage img;
    const std::string e = slam_parse(v.chunk[kSlam].p, v.chunk[kSlam].n, img);
    if (!e.empty()) return "session file: SLAM chunk: " + e;
  }
  return "";
}

}  // namespace rgbdfe_session
