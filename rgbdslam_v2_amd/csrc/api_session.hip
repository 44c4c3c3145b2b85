// api_session.hip -- what leaves a context and what goes back in (include/rgbdfe.h, "node read-back" and "session files"):
// resident nodes as the rows they were uploaded with (the pack kernel: session.hip), the setters a restore needs for state no
// upload carries (a node's feature_matching_stats_, the grid detector's thresholds, a resident cloud from its points), and
// rgbdfe_session_save / rgbdfe_session_load over them and the byte strings of session_format.h.
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"
#include "session.h"
#include "session_format.h"

namespace impl {

// The mirror image of rgbdfe_upload_nodes: one table upload, ONE launch of node_pack_kernel into the context's staging
// buffer, one device-to-host copy per array the caller asked for and one wait -- none of them grows with n_nodes.
static int download_nodes_common(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc, float* xyz1,
                                 float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds, bool copy_loop) {
  if (!ctx || n_nodes < 0 || capacity_rows < 0 || (n_nodes > 0 && !node_ids))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad read-back arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->node_pack_launches = ctx->node_pack_copies = 0;
  std::vector<rgbdfe::NodePackEntry> table((size_t)n_nodes);
  uint64_t total = 0;
  uint32_t kind = 0, max_rows = 0;
  for (int32_t i = 0; i < n_nodes; ++i) {   // every id is checked before any device work
    const auto it = ctx->nodes.find(node_ids[i]);
    if (it == ctx->nodes.end()) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "read-back of a node that is not resident");
    const NodeEntry& e = it->second;
    if (i == 0) kind = e.kind;
    else if (e.kind != kind) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "read-back of nodes of different kinds in one call");
    table[(size_t)i] = rgbdfe::NodePackEntry{e.slot, e.n, (uint32_t)total, (e.flags & kNodeHasKeypoints) ? 1u : 0u};
    total += e.n;
    max_rows = std::max(max_rows, e.n);
  }
  if (total > (uint64_t)UINT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "read-back of more than 2^32 - 1 rows in one call");
  if ((uint64_t)capacity_rows < total) {
    if (row_offsets) row_offsets[n_nodes] = (int64_t)total;
    return fail(ctx, RGBDFE_ERR_CAPACITY, "read-back: capacity_rows below the nodes' rows (row_offsets[n_nodes] holds them)");
  }
  for (int32_t i = 0; i < n_nodes; ++i) {
    if (row_offsets) row_offsets[i] = (int64_t)table[(size_t)i].first_row;
    if (kinds) kinds[i] = (int32_t)kind | (table[(size_t)i].has_kp ? RGBDFE_NODE_HAS_KEYPOINTS : 0);
  }
  if (row_offsets) row_offsets[n_nodes] = (int64_t)total;
  if (total == 0 || (!desc && !xyz1 && !kp_xy && !stats)) return RGBDFE_OK;

  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  if (const int rc = wait_for_pair_lanes(ctx)) return rc;   // as overwriting a node does
  if (ctx->nodes_ready) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->nodes_ready, 0));   // rgbdfe_upload_node_device
  const size_t desc_row = kind == 0u ? 32 : 512;
  if (copy_loop) {   // the baseline of tools/bench_session.py: per node one copy per array straight out of the slabs, one wait
    const uint8_t* d_desc = kind == 0u ? reinterpret_cast<const uint8_t*>(ctx->d_desc) : reinterpret_cast<const uint8_t*>(ctx->d_sift_f32);
    if (kp_xy) memset(kp_xy, 0, (size_t)total * 8);
    if (stats) memset(stats, 0, (size_t)total);
    for (const rgbdfe::NodePackEntry& e : table) {
      if (e.rows == 0) continue;
      const size_t src = (size_t)e.slot * (size_t)ctx->cfg.max_keypoints, dst = e.first_row, n = e.rows;
      if (desc) { HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(desc) + dst * desc_row, d_desc + src * desc_row, n * desc_row, hipMemcpyDeviceToHost, ctx->stream)); ++ctx->node_pack_copies; }
      if (xyz1) { HIP_TRY(ctx, hipMemcpyAsync(xyz1 + dst * 4, ctx->d_xyz + src, n * 16, hipMemcpyDeviceToHost, ctx->stream)); ++ctx->node_pack_copies; }
      if (kp_xy && ctx->d_kp2d && e.has_kp) { HIP_TRY(ctx, hipMemcpyAsync(kp_xy + dst * 2, ctx->d_kp2d + src * 2, n * 8, hipMemcpyDeviceToHost, ctx->stream)); ++ctx->node_pack_copies; }
      if (stats && ctx->d_feat_stats) { HIP_TRY(ctx, hipMemcpyAsync(stats + dst, ctx->d_feat_stats + (size_t)e.slot * ctx->feat_stats_stride(), n, hipMemcpyDeviceToHost, ctx->stream)); ++ctx->node_pack_copies; }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RGBDFE_OK;
  }
  Arena arena;
  const size_t o_table = arena.carve(sizeof(rgbdfe::NodePackEntry) * table.size());
  const size_t o_desc = arena.carve(desc ? total * desc_row : 0), o_xyz = arena.carve(xyz1 ? total * 16 : 0);
  const size_t o_kp = arena.carve(kp_xy ? total * 8 : 0), o_stats = arena.carve(stats ? total : 0);
  if (const int rc = ctx->node_pack.ensure(ctx, arena.size, "node read-back staging")) return rc;
  void* base = ctx->node_pack.p;
  rgbdfe::NodePackArgs a{};
  a.desc = reinterpret_cast<const uint4*>(kind == 0u ? (const void*)ctx->d_desc : (const void*)ctx->d_sift_f32);
  a.desc_units = (uint32_t)(desc_row / 16);
  a.xyz = reinterpret_cast<const uint4*>(ctx->d_xyz);
  a.kp = reinterpret_cast<const float2*>(ctx->d_kp2d);
  a.stats = ctx->d_feat_stats;   // never allocated: every counter is 0 by definition, and stays unallocated
  a.max_kp = (uint32_t)ctx->cfg.max_keypoints;
  a.stats_stride = (uint32_t)ctx->feat_stats_stride();
  a.out_desc = desc ? at<uint4>(base, o_desc) : nullptr;
  a.out_xyz = xyz1 ? at<uint4>(base, o_xyz) : nullptr;
  a.out_kp = kp_xy ? at<float2>(base, o_kp) : nullptr;
  a.out_stats = stats ? at<uint8_t>(base, o_stats) : nullptr;
  if (desc && !a.desc) return fail(ctx, RGBDFE_ERR_INTERNAL, "read-back: a float node without the float slab");
  HIP_TRY(ctx, hipMemcpyAsync(at<void>(base, o_table), table.data(), sizeof(rgbdfe::NodePackEntry) * table.size(),
                              hipMemcpyHostToDevice, ctx->stream));
  ctx->node_pack_launches = rgbdfe::launch_node_pack(at<rgbdfe::NodePackEntry>(base, o_table), (uint32_t)n_nodes, max_rows, a, ctx->stream);
  HIP_TRY(ctx, hipGetLastError());
  const struct { void* dst; size_t off, bytes; } copies[4] = {
      {desc, o_desc, total * desc_row}, {xyz1, o_xyz, total * 16}, {kp_xy, o_kp, total * 8}, {stats, o_stats, total}};
  for (const auto& c : copies) {
    if (!c.dst) continue;
    HIP_TRY(ctx, hipMemcpyAsync(c.dst, at<void>(base, c.off), c.bytes, hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->node_pack_copies;
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return RGBDFE_OK;
}

int rgbdfe_download_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc, float* xyz1,
                          float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds) {
  return download_nodes_common(ctx, n_nodes, node_ids, capacity_rows, desc, xyz1, kp_xy, stats, row_offsets, kinds, false);
}

int rgbdfe_debug_download_nodes_copy_loop(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc,
                                          float* xyz1, float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds) {
  return download_nodes_common(ctx, n_nodes, node_ids, capacity_rows, desc, xyz1, kp_xy, stats, row_offsets, kinds, true);
}

int rgbdfe_download_node(rgbdfe_ctx* ctx, int32_t node_id, int32_t capacity_rows, void* desc, float* xyz1, float* kp_xy,
                         uint8_t* stats, int32_t* kind, int32_t* has_keypoints) {
  if (!ctx || capacity_rows < 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad read-back arguments");
  int64_t offsets[2] = {0, 0};
  int32_t k = 0;
  const int rc = impl::rgbdfe_download_nodes(ctx, 1, &node_id, capacity_rows, desc, xyz1, kp_xy, stats, offsets, &k);
  if (rc != RGBDFE_OK) return rc;   // (RGBDFE_ERR_CAPACITY: the rows are rgbdfe_node_count's)
  if (kind) *kind = k & 0xff;
  if (has_keypoints) *has_keypoints = (k & RGBDFE_NODE_HAS_KEYPOINTS) ? 1 : 0;
  return (int)offsets[1];
}

int rgbdfe_download_nodes_stats(rgbdfe_ctx* ctx, int64_t* out, int32_t n_out) {
  if (!ctx || !out || n_out < 0) return RGBDFE_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  const int64_t v[RGBDFE_DOWNLOAD_STATS] = {ctx->node_pack_launches, ctx->node_pack_copies, (int64_t)ctx->node_pack.bytes,
                                            ctx->d_feat_stats ? 1 : 0};
  for (int32_t i = 0; i < n_out && i < RGBDFE_DOWNLOAD_STATS; ++i) out[i] = v[i];
  return RGBDFE_OK;
}

int rgbdfe_set_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, const uint8_t* stats, int32_t n) {
  if (!ctx || n < 0 || (n > 0 && !stats)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const auto it = ctx->nodes.find(node_id);
  if (it == ctx->nodes.end()) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "feature statistics of a node that is not resident");
  if ((uint32_t)n != it->second.n) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "feature statistics: count differs from the node's rows");
  if (n == 0) return RGBDFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  if (const int rc = ensure_feature_stats(ctx)) return rc;
  // on the context's stream, behind the zeroing an upload into the slot enqueued there and in front of the next statistics launch
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_feat_stats + (size_t)it->second.slot * ctx->feat_stats_stride(), stats, (size_t)n,
                              hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return RGBDFE_OK;
}

// The inverse of rgbdfe_detector_thresholds.  The per-cell thresholds are all a grid detector carries from frame to frame
// (OrbWorkspace::thresh: the adjusters' only member that a detection writes; the FAST type reads and writes the same array,
// api_fast.hip) -- everything else in the workspace is configuration or rebuilt per frame.
int rgbdfe_detector_set_thresholds(rgbdfe_ctx* ctx, const double* thresholds, int32_t n_cells) {
  if (!ctx || !thresholds) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  ensure_detector(ctx);
  if (n_cells != ctx->orb.grid * ctx->orb.grid)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "detector thresholds: n_cells differs from the configured grid (grid_resolution squared)");
  for (int32_t i = 0; i < n_cells; ++i)
    if (!std::isfinite(thresholds[i])) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "detector thresholds: a threshold is not finite");
  for (int32_t i = 0; i < n_cells; ++i) ctx->orb.thresh[i] = thresholds[i];
  return RGBDFE_OK;
}


// ---- clouds -----------------------------------------------------------------------------------------------------------
int rgbdfe_node_cloud_info(rgbdfe_ctx* ctx, int32_t node_id, double* out8) {
  if (!ctx || !out8) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const CloudEntry* ce = resident_cloud(ctx, node_id);
  if (!ce) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "no cloud for this node");
  const double v[8] = {(double)ce->ch, (double)ce->cw, (double)ce->cloud_skip, ce->fx, ce->fy, ce->cx, ce->cy, 0.0};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return RGBDFE_OK;
}

// The cloud as rgbdfe_upload_node_cloud leaves it: rows x cols points and, behind them, the plane of their z (what
// create_cloud_kernel writes there and the measurement model gathers from); the cached samples start unbuilt.
int rgbdfe_restore_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, const float* points, int32_t rows, int32_t cols, double fx, double fy,
                              double cx, double cy, int32_t cloud_skip) {
  if (!ctx || rows < 1 || cols < 0 || cloud_skip < 1 || (cols > 0 && !points)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  const size_t n = (size_t)rows * (size_t)cols;
  std::vector<float> host(n * 5);   // one copy: the points, then their z
  if (n) memcpy(host.data(), points, n * 16);
  for (size_t i = 0; i < n; ++i) host[n * 4 + i] = points[4 * i + 2];
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  if (const int rc = wait_for_pair_lanes(ctx)) return rc;   // nothing may still read a cloud this one replaces
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float4* d_new = nullptr;
  if (hipMalloc((void**)&d_new, (n > 0 ? n : 1) * (sizeof(float4) + sizeof(float))) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "cloud allocation failed");
  }
  if (n) {
    hipError_t he = hipMemcpyAsync(d_new, host.data(), n * 20, hipMemcpyHostToDevice, ctx->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
    if (he != hipSuccess) {
      (void)hipFree(d_new);
      return fail(ctx, RGBDFE_ERR_HIP, std::string("rgbdfe_restore_node_cloud: ") + hipGetErrorString(he));
    }
  }
  CloudEntry& ce = ctx->clouds[node_id];
  if (ce.d) (void)hipFree(ce.d);
  if (ce.d_samples) (void)hipFree(ce.d_samples);
  ce = CloudEntry{};
  ce.d = d_new;
  ce.ch = rows; ce.cw = cols; ce.cloud_skip = cloud_skip;
  ce.fx = (float)fx; ce.fy = (float)fy; ce.cx = (float)cx; ce.cy = (float)cy;
  return RGBDFE_OK;
}

// ---- the session file (layout: include/rgbdfe.h; bytes: session_format.h) ----------------------------------------------
namespace {
namespace sf = rgbdfe_session;

struct NodeRow { int32_t id; NodeEntry e; };

// ascending id: nothing in the file depends on the hash map's order or on the slots
std::vector<NodeRow> sorted_nodes(rgbdfe_ctx* ctx) {
  std::vector<NodeRow> v;
  for (const auto& kv : ctx->nodes) v.push_back(NodeRow{kv.first, kv.second});
  std::sort(v.begin(), v.end(), [](const NodeRow& a, const NodeRow& b) { return a.id < b.id; });
  return v;
}

int read_file(rgbdfe_ctx* ctx, const char* path, std::vector<uint8_t>& bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) return fail(ctx, RGBDFE_ERR_INVALID_ARG, std::string("session file: cannot open for reading: ") + path);
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return fail(ctx, RGBDFE_ERR_INVALID_ARG, std::string("session file: reading failed: ") + path);
  return RGBDFE_OK;
}

int call_string(rgbdfe_ctx* ctx, const std::function<int(uint8_t*, int64_t, int64_t*)>& fn, std::vector<uint8_t>& out) {
  int64_t bytes = 0;
  int rc = fn(nullptr, 0, &bytes);
  if (rc != RGBDFE_ERR_CAPACITY) return rc == RGBDFE_OK ? RGBDFE_ERR_INTERNAL : fail(ctx, rc, sf::contextless_error());
  out.resize((size_t)bytes);
  rc = fn(out.data(), bytes, &bytes);
  return rc == RGBDFE_OK ? rc : fail(ctx, rc, sf::contextless_error());
}
}  // namespace

int rgbdfe_session_save(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, uint32_t flags, const char* path) {
  if (!ctx || !path || !*path || (flags & ~(uint32_t)RGBDFE_SESSION_CLOUDS)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session save: bad arguments");
  if (slam && slam_context(slam) && slam_context(slam) != ctx)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session save: the slam object lives on another context");
  std::vector<uint8_t> conf, dete, node, clou, grph, slam_bytes;
  // the machine first: a step in flight refuses the save before anything is read
  if (slam) {
    const int rc = call_string(ctx, [&](uint8_t* o, int64_t c, int64_t* b) { return ::rgbdfe_slam_serialize(slam, o, c, b); }, slam_bytes);
    if (rc != RGBDFE_OK) return rc;
  }
  if (graph) {
    const int rc = call_string(ctx, [&](uint8_t* o, int64_t c, int64_t* b) { return ::rgbdfe_pose_graph_serialize(graph, o, c, b); }, grph);
    if (rc != RGBDFE_OK) return rc;
  }
  std::vector<NodeRow> nodes;
  std::vector<int32_t> cloud_ids;
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    for (const auto& job : ctx->host_jobs)
      if (job.pending) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session save: busy: a host job is pending (rgbdfe_wait_host first)");
    ensure_detector(ctx);
    nodes = sorted_nodes(ctx);
    for (const auto& kv : ctx->clouds) if (kv.second.d) cloud_ids.push_back(kv.first);
    std::sort(cloud_ids.begin(), cloud_ids.end());
    uint32_t kinds = 0;
    for (const NodeRow& r : nodes) kinds |= 1u << r.e.kind;
    sf::Writer w;
    w.put<int32_t>(ctx->cfg.max_keypoints); w.put<int32_t>(impl::rgbdfe_abi_version()); w.put<uint32_t>(kinds); w.put<uint32_t>(0);
    conf.swap(w.b);
    sf::Writer d;
    const int cells = ctx->orb.grid * ctx->orb.grid;
    d.put<int32_t>(ctx->detector_type); d.put<int32_t>(ctx->orb_max_keypoints); d.put<int32_t>(ctx->orb.grid);
    d.put<int32_t>(ctx->orb.adjuster_iters); d.put<int32_t>(ctx->feature_min_depth ? 1 : 0); d.put<int32_t>(cells);
    for (int i = 0; i < cells; ++i) d.put<double>(ctx->orb.thresh[i]);
    dete.swap(d.b);
  }
  {
    sf::Writer w;
    w.put<uint32_t>((uint32_t)nodes.size()); w.put<uint32_t>(0);
    for (const NodeRow& r : nodes) w.put<int32_t>(r.id);
    for (const NodeRow& r : nodes) w.put<int32_t>((int32_t)r.e.kind);
    for (const NodeRow& r : nodes) w.put<int32_t>((int32_t)r.e.n);
    for (const NodeRow& r : nodes) w.put<int32_t>((r.e.flags & kNodeHasKeypoints) ? 1 : 0);
    for (uint32_t kind = 0; kind < 3; ++kind) {   // one read-back per kind, whatever the number of nodes
      std::vector<int32_t> ids;
      size_t rows = 0;
      for (const NodeRow& r : nodes) if (r.e.kind == kind) { ids.push_back(r.id); rows += r.e.n; }
      if (ids.empty()) continue;
      const size_t desc_row = kind == 0 ? 32 : 512;
      std::vector<uint8_t> desc(rows * desc_row), stats(rows);
      std::vector<float> xyz(rows * 4), kp(rows * 2);
      const int rc = impl::rgbdfe_download_nodes(ctx, (int32_t)ids.size(), ids.data(), (int64_t)rows, desc.data(), xyz.data(), kp.data(),
                                                 stats.data(), nullptr, nullptr);
      if (rc != RGBDFE_OK) return rc;
      w.bytes(desc.data(), desc.size()); w.pad8();
      w.bytes(xyz.data(), xyz.size() * 4); w.pad8();
      w.bytes(kp.data(), kp.size() * 4); w.pad8();
      w.bytes(stats.data(), stats.size()); w.pad8();
    }
    node.swap(w.b);
  }
  if (flags & RGBDFE_SESSION_CLOUDS) {
    sf::Writer w;
    w.put<uint32_t>((uint32_t)cloud_ids.size()); w.put<uint32_t>(0);
    std::vector<float> pts;
    for (int32_t id : cloud_ids) {
      double info[8];
      int rc = impl::rgbdfe_node_cloud_info(ctx, id, info);
      if (rc != RGBDFE_OK) return rc;
      const size_t n = (size_t)info[0] * (size_t)info[1];
      pts.resize(n * 4);
      int32_t rows = 0, cols = 0;
      rc = impl::rgbdfe_download_node_cloud(ctx, id, pts.data(), (int64_t)n, &rows, &cols);
      if (rc != RGBDFE_OK) return rc;
      w.put<int32_t>(id); w.put<int32_t>(rows); w.put<int32_t>(cols); w.put<int32_t>((int32_t)info[2]);
      w.put<float>((float)info[3]); w.put<float>((float)info[4]); w.put<float>((float)info[5]); w.put<float>((float)info[6]);
      w.bytes(pts.data(), n * 16);
    }
    clou.swap(w.b);
  }
  sf::Writer file;
  sf::begin_file(file, flags);
  sf::put_chunk(file, sf::kConf, conf);
  sf::put_chunk(file, sf::kDete, dete);
  sf::put_chunk(file, sf::kNode, node);
  if (flags & RGBDFE_SESSION_CLOUDS) sf::put_chunk(file, sf::kClou, clou);
  if (graph) sf::put_chunk(file, sf::kGrph, grph);
  if (slam) sf::put_chunk(file, sf::kSlam, slam_bytes);
  sf::end_file(file);
  // to path + ".tmp", then renamed: nothing partial is ever seen under `path`, and nothing stays under either name on failure
  const std::string tmp = std::string(path) + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return fail(ctx, RGBDFE_ERR_INVALID_ARG, std::string("session save: cannot open for writing: ") + tmp);
  bool ok = fwrite(file.b.data(), 1, file.b.size(), f) == file.b.size();
  ok = (fflush(f) == 0) && ok;
  ok = (fclose(f) == 0) && ok;
  if (ok && rename(tmp.c_str(), path) != 0) ok = false;
  if (!ok) {
    (void)remove(tmp.c_str());
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, std::string("session save: writing failed (nothing was left behind): ") + path);
  }
  return RGBDFE_OK;
}

int rgbdfe_session_load(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, const char* path) {
  if (!ctx || !path) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: bad arguments");
  if (slam && slam_context(slam) && slam_context(slam) != ctx)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: the slam object lives on another context");
  std::vector<uint8_t> bytes;
  if (const int rc = read_file(ctx, path, bytes)) return rc;
  sf::SessionView v;
  const std::string err = sf::session_parse(bytes.data(), bytes.size(), v);
  if (!err.empty()) return fail(ctx, RGBDFE_ERR_INVALID_ARG, err);
  // ---- capacity, then the id rule: still nothing has changed
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    for (const auto& job : ctx->host_jobs)
      if (job.pending) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: busy: a host job is pending (rgbdfe_wait_host first)");
    if (v.max_rows > ctx->cfg.max_keypoints)
      return fail(ctx, RGBDFE_ERR_CAPACITY, "session load: a node of the file has more rows than the context's max_keypoints");
    if (v.ids.size() > ctx->free_slots.size())
      return fail(ctx, RGBDFE_ERR_CAPACITY, "session load: the file holds more nodes than the context has free slots (max_nodes)");
    for (int32_t id : v.ids)
      if (ctx->nodes.count(id)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: node id " + std::to_string(id) + " of the file is already resident");
    for (const sf::CloudView& c : v.clouds)
      if (ctx->clouds.count(c.id)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: node id " + std::to_string(c.id) + " of the file already has a resident cloud");
  }
  // (a GRPH / SLAM chunk without an object to take it is validated and left where it is: a viewer needs the nodes and the graph only)
  const bool take_graph = v.chunk[sf::kGrph].present && graph, take_slam = v.chunk[sf::kSlam].present && slam;
  if (graph && !sf::graph_is_empty(*graph)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: the graph target is not empty (rgbdfe_pose_graph_clear)");
  if (slam) {
    if (take_slam) {
      const int rc = slam_deserialize(slam, v.chunk[sf::kSlam].p, (int64_t)v.chunk[sf::kSlam].n, false);
      if (rc != RGBDFE_OK) return fail(ctx, rc, "session load: " + sf::contextless_error());
    } else if (::rgbdfe_slam_node_count(slam) != 0) {
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: the slam target is not empty (rgbdfe_slam_reset)");
    }
    if (take_graph && slam_graph(slam) != graph)
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "session load: the slam object works on another graph than the one passed");
  }
  // ---- the nodes, through the paths an upload takes
  {
    const sf::NodeGroup& g0 = v.group[0];
    if (!g0.ids.empty()) {
      std::vector<const uint8_t*> desc;
      std::vector<const float*> xyz;
      std::vector<std::vector<float>> aligned(g0.ids.size());   // (the file's arrays sit on 8-byte boundaries of a byte vector)
      size_t row = 0;
      for (size_t i = 0; i < g0.ids.size(); ++i) {
        desc.push_back(g0.desc + row * 32);
        aligned[i].resize((size_t)g0.rows[i] * 4);
        if (g0.rows[i]) memcpy(aligned[i].data(), g0.xyz + row * 16, (size_t)g0.rows[i] * 16);
        xyz.push_back(aligned[i].data());
        row += (size_t)g0.rows[i];
      }
      const int rc = impl::rgbdfe_upload_nodes(ctx, (int32_t)g0.ids.size(), g0.ids.data(), desc.data(), xyz.data(), g0.rows.data());
      if (rc != RGBDFE_OK) return rc;
    }
    for (int kind = 1; kind < 3; ++kind) {
      const sf::NodeGroup& g = v.group[kind];
      size_t row = 0;
      std::vector<float> d, x;
      for (size_t i = 0; i < g.ids.size(); ++i) {
        const size_t n = (size_t)g.rows[i];
        d.resize(n * 128); x.resize(n * 4);
        if (n) { memcpy(d.data(), g.desc + row * 512, n * 512); memcpy(x.data(), g.xyz + row * 16, n * 16); }
        const int rc = kind == 1 ? impl::rgbdfe_upload_sift_node(ctx, g.ids[i], d.data(), x.data(), (int32_t)n)
                                 : impl::rgbdfe_upload_float_node(ctx, g.ids[i], d.data(), 128, x.data(), (int32_t)n);
        if (rc != RGBDFE_OK) return rc;
        row += n;
      }
    }
    for (int kind = 0; kind < 3; ++kind) {
      const sf::NodeGroup& g = v.group[kind];
      size_t row = 0;
      std::vector<float> kp;
      for (size_t i = 0; i < g.ids.size(); ++i) {
        const size_t n = (size_t)g.rows[i];
        if (g.has_kp[i]) {
          kp.resize(n * 2);
          if (n) memcpy(kp.data(), g.kp + row * 8, n * 8);
          const int rc = impl::rgbdfe_upload_node_keypoints(ctx, g.ids[i], kp.data(), (int32_t)n);
          if (rc != RGBDFE_OK) return rc;
        }
        bool counted = false;   // a node whose counters are all zero has them from its upload: no counter is allocated for it
        for (size_t r = 0; r < n && !counted; ++r) counted = g.stats[row + r] != 0;
        if (counted) {
          const int rc = impl::rgbdfe_set_node_feature_stats(ctx, g.ids[i], g.stats + row, (int32_t)n);
          if (rc != RGBDFE_OK) return rc;
        }
        row += n;
      }
    }
  }
  {
    std::vector<float> pts;
    for (const sf::CloudView& c : v.clouds) {
      const size_t n = (size_t)c.ch * (size_t)c.cw;
      pts.resize(n * 4);
      if (n) memcpy(pts.data(), c.points, n * 16);
      const int rc = impl::rgbdfe_restore_node_cloud(ctx, c.id, pts.data(), c.ch, c.cw, c.fx, c.fy, c.cx, c.cy, c.cloud_skip);
      if (rc != RGBDFE_OK) return rc;
    }
  }
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    ensure_detector(ctx);
    ctx->orb_max_keypoints = v.detector_max_keypoints;
    ctx->orb.reset_detector(v.detector_max_keypoints, v.grid, v.adjuster_iters);
    ctx->detector_type = v.detector_type;
    for (int i = 0; i < 64; ++i) ctx->orb.thresh[i] = i < v.n_cells ? v.thresholds[i] : 20.0;
    ctx->feature_min_depth = v.feature_min_depth != 0;
  }
  if (take_graph) {
    const int rc = ::rgbdfe_pose_graph_deserialize(graph, v.chunk[sf::kGrph].p, (int64_t)v.chunk[sf::kGrph].n);
    if (rc != RGBDFE_OK) return fail(ctx, rc, "session load: " + sf::contextless_error());
  }
  if (take_slam) {
    const int rc = slam_deserialize(slam, v.chunk[sf::kSlam].p, (int64_t)v.chunk[sf::kSlam].n, true);
    if (rc != RGBDFE_OK) return fail(ctx, rc, "session load: " + sf::contextless_error());
  }
  return RGBDFE_OK;
}

}  // namespace impl
