// api_map_files.hip -- map files: the assembled map and the node clouds as PCD / PLY files (kernels: map_assembly.hip,
// map_files.hip; the bytes: cloud_file_format.h), and the host-only calls that write, describe and read such a file
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"

#include <sys/stat.h>

#include "cloud_file_format.h"
#include "map_files.h"
#include "pose_graph_host.h"
#include "session_format.h"
#include "staging_ring.h"

namespace cf = rgbdfe_cloud_file;

namespace {

constexpr int64_t kDefaultChunkPoints = (int64_t)1 << 20;   // 16 MiB of rows per buffer
constexpr int64_t kMinChunkPoints = 64;                     // a slot of 64 rows also holds 64 + 3 vertices and their padding

struct PinnedBuffer {   // page-locked host memory that lives for one call
  void* p = nullptr;
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  ~PinnedBuffer() { if (p) (void)hipHostFree(p); }
  int alloc(rgbdfe_ctx* ctx, size_t bytes, const char* msg) {
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, msg);
    }
    return RGBDFE_OK;
  }
};

struct EventPair {
  hipEvent_t e[2] = {nullptr, nullptr};
  ~EventPair() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// a file being written: gone again unless keep() was reached (a failed write leaves nothing behind, as rgbdfe_octomap_write)
struct OutFile {
  FILE* f = nullptr;
  std::string path;
  bool ok = true;
  bool open(const std::string& p) {
    path = p;
    f = fopen(p.c_str(), "wb");
    return f != nullptr;
  }
  void write(const void* p, size_t n) {
    if (ok && n && fwrite(p, 1, n, f) != n) ok = false;
  }
  bool keep() {   // closes; false: the write failed and the file is removed
    if (!f) return false;
    ok = (fclose(f) == 0) && ok;
    f = nullptr;
    if (!ok) remove(path.c_str());
    return ok;
  }
  ~OutFile() {
    if (f) { fclose(f); remove(path.c_str()); }
  }
};

int contextless_fail(int code, const std::string& msg) {
  rgbdfe_session::contextless_error() = msg;
  return code;
}

// Eigen's Quaternionf::toRotationMatrix() for (w, x, y, z), row-major, every product and sum in float
void quaternionf_to_rotation(float w, float x, float y, float z, float R[9]) {
  const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0f - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0f - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0f - (txx + tyy);
}

}  // namespace

namespace impl {

// GraphManager::saveAllCloudsToFile (graph_mgr_io.cpp:502-582): the loop of rgbdfe_assemble_map group by group, each group's
// file bytes through one of two page-locked slots while the next group runs.
int rgbdfe_save_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth,
                    int32_t preserve_raster, const char* path, int64_t chunk_points, char* path_written, int64_t path_capacity,
                    rgbdfe_map_file_stats* stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!ctx || n_nodes < 0 || !path || !path[0] || chunk_points < 0 || path_capacity < 0 || (path_capacity > 0 && !path_written) ||
      (n_nodes > 0 && (!node_ids || !transforms)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad map file arguments");
  std::string final_path;
  const int32_t format = cf::format_of_path(path, final_path);
  if (stats) stats->format = format;
  if (path_written) {
    if ((size_t)path_capacity < final_path.size() + 1) return fail(ctx, RGBDFE_ERR_CAPACITY, "map file: path_written is too small");
    memcpy(path_written, final_path.c_str(), final_path.size() + 1);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (n_nodes == 0) return RGBDFE_OK;

  // the node table of the whole list (the count and the scan run over it) ...
  const size_t n = (size_t)n_nodes;
  std::vector<MapNode> table(n + 1);
  int64_t points = 0, tiles = 0, largest = 0;
  for (size_t k = 0; k < n; ++k) {
    const CloudEntry* ce = resident_cloud(ctx, node_ids[k]);
    if (!ce) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "map file: no cloud for a listed node");
    MapNode& m = table[k];
    m.cloud = ce->d;
    m.first_point = points;
    m.n_points = (uint32_t)((size_t)ce->ch * (size_t)ce->cw);
    m.first_tile = (uint32_t)tiles;
    rigid_of_matrix4f(transforms + k * 16, m.R, m.t);
    points += (int64_t)m.n_points;
    tiles += (int64_t)((m.n_points + kMapTile - 1) / kMapTile);
    largest = std::max(largest, (int64_t)m.n_points);
    if (tiles > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "map file: more than 2^31 tiles in one call");
  }
  MapNode& end = table[n];
  memset(&end, 0, sizeof(end));
  end.first_point = points;
  end.first_tile = (uint32_t)tiles;
  const size_t n_tiles = (size_t)tiles;

  // ... cut into groups of consecutive nodes of at most `chunk` points (a larger cloud alone), and the table again with every
  // node's first tile and first row counted from its group's start: what the assembly kernels take for one group
  const int64_t chunk = chunk_points == 0 ? kDefaultChunkPoints : std::max(chunk_points, kMinChunkPoints);
  std::vector<size_t> group_start;   // node index; a sentinel n behind the last
  int64_t cap = kMinChunkPoints;
  {
    int64_t in_group = 0;
    for (size_t k = 0; k < n; ++k) {
      if (k == 0 || in_group + (int64_t)table[k].n_points > chunk) {
        group_start.push_back(k);
        in_group = 0;
      }
      in_group += (int64_t)table[k].n_points;
      cap = std::max(cap, in_group);
    }
    group_start.push_back(n);
  }
  const size_t n_groups = group_start.size() - 1;
  std::vector<MapNode> local(table.begin(), table.end() - 1);
  std::vector<uint32_t> local_tile_node(n_tiles);
  for (size_t gi = 0; gi < n_groups; ++gi) {
    const size_t a = group_start[gi], b = group_start[gi + 1];
    for (size_t k = a; k < b; ++k) {
      local[k].first_point = table[k].first_point - table[a].first_point;
      local[k].first_tile = table[k].first_tile - table[a].first_tile;
      std::fill(local_tile_node.begin() + table[k].first_tile, local_tile_node.begin() + table[k + 1].first_tile, (uint32_t)(k - a));
    }
  }

  DeviceLayout lay;
  const NodeTableBlocks b_nodes_in = put_node_table(lay, table);
  const Block b_local = lay.put(local.data(), sizeof(MapNode) * n), b_local_tiles = lay.put(local_tile_node.data(), 4 * n_tiles);
  const Block b_count = lay.room(4 * n_tiles), b_first = lay.room(8 * (n_tiles + 1)), b_node_first = lay.room(8 * (n + 1));
  const Block b_carry = lay.room(2 * 64);   // two carries of three rows, 64 bytes apart

  const bool compact = preserve_raster == 0;
  const float md = (float)maximum_depth;  // `float max_Depth` (misc.cpp:185)
  const bool clip = md >= 0.0f;           // :217
  const float md2 = md * md;              // :218

  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = ctx->stream;
  int rc = ensure_scratch(ctx, lay.total());
  if (rc != RGBDFE_OK) return rc;
  void* base = ctx->d_scratch;
  const MapNode* d_local = at<MapNode>(base, b_local);
  const uint32_t* d_local_tiles = at<uint32_t>(base, b_local_tiles);
  int64_t* d_first = at<int64_t>(base, b_first);
  float4* d_carry[2] = {at<float4>(base, b_carry), at<float4>(base, b_carry) + 4};
  HIP_TRY(ctx, hipMemcpyAsync(base, lay.staged(), lay.staged_bytes(), hipMemcpyHostToDevice, st));

  // every node's first row of the file, and the total: the header is written from them
  std::vector<int64_t> first(n + 1);
  if (compact) {
    launch_map_count_scan(at<MapNode>(base, b_nodes_in.table), at<uint32_t>(base, b_nodes_in.tile_node), (uint32_t)n, (uint32_t)n_tiles,
                          clip, md2, at<uint32_t>(base, b_count), d_first, at<int64_t>(base, b_node_first), st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(first.data(), at<int64_t>(base, b_node_first), 8 * (n + 1), hipMemcpyDeviceToHost, st));
  } else {
    for (size_t k = 0; k <= n; ++k) first[k] = table[k].first_point;
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));   // (the tables' copy reads the layout's staging)
  const int64_t total = first[n];
  if (total == 0) return RGBDFE_OK;   // PCL throws on an empty cloud; here: no file, a count of 0
  if (total > cf::kMaxPoints) return fail(ctx, RGBDFE_ERR_CAPACITY, "map file: 2^31 points or more");

  OutFile file;
  if (!file.open(final_path)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "map file: cannot open " + final_path);
  const bool ply = format == RGBDFE_CLOUD_FILE_PLY;
  const float origin[7] = {0, 0, 0, 1, 0, 0, 0};
  const std::string header = ply ? cf::ply_header(total) : cf::pcd_header(total, 1, origin);
  file.write(header.data(), header.size());

  // two device buffers of `cap` rows and two page-locked slots of as many bytes
  const size_t buf_bytes = (size_t)cap * sizeof(float4);
  DeviceBuffer dbuf[2];
  PinnedBuffer slot[2];
  EventPair done;
  for (int i = 0; i < 2; ++i) {
    rc = dbuf[i].alloc(ctx, buf_bytes, "map file: device buffer allocation failed");
    if (rc != RGBDFE_OK) return rc;
    rc = slot[i].alloc(ctx, buf_bytes, "map file: page-locked slot allocation failed");
    if (rc != RGBDFE_OK) return rc;
    HIP_TRY(ctx, hipEventCreateWithFlags(&done.e[i], hipEventDisableTiming));
  }

  // the writer: group i's bytes leave slot i % 2 once the stream has passed the group, while the calling thread enqueues the
  // groups behind it (a StagingRing of depth 0: item i is written once it has been marked enqueued)
  std::vector<size_t> slot_bytes(n_groups, 0);
  std::atomic<int> hip_failed{0};
  const int device_id = ctx->cfg.device_id;
  StagingRing writer((int)n_groups, 0, [&](int i) {
    if (hip_failed.load() || !file.ok) return;
    if (hipSetDevice(device_id) != hipSuccess || hipEventSynchronize(done.e[i % 2]) != hipSuccess) {
      hip_failed.store(1);
      return;
    }
    file.write(slot[i % 2].p, slot_bytes[(size_t)i]);
  });

  uint32_t carry = 0;
  for (size_t gi = 0; gi < n_groups; ++gi) {
    const size_t a = group_start[gi], b = group_start[gi + 1];
    const uint32_t t0 = table[a].first_tile, nt = table[b].first_tile - t0;
    const int64_t m = first[b] - first[a];   // rows of the file this group gives: at most its clouds' points, so at most cap
    const int s = (int)(gi % 2);
    if (gi >= 2) writer.wait_staged((int)gi - 2);   // the slot's previous bytes are in the file
    float4* buf = (float4*)dbuf[s].p;
    if (compact)   // map_write_kernel stores at the rows of the whole map: first[a] is the buffer's row 0
      launch_map_write(d_local + a, d_local_tiles + t0, nt, d_first + t0, clip, md2,
                       reinterpret_cast<float4*>(reinterpret_cast<uintptr_t>(buf) - sizeof(float4) * (uintptr_t)first[a]), st);
    else
      launch_map_raster(d_local + a, d_local_tiles + t0, nt, clip, md2, buf, st);
    HIP_TRY(ctx, hipGetLastError());
    if (ply) {   // the vertices go straight into the slot
      const uint32_t packed = launch_cloud_pack_ply(d_carry[s], carry, buf, (uint32_t)m, gi + 1 == n_groups, (uint32_t*)slot[s].p,
                                                    d_carry[1 - s], st);
      HIP_TRY(ctx, hipGetLastError());
      slot_bytes[gi] = cf::kPlyVertexBytes * (size_t)packed;
      carry = carry + (uint32_t)m - packed;
    } else if (m > 0) {
      slot_bytes[gi] = sizeof(float4) * (size_t)m;
      HIP_TRY(ctx, hipMemcpyAsync(slot[s].p, buf, slot_bytes[gi], hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipEventRecord(done.e[s], st));
    writer.mark_consumed((int)gi);
  }
  writer.wait_staged((int)n_groups - 1);
  writer.stop();
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (hip_failed.load()) return fail(ctx, RGBDFE_ERR_HIP, "map file: waiting for a group failed");
  if (ply) {
    uint8_t cam[cf::kPlyCameraBytes];
    cf::ply_camera((int32_t)total, 1, cam);
    file.write(cam, sizeof(cam));
  }
  if (!file.keep()) return fail(ctx, RGBDFE_ERR_INTERNAL, "map file: writing " + final_path + " failed");
  if (stats) {
    stats->points = total;
    stats->bytes_written = (int64_t)header.size() + (ply ? (int64_t)cf::kPlyVertexBytes * total + (int64_t)cf::kPlyCameraBytes
                                                         : (int64_t)cf::kRowBytes * total);
    stats->groups = (int32_t)n_groups;
    stats->device_scratch_bytes = (int64_t)(2 * buf_bytes);
    stats->pinned_bytes = (int64_t)(2 * buf_bytes);
    stats->table_bytes = (int64_t)lay.total();
  }
  return RGBDFE_OK;
}

// GraphManager::saveIndividualCloudsToFile (graph_mgr_io.cpp:330-433) without its ground-truth branch: node k + 1's rows
// travel to their slot while node k's files are written.
int rgbdfe_save_node_clouds(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const int32_t* graph_ids, const double* poses,
                            int32_t transform_individual_clouds, const char* basename, int32_t* n_written) {
  if (n_written) *n_written = 0;
  if (!ctx || n_nodes < 0 || !basename || !basename[0] || (n_nodes > 0 && (!node_ids || !poses)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad node cloud file arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  struct Job { const CloudEntry* ce; size_t k, rows; };
  std::vector<Job> jobs;
  size_t largest = 0;
  for (int32_t k = 0; k < n_nodes; ++k) {
    const auto it = ctx->clouds.find(node_ids[k]);
    if (it == ctx->clouds.end()) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "node cloud files: no cloud for a listed node");
    const size_t rows = (size_t)it->second.ch * (size_t)it->second.cw;
    if (!it->second.d || rows == 0) continue;   // "Skipping Node %i, point cloud data is empty!" (:355)
    jobs.push_back(Job{&it->second, (size_t)k, rows});
    largest = std::max(largest, rows);
  }
  if (jobs.empty()) return RGBDFE_OK;
  const bool moved = transform_individual_clouds != 0;

  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = ctx->stream;
  // flag on: pcl::transformPointCloud with the pose cast to float == raster assembly of the node alone with the clip off.  One
  // table row per job, each a group of its own (first row 0, first tile 0), and a tile -> node map of zeros.
  DeviceLayout lay;
  Block b_table, b_tiles;
  if (moved) {
    std::vector<MapNode> table(jobs.size());
    for (size_t j = 0; j < jobs.size(); ++j) {
      MapNode& m = table[j];
      float mf[16];
      for (int i = 0; i < 16; ++i) mf[i] = (float)poses[16 * jobs[j].k + (size_t)i];   // v->estimate().matrix().cast<float>()
      m.cloud = jobs[j].ce->d;
      m.first_point = 0;
      m.n_points = (uint32_t)jobs[j].rows;
      m.first_tile = 0;
      rigid_of_matrix4f(mf, m.R, m.t);
    }
    b_table = lay.put(table.data(), sizeof(MapNode) * table.size());
    b_tiles = lay.put(nullptr, 4 * ((largest + kMapTile - 1) / kMapTile));
    const int rc = ensure_scratch(ctx, lay.total());
    if (rc != RGBDFE_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_scratch, lay.staged(), lay.staged_bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));   // (the copy reads the layout's staging)
  }
  const size_t buf_bytes = largest * sizeof(float4);
  DeviceBuffer dbuf[2];
  PinnedBuffer slot[2];
  EventPair done;
  for (int i = 0; i < 2; ++i) {
    int rc = moved ? dbuf[i].alloc(ctx, buf_bytes, "node cloud files: device buffer allocation failed") : RGBDFE_OK;
    if (rc != RGBDFE_OK) return rc;
    rc = slot[i].alloc(ctx, buf_bytes, "node cloud files: page-locked slot allocation failed");
    if (rc != RGBDFE_OK) return rc;
    HIP_TRY(ctx, hipEventCreateWithFlags(&done.e[i], hipEventDisableTiming));
  }
  auto enqueue = [&](size_t j) -> int {
    const int s = (int)(j % 2);
    const size_t bytes = jobs[j].rows * sizeof(float4);
    const void* src = jobs[j].ce->d;   // flag off: the resident cloud untouched
    if (moved) {
      launch_map_raster(at<MapNode>(ctx->d_scratch, b_table) + j, at<uint32_t>(ctx->d_scratch, b_tiles),
                        (uint32_t)((jobs[j].rows + kMapTile - 1) / kMapTile), false, 0.0f, (float4*)dbuf[s].p, st);
      HIP_TRY(ctx, hipGetLastError());
      src = dbuf[s].p;
    }
    HIP_TRY(ctx, hipMemcpyAsync(slot[s].p, src, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipEventRecord(done.e[s], st));
    return RGBDFE_OK;
  };
  int rc = enqueue(0);
  for (size_t j = 0; j < jobs.size() && rc == RGBDFE_OK; ++j) {
    if (j + 1 < jobs.size()) rc = enqueue(j + 1);   // slot (j + 1) % 2 was written out in the previous round
    if (rc != RGBDFE_OK) break;
    HIP_TRY(ctx, hipEventSynchronize(done.e[j % 2]));
    const size_t k = jobs[j].k;
    const double* P = poses + 16 * k;   // column-major
    float view[7], R[9], origin[3];
    if (moved) {   // Eigen::Vector4f sensor_origin(0,0,0,0); Eigen::Quaternionf sensor_orientation(0,0,0,1): (w, x, y, z) (:374-375)
      const float quirk[7] = {0, 0, 0, 0, 0, 0, 1};
      memcpy(view, quirk, sizeof(view));
    } else {
      double Rd[9], q[4];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rd[3 * r + c] = P[4 * c + r];
      quat_from_rot_xyzw(Rd, q);
      for (int r = 0; r < 3; ++r) view[r] = (float)P[12 + r];
      view[3] = (float)q[3]; view[4] = (float)q[0]; view[5] = (float)q[1]; view[6] = (float)q[2];
    }
    quaternionf_to_rotation(view[3], view[4], view[5], view[6], R);
    for (int r = 0; r < 3; ++r) origin[r] = view[r];
    char tail[32];
    snprintf(tail, sizeof(tail), "_%04d", (int)(graph_ids ? graph_ids[k] : node_ids[k]));
    const std::string stem = std::string(basename) + tail;
    OutFile pcd, txt;
    if (!pcd.open(stem + ".pcd")) { rc = fail(ctx, RGBDFE_ERR_INVALID_ARG, "node cloud files: cannot open " + stem + ".pcd"); break; }
    const std::string header = cf::pcd_header(jobs[j].ce->cw, jobs[j].ce->ch, view);
    pcd.write(header.data(), header.size());
    pcd.write(slot[j % 2].p, jobs[j].rows * sizeof(float4));
    if (!txt.open(stem + ".txt")) { rc = fail(ctx, RGBDFE_ERR_INVALID_ARG, "node cloud files: cannot open " + stem + ".txt"); break; }
    std::string text;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) text += cf::fmt_g(R[3 * r + c]) + " ";
      text += cf::fmt_g(origin[r]) + " ";
    }
    text += "0 0 0 1\n";
    txt.write(text.data(), text.size());
    const bool ok_pcd = pcd.keep(), ok_txt = txt.keep();
    if (!ok_pcd || !ok_txt) {
      remove((stem + ".pcd").c_str());
      remove((stem + ".txt").c_str());
      rc = fail(ctx, RGBDFE_ERR_INTERNAL, "node cloud files: writing " + stem + " failed");
      break;
    }
    if (n_written) ++*n_written;
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));   // nothing of this call is in flight when its buffers go
  return rc;
}

}  // namespace impl

// ---- host-only calls: no device, no context (a failed call's cause: rgbdfe_last_error(NULL)) -------------------------------
namespace {

int save_cloud_file(const float* points, int32_t width, int32_t height, const float* viewpoint, int32_t format, const char* path) {
  if (!path || !path[0] || width < 0 || height < 0 || (format != RGBDFE_CLOUD_FILE_PCD && format != RGBDFE_CLOUD_FILE_PLY))
    return contextless_fail(RGBDFE_ERR_INVALID_ARG, "cloud file: bad arguments");
  const int64_t n = (int64_t)width * (int64_t)height;
  if (n > cf::kMaxPoints) return contextless_fail(RGBDFE_ERR_CAPACITY, "cloud file: 2^31 points or more");
  if (n > 0 && !points) return contextless_fail(RGBDFE_ERR_INVALID_ARG, "cloud file: bad arguments");
  OutFile file;
  if (!file.open(path)) return contextless_fail(RGBDFE_ERR_INVALID_ARG, std::string("cloud file: cannot open ") + path);
  const float origin[7] = {0, 0, 0, 1, 0, 0, 0};
  const uint8_t* rows = reinterpret_cast<const uint8_t*>(points);
  if (format == RGBDFE_CLOUD_FILE_PCD) {
    const std::string header = cf::pcd_header(width, height, viewpoint ? viewpoint : origin);
    file.write(header.data(), header.size());
    file.write(rows, cf::kRowBytes * (size_t)n);
  } else {
    const std::string header = cf::ply_header(n);
    file.write(header.data(), header.size());
    std::vector<uint8_t> v(cf::kPlyVertexBytes * (size_t)std::min<int64_t>(n, 1 << 16));
    for (int64_t i = 0; i < n; i += 1 << 16) {
      const size_t k = (size_t)std::min<int64_t>(n - i, 1 << 16);
      cf::ply_pack_rows(rows + cf::kRowBytes * (size_t)i, k, v.data());
      file.write(v.data(), cf::kPlyVertexBytes * k);
    }
    uint8_t cam[cf::kPlyCameraBytes];
    cf::ply_camera(width, height, cam);
    file.write(cam, sizeof(cam));
  }
  if (!file.keep()) return contextless_fail(RGBDFE_ERR_INTERNAL, std::string("cloud file: writing ") + path + " failed");
  return RGBDFE_OK;
}

struct InFile {
  FILE* f = nullptr;
  ~InFile() { if (f) fclose(f); }
};

// header and lengths of the file at `path`; `in` stays open at the start of the data section
int open_cloud_file(const char* path, InFile& in, rgbdfe_cloud_file_header& info) {
  in.f = fopen(path, "rb");
  struct stat sb;
  if (!in.f || fstat(fileno(in.f), &sb) != 0 || !S_ISREG(sb.st_mode))
    return contextless_fail(RGBDFE_ERR_INVALID_ARG, std::string("cloud file: cannot open ") + path);
  uint8_t head[cf::kMaxHeaderBytes];
  const size_t got = fread(head, 1, sizeof(head), in.f);
  const std::string err = cf::parse_header(head, got, (uint64_t)sb.st_size, info);
  if (!err.empty()) return contextless_fail(RGBDFE_ERR_INVALID_ARG, err);
  if (info.format == RGBDFE_CLOUD_FILE_PLY) {   // the viewport of the camera record behind the vertices
    uint8_t cam[cf::kPlyCameraBytes];
    if (fseeko(in.f, (off_t)(sb.st_size - (off_t)sizeof(cam)), SEEK_SET) != 0 || fread(cam, 1, sizeof(cam), in.f) != sizeof(cam))
      return contextless_fail(RGBDFE_ERR_INVALID_ARG, "cloud file: the file ends inside its data section");
    const std::string e2 = cf::parse_ply_camera(cam, info);
    if (!e2.empty()) return contextless_fail(RGBDFE_ERR_INVALID_ARG, e2);
  }
  if (fseeko(in.f, (off_t)info.header_bytes, SEEK_SET) != 0) return contextless_fail(RGBDFE_ERR_INVALID_ARG, "cloud file: cannot seek");
  return RGBDFE_OK;
}

int load_cloud_file(const char* path, float* out, int64_t capacity, rgbdfe_cloud_file_header* info_out) {
  rgbdfe_cloud_file_header info;
  if (info_out) memset(info_out, 0, sizeof(*info_out));
  if (!path || capacity < 0 || (capacity > 0 && !out)) return contextless_fail(RGBDFE_ERR_INVALID_ARG, "cloud file: bad arguments");
  InFile in;
  const int rc = open_cloud_file(path, in, info);
  if (rc != RGBDFE_OK) return rc;
  if (info_out) *info_out = info;
  if (capacity < info.points) return contextless_fail(RGBDFE_ERR_CAPACITY, "cloud file: `out` is too small (info.points rows are needed)");
  uint8_t* rows = reinterpret_cast<uint8_t*>(out);
  const size_t n = (size_t)info.points;
  const char* short_file = "cloud file: the file ends inside its data section";
  if (info.format == RGBDFE_CLOUD_FILE_PCD) {
    if (n && fread(rows, cf::kRowBytes, n, in.f) != n) return contextless_fail(RGBDFE_ERR_INVALID_ARG, short_file);
  } else {
    std::vector<uint8_t> v(cf::kPlyVertexBytes * std::min<size_t>(n, 1 << 16));
    for (size_t i = 0; i < n; i += 1 << 16) {
      const size_t k = std::min<size_t>(n - i, 1 << 16);
      if (fread(v.data(), cf::kPlyVertexBytes, k, in.f) != k) return contextless_fail(RGBDFE_ERR_INVALID_ARG, short_file);
      cf::ply_unpack_rows(v.data(), k, rows + cf::kRowBytes * i);
    }
  }
  return RGBDFE_OK;
}

template <class F>
int contextless_guarded(F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return RGBDFE_ERR_OUT_OF_MEMORY;
  } catch (...) {
    return RGBDFE_ERR_INTERNAL;   // no exception crosses the C ABI
  }
}

}  // namespace

extern "C" {

int rgbdfe_save_cloud_file(const float* points, int32_t width, int32_t height, const float* viewpoint, int32_t format,
                           const char* path) {
  return contextless_guarded([&] { return save_cloud_file(points, width, height, viewpoint, format, path); });
}

int rgbdfe_cloud_file_info(const char* path, rgbdfe_cloud_file_header* info) {
  return contextless_guarded([&]() -> int {
    if (!path || !info) return contextless_fail(RGBDFE_ERR_INVALID_ARG, "cloud file: bad arguments");
    InFile in;
    return open_cloud_file(path, in, *info);
  });
}

int rgbdfe_load_cloud_file(const char* path, float* out, int64_t capacity, rgbdfe_cloud_file_header* info) {
  return contextless_guarded([&] { return load_cloud_file(path, out, capacity, info); });
}

int rgbdfe_cloud_file_path(const char* path, char* path_out, int64_t capacity, int32_t* format) {
  return contextless_guarded([&]() -> int {
    if (!path || capacity < 0 || (capacity > 0 && !path_out)) return contextless_fail(RGBDFE_ERR_INVALID_ARG, "cloud file: bad arguments");
    std::string final_path;
    const int32_t f = cf::format_of_path(path, final_path);
    if (format) *format = f;
    if ((size_t)capacity < final_path.size() + 1) return contextless_fail(RGBDFE_ERR_CAPACITY, "cloud file: path_out is too small");
    memcpy(path_out, final_path.c_str(), final_path.size() + 1);
    return RGBDFE_OK;
  });
}

}  // extern "C"
