// api_map.hip -- map assembly: the resident node clouds as one world-frame cloud (kernels: map_assembly.hip), and the way back
// to the host for a single resident cloud
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"

namespace impl {

namespace {

// GraphManager::saveAllCloudsToFile's loop (graph_mgr_io.cpp:529-552).  Exactly one of h_out / d_out receives the points.
int assemble_map_common(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth,
                        int32_t preserve_raster, float* h_out, void* d_out, bool to_device, int64_t capacity, int64_t* n_out,
                        int64_t* node_offsets, void* stream) {
  if (!ctx || n_nodes < 0 || !n_out || capacity < 0 || (n_nodes > 0 && (!node_ids || !transforms)) ||
      (capacity > 0 && !(to_device ? d_out != nullptr : h_out != nullptr)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad map assembly arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  *n_out = 0;
  if (n_nodes == 0) {
    if (node_offsets) node_offsets[0] = 0;
    return RGBDFE_OK;
  }
  // the node table and the tile -> node map: one blob, one copy
  const size_t n = (size_t)n_nodes;
  std::vector<MapNode> table(n + 1);
  int64_t points = 0, tiles = 0;
  for (size_t k = 0; k < n; ++k) {
    const CloudEntry* ce = resident_cloud(ctx, node_ids[k]);
    if (!ce) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "map assembly: no cloud for a listed node");
    MapNode& m = table[k];
    m.cloud = ce->d;
    m.first_point = points;
    m.n_points = (uint32_t)((size_t)ce->ch * (size_t)ce->cw);
    m.first_tile = (uint32_t)tiles;
    rigid_of_matrix4f(transforms + k * 16, m.R, m.t);
    points += (int64_t)m.n_points;
    tiles += (int64_t)((m.n_points + kMapTile - 1) / kMapTile);
    if (tiles > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "map assembly: more than 2^31 tiles in one call");
  }
  MapNode& end = table[n];
  memset(&end, 0, sizeof(end));
  end.first_point = points;
  end.first_tile = (uint32_t)tiles;
  const size_t n_tiles = (size_t)tiles;
  DeviceLayout lay;
  const NodeTableBlocks b_nodes_in = put_node_table(lay, table);

  const bool compact = preserve_raster == 0;
  const float md = (float)maximum_depth;  // `float max_Depth` (misc.cpp:185)
  const bool clip = md >= 0.0f;           // :217
  const float md2 = md * md;              // :218
  if (!compact) {  // every point keeps its row: the sizes are known before any device work
    *n_out = points;
    if (node_offsets)
      for (size_t k = 0; k <= n; ++k) node_offsets[k] = table[k].first_point;
    if (capacity < points) return fail(ctx, RGBDFE_ERR_CAPACITY, "map assembly: `out` is too small (*n_out rows are needed)");
  }

  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const Block b_count = lay.room(4 * n_tiles), b_first = lay.room(8 * (n_tiles + 1)), b_nodes = lay.room(8 * (n + 1));
  int rc = ensure_scratch(ctx, lay.total());
  if (rc != RGBDFE_OK) return rc;
  void* base = ctx->d_scratch;
  const MapNode* d_table = at<MapNode>(base, b_nodes_in.table);
  const uint32_t* d_tile_node = at<uint32_t>(base, b_nodes_in.tile_node);
  uint32_t* d_count = at<uint32_t>(base, b_count);
  int64_t* d_first = at<int64_t>(base, b_first);
  int64_t* d_node_first = at<int64_t>(base, b_nodes);
  HIP_TRY(ctx, hipMemcpyAsync(base, lay.staged(), lay.staged_bytes(), hipMemcpyHostToDevice, st));

  int64_t total = points;
  if (compact) {
    launch_map_count_scan(d_table, d_tile_node, (uint32_t)n, (uint32_t)n_tiles, clip, md2, d_count, d_first, d_node_first, st);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int64_t> first(n + 1);  // the one read of the sizes: the nodes' first rows and the total
    HIP_TRY(ctx, hipMemcpyAsync(first.data(), d_node_first, 8 * (n + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    total = first[n];
    *n_out = total;
    if (node_offsets) memcpy(node_offsets, first.data(), 8 * (n + 1));
    if (capacity < total) return fail(ctx, RGBDFE_ERR_CAPACITY, "map assembly: `out` is too small (*n_out rows are needed)");
  }
  if (total == 0) {
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (the table's copy reads the layout's staging)
    return RGBDFE_OK;
  }
  OutputSink sink(to_device ? d_out : nullptr);
  rc = sink.ready(ctx, (size_t)total * sizeof(float4), "map assembly: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  float4* d_points = (float4*)sink.d;
  if (compact) launch_map_write(d_table, d_tile_node, (uint32_t)n_tiles, d_first, clip, md2, d_points, st);
  else launch_map_raster(d_table, d_tile_node, (uint32_t)n_tiles, clip, md2, d_points, st);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, sink.finish(h_out, st));
  // the table in the context's scratch and the layout's staging are this call's: it returns when the stream has passed them
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return RGBDFE_OK;
}

}  // namespace

int rgbdfe_assemble_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth,
                        int32_t preserve_raster, float* out, int64_t capacity, int64_t* n_out, int64_t* node_offsets) {
  return assemble_map_common(ctx, n_nodes, node_ids, transforms, maximum_depth, preserve_raster, out, nullptr, false, capacity,
                             n_out, node_offsets, nullptr);
}

int rgbdfe_assemble_map_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                               double maximum_depth, int32_t preserve_raster, void* d_out, int64_t capacity, int64_t* n_out,
                               int64_t* node_offsets, void* stream) {
  return assemble_map_common(ctx, n_nodes, node_ids, transforms, maximum_depth, preserve_raster, nullptr, d_out, true, capacity,
                             n_out, node_offsets, stream);
}

int rgbdfe_download_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, float* cloud_out, int64_t capacity_points, int32_t* rows,
                               int32_t* cols) {
  if (!ctx || capacity_points < 0 || (capacity_points > 0 && !cloud_out))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const CloudEntry* found = resident_cloud(ctx, node_id);
  if (!found) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "no cloud for this node");
  const CloudEntry& ce = *found;
  if (rows) *rows = ce.ch;
  if (cols) *cols = ce.cw;
  const size_t n = (size_t)ce.ch * (size_t)ce.cw;
  if ((size_t)capacity_points < n) return fail(ctx, RGBDFE_ERR_CAPACITY, "cloud_out is too small (rows x cols points are needed)");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  HIP_TRY(ctx, hipMemcpyAsync(cloud_out, ce.d, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return RGBDFE_OK;
}

}  // namespace impl
