// api_display.hip -- display geometry: the resident node clouds as GL points, triangles and triangle strips (kernels:
// display_geometry.hip)
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"

#include "display_geometry.h"

namespace impl {

// GLViewer::addPointCloud (glviewer.cpp:693-711) for every listed node.  Exactly one of the host / device pairs receives
// the output.  ctx->mu is held.  sizes_only: the sizes, offsets and forms, then RGBDFE_OK without a vertex written.
int display_locked(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                   const rgbdfe_display_params* params, float* h_vertices, void* d_vertices, int64_t vertex_capacity,
                   int64_t* n_vertices, int64_t* node_offsets, int64_t* h_strips, void* d_strips, int64_t strip_capacity,
                   int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types, bool to_device, void* stream,
                   bool sizes_only) {
  if (!ctx || n_nodes < 0 || !params || !n_vertices || !n_strips || vertex_capacity < 0 || strip_capacity < 0 ||
      (n_nodes > 0 && !node_ids) || (vertex_capacity > 0 && !(to_device ? d_vertices != nullptr : h_vertices != nullptr)) ||
      (strip_capacity > 0 && !(to_device ? d_strips != nullptr : h_strips != nullptr)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad display geometry arguments");
  if (params->display_type != RGBDFE_DISPLAY_POINTS && params->display_type != RGBDFE_DISPLAY_TRIANGLES &&
      params->display_type != RGBDFE_DISPLAY_TRIANGLE_STRIP)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "display geometry: unknown display_type");
  if (params->visualization_skip_step < 1)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "display geometry: visualization_skip_step must be at least 1");
  // the node table and the tile -> node map: one blob, one copy
  const size_t n = (size_t)n_nodes;
  std::vector<DispNode> table(n + 1);
  const bool as_points = params->squared_meshing_threshold < 0;  // :697
  const int64_t step = params->visualization_skip_step;
  int64_t tiles = 0, rows = 0;
  bool have_items = false, have_rows = false;
  for (size_t k = 0; k < n; ++k) {
    const CloudEntry* found = resident_cloud(ctx, node_ids[k]);
    if (!found) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "display geometry: no cloud for a listed node");
    const CloudEntry& ce = *found;
    const int64_t w = ce.cw, h = ce.ch;
    if (w * h > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "display geometry: a cloud of more than 2^31 points");
    DispNode& m = table[k];
    memset(&m, 0, sizeof(m));
    m.cloud = ce.d;
    m.w = (int32_t)w;
    m.h = (int32_t)h;
    m.type = (h <= 1 || as_points) ? RGBDFE_DISPLAY_POINTS : params->display_type;  // !isOrganized(): height == 1
    m.step = (int32_t)step;
    int64_t items = 0, tile = kDispItemTile;
    if (m.type == RGBDFE_DISPLAY_POINTS) {
      items = w * h;
      m.items_h = (uint32_t)h;
    } else if (m.type == RGBDFE_DISPLAY_TRIANGLES) {
      items = w >= 2 ? (w - 1) * (h - 1) : 0;
      m.items_h = (uint32_t)(h - 1);
    } else {  // the rows y = 0, step, ... < h - step; none of them visits a column unless 0 < w - step
      items = (h > step && w > step) ? (h - 1) / step : 0;
      tile = kDispRowTile;
      m.first_row = (uint32_t)rows;
      rows += items;
    }
    m.n_items = (uint32_t)items;
    m.first_tile = (uint32_t)tiles;
    if (items > 0) (m.type == RGBDFE_DISPLAY_TRIANGLE_STRIP ? have_rows : have_items) = true;
    if (transforms) rigid_of_matrix4f(transforms + k * 16, m.R, m.t);
    tiles += (items + tile - 1) / tile;
    if (tiles > (int64_t)INT32_MAX || rows > (int64_t)INT32_MAX)
      return fail(ctx, RGBDFE_ERR_CAPACITY, "display geometry: more than 2^31 tiles in one call");
  }
  *n_vertices = 0;
  *n_strips = 0;
  if (node_types)
    for (size_t k = 0; k < n; ++k) node_types[k] = table[k].type;
  if (n_nodes == 0) {
    if (node_offsets) node_offsets[0] = 0;
    if (node_strip_offsets) node_strip_offsets[0] = 0;
    return RGBDFE_OK;
  }
  DispNode& end = table[n];
  memset(&end, 0, sizeof(end));
  end.first_tile = (uint32_t)tiles;
  end.first_row = (uint32_t)rows;
  const size_t n_tiles = (size_t)tiles;
  DeviceLayout lay;
  const NodeTableBlocks b_nodes_in = put_node_table(lay, table);

  DispParams prm;
  prm.mesh_thresh = (float)params->squared_meshing_threshold;  // `const float mesh_thresh` (:784, :997)
  prm.max_depth = (float)params->maximum_depth;                // `const float max_depth` (:785, :972, :1007)
  prm.transform = transforms ? 1u : 0u;

  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const Block b_count = lay.room(8 * n_tiles), b_rows = lay.room(8 * (size_t)rows), b_first = lay.room(16 * (n_tiles + 1)),
              b_nodes = lay.room(16 * (n + 1));
  int rc = ensure_scratch(ctx, lay.total());
  if (rc != RGBDFE_OK) return rc;
  void* base = ctx->d_scratch;
  const DispNode* d_table = at<DispNode>(base, b_nodes_in.table);
  const uint32_t* d_tile_node = at<uint32_t>(base, b_nodes_in.tile_node);
  uint2* d_count = at<uint2>(base, b_count);
  uint2* d_rows = at<uint2>(base, b_rows);
  int64_t* d_first = at<int64_t>(base, b_first);
  int64_t* d_node_first = at<int64_t>(base, b_nodes);
  HIP_TRY(ctx, hipMemcpyAsync(base, lay.staged(), lay.staged_bytes(), hipMemcpyHostToDevice, st));

  launch_display_count_scan(d_table, d_tile_node, (uint32_t)n, (uint32_t)n_tiles, prm, have_items, have_rows, d_count, d_rows,
                            d_first, d_node_first, st);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<int64_t> first(2 * (n + 1));  // the one read of the sizes: the nodes' firsts and the totals
  HIP_TRY(ctx, hipMemcpyAsync(first.data(), d_node_first, 16 * (n + 1), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const int64_t total_v = first[2 * n], total_s = first[2 * n + 1];
  *n_vertices = total_v;
  *n_strips = total_s;
  for (size_t k = 0; k <= n; ++k) {
    if (node_offsets) node_offsets[k] = first[2 * k];
    if (node_strip_offsets) node_strip_offsets[k] = first[2 * k + 1];
  }
  if (sizes_only) return RGBDFE_OK;
  if (vertex_capacity < total_v || strip_capacity < total_s)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "display geometry: a buffer is too small (*n_vertices rows and *n_strips records are needed)");
  if (total_v == 0) return RGBDFE_OK;  // no vertex, so no strip either
  OutputSink sink_v(to_device ? d_vertices : nullptr), sink_s(to_device ? d_strips : nullptr);
  const char* no_staging = "display geometry: staging allocation failed";
  rc = sink_v.ready(ctx, (size_t)total_v * sizeof(float4), no_staging);
  if (rc == RGBDFE_OK && total_s > 0) rc = sink_s.ready(ctx, (size_t)total_s * 16, no_staging);
  if (rc != RGBDFE_OK) return rc;
  launch_display_write(d_table, d_tile_node, (uint32_t)n_tiles, prm, have_items, have_rows, d_rows, d_first, (float4*)sink_v.d,
                       (int64_t*)sink_s.d, st);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, sink_v.finish(h_vertices, st));
  if (total_s > 0) HIP_TRY(ctx, sink_s.finish(h_strips, st));
  // the table in the context's scratch is this call's: it returns when the stream has passed it
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return RGBDFE_OK;
}

namespace {

int display_common(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                   const rgbdfe_display_params* params, float* h_vertices, void* d_vertices, int64_t vertex_capacity,
                   int64_t* n_vertices, int64_t* node_offsets, int64_t* h_strips, void* d_strips, int64_t strip_capacity,
                   int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types, bool to_device, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  return display_locked(ctx, n_nodes, node_ids, transforms, params, h_vertices, d_vertices, vertex_capacity, n_vertices,
                        node_offsets, h_strips, d_strips, strip_capacity, n_strips, node_strip_offsets, node_types, to_device,
                        stream, false);
}

}  // namespace

void rgbdfe_display_default_params(rgbdfe_display_params* p) {
  if (!p) return;
  p->display_type = RGBDFE_DISPLAY_POINTS;        // parameter_server.cpp:151
  p->visualization_skip_step = 1;                 // :139
  p->squared_meshing_threshold = 0.0009;          // :148
  p->maximum_depth = std::numeric_limits<double>::infinity();  // :38
}

int rgbdfe_display_geometry(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                            const rgbdfe_display_params* params, float* vertices, int64_t vertex_capacity, int64_t* n_vertices,
                            int64_t* node_offsets, int64_t* strips, int64_t strip_capacity, int64_t* n_strips,
                            int64_t* node_strip_offsets, int32_t* node_types) {
  return display_common(ctx, n_nodes, node_ids, transforms, params, vertices, nullptr, vertex_capacity, n_vertices, node_offsets,
                        strips, nullptr, strip_capacity, n_strips, node_strip_offsets, node_types, false, nullptr);
}

int rgbdfe_display_geometry_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                                   const rgbdfe_display_params* params, void* d_vertices, int64_t vertex_capacity,
                                   int64_t* n_vertices, int64_t* node_offsets, void* d_strips, int64_t strip_capacity,
                                   int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types, void* stream) {
  return display_common(ctx, n_nodes, node_ids, transforms, params, nullptr, d_vertices, vertex_capacity, n_vertices, node_offsets,
                        nullptr, d_strips, strip_capacity, n_strips, node_strip_offsets, node_types, true, stream);
}

}  // namespace impl
