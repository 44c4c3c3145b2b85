// api_render.hip -- rendering: the display-geometry stream of the listed nodes rasterised into images (kernels: render.hip;
// the camera helpers: render_camera.h)
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"

#include "render.h"
#include "render_camera.h"

namespace impl {

namespace {

constexpr int64_t kRenderDefaultGroup = (int64_t)1 << 23;  // vertices in flight when the caller names no cap
constexpr double kReferenceFovy = 100.0 / 180.0 * rgbdfe::kRenderPi;  // fov_ (glviewer.cpp:118), handed over as degrees (:444)

bool all_finite(const double* m, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(m[i])) return false;
  return true;
}

// Exactly one of the host / device quadruples receives the images.
int render_common(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                  const rgbdfe_display_params* dp, const rgbdfe_render_params* rp, uint8_t* h_rgba, float* h_depth,
                  int64_t* h_ids, int32_t* h_node, void* d_rgba, void* d_depth, void* d_ids, void* d_node, bool to_device,
                  void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (n_nodes < 0 || !dp || !rp || (n_nodes > 0 && !node_ids) ||
      !(to_device ? d_rgba != nullptr && d_depth != nullptr : h_rgba != nullptr && h_depth != nullptr))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad render arguments");
  if (rp->width < 1 || rp->width > kRenderMaxSize || rp->height < 1 || rp->height > kRenderMaxSize)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "render: width and height must be in [1, 4096]");
  if (!all_finite(rp->view, 16) || !all_finite(rp->projection, 16))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "render: view and projection must be finite");
  if (!std::isfinite(rp->gl_point_size) || rp->gl_point_size <= 0.0)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "render: gl_point_size must be positive and finite");
  if ((rp->cull != 0 && rp->cull != 1) || rp->max_vertices_in_flight < 0)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "render: cull must be 0 or 1 and max_vertices_in_flight at least 0");
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t n = (size_t)n_nodes;
  // the sizes of the whole stream: every node's first vertex and form (this is also where an unknown id is found)
  std::vector<int64_t> off(n + 1), soff(n + 1);
  std::vector<int32_t> types(n + 1);
  int64_t total_v = 0, total_s = 0;
  int rc = display_locked(ctx, n_nodes, node_ids, transforms, dp, nullptr, nullptr, 0, &total_v, off.data(), nullptr, nullptr, 0,
                          &total_s, soff.data(), types.data(), true, stream, true);
  if (rc != RGBDFE_OK) return rc;
  if (total_v > (int64_t)0xfffffffell)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "render: a stream of more than 2^32 - 2 vertices");
  const int64_t cap = rp->max_vertices_in_flight > 0 ? std::min(rp->max_vertices_in_flight, kRenderMaxGroup) : kRenderDefaultGroup;
  // groups of consecutive nodes whose vertices together stay within the cap; nodes without a vertex join any group
  struct Group { size_t k0, k1; };
  std::vector<Group> groups;
  int64_t max_v = 0, max_s = 0;
  for (size_t k = 0; k < n;) {
    size_t e = k;
    while (e < n && off[e + 1] - off[k] <= cap) ++e;
    if (e == k) return fail(ctx, RGBDFE_ERR_CAPACITY, "render: a node's stream exceeds max_vertices_in_flight");
    if (off[e] > off[k]) {
      groups.push_back(Group{k, e});
      max_v = std::max(max_v, off[e] - off[k]);
      max_s = std::max(max_s, soff[e] - soff[k]);
    }
    k = e;
  }
  const size_t npix = (size_t)rp->width * (size_t)rp->height;
  DeviceLayout lay;
  std::vector<Block> b_first(groups.size());
  for (size_t gi = 0; gi < groups.size(); ++gi) {  // the nodes' firsts, counted from the group's own first vertex
    const Group& gr = groups[gi];
    std::vector<int64_t> first(gr.k1 - gr.k0 + 1);
    for (size_t k = gr.k0; k <= gr.k1; ++k) first[k - gr.k0] = off[k] - off[gr.k0];
    b_first[gi] = lay.put(first.data(), 8 * first.size());
  }
  const Block b_types = lay.put(types.data(), 4 * (n + 1));
  const Block b_vis = lay.room(8 * npix), b_count = lay.room(4), b_stats = lay.room(16), b_vertices = lay.room(16 * (size_t)max_v),
              b_strips = lay.room(16 * (size_t)max_s), b_queue = lay.room(4 * (size_t)max_v);
  Block b_rgba, b_depth, b_ids, b_node;
  if (!to_device) {
    b_rgba = lay.room(4 * npix);
    b_depth = lay.room(4 * npix);
    if (h_ids) b_ids = lay.room(8 * npix);
    if (h_node) b_node = lay.room(4 * npix);
  }
  rc = ctx->render.ensure(ctx, lay.total(), "render: scratch allocation failed");
  if (rc != RGBDFE_OK) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  void* base = ctx->render.p;
  if (lay.staged_bytes() > 0) HIP_TRY(ctx, hipMemcpyAsync(base, lay.staged(), lay.staged_bytes(), hipMemcpyHostToDevice, st));

  RenderCamera cam;
  memcpy(cam.view, rp->view, sizeof(cam.view));
  memcpy(cam.proj, rp->projection, sizeof(cam.proj));
  cam.W = rp->width;
  cam.H = rp->height;
  cam.point_n = (int32_t)std::min(std::max(std::floor(rp->gl_point_size + 0.5), 1.0), (double)kRenderMaxPoint);
  cam.cull = rp->cull;
  RenderImages img;
  img.rgba = to_device ? (uchar4*)d_rgba : at<uchar4>(base, b_rgba);
  img.depth = to_device ? (float*)d_depth : at<float>(base, b_depth);
  img.ids = to_device ? (int64_t*)d_ids : (h_ids ? at<int64_t>(base, b_ids) : nullptr);
  img.node_index = to_device ? (int32_t*)d_node : (h_node ? at<int32_t>(base, b_node) : nullptr);
  unsigned long long* vis = at<unsigned long long>(base, b_vis);
  uint32_t* queue_count = at<uint32_t>(base, b_count);
  unsigned long long* stats = at<unsigned long long>(base, b_stats);
  launch_render_clear(cam, make_uchar4(rp->clear_rgba[0], rp->clear_rgba[1], rp->clear_rgba[2], rp->clear_rgba[3]), vis, img,
                      queue_count, stats, st);
  HIP_TRY(ctx, hipGetLastError());

  // a group's stream becomes resident (the display-geometry call itself, into this call's buffer), is drawn and shaded;
  // the next group's vertices replace it behind the same stream
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const Group& gr = groups[gi];
    const int64_t gv = off[gr.k1] - off[gr.k0], gs = soff[gr.k1] - soff[gr.k0];
    int64_t nv = 0, ns = 0;
    rc = display_locked(ctx, (int32_t)(gr.k1 - gr.k0), node_ids + gr.k0, transforms ? transforms + 16 * gr.k0 : nullptr, dp, nullptr,
                        at<void>(base, b_vertices), gv, &nv, nullptr, nullptr, gs > 0 ? at<void>(base, b_strips) : nullptr, gs, &ns,
                        nullptr, nullptr, true, stream, false);
    if (rc != RGBDFE_OK) return rc;
    if (nv != gv || ns != gs) return fail(ctx, RGBDFE_ERR_INTERNAL, "render: a group's stream changed size");
    RenderGroup g;
    g.vertices = at<float4>(base, b_vertices);
    g.strips = at<int64_t>(base, b_strips);
    g.node_first = at<int64_t>(base, b_first[gi]);
    g.node_type = at<int32_t>(base, b_types) + gr.k0;
    g.n_vertices = (uint32_t)gv;
    g.n_strips = (uint32_t)gs;
    g.n_nodes = (uint32_t)(gr.k1 - gr.k0);
    g.node0 = (int32_t)gr.k0;
    g.base = (uint64_t)off[gr.k0];
    launch_render_group(g, cam, vis, at<uint32_t>(base, b_queue), queue_count, img, render_large_blocks(g.n_vertices), stats,
                        ctx->render_count_fragments, st);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (!to_device) {
    HIP_TRY(ctx, hipMemcpyAsync(h_rgba, img.rgba, 4 * npix, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(h_depth, img.depth, 4 * npix, hipMemcpyDeviceToHost, st));
    if (h_ids) HIP_TRY(ctx, hipMemcpyAsync(h_ids, img.ids, 8 * npix, hipMemcpyDeviceToHost, st));
    if (h_node) HIP_TRY(ctx, hipMemcpyAsync(h_node, img.node_index, 4 * npix, hipMemcpyDeviceToHost, st));
  }
  ctx->render_fragments[0] = ctx->render_fragments[1] = 0;
  if (ctx->render_count_fragments) HIP_TRY(ctx, hipMemcpyAsync(ctx->render_fragments, stats, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return RGBDFE_OK;
}

}  // namespace

int rgbdfe_render_fragment_stats(rgbdfe_ctx* ctx, int32_t enable, int64_t* out2) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (out2) {
    out2[0] = ctx->render_fragments[0];
    out2[1] = ctx->render_fragments[1];
  }
  if (enable >= 0) ctx->render_count_fragments = enable != 0;
  return RGBDFE_OK;
}

void rgbdfe_render_default_params(rgbdfe_render_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->width = 640;
  p->height = 480;
  render_viewer_view(0.0, 0.0, -50.0, 180.0 * 16.0, 0.0, 0.0, 1.0, nullptr, p->view);  // initialPosition (glviewer.cpp:137-144)
  render_perspective(kReferenceFovy, (double)((float)p->width / (float)p->height), 0.1, 1e4, p->projection);  // :443-444
  p->gl_point_size = 1.0;  // parameter_server.cpp:143
  p->cull = 1;             // glEnable(GL_CULL_FACE)
  p->clear_rgba[0] = p->clear_rgba[1] = p->clear_rgba[2] = p->clear_rgba[3] = 3;  // bg_col_ = 0.01 (:128)
  p->max_vertices_in_flight = 0;
}

int rgbdfe_render_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                        const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params, uint8_t* rgba,
                        float* depth, int64_t* ids, int32_t* node_index) {
  return render_common(ctx, n_nodes, node_ids, transforms, display_params, render_params, rgba, depth, ids, node_index, nullptr,
                       nullptr, nullptr, nullptr, false, nullptr);
}

int rgbdfe_render_nodes_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                               const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params,
                               void* d_rgba, void* d_depth, void* d_ids, void* d_node_index, void* stream) {
  return render_common(ctx, n_nodes, node_ids, transforms, display_params, render_params, nullptr, nullptr, nullptr, nullptr,
                       d_rgba, d_depth, d_ids, d_node_index, true, stream);
}

void rgbdfe_render_perspective(double fovy, double aspect, double z_near, double z_far, double* out16) {
  if (out16) render_perspective(fovy, aspect, z_near, z_far, out16);
}

void rgbdfe_render_viewer_view(double x_tra, double y_tra, double z_tra, double x_rot, double y_rot, double z_rot,
                               double rotation_stepping, const double* viewpoint, double* out16) {
  if (out16) render_viewer_view(x_tra, y_tra, z_tra, x_rot, y_rot, z_rot, rotation_stepping, viewpoint, out16);
}

void rgbdfe_render_sensor_camera(double fx, double fy, double cx, double cy, int32_t width, int32_t height, double z_near,
                                 double z_far, const double* pose, double* view_out16, double* projection_out16) {
  if (view_out16 && projection_out16)
    render_sensor_camera(fx, fy, cx, cy, width, height, z_near, z_far, pose, view_out16, projection_out16);
}

int rgbdfe_render_unproject(double x, double y, double depth, const double* view, const double* projection, int32_t width,
                            int32_t height, double* out3) {
  if (!view || !projection || !out3 || width < 1 || height < 1) return RGBDFE_ERR_INVALID_ARG;
  return render_unproject(x, y, depth, view, projection, width, height, out3) ? RGBDFE_OK : RGBDFE_ERR_INVALID_ARG;
}

}  // namespace impl
