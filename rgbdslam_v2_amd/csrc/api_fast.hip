// api_fast.hip -- feature_detector_type "FAST": the host side of fast_detect.hip (one of the host-side translation units of
// librgbdfe.so; shared declarations: rgbdfe_host.h).  DESIGN.md section 4.13.
//
// Frames go through in chunks (up to 32 at 640 x 480, fewer for larger frames) with kSlots chunks in flight: a helper thread
// copies chunk c + 2's pageable images into its page-locked staging buffer while chunk c + 1 is uploaded (its own stream,
// with the blur of its gray images) and chunk c runs its four launches (pass, adjuster, select, rBRIEF) on the kernel
// stream.  Nothing of a chunk returns to the host before its outputs: the kernels write the keypoints, descriptors and points
// straight into the node slabs and / or the chunk's output rows (copied to page-locked memory behind the chunk only when
// the caller asked for them), and the per-cell thresholds stay on the device for the whole call (read back once at its end).
#include <cmath>

#include "rgbdfe_host.h"
#include "staging_ring.h"

#include "orb_pattern.inc"  // kOrbBitPattern31

namespace rgbdfe {

namespace {
// frames per chunk: about 10 Mpixel (32 frames at 640 x 480, 8 at 1280 x 960)
int chunk_frames(int rows, int cols) {
  const double px = (double)rows * (double)cols;
  return std::max(1, std::min(32, (int)(10.0e6 / px)));
}
}  // namespace

FastWorkspace::~FastWorkspace() { release(); }

void FastWorkspace::release_slot(Slot& s) {
  if (s.dev) (void)hipFree(s.dev);
  if (s.pin) (void)hipHostFree(s.pin);
  if (s.uploaded) (void)hipEventDestroy(s.uploaded);
  if (s.done) (void)hipEventDestroy(s.done);
  s = Slot();
}

void FastWorkspace::release() {
  for (Slot& s : slot) release_slot(s);
  if (st) (void)hipStreamDestroy(st);
  if (up) (void)hipStreamDestroy(up);
  if (d_thresh) (void)hipFree(d_thresh);
  if (h_thresh) (void)hipHostFree(h_thresh);
  if (d_pattern) (void)hipFree(d_pattern);
  st = up = nullptr; d_thresh = nullptr; h_thresh = nullptr; d_pattern = nullptr;
  W = H = 0;
}

int FastWorkspace::ensure_common(std::string& err) {
  if (st) return RGBDFE_OK;
  if (create_side_stream(&st, +1) != hipSuccess || create_side_stream(&up, -1) != hipSuccess) { err = "stream creation"; return RGBDFE_ERR_HIP; }
  if (hipMalloc((void**)&d_thresh, 64 * sizeof(double)) != hipSuccess ||
      hipHostMalloc((void**)&h_thresh, 64 * sizeof(double), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&d_pattern, 1024) != hipSuccess) {
    err = "FAST workspace allocation";
    return RGBDFE_ERR_OUT_OF_MEMORY;
  }
  if (hipMemcpyAsync(d_pattern, kOrbBitPattern31, 1024, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    err = "pattern upload";
    return RGBDFE_ERR_HIP;
  }
  return RGBDFE_OK;
}

int FastWorkspace::prepare(int cols, int rows, int grid_res, bool grid_mode, int max_total, int max_kp, bool desc, std::string& err) {
  if (cols > 65535 || rows > 65535 || (size_t)rows * cols > ((size_t)1 << 28)) { err = "FAST: frame too large"; return RGBDFE_ERR_CAPACITY; }
  const int G = grid_mode ? grid_res : 1;
  const int lcap = grid_mode ? std::max(max_total, 1) : std::max(((cols + 1) / 2) * ((rows + 1) / 2), 1);
  const int orows = desc ? max_kp : 0;
  if (cols == W && rows == H && G == grid && grid_mode == use_grid && lcap == list_cap && orows == out_rows && desc == describe)
    return RGBDFE_OK;
  ++version;
  W = cols; H = rows; grid = G; use_grid = grid_mode; list_cap = lcap; out_rows = orows; describe = desc;
  plane = (uint32_t)((size_t)rows * cols);
  const int edge = grid_mode ? 31 : 0;  // VideoGridAdaptedFeatureDetector edgeThreshold (feature_adjuster.h)
  geom = FastGeom{};
  geom.n_cells = G * G; geom.rows = rows; geom.cols = cols; geom.plane = plane;
  int tiles = 0;
  uint32_t keep_words = 0, score_bytes = 0;
  for (int i = 0; i < G; ++i) {
    const int rowstart = std::max((i * rows) / G - edge, 0);
    const int rowend = std::min(rows, ((i + 1) * rows) / G + edge);
    for (int j = 0; j < G; ++j) {
      const int colstart = std::max((j * cols) / G - edge, 0);
      const int colend = std::min(cols, ((j + 1) * cols) / G + edge);
      FastCellGeom& c = geom.cell[i * G + j];
      c.x0 = colstart; c.y0 = rowstart; c.w = colend - colstart; c.h = rowend - rowstart;
      c.tiles_x = (c.w + 63) / 64;
      c.tile_begin = tiles;
      tiles += c.tiles_x * ((c.h + 15) / 16);
      c.keep_off = keep_words;
      keep_words += (uint32_t)(c.tiles_x * c.h);
      c.score_off = score_bytes;
      score_bytes += (uint32_t)(c.w * c.h);
    }
  }
  geom.tiles_per_frame = tiles;
  geom.keep_words = keep_words;
  geom.score_bytes = (score_bytes + 3u) & ~3u;
  blur_units_per_frame = ((cols + 63) / 64) * ((rows + 15) / 16);
  return RGBDFE_OK;
}

int FastWorkspace::ensure_slot(int i, int frames, std::string& err) {
  Slot& s = slot[i];
  if (s.dev && s.version == version && s.cap >= frames) return RGBDFE_OK;
  const size_t B = (size_t)frames, cells = (size_t)geom.n_cells;
  if ((size_t)blur_units_per_frame * B > 65535 * 64 || B * plane * 2 + 256 > 0xFFFFFFFFull) { err = "FAST: chunk too large"; return RGBDFE_ERR_CAPACITY; }
  // device
  Arena dv;
  const size_t o_img = dv.carve(2 * B * plane + 256), o_blur = dv.carve(describe ? B * plane : 0),
               o_depth = dv.carve(describe ? B * plane * 4 : 0), o_hm = dv.carve(B * 4), o_keep = dv.carve(B * geom.keep_words * 8),
               o_score = dv.carve(B * geom.score_bytes), o_hist = dv.carve(B * cells * 257 * 4), o_cut = dv.carve(B * cells * sizeof(FastCut)),
               o_list = dv.carve(B * (size_t)list_cap * sizeof(FastKp)), o_n = dv.carve(B * 4), o_outs = dv.carve(B * sizeof(FastFrameOut)),
               o_imgs = dv.carve(B * sizeof(ImgDesc)), o_units = dv.carve(B * blur_units_per_frame * sizeof(TileUnit)),
               o_kp = dv.carve(B * (size_t)out_rows * sizeof(FastKpOut)), o_desc = dv.carve(B * (size_t)out_rows * 32),
               o_xyz = dv.carve(B * (size_t)out_rows * 16);
  if (dv.size > s.dev_bytes) {
    if (s.dev) (void)hipFree(s.dev);
    s.dev = nullptr; s.dev_bytes = 0; s.version = -1;
    if (hipMalloc(&s.dev, dv.size) != hipSuccess) { s.dev = nullptr; err = "FAST chunk buffers"; return RGBDFE_ERR_OUT_OF_MEMORY; }
    s.dev_bytes = dv.size;
  }
  char* d = (char*)s.dev;
  s.d_img = (uint8_t*)(d + o_img); s.d_blur = (uint8_t*)(d + o_blur); s.d_depth = (float*)(d + o_depth);
  s.d_has_mask = (int32_t*)(d + o_hm); s.d_keep = (uint64_t*)(d + o_keep); s.d_score = (uint8_t*)(d + o_score);
  s.d_hist = (int32_t*)(d + o_hist); s.d_mask_nz = s.d_hist + B * cells * 256; s.hist_bytes = B * cells * 257 * 4;
  s.d_cut = (FastCut*)(d + o_cut); s.d_list = (FastKp*)(d + o_list); s.d_n = (int32_t*)(d + o_n);
  s.d_outs = (FastFrameOut*)(d + o_outs); s.d_frame_imgs = (ImgDesc*)(d + o_imgs); s.d_blur_units = (TileUnit*)(d + o_units);
  s.d_kp = (FastKpOut*)(d + o_kp); s.d_desc = (uint8_t*)(d + o_desc); s.d_xyz = (float4*)(d + o_xyz);
  // page-locked
  Arena pn;
  const size_t rows_out = (size_t)out_rows;
  const size_t p_img = pn.carve(2 * B * plane), p_depth = pn.carve(describe ? B * plane * 4 : 0), p_hm = pn.carve(B * 4),
               p_outs = pn.carve(B * sizeof(FastFrameOut)), p_n = pn.carve(B * 4), p_kp = pn.carve(B * rows_out * sizeof(FastKpOut)),
               p_desc = pn.carve(B * rows_out * 32), p_xyz = pn.carve(B * rows_out * 16),
               p_list = pn.carve(describe ? 0 : B * (size_t)list_cap * sizeof(FastKp)), p_tab = pn.carve(B * sizeof(ImgDesc) + B * blur_units_per_frame * sizeof(TileUnit));
  if (pn.size > s.pin_bytes) {
    if (s.pin) (void)hipHostFree(s.pin);
    s.pin = nullptr; s.pin_bytes = 0; s.version = -1;
    if (hipHostMalloc(&s.pin, pn.size, hipHostMallocDefault) != hipSuccess) { s.pin = nullptr; err = "FAST staging buffers"; return RGBDFE_ERR_OUT_OF_MEMORY; }
    s.pin_bytes = pn.size;
  }
  char* h = (char*)s.pin;
  s.h_img = (uint8_t*)(h + p_img); s.h_depth = (float*)(h + p_depth); s.h_has_mask = (int32_t*)(h + p_hm);
  s.h_outs = (FastFrameOut*)(h + p_outs); s.h_n = (int32_t*)(h + p_n); s.h_kp = (FastKpOut*)(h + p_kp);
  s.h_desc = (uint8_t*)(h + p_desc); s.h_xyz = (float4*)(h + p_xyz); s.h_list = (FastKp*)(h + p_list);
  if ((!s.uploaded && hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming) != hipSuccess) ||
      (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess)) {
    err = "event creation";
    return RGBDFE_ERR_HIP;
  }
  // the blur's image table (frame k: gray at k x plane, blurred copy at k x plane of d_blur) and its 64 x 16 tiles
  ImgDesc* imgs = (ImgDesc*)(h + p_tab);
  TileUnit* units = (TileUnit*)(imgs + B);
  const int tx = (W + 63) / 64, ty = (H + 15) / 16;
  for (size_t k = 0; k < B; ++k) {
    ImgDesc im{};
    im.off = (uint32_t)(k * plane); im.w = W; im.h = H; im.stride = W; im.score_off = (uint32_t)(k * plane);
    imgs[k] = im;
    for (int by = 0; by < ty; ++by)
      for (int bx = 0; bx < tx; ++bx) units[k * blur_units_per_frame + (size_t)by * tx + bx] = TileUnit{(uint16_t)k, (uint16_t)bx, (uint16_t)by, 0};
  }
  if (hipMemcpyAsync(s.d_frame_imgs, imgs, B * sizeof(ImgDesc), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(s.d_blur_units, units, B * blur_units_per_frame * sizeof(TileUnit), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    err = "FAST table upload";
    return RGBDFE_ERR_HIP;
  }
  s.cap = (int)B;
  s.version = version;
  return RGBDFE_OK;
}

}  // namespace rgbdfe

namespace impl {

namespace {

// One call of the FAST pipeline over n_frames frames.  describe = false: the aggregated grid keypoints (grid) or the
// keypoints at fixed_thr (!grid) of frame 0 into *list_out.
struct FastCall {
  rgbdfe_ctx* ctx = nullptr;
  int32_t n_frames = 0;
  const uint8_t* const* gray = nullptr; const uint8_t* const* mask = nullptr; const float* const* depth = nullptr;
  const SensorRun* sensor = nullptr;   // sensor frames in place of the three plane arrays: ingest.hip's kernel fills the chunk's planes
  int32_t rows = 0, cols = 0;
  bool grid = true, describe = true;
  int fixed_thr = -1;
  double fx = 0, fy = 0, cx = 0, cy = 0, depth_scaling = 1;
  int32_t out_stride = 0;
  rgbdfe_keypoint* keypoints = nullptr; uint8_t* descriptors = nullptr; float* xyz1 = nullptr; int32_t* n_out = nullptr;
  const int32_t* node_ids = nullptr;
  std::vector<KpOut>* list_out = nullptr;

  int run(std::string& err);
};

int FastCall::run(std::string& err) {
  FastWorkspace& fw = ctx->fast;
  const OrbWorkspace& det = ctx->orb;  // the detector configuration and state
  const int max_kp = ctx->orb_max_keypoints;
  int rc = fw.ensure_common(err);
  if (rc == RGBDFE_OK) rc = fw.prepare(cols, rows, det.grid, grid, det.max_total, max_kp, describe, err);
  if (rc != RGBDFE_OK) return rc;
  const int B = describe ? std::min(n_frames, chunk_frames(rows, cols)) : 1;
  const int n_chunks = (n_frames + B - 1) / B;
  const int K = FastWorkspace::kSlots;
  for (int i = 0; i < std::min(K, n_chunks); ++i)
    if ((rc = fw.ensure_slot(i, B, err)) != RGBDFE_OK) return rc;
  if (sensor && (rc = sensor_ensure(ctx, K, K, sensor->frame_bytes * (size_t)B, 0, 0)) != RGBDFE_OK) { err.clear(); return rc; }
  hipStream_t st = fw.st, up = fw.up;
  const size_t plane = fw.plane;
  const int cells = fw.geom.n_cells;
  FastAdjust adj{cells, det.cell_min, det.cell_max, det.adjuster_iters, grid ? det.max_total / cells : INT32_MAX,
                 grid ? -1 : std::min(std::max(fixed_thr, 0), 255)};
  const int floor_thr = grid ? 2 : adj.fixed_thr;  // the adjuster never asks for less than 2 (min_thresh, feature_adjuster.h)
  FastSelect sel{};
  sel.n_cells = cells; sel.list_cap = fw.list_cap; sel.max_kp = max_kp; sel.min_depth = ctx->feature_min_depth ? 1 : 0;
  sel.describe = describe ? 1 : 0; sel.rows = rows; sel.cols = cols;
  sel.fxinv = (float)(1. / fx); sel.fyinv = (float)(1. / fy); sel.cx = (float)cx; sel.cy = (float)cy;
  sel.depth_scaling = depth_scaling;
  // computeOrbDescriptors' rotation for angle -1 (orb_host.hip compute_prepare: the double functions rounded to float)
  float angle = -1.f;
  angle *= (float)(M_PI / 180.f);
  const float cos_a = (float)std::cos((double)angle), sin_a = (float)std::sin((double)angle);
  if (grid) {
    for (int i = 0; i < cells; ++i) fw.h_thresh[i] = det.thresh[i];
    if (hipMemcpyAsync(fw.d_thresh, fw.h_thresh, sizeof(double) * cells, hipMemcpyHostToDevice, st) != hipSuccess) return RGBDFE_ERR_HIP;
  }
  auto first_of = [&](int c) { return c * B; };
  auto count_of = [&](int c) { return std::min(B, n_frames - c * B); };
  // staging: the caller's pageable images -> the slot's page-locked buffers (pure CPU work, any thread)
  auto stage = [&](int c, TaskPool* pool) {
    FastWorkspace::Slot& s = fw.slot[c % K];
    const int nf = count_of(c);
    for (int k = 0; k < nf; ++k) {
      const int f = first_of(c) + k;
      const uint8_t* mk = mask ? mask[f] : nullptr;
      s.h_has_mask[k] = (mk || sensor) ? 1 : 0;
      uint8_t* const raw = sensor ? ctx->sensor.h_raw[c % K] + (size_t)k * sensor->frame_bytes : nullptr;
      auto job = [&s, &plane, this, f, k, mk, B, raw]() {
        if (sensor) { sensor->stage(f, raw); return; }   // the raw bytes, nothing else
        memcpy(s.h_img + (size_t)k * plane, gray[f], plane);
        if (mk) memcpy(s.h_img + ((size_t)B + k) * plane, mk, plane);
        if (describe) memcpy(s.h_depth + (size_t)k * plane, depth[f], plane * 4);
      };
      if (pool) pool->submit(job); else job();
    }
    if (pool) pool->wait_all();
  };
  // runs of several chunks: a helper thread stages chunk c once chunk c - K has been collected (its slot is free then)
  TaskPool* const copy_pool = n_chunks > 1 ? &stage_pool(ctx) : nullptr;
  StagingRing ring(n_chunks > 1 ? n_chunks : 0, K, [&](int c) { stage(c, copy_pool); });
  const size_t ms = (size_t)ctx->cfg.max_keypoints;
  auto enqueue = [&](int c) -> int {
    FastWorkspace::Slot& s = fw.slot[c % K];
    const int nf = count_of(c), f0 = first_of(c);
    if (n_chunks > 1) ring.wait_staged(c);
    else stage(c, nullptr);
    bool any_mask = false;
    for (int k = 0; k < nf; ++k) any_mask = any_mask || s.h_has_mask[k];
    // where the outputs go; nodes are registered before anything can fail (no slot goes missing), their counts at collect()
    for (int k = 0; k < nf; ++k) {
      const int f = f0 + k;
      FastFrameOut o{};
      if (describe) {
        const size_t r = (size_t)k * fw.out_rows;
        if (keypoints) o.out_kp = s.d_kp + r;
        if (descriptors) o.out_desc = s.d_desc + r * 32;
        if (xyz1) o.out_xyz = s.d_xyz + r;
        if (node_ids && node_ids[f] >= 0) {
          uint32_t sl;
          const int rc_slot = acquire_node_slot(ctx, node_ids[f], 0u, &sl, true);   // (the lanes: fast_detect_describe waited)
          if (rc_slot != RGBDFE_OK) { err = ctx->last_error; return rc_slot; }
          ctx->nodes[node_ids[f]] = NodeEntry{sl, 0u, 0u, 0u};
          o.node_desc = ctx->d_desc + (size_t)sl * ms * 8;
          o.node_xyz = ctx->d_xyz + (size_t)sl * ms;
        }
      }
      s.h_outs[k] = o;
    }
    // uploads + the blur (it needs nothing but the gray images) on their own stream
    if (sensor) {  // frame k: gray at k x plane, mask at (B + k) x plane of d_img, depth at k x plane of d_depth
      IngestParams o{};
      o.gray = s.d_img; o.gray_stride = plane;
      o.mask = s.d_img + (size_t)B * plane; o.mask_stride = plane;
      if (describe) { o.depth_m = s.d_depth; o.depth_stride = plane; }
      const int r = sensor_upload_ingest(ctx, *sensor, c % K, c % K, nf, o, up);
      if (r != RGBDFE_OK) { err.clear(); return r; }
    }
    if ((!sensor && hipMemcpyAsync(s.d_img, s.h_img, (size_t)nf * plane, hipMemcpyHostToDevice, up) != hipSuccess) ||
        (!sensor && any_mask && hipMemcpyAsync(s.d_img + (size_t)B * plane, s.h_img + (size_t)B * plane, (size_t)nf * plane,
                                    hipMemcpyHostToDevice, up) != hipSuccess) ||
        hipMemcpyAsync(s.d_has_mask, s.h_has_mask, (size_t)nf * 4, hipMemcpyHostToDevice, up) != hipSuccess ||
        (!sensor && describe && hipMemcpyAsync(s.d_depth, s.h_depth, (size_t)nf * plane * 4, hipMemcpyHostToDevice, up) != hipSuccess) ||
        hipMemcpyAsync(s.d_outs, s.h_outs, (size_t)nf * sizeof(FastFrameOut), hipMemcpyHostToDevice, up) != hipSuccess) {
      err = "FAST chunk upload";
      return RGBDFE_ERR_HIP;
    }
    if (describe) launch_orb_blur_always(s.d_img, s.d_frame_imgs, s.d_blur_units, nf * fw.blur_units_per_frame, s.d_blur, up);
    if (hipGetLastError() != hipSuccess || hipEventRecord(s.uploaded, up) != hipSuccess) { err = "FAST upload enqueue"; return RGBDFE_ERR_HIP; }
    if (hipStreamWaitEvent(st, s.uploaded, 0) != hipSuccess ||
        hipMemsetAsync(s.d_hist, 0, s.hist_bytes, st) != hipSuccess) { err = "FAST chunk setup"; return RGBDFE_ERR_HIP; }
    launch_fast_pass(s.d_img, s.d_img + (size_t)B * plane, s.d_has_mask, fw.geom, nf, floor_thr, s.d_keep, s.d_score, s.d_hist,
                     s.d_mask_nz, st);
    launch_fast_adjust(s.d_hist, s.d_mask_nz, s.d_has_mask, nf, adj, fw.d_thresh, s.d_cut, st);
    launch_fast_select(fw.geom, nf, s.d_keep, s.d_score, s.d_cut, s.d_depth, sel, s.d_list, s.d_outs, s.d_n, st);
    if (describe)
      launch_fast_brief(s.d_img, s.d_blur, (uint32_t)plane, rows, cols, nf, max_kp, s.d_list, fw.list_cap, s.d_n, s.d_outs,
                        fw.d_pattern, cos_a, sin_a, st);
    const size_t rows_out = (size_t)nf * fw.out_rows;   // the output rows the caller asked for: one copy per array
    if (hipGetLastError() != hipSuccess ||
        (describe && keypoints && hipMemcpyAsync(s.h_kp, s.d_kp, rows_out * sizeof(FastKpOut), hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (describe && descriptors && hipMemcpyAsync(s.h_desc, s.d_desc, rows_out * 32, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (describe && xyz1 && hipMemcpyAsync(s.h_xyz, s.d_xyz, rows_out * 16, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipMemcpyAsync(s.h_n, s.d_n, (size_t)nf * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipEventRecord(s.done, st) != hipSuccess) {
      err = "FAST launch";
      return RGBDFE_ERR_HIP;
    }
    return RGBDFE_OK;
  };
  auto collect = [&](int c) -> int {
    FastWorkspace::Slot& s = fw.slot[c % K];
    const int nf = count_of(c), f0 = first_of(c);
    if (hipEventSynchronize(s.done) != hipSuccess) { err = "FAST chunk"; return RGBDFE_ERR_HIP; }
    if (!describe) {  // one frame: its aggregated keypoint list
      const int n = s.h_n[0];
      if (n > 0 && (hipMemcpyAsync(s.h_list, s.d_list, (size_t)n * sizeof(FastKp), hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess)) {
        err = "FAST keypoint read-back";
        return RGBDFE_ERR_HIP;
      }
      list_out->resize((size_t)n);
      for (int i = 0; i < n; ++i) {
        const FastKp& q = s.h_list[i];
        (*list_out)[(size_t)i] = KpOut{(float)q.x, (float)q.y, 7.f, -1.f, (float)q.s, 0};
      }
    } else {
      for (int k = 0; k < nf; ++k) {
        const int f = f0 + k;
        const int n = s.h_n[k];
        const size_t r = (size_t)k * fw.out_rows, o = (size_t)f * out_stride;
        n_out[f] = n;
        if (keypoints && n) memcpy(keypoints + o, s.h_kp + r, sizeof(rgbdfe_keypoint) * (size_t)n);
        if (descriptors && n) memcpy(descriptors + o * 32, s.h_desc + r * 32, (size_t)32 * n);
        if (xyz1 && n) memcpy(xyz1 + o * 4, s.h_xyz + r, (size_t)16 * n);
        if (node_ids && node_ids[f] >= 0) {
          NodeEntry& e = ctx->nodes[node_ids[f]];
          e.n = (uint32_t)n;
          launch_hamming_expand(ctx->d_desc + (size_t)e.slot * ms * 8, ctx->d_desc4, e.slot, (uint32_t)ms, (uint32_t)n, st);
        }
      }
      if (hipGetLastError() != hipSuccess) { err = "hamming expand"; return RGBDFE_ERR_HIP; }
    }
    ring.mark_consumed(c);
    return RGBDFE_OK;
  };
  for (int c = 0; c < n_chunks && rc == RGBDFE_OK; ++c) {
    if (c >= K) rc = collect(c - K);
    if (rc == RGBDFE_OK) rc = enqueue(c);
  }
  for (int c = std::max(0, n_chunks - K); c < n_chunks && rc == RGBDFE_OK; ++c) rc = collect(c);
  ring.stop();
  (void)hipStreamSynchronize(up);
  (void)hipStreamSynchronize(st);
  if (rc != RGBDFE_OK) return rc;
  if (grid) {  // the detector's state goes back to the context
    if (hipMemcpyAsync(fw.h_thresh, fw.d_thresh, sizeof(double) * cells, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      err = "threshold read-back";
      return RGBDFE_ERR_HIP;
    }
    for (int i = 0; i < cells; ++i) ctx->orb.thresh[i] = fw.h_thresh[i];
  }
  return RGBDFE_OK;
}

}  // namespace

int fast_detect_describe(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                         const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy,
                         double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints, uint8_t* descriptors,
                         float* xyz1, int32_t* n_out, const int32_t* node_ids, const SensorRun* sensor) {
  if (n_frames == 0) return RGBDFE_OK;
  const int max_kp = ctx->orb_max_keypoints;
  if (node_ids) {  // all-or-nothing on capacity, as the ORB batch (every fresh id counted: empty frames become empty nodes)
    if (max_kp > ctx->cfg.max_keypoints)
      return fail(ctx, RGBDFE_ERR_CAPACITY, "the detector's max_keypoints exceeds the context's max_keypoints (node rows)");
    const int rc = reserve_node_slots(ctx, n_frames, node_ids, 0u, nullptr);   // (the slots: taken chunk by chunk)
    if (rc != RGBDFE_OK) return rc;
  }
  for (int32_t f = 0; f < n_frames; ++f) n_out[f] = 0;
  FastCall call;
  call.ctx = ctx; call.n_frames = n_frames; call.gray = gray; call.mask = mask; call.depth = depth; call.rows = rows; call.cols = cols;
  call.fx = fx; call.fy = fy; call.cx = cx; call.cy = cy; call.depth_scaling = depth_scaling;
  call.out_stride = out_stride; call.keypoints = keypoints; call.descriptors = descriptors; call.xyz1 = xyz1; call.n_out = n_out;
  call.node_ids = node_ids; call.sensor = sensor;
  std::string err;
  const int rc = call.run(err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err.empty() ? "FAST detection failed" : err);
  return RGBDFE_OK;
}

int fast_grid_keypoints(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                        std::vector<KpOut>& kps) {
  FastCall call;
  call.ctx = ctx; call.n_frames = 1; call.gray = &gray; call.mask = &mask; call.rows = rows; call.cols = cols;
  call.describe = false; call.list_out = &kps;
  std::string err;
  const int rc = call.run(err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err.empty() ? "FAST detection failed" : err);
  return RGBDFE_OK;
}

int rgbdfe_set_detector_type(rgbdfe_ctx* ctx, int32_t type) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (type != RGBDFE_DETECTOR_ORB && type != RGBDFE_DETECTOR_FAST) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "unknown detector type");
  std::lock_guard<std::mutex> g(ctx->mu);
  ensure_detector(ctx);
  ctx->detector_type = type;
  for (int i = 0; i < 64; ++i) ctx->orb.thresh[i] = 20.0;  // a fresh createDetector: DetectorAdjuster(type, 20)
  return RGBDFE_OK;
}

int rgbdfe_fast_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols, int32_t threshold,
                       rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out) {
  if (!ctx || !gray || rows < 1 || cols < 1 || !n_out || capacity < 0 || (capacity > 0 && !keypoints))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  std::vector<KpOut> kps;
  FastCall call;
  call.ctx = ctx; call.n_frames = 1; call.gray = &gray; call.mask = &mask; call.rows = rows; call.cols = cols;
  call.grid = false; call.describe = false; call.fixed_thr = threshold; call.list_out = &kps;
  std::string err;
  const int rc = call.run(err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err.empty() ? "FAST detection failed" : err);
  *n_out = (int32_t)kps.size();
  if ((int)kps.size() > capacity) return fail(ctx, RGBDFE_ERR_CAPACITY, "more FAST keypoints than the output array holds");
  kp_to_abi(kps, keypoints);
  return RGBDFE_OK;
}

}  // namespace impl
