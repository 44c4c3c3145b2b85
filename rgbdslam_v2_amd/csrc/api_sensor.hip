// api_sensor.hip -- the sensor entry points: colour + raw depth images as the sensor messages carry them, prepared on the
// device by ingest.hip's kernel in front of the existing detect / describe / project chains (one of the host-side
// translation units of librgbdfe.so; shared declarations: rgbdfe_host.h, sensor_host.h).  DESIGN.md section 4.16.
#include "rgbdfe_host.h"

namespace impl {

void sensor_release(rgbdfe_ctx* ctx) {
  rgbdfe_ctx::SensorBufs& sb = ctx->sensor;
  for (uint8_t* p : sb.h_raw) if (p) (void)hipHostFree(p);
  for (uint8_t* p : sb.d_raw) if (p) (void)hipFree(p);
  for (float* p : sb.d_depth) if (p) (void)hipFree(p);
  if (sb.d_planes) (void)hipFree(sb.d_planes);
  if (sb.d_maps) (void)hipFree(sb.d_maps);
  sb = rgbdfe_ctx::SensorBufs{};
}

int sensor_ensure(rgbdfe_ctx* ctx, int n_pinned, int n_device, size_t bytes, int depth_planes, size_t plane) {
  rgbdfe_ctx::SensorBufs& sb = ctx->sensor;
  if (n_pinned > rgbdfe_ctx::SensorBufs::kPinned || n_device > rgbdfe_ctx::SensorBufs::kDevice || depth_planes > 2)
    return fail(ctx, RGBDFE_ERR_INTERNAL, "sensor buffers: more buffers than the context holds");
  // (the previous users of a buffer that is replaced have been waited for: every sensor call drains its streams before it returns)
  for (int i = 0; i < n_pinned; ++i)
    if (sb.h_cap[i] < bytes) {
      if (sb.h_raw[i]) (void)hipHostFree(sb.h_raw[i]);
      sb.h_raw[i] = nullptr; sb.h_cap[i] = 0;
      if (hipHostMalloc((void**)&sb.h_raw[i], bytes, hipHostMallocDefault) != hipSuccess)
        return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "sensor frame staging");
      sb.h_cap[i] = bytes;
    }
  for (int i = 0; i < n_device; ++i)
    if (sb.d_cap[i] < bytes) {
      if (sb.d_raw[i]) (void)hipFree(sb.d_raw[i]);
      sb.d_raw[i] = nullptr; sb.d_cap[i] = 0;
      if (hipMalloc((void**)&sb.d_raw[i], bytes) != hipSuccess) return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "sensor frame buffers");
      sb.d_cap[i] = bytes;
    }
  for (int i = 0; i < depth_planes; ++i)
    if (sb.depth_cap[i] < plane) {
      if (sb.d_depth[i]) (void)hipFree(sb.d_depth[i]);
      sb.d_depth[i] = nullptr; sb.depth_cap[i] = 0;
      if (hipMalloc((void**)&sb.d_depth[i], plane * 4) != hipSuccess) return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "sensor depth plane");
      sb.depth_cap[i] = plane;
    }
  return RGBDFE_OK;
}

// Validation of a run (no device work, no state change) and the two index tables of step 1.
int sensor_run_build(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, SensorRun& run) {
  if (n_frames < 0 || (n_frames > 0 && !frames)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  run = SensorRun{};
  run.frames = frames; run.n = n_frames;
  if (n_frames == 0) return RGBDFE_OK;
  const rgbdfe_sensor_frame& f0 = frames[0];
  for (int32_t f = 0; f < n_frames; ++f) {
    const rgbdfe_sensor_frame& fr = frames[f];
    if (!fr.visual || !fr.depth) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "sensor frame: null image pointer");
    if (fr.visual_encoding != RGBDFE_VISUAL_MONO8 && fr.visual_encoding != RGBDFE_VISUAL_RGB8 && fr.visual_encoding != RGBDFE_VISUAL_BGR8)
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "sensor frame: unknown visual encoding");
    if (fr.depth_encoding != RGBDFE_DEPTH_32FC1 && fr.depth_encoding != RGBDFE_DEPTH_16UC1)
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "sensor frame: unknown depth encoding");
    if (fr.visual_rows < 1 || fr.visual_cols < 1 || fr.depth_rows < 1 || fr.depth_cols < 1)
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "sensor frame: non-positive image size");
    const int64_t vrow = (int64_t)fr.visual_cols * (fr.visual_encoding == RGBDFE_VISUAL_MONO8 ? 1 : 3);
    const int64_t drow = (int64_t)fr.depth_cols * (fr.depth_encoding == RGBDFE_DEPTH_16UC1 ? 2 : 4);
    if ((int64_t)fr.visual_step < vrow || (int64_t)fr.depth_step < drow)
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "sensor frame: step smaller than a row");
    if (fr.visual_rows != f0.visual_rows || fr.visual_cols != f0.visual_cols || fr.depth_rows != f0.depth_rows ||
        fr.depth_cols != f0.depth_cols || fr.visual_encoding != f0.visual_encoding || fr.depth_encoding != f0.depth_encoding)
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "sensor frames of one batch must share sizes and encodings");
  }
  run.W = f0.visual_cols; run.H = f0.visual_rows; run.dW = f0.depth_cols; run.dH = f0.depth_rows;
  run.channels = f0.visual_encoding == RGBDFE_VISUAL_MONO8 ? 1 : 3;
  run.u16 = f0.depth_encoding == RGBDFE_DEPTH_16UC1;
  run.layout();   // staged sizes + the index tables of step 1
  return RGBDFE_OK;
}

// the resampling tables on the device (ctx->mu held, device set); kept for the next run of the same geometry
int sensor_run_device(rgbdfe_ctx* ctx, SensorRun& run) {
  if (!run.resample) return RGBDFE_OK;
  rgbdfe_ctx::SensorBufs& sb = ctx->sensor;
  const size_t n = (size_t)run.W + (size_t)run.H;
  const int key[4] = {run.W, run.H, run.dW, run.dH};
  if (!sb.d_maps || memcmp(key, sb.maps_key, sizeof(key)) != 0) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sb.maps_cap < n) {
      if (sb.d_maps) (void)hipFree(sb.d_maps);
      sb.d_maps = nullptr; sb.maps_cap = 0;
      if (hipMalloc((void**)&sb.d_maps, n * 4) != hipSuccess) return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "sensor resampling tables");
      sb.maps_cap = n;
    }
    memset(sb.maps_key, 0, sizeof(sb.maps_key));
    HIP_TRY(ctx, hipMemcpy(sb.d_maps, run.xmap.data(), (size_t)run.W * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(sb.d_maps + run.W, run.ymap.data(), (size_t)run.H * 4, hipMemcpyHostToDevice));
    memcpy(sb.maps_key, key, sizeof(key));
  }
  run.d_maps = sb.d_maps;
  return RGBDFE_OK;
}

// nf raw frames staged in ctx->sensor.h_raw[hbuf] -> d_raw[dbuf] on `s`, then the ingest launch into the outputs of `outs`
int sensor_upload_ingest(rgbdfe_ctx* ctx, const SensorRun& run, int hbuf, int dbuf, int nf, IngestParams outs, hipStream_t s) {
  rgbdfe_ctx::SensorBufs& sb = ctx->sensor;
  const size_t bytes = run.frame_bytes * (size_t)nf;
  if (!sb.h_raw[hbuf] || !sb.d_raw[dbuf] || sb.h_cap[hbuf] < bytes || sb.d_cap[dbuf] < bytes)
    return fail(ctx, RGBDFE_ERR_INTERNAL, "sensor buffers too small for the chunk");
  HIP_TRY(ctx, hipMemcpyAsync(sb.d_raw[dbuf], sb.h_raw[hbuf], bytes, hipMemcpyHostToDevice, s));
  IngestParams p = run.params(sb.d_raw[dbuf]);
  p.gray = outs.gray; p.gray_stride = outs.gray_stride;
  p.mask = outs.mask; p.mask_stride = outs.mask_stride;
  p.depth_m = outs.depth_m; p.depth_stride = outs.depth_stride;
  launch_ingest(p, nf, s);
  HIP_TRY(ctx, hipGetLastError());
  return RGBDFE_OK;
}

int rgbdfe_ingest_frame(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, uint8_t* gray, uint8_t* mono8, float* depth_m) {
  if (!ctx || !frame) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  SensorRun run;
  int rc = sensor_run_build(ctx, 1, frame, run);
  if (rc != RGBDFE_OK) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  const size_t plane = (size_t)run.W * run.H, pl16 = (plane + 15) & ~(size_t)15;
  rc = sensor_ensure(ctx, 1, 1, run.frame_bytes, 1, plane);
  if (rc == RGBDFE_OK) rc = sensor_run_device(ctx, run);
  if (rc != RGBDFE_OK) return rc;
  rgbdfe_ctx::SensorBufs& sb = ctx->sensor;
  if (sb.planes_cap < 2 * pl16) {
    if (sb.d_planes) (void)hipFree(sb.d_planes);
    sb.d_planes = nullptr; sb.planes_cap = 0;
    if (hipMalloc((void**)&sb.d_planes, 2 * pl16) != hipSuccess) return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "sensor planes");
    sb.planes_cap = 2 * pl16;
  }
  run.stage(0, sb.h_raw[0]);
  IngestParams o{};
  o.gray = gray ? sb.d_planes : nullptr;
  o.mask = mono8 ? sb.d_planes + pl16 : nullptr;
  o.depth_m = depth_m ? sb.d_depth[0] : nullptr;
  rc = sensor_upload_ingest(ctx, run, 0, 0, 1, o, ctx->stream);
  if (rc != RGBDFE_OK) return rc;
  if (gray) HIP_TRY(ctx, hipMemcpyAsync(gray, o.gray, plane, hipMemcpyDeviceToHost, ctx->stream));
  if (mono8) HIP_TRY(ctx, hipMemcpyAsync(mono8, o.mask, plane, hipMemcpyDeviceToHost, ctx->stream));
  if (depth_m) HIP_TRY(ctx, hipMemcpyAsync(depth_m, o.depth_m, plane * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return RGBDFE_OK;
}

int rgbdfe_sensor_detect_describe(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, double fx, double fy, double cx, double cy,
                                  double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1,
                                  int32_t* n_out) {
  if (!ctx || !frame || !keypoints || !descriptors || !xyz1 || !n_out) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  SensorRun run;
  int rc = sensor_run_build(ctx, 1, frame, run);
  if (rc != RGBDFE_OK) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  rc = sensor_run_device(ctx, run);
  if (rc != RGBDFE_OK) return rc;
  if (ctx->detector_type == RGBDFE_DETECTOR_FAST)
    return fast_detect_describe(ctx, 1, nullptr, nullptr, nullptr, run.H, run.W, fx, fy, cx, cy, depth_scaling, ctx->orb_max_keypoints,
                                keypoints, descriptors, xyz1, n_out, nullptr, &run);
  rc = sensor_ensure(ctx, 1, 1, run.frame_bytes, ctx->feature_min_depth ? 1 : 0, (size_t)run.W * run.H);
  if (rc != RGBDFE_OK) return rc;
  return detect_describe_sensor_frame(ctx, run, fx, fy, cx, cy, depth_scaling, keypoints, descriptors, xyz1, n_out);
}

// validation shared by the single-device and the multi-device form of the batch call
int sensor_batch_validate(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, const int32_t* node_ids,
                          const rgbdfe_sensor_cloud* cloud, SensorRun& run) {
  const int rc = sensor_run_build(ctx, n_frames, frames, run);
  if (rc != RGBDFE_OK) return rc;
  if (cloud) {
    if (!node_ids) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "cloud needs node_ids");
    if (cloud->cloud_skip < 1 || (n_frames > 0 && (run.H % cloud->cloud_skip != 0 || run.W % cloud->cloud_skip != 0)))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "cloud_creation_skip_step must divide the image dimensions");  // misc.cpp:479-481
  }
  return RGBDFE_OK;
}

int rgbdfe_sensor_detect_describe_batch(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, double fx, double fy,
                                        double cx, double cy, double depth_scaling, int32_t out_stride,
                                        rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out,
                                        const int32_t* node_ids) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  SensorRun run;
  const int rc = sensor_batch_validate(ctx, n_frames, frames, node_ids, nullptr, run);
  if (rc != RGBDFE_OK) return rc;
  // the existing batch entry point with the run in place of the planes; for an empty run the size checks have nothing to look at
  return rgbdfe_detect_describe_batch(ctx, n_frames, nullptr, nullptr, nullptr, n_frames > 0 ? run.H : 1, n_frames > 0 ? run.W : 1, fx,
                                      fy, cx, cy, depth_scaling, out_stride, keypoints, descriptors, xyz1, n_out, node_ids, &run);
}

// createXYZRGBPointCloud (node.cpp:126-132) for the frames of a run whose node id is >= 0: the raw frame goes up, the ingest
// kernel writes its float depth plane, create_cloud_kernel reads that plane and the visual image as stored (the staged rows
// are tightly packed: the layout the kernel expects).  The cloud is kept as rgbdfe_upload_node_cloud keeps it.
int rgbdfe_sensor_clouds(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, double fx, double fy, double cx,
                         double cy, double depth_scaling, const int32_t* node_ids, const rgbdfe_sensor_cloud* cloud) {
  if (!ctx || !cloud) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  SensorRun run;
  int rc = sensor_batch_validate(ctx, n_frames, frames, node_ids, cloud, run);
  if (rc != RGBDFE_OK || n_frames == 0) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  const size_t plane = (size_t)run.W * run.H;
  rc = sensor_ensure(ctx, 2, 2, run.frame_bytes, 2, plane);
  if (rc == RGBDFE_OK) rc = sensor_run_device(ctx, run);
  if (rc != RGBDFE_OK) return rc;
  const int s = cloud->cloud_skip, ch = run.H / s, cw = run.W / s;
  for (int32_t f = 0; f < n_frames; ++f) {
    if (node_ids[f] < 0) continue;
    const int b = f & 1;   // two buffer sets: frame f + 1 is staged while frame f's copy and launches run
    CloudEntry& ce = ctx->clouds[node_ids[f]];
    if (ce.d && (ce.ch != ch || ce.cw != cw)) {
      if (const int rc_ = wait_for_pair_lanes(ctx)) return rc_;
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      (void)hipFree(ce.d);
      ce.d = nullptr;
    }
    if (!ce.d && hipMalloc((void**)&ce.d, (size_t)ch * cw * (sizeof(float4) + sizeof(float))) != hipSuccess) {
      ctx->clouds.erase(node_ids[f]);
      return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "cloud allocation failed");
    }
    ce.ch = ch; ce.cw = cw; ce.cloud_skip = s;
    ce.samples_skip = 0;
    ce.fx = (float)fx; ce.fy = (float)fy; ce.cx = (float)cx; ce.cy = (float)cy;  // misc.cpp:59-62
    if (f >= 2) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (set b's previous frame has left its staging buffer)
    run.stage(f, ctx->sensor.h_raw[b]);
    IngestParams o{};
    o.depth_m = ctx->sensor.d_depth[b];
    rc = sensor_upload_ingest(ctx, run, b, b, 1, o, ctx->stream);
    if (rc != RGBDFE_OK) return rc;
    const float fxinv = (float)(1. / ce.fx), fyinv = (float)(1. / ce.fy);
    launch_create_cloud(ctx->sensor.d_depth[b], run.H, run.W, ctx->sensor.d_raw[b], run.channels, cloud->encoding_bgr, fxinv, fyinv,
                        ce.cx, ce.cy, depth_scaling, (float)cloud->min_depth, s, ch, cw, ce.d,
                        reinterpret_cast<float*>(ce.d + (size_t)ch * cw), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return RGBDFE_OK;
}

}  // namespace impl
