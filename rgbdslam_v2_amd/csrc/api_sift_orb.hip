// api_sift_orb.hip -- feature_detector_type "SIFTGPU" with feature_extractor_type "ORB" (node.cpp:149-152, 183-210), one frame
// or a run of frames into resident ORB nodes (one of the host-side translation units of librgbdfe.so; rgbdfe_host.h).
// DESIGN.md section 4.15.
//
// sift_chunk_pipeline (api_detect.hip: three extractors, three chunks of up to 8 frames in flight, the depth images staged
// by a helper thread and copied on a stream of their own), with the extractors in keys-only mode: the SIFT
// pipeline stops after the orientations and leaves the kept features on the device (no descriptor launch, no descriptor
// read-back).  Behind each chunk, on the chunk's stream:
//   1. orb_blur_kernel on the chunk's gray images (the extractor's own device copy of them)
//   2. sift_orb_keys: conversions, removeDepthless, the cut, the border filter and projectTo3D, one workgroup per frame
//   3. sift_orb_brief: rBRIEF into the node slabs and / or the output rows
//   4. the counts (and the host outputs, when asked for) on their way back
// After the chunk's wait the host registers the nodes and enqueues their fp4 expansion (hamming_mfma.hip).
#include "rgbdfe_host.h"
#include "sift_orb.h"

#include "orb_pattern.inc"  // kOrbBitPattern31

namespace impl {

namespace {

constexpr int B = SiftExtractor::kMaxBatch, D = 3;
static_assert(B == kSiftNodeFramesMax, "a chunk is one launch of the keypoint kernel");

// the layout of rgbdfe_ctx::so: D chunk sets of B frames of `plane` pixels, R rows per frame; the blur's image table and tiles
// (frame k of a set: gray image at k * plane of the extractor's copy, blurred at k * plane of the set's blur pool)
struct Layout {
  size_t d_blur, d_imgs, d_units, d_list, d_kp, d_desc, d_xyz, d_n, dev_bytes;
  size_t h_kp, h_desc, h_xyz, h_n, h_tab, pin_bytes;
  int units_per_frame;
  Layout(size_t plane, int rows, int cols, size_t R) {
    const size_t S = (size_t)D * B;
    units_per_frame = ((cols + 63) / 64) * ((rows + 15) / 16);
    Arena d, h;
    d_blur = d.carve(S * plane); d_imgs = d.carve(B * sizeof(ImgDesc)); d_units = d.carve((size_t)B * units_per_frame * sizeof(TileUnit));
    d_list = d.carve(S * R * sizeof(SiftOrbDescKp)); d_kp = d.carve(S * R * sizeof(rgbdfe_keypoint)); d_desc = d.carve(S * R * 32);
    d_xyz = d.carve(S * R * 16); d_n = d.carve(S * 4);
    dev_bytes = d.size;
    h_kp = h.carve(S * R * sizeof(rgbdfe_keypoint)); h_desc = h.carve(S * R * 32); h_xyz = h.carve(S * R * 16); h_n = h.carve(S * 4);
    h_tab = h.carve(B * sizeof(ImgDesc) + (size_t)B * units_per_frame * sizeof(TileUnit));
    pin_bytes = h.size;
  }
};

int prepare_bufs(rgbdfe_ctx* ctx, int rows, int cols) {
  rgbdfe_ctx::SiftOrbBufs& so = ctx->so;
  const size_t plane = (size_t)rows * (size_t)cols, R = (size_t)ctx->cfg.max_keypoints;
  if (so.dev && so.rows == rows && so.cols == cols) return RGBDFE_OK;
  if ((size_t)B * D * plane > 0xFFFFFFFFull) return fail(ctx, RGBDFE_ERR_CAPACITY, "frame too large for the ORB describer");
  if (so.dev) (void)hipFree(so.dev);
  if (so.pin) (void)hipHostFree(so.pin);
  so.dev = so.pin = nullptr; so.rows = so.cols = 0;
  const Layout L(plane, rows, cols, R);
  if (hipMalloc(&so.dev, L.dev_bytes) != hipSuccess || hipHostMalloc(&so.pin, L.pin_bytes, hipHostMallocDefault) != hipSuccess ||
      (!so.d_pattern && hipMalloc((void**)&so.d_pattern, 1024) != hipSuccess))
    return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "SIFT-ORB buffers");
  ImgDesc* imgs = at<ImgDesc>(so.pin, L.h_tab);
  TileUnit* units = reinterpret_cast<TileUnit*>(imgs + B);
  const int tx = (cols + 63) / 64, ty = (rows + 15) / 16;
  for (int k = 0; k < B; ++k) {
    ImgDesc im{};
    im.off = (uint32_t)(k * plane); im.w = cols; im.h = rows; im.stride = cols; im.score_off = (uint32_t)(k * plane);
    imgs[k] = im;
    for (int by = 0; by < ty; ++by)
      for (int bx = 0; bx < tx; ++bx)
        units[(size_t)k * L.units_per_frame + (size_t)by * tx + bx] = TileUnit{(uint16_t)k, (uint16_t)bx, (uint16_t)by, 0};
  }
  HIP_TRY(ctx, hipMemcpyAsync(at<void>(so.dev, L.d_imgs), imgs, B * sizeof(ImgDesc), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(at<void>(so.dev, L.d_units), units, (size_t)B * L.units_per_frame * sizeof(TileUnit),
                              hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(so.d_pattern, kOrbBitPattern31, 1024, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  so.rows = rows; so.cols = cols;
  return RGBDFE_OK;
}

// where a call's outputs go (every pointer may be NULL); frame f's rows start at row f * stride
struct Outputs {
  int32_t stride = 0;
  rgbdfe_keypoint* keypoints = nullptr; uint8_t* descriptors = nullptr; float* xyz1 = nullptr;
  int32_t* n_out = nullptr;
};

// the whole pipeline for n_frames frames; ctx->mu is held.  node_ids: NULL (no nodes) or one id per frame, with the slots
// reserved by the caller (slot_of[f] >= 0 for a frame with a node)
int run_frames(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const float* const* depth, int32_t rows, int32_t cols,
               double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints, const int32_t* node_ids,
               const std::vector<int64_t>& slot_of, const Outputs& out) {
  const size_t plane = (size_t)rows * (size_t)cols, mk = (size_t)ctx->cfg.max_keypoints;
  int rc = sift_nodes_prepare(ctx, plane, false);   // the depth staging of rgbdfe_sift_detect_batch_nodes
  if (rc == RGBDFE_OK) rc = prepare_bufs(ctx, rows, cols);
  if (rc != RGBDFE_OK) return rc;
  rgbdfe_ctx::SiftOrbBufs& so = ctx->so;
  const Layout L(plane, rows, cols, mk);
  void* Dv = so.dev;
  void* P = so.pin;
  const bool host_out = out.keypoints || out.descriptors || out.xyz1;
  struct KeysOnly {   // the extractors stop after the orientations for the length of this call
    SiftExtractor* ex[D];
    KeysOnly(rgbdfe_ctx* c) : ex{&c->sift, &c->sift2, &c->sift3} { for (SiftExtractor* e : ex) e->keys_only = true; }
    ~KeysOnly() { for (SiftExtractor* e : ex) e->keys_only = false; }
  } keys_only(ctx);
  SiftChunkSteps steps;
  // behind chunk c's keys-only step: the blur, the keypoint launch, rBRIEF, then the counts (and host outputs) on their way back
  steps.behind = [&](const SiftChunk& c, std::string& err) -> int {
    const int set = c.set, nf = c.nf;
    hipStream_t s = c.stream;
    const SiftExtractor& X = *c.ex;
    uint8_t* blur = at<uint8_t>(Dv, L.d_blur) + (size_t)set * B * plane;
    launch_orb_blur_always(X.d_gray, at<ImgDesc>(Dv, L.d_imgs), at<TileUnit>(Dv, L.d_units), nf * L.units_per_frame, blur, s);
    SiftOrbChunk ch{};
    ch.n_frames = nf;
    ch.n_out = at<int32_t>(Dv, L.d_n) + (size_t)set * B;
    for (int k = 0; k < nf; ++k) {
      const int32_t f = c.c * B + k;
      const SiftExtractor::FrameState& F = X.fs[(size_t)k];
      SiftOrbFrame& o = ch.frame[k];
      o.n_keys = X.fin_grand2 > 0 ? F.total : 0;
      if (o.n_keys > 0) o.keys = reinterpret_cast<const SiftOrbKey*>(X.d_keys + (size_t)F.base * 2);
      o.depth = c.d_depth + (size_t)k * plane;
      const size_t r0 = ((size_t)set * B + k) * mk;
      o.list = at<SiftOrbDescKp>(Dv, L.d_list) + r0;
      if (node_ids && slot_of[(size_t)f] >= 0) {
        const size_t row0 = (size_t)slot_of[(size_t)f] * mk;
        o.node_desc = ctx->d_desc + row0 * 8;
        o.node_xyz = ctx->d_xyz + row0;
      }
      if (out.keypoints) o.out_kp = at<rgbdfe_keypoint>(Dv, L.d_kp) + r0;
      if (out.descriptors) o.out_desc = at<uint8_t>(Dv, L.d_desc) + r0 * 32;
      if (out.xyz1) o.out_xyz = at<float4>(Dv, L.d_xyz) + r0;
    }
    launch_sift_orb_keys(ch, rows, cols, (float)(1. / fx), (float)(1. / fy), (float)cx, (float)cy, depth_scaling, max_keypoints,
                         ctx->feature_min_depth, s);
    launch_sift_orb_brief(ch, X.d_gray, blur, (uint32_t)plane, rows, cols, max_keypoints, so.d_pattern, s);
    hipError_t e = hipGetLastError();
    const size_t r0 = (size_t)set * B * mk, nr = (size_t)nf * mk;
    if (e == hipSuccess)
      e = hipMemcpyAsync(at<int32_t>(P, L.h_n) + (size_t)set * B, ch.n_out, (size_t)nf * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && out.keypoints)
      e = hipMemcpyAsync(at<rgbdfe_keypoint>(P, L.h_kp) + r0, at<rgbdfe_keypoint>(Dv, L.d_kp) + r0, nr * sizeof(rgbdfe_keypoint),
                         hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && out.descriptors)
      e = hipMemcpyAsync(at<uint8_t>(P, L.h_desc) + r0 * 32, at<uint8_t>(Dv, L.d_desc) + r0 * 32, nr * 32, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && out.xyz1)
      e = hipMemcpyAsync(at<float4>(P, L.h_xyz) + r0, at<float4>(Dv, L.d_xyz) + r0, nr * 16, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { err = std::string("SIFT-ORB launch: ") + hipGetErrorString(e); return RGBDFE_ERR_HIP; }
    return RGBDFE_OK;
  };
  // after the chunk's wait: the node table, the nodes' expansion for the Hamming matcher, the caller's arrays
  steps.after = [&](const SiftChunk& c, std::string& err) -> int {
    const int set = c.set;
    if (hipStreamSynchronize(c.stream) != hipSuccess) { err = "hipStreamSynchronize"; return RGBDFE_ERR_HIP; }
    for (int k = 0; k < c.nf; ++k) {
      const int32_t f = c.c * B + k;
      const int32_t n = at<int32_t>(P, L.h_n)[(size_t)set * B + k];
      out.n_out[f] = n;
      if (node_ids && node_ids[f] >= 0) {
        const uint32_t slot = (uint32_t)slot_of[(size_t)f];
        ctx->nodes[node_ids[f]] = NodeEntry{slot, (uint32_t)n, 0u, 0u};
        launch_hamming_expand(ctx->d_desc + (size_t)slot * mk * 8, ctx->d_desc4, slot, (uint32_t)mk, (uint32_t)n, c.stream);
        if (hipGetLastError() != hipSuccess) { err = "hamming expand"; return RGBDFE_ERR_HIP; }
      }
      if (!host_out || n == 0) continue;
      const size_t r0 = ((size_t)set * B + k) * mk, o = (size_t)f * (size_t)out.stride;
      if (out.keypoints) memcpy(out.keypoints + o, at<rgbdfe_keypoint>(P, L.h_kp) + r0, (size_t)n * sizeof(rgbdfe_keypoint));
      if (out.descriptors) memcpy(out.descriptors + o * 32, at<uint8_t>(P, L.h_desc) + r0 * 32, (size_t)n * 32);
      if (out.xyz1) memcpy(out.xyz1 + o * 4, at<float4>(P, L.h_xyz) + r0, (size_t)n * 16);
    }
    return RGBDFE_OK;
  };
  rc = sift_chunk_pipeline(ctx, n_frames, gray, depth, rows, cols, max_keypoints, steps);
  if (rc != RGBDFE_OK) return rc;
  for (int i = 0; i < D; ++i) HIP_TRY(ctx, hipStreamSynchronize(sift_chunk_stream(ctx, i)));   // the last expansions
  return RGBDFE_OK;
}

}  // namespace

void sift_orb_release(rgbdfe_ctx* ctx) {
  rgbdfe_ctx::SiftOrbBufs& so = ctx->so;
  if (so.dev) (void)hipFree(so.dev);
  if (so.pin) (void)hipHostFree(so.pin);
  if (so.d_pattern) (void)hipFree(so.d_pattern);
  so = rgbdfe_ctx::SiftOrbBufs{};
}

// Node::Node for feature_detector_type SIFTGPU and feature_extractor_type ORB (node.cpp:149-152, 183-210), one frame:
// SiftGPUWrapper::detect's own detection, removeDepthless, the max_keypoints cut, cv::ORB::compute, projectTo3D.  The same bits
// as rgbdfe_sift_detect(max_keypoints) -> removeDepthless and the cut on the host -> rgbdfe_orb_compute ->
// rgbdfe_project_to_3d(_min_depth).
int rgbdfe_sift_detect_orb_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const float* depth, int32_t rows, int32_t cols, double fx,
                                    double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                    rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out) {
  if (!ctx || !gray || !depth || rows < 1 || cols < 1 || !keypoints || !descriptors || !xyz1 || !n_out)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (max_keypoints < 1 || max_keypoints > ctx->cfg.max_keypoints)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "max_keypoints must lie in [1, the context's max_keypoints]");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  *n_out = 0;
  Outputs out;
  out.stride = 0; out.keypoints = keypoints; out.descriptors = descriptors; out.xyz1 = xyz1; out.n_out = n_out;
  return run_frames(ctx, 1, &gray, &depth, rows, cols, fx, fy, cx, cy, depth_scaling, max_keypoints, nullptr, {}, out);
}

// A run of frames: the results of n_frames calls of rgbdfe_sift_detect_orb_describe, frame f's features becoming the ORB node
// node_ids[f] (rgbdfe_upload_node(id, descriptors, xyz1, n)).  The node table follows rgbdfe_detect_describe_batch_nodes: free
// slots are checked and reserved for the whole batch before any work (every fresh id takes one; a frame without features
// becomes an empty node), an existing id is rewritten in place after the pair lanes that may read it have finished.
int rgbdfe_sift_detect_orb_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                                const float* const* depth, int32_t rows, int32_t cols, double fx, double fy,
                                                double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                                const int32_t* node_ids, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                                uint8_t* descriptors, float* xyz1, int32_t* n_out) {
  if (!ctx || n_frames < 0 || rows < 1 || cols < 1 || out_stride < 0 || (n_frames > 0 && (!gray || !depth || !node_ids || !n_out)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (max_keypoints < 1 || max_keypoints > ctx->cfg.max_keypoints)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "max_keypoints must lie in [1, the context's max_keypoints (node rows)]");
  if (!frames_non_null(n_frames, gray, depth)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "null frame");
  if (n_frames > 0 && (keypoints || descriptors || xyz1) && out_stride < max_keypoints)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "out_stride below max_keypoints while a host output is asked for");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  for (int32_t f = 0; f < n_frames; ++f) n_out[f] = 0;
  if (n_frames == 0) return RGBDFE_OK;
  // all-or-nothing; fresh ids are registered (as empty ORB nodes) before any work, a resident node of any kind keeps its
  // entry until its frame's final one is written: an ORB node afterwards
  std::vector<int64_t> slot_of;
  const int rc = reserve_node_slots(ctx, n_frames, node_ids, 0u, &slot_of);
  if (rc != RGBDFE_OK) return rc;
  Outputs out;
  out.stride = out_stride; out.keypoints = keypoints; out.descriptors = descriptors; out.xyz1 = xyz1; out.n_out = n_out;
  return run_frames(ctx, n_frames, gray, depth, rows, cols, fx, fy, cx, cy, depth_scaling, max_keypoints, node_ids, slot_of, out);
}

}  // namespace impl
