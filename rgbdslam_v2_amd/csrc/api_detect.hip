// api_detect.hip -- the feature path: ORB detect / describe (single calls, super-frames), SIFT extraction
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include <chrono>
#include <future>

#include "rgbdfe_host.h"
#include "staging_ring.h"

namespace impl {

// ---------------------------------------------------------------------------------------------
// per-frame feature path
// ---------------------------------------------------------------------------------------------
void ensure_detector(rgbdfe_ctx* ctx) {
  static const bool lookahead_env = !(getenv("RGBDFE_DETECT_LOOKAHEAD") && atoi(getenv("RGBDFE_DETECT_LOOKAHEAD")) == 0);
  ctx->orb.lookahead = lookahead_env;  // A/B switch: one device pass per adjuster iteration when 0
  if (ctx->orb_max_keypoints == 0) {
    ctx->orb_max_keypoints = 600;  // parameter_server.cpp:83
    ctx->orb.reset_detector(600, 3, 5);  // detector_grid_resolution 3, adjuster_max_iterations 5 (:87,:89)
  }
}

int rgbdfe_detector_configure(rgbdfe_ctx* ctx, int32_t max_keypoints, int32_t grid_resolution,
                              int32_t adjuster_max_iterations) {
  if (!ctx || max_keypoints < 1 || grid_resolution < 1 || grid_resolution > 8 || adjuster_max_iterations < 1)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad detector configuration");
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->orb_max_keypoints = max_keypoints;
  ctx->orb.reset_detector(max_keypoints, grid_resolution, adjuster_max_iterations);
  return RGBDFE_OK;
}

int rgbdfe_detector_thresholds(rgbdfe_ctx* ctx, double* thresholds, int32_t* n_cells) {
  if (!ctx || !thresholds || !n_cells) return RGBDFE_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  ensure_detector(ctx);
  *n_cells = ctx->orb.grid * ctx->orb.grid;
  for (int i = 0; i < *n_cells; ++i) thresholds[i] = ctx->orb.thresh[i];
  return RGBDFE_OK;
}

void kp_to_abi(const std::vector<KpOut>& v, rgbdfe_keypoint* out) {
  for (size_t i = 0; i < v.size(); ++i) {
    out[i].x = v[i].x; out[i].y = v[i].y; out[i].size = v[i].size; out[i].angle = v[i].angle;
    out[i].response = v[i].response; out[i].octave = v[i].octave;
  }
}

int rgbdfe_orb_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                      int32_t fast_threshold, rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out) {
  if (!ctx || !gray || rows < 1 || cols < 1 || !keypoints || !n_out || capacity < 0)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  std::string err;
  int rc = ctx->orb.prepare(cols, rows, false, err);
  if (rc == RGBDFE_OK) rc = ctx->orb.upload_and_build(gray, mask, ctx->stream, err);
  std::vector<KpOut> out;
  if (rc == RGBDFE_OK) rc = ctx->orb.detect_pass(fast_threshold, out, ctx->stream, err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err);
  *n_out = (int32_t)out.size();
  if ((int)out.size() > capacity) return fail(ctx, RGBDFE_ERR_CAPACITY, "more ORB keypoints than the output array holds");
  kp_to_abi(out, keypoints);
  return RGBDFE_OK;
}

int rgbdfe_orb_compute(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols,
                       rgbdfe_keypoint* keypoints, int32_t n, uint8_t* descriptors, int32_t* n_out) {
  if (!ctx || !gray || rows < 1 || cols < 1 || n < 0 || (n > 0 && (!keypoints || !descriptors)) || !n_out)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  std::string err;
  int rc = ctx->orb.prepare(cols, rows, false, err);
  if (rc == RGBDFE_OK) rc = ctx->orb.upload_and_build(gray, nullptr, ctx->stream, err);
  std::vector<KpOut> kps((size_t)n);
  for (int i = 0; i < n; ++i)
    kps[i] = KpOut{keypoints[i].x, keypoints[i].y, keypoints[i].size, keypoints[i].angle, keypoints[i].response,
                   keypoints[i].octave};
  std::vector<uint8_t> desc;
  if (rc == RGBDFE_OK) rc = ctx->orb.compute(kps, desc, ctx->stream, err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err);
  kp_to_abi(kps, keypoints);
  if (!desc.empty()) memcpy(descriptors, desc.data(), desc.size());
  *n_out = (int32_t)kps.size();
  return RGBDFE_OK;
}

// SiftGPUWrapper::detect (src/sift_gpu_wrapper.cpp:113-167): SIFT keypoints + 128-d descriptors of one mono8 image.  The
// mask is accepted and ignored, as the reference ignores it.  Keypoints as the wrapper builds them (:156-160):
// pt = SiftGPU's (x, y), size = 12 * scale, angle = orientation in degrees; response and octave stay 0.
int rgbdfe_sift_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* /*mask*/, int32_t rows, int32_t cols,
                       int32_t max_keypoints, rgbdfe_keypoint* keypoints, float* desc128, int32_t capacity, int32_t* n_out) {
  if (!ctx || !gray || rows < 1 || cols < 1 || !n_out || capacity < 0 || (capacity > 0 && (!keypoints || !desc128)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  *n_out = 0;
  std::vector<SiftKey> keys;
  const float* desc = nullptr;
  std::string err;
  const int rc = ctx->sift.run(gray, rows, cols, max_keypoints, keys, desc, ctx->stream, err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err);
  *n_out = (int32_t)keys.size();
  if ((int32_t)keys.size() > capacity) return fail(ctx, RGBDFE_ERR_CAPACITY, "more SIFT features than the output arrays hold");
  for (size_t i = 0; i < keys.size(); ++i) keypoints[i] = sift_key_to_keypoint(keys[i]);
  if (!keys.empty()) memcpy(desc128, desc, keys.size() * 128 * sizeof(float));
  return RGBDFE_OK;
}

// SiftGPUWrapper::detect with a non-empty keypoint list (sift_gpu_wrapper.cpp:132-142, 161-165): feature_extractor_type ==
// "SIFTGPU" behind another detector (node.cpp:166-171).  The keypoints' positions, sizes and angles go through the wrapper's
// conversions (o = angle / 180 * 3.1415927, s = size / 12) and come back as the wrapper rebuilds them (12 * s, o * 180 /
// 3.1415927, response = octave = 0); desc128 gets one row per keypoint, in the callers' order.
int rgbdfe_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols, rgbdfe_keypoint* keypoints, int32_t n,
                         float* desc128) {
  if (!ctx || !gray || rows < 1 || cols < 1 || n < 0 || (n > 0 && (!keypoints || !desc128)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  if (n == 0) return RGBDFE_OK;
  std::vector<SiftKey> keys((size_t)n);
  for (int32_t i = 0; i < n; ++i) keys[(size_t)i] = keypoint_to_sift_key(keypoints[i]);
  const float* desc = nullptr;
  std::string err;
  const int rc = ctx->sift.describe(gray, rows, cols, keys.data(), n, &desc, ctx->stream, err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err);
  memcpy(desc128, desc, (size_t)n * 128 * sizeof(float));
  for (int32_t i = 0; i < n; ++i) keypoints[i] = sift_key_to_keypoint(keys[(size_t)i]);   // (x, y: as they came)
  return RGBDFE_OK;
}

}  // namespace impl

namespace rgbdfe_host {

// Three extractors, three streams, a software pipeline over chunks of up to 8 frames.  A chunk passes four steps, each of
// which waits for the launches of the one before, does the host's part and enqueues the next launches (sift_extract.hip):
//   begin_batch           images staged + uploaded, pyramids, extremum flags, candidate lists     ~1.0 ms of device time
//   finish_orientations   feature-count limits -> the orientation launch                          ~0.06 ms
//   finish_descriptors    one feature per orientation -> the descriptor launch + 6 MB download    ~0.45 ms
//   finish_outputs        keys / descriptor pointers; then the copy into the caller's arrays      host only, ~0.35 ms
// One host thread drives all of it, so the ORDER of the steps decides what the device has to do while the host works or
// waits: within an iteration the descriptor launch of chunk c goes out first (with the caller's launches behind it:
// steps.behind), then chunk c + 2 is begun (its extractor's device buffers were released by chunk c - 1's last wait; the
// results of c - 1 sit in host memory begin_batch does not touch), then chunk c - 1 is copied out (steps.after) -- with two
// launch chains and a descriptor launch enqueued behind the host's back -- and only then the host waits: for chunk c + 1's
// first half (begun a whole iteration ago) and chunk c's descriptors.  Rounds 3 - 4 ran begin(c + 1) | all of finish(c) |
// copy-out(c) with two extractors: the device idled through every copy-out and most waits
// (profiles/r05_logs/sift_pipeline.txt).
int sift_chunk_pipeline(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const float* const* depth, int32_t rows,
                        int32_t cols, int32_t max_keypoints, const SiftChunkSteps& steps, bool timing) {
  constexpr int B = SiftExtractor::kMaxBatch, D = 3;   // (chunks of 4 or 6 frames measured no faster: 6820 / 6944 vs 6870 frames/s)
  static_assert(B == kSiftNodeFramesMax, "a chunk is one node launch");
  const int32_t n_chunks = (n_frames + B - 1) / B;
  SiftExtractor* ex[D] = {&ctx->sift, &ctx->sift2, &ctx->sift3};
  // (the chunk streams come from the high-priority class, created back to back: queues of a pool nothing else in the
  // process is likely to use -- see create_side_stream; equal priority, so no chunk starves another)
  if (n_chunks > 1 && !ctx->sift_stream3) {
    if (!ctx->sift_stream1) HIP_TRY(ctx, create_side_stream(&ctx->sift_stream1, +1));
    if (!ctx->sift_stream2) HIP_TRY(ctx, create_side_stream(&ctx->sift_stream2, +1));
    HIP_TRY(ctx, create_side_stream(&ctx->sift_stream3, +1));
  }
  const hipStream_t st[D] = {sift_chunk_stream(ctx, 0), sift_chunk_stream(ctx, 1), sift_chunk_stream(ctx, 2)};
  std::vector<SiftKey> keys[D][B];
  const float* desc[D][B];
  std::string err;
  rgbdfe_ctx::SiftNodeBufs& sn = ctx->sn;
  const size_t plane = (size_t)rows * (size_t)cols;
  auto count_of = [&](int32_t c) { return std::min<int32_t>(B, n_frames - c * B); };
  auto chunk = [&](int32_t c) {
    const int set = c % D;
    return SiftChunk{c, set, count_of(c), st[set], ex[set], keys[set], desc[set], depth ? sn.d_depth + (size_t)set * B * plane : nullptr};
  };
  // helper thread per chunk: the caller's depth images -> pinned set c % D -> device set c % D (depth stream), then the set's
  // event.  The set's previous copy (chunk c - D) has finished before its pinned images are overwritten: its chunk has been
  // waited for unless that chunk had no features at all (finish_outputs does not wait then), so the event is waited for here.
  const int dev = ctx->cfg.device_id;
  std::future<hipError_t> staged[D];
  auto stage_depth = [&](int32_t c) {
    const int set = c % D, nf = count_of(c);
    const float* const* src = depth + (size_t)c * B;
    float* h = sn.h_depth + (size_t)set * B * plane;
    float* d = sn.d_depth + (size_t)set * B * plane;
    hipStream_t ds = sn.depth_stream;
    hipEvent_t ev = sn.depth_done[set];
    const bool reused = c >= D;
    staged[set] = std::async(std::launch::async, [=]() -> hipError_t {
      hipError_t e = hipSetDevice(dev);
      if (e == hipSuccess && reused) e = hipEventSynchronize(ev);
      for (int k = 0; k < nf; ++k) memcpy(h + (size_t)k * plane, src[k], plane * 4);
      if (e == hipSuccess) e = hipMemcpyAsync(d, h, (size_t)nf * plane * 4, hipMemcpyHostToDevice, ds);
      if (e == hipSuccess) e = hipEventRecord(ev, ds);
      return e;
    });
  };
  auto begin = [&](int32_t c) -> int {
    if (depth) stage_depth(c);
    return ex[c % D]->begin_batch(gray + (size_t)c * B, count_of(c), rows, cols, st[c % D], err);
  };
  // the caller's launches behind chunk c's descriptor launch, its depth images ordered before them
  auto behind = [&](int32_t c) -> int {
    if (depth) {
      const hipError_t se = staged[c % D].get();
      if (se != hipSuccess) { err = std::string("depth staging: ") + hipGetErrorString(se); return RGBDFE_ERR_HIP; }
      if (hipStreamWaitEvent(st[c % D], sn.depth_done[c % D], 0) != hipSuccess) { err = "hipStreamWaitEvent"; return RGBDFE_ERR_HIP; }
    }
    return steps.behind ? steps.behind(chunk(c), err) : RGBDFE_OK;
  };
  auto drain = [&]() {
    for (int i = 0; i < D; ++i) if (staged[i].valid()) (void)staged[i].get();
    for (int i = 0; i < D; ++i) (void)hipStreamSynchronize(st[i]);
    if (depth) (void)hipStreamSynchronize(sn.depth_stream);
  };
  // RGBDFE_SIFT_TIMING=1: the calling thread's time per step, summed over the call, on stderr (how the order above was found)
  double t_step[5] = {0, 0, 0, 0, 0};   // begin, orientations, descriptors (+ behind), outputs, after (copy-out)
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_call = timing ? now() : 0;
  const double stage0 = ctx->sift.stage_us + ctx->sift2.stage_us + ctx->sift3.stage_us;
#define SIFT_STEP(slot, expr)                                 \
  do {                                                        \
    const double t0_ = timing ? now() : 0;                    \
    const int rc_ = (expr);                                   \
    if (timing) t_step[slot] += now() - t0_;                  \
    if (rc_ != RGBDFE_OK) { drain(); return fail(ctx, rc_, err); } \
  } while (0)
  // round c: every step for the chunk it belongs to, where that chunk exists (rounds -2 and -1 fill the pipeline, round
  // n_chunks empties it)
  auto live = [&](int32_t c) { return c >= 0 && c < n_chunks; };
  for (int32_t c = -2; c <= n_chunks; ++c) {
    if (live(c)) {
      SIFT_STEP(2, ex[c % D]->finish_descriptors(st[c % D], err));
      SIFT_STEP(2, behind(c));
    }
    if (live(c + 2)) SIFT_STEP(0, begin(c + 2));
    if (live(c - 1)) SIFT_STEP(4, steps.after(chunk(c - 1), err));
    if (live(c + 1)) SIFT_STEP(1, ex[(c + 1) % D]->finish_orientations(max_keypoints, st[(c + 1) % D], err));
    if (live(c)) SIFT_STEP(3, ex[c % D]->finish_outputs(keys[c % D], desc[c % D], st[c % D], err));
  }
#undef SIFT_STEP
  if (timing)
    fprintf(stderr, "sift_detect_batch %d frames: %.0f us; host us in begin %.0f orientations %.0f descriptors %.0f outputs %.0f copy-out %.0f; of begin, image staging %.0f\n",
            (int)n_frames, now() - t_call, t_step[0], t_step[1], t_step[2], t_step[3], t_step[4],
            ctx->sift.stage_us + ctx->sift2.stage_us + ctx->sift3.stage_us - stage0);
  return RGBDFE_OK;
}

}  // namespace rgbdfe_host

namespace impl {

// A run of frames (a recorded sequence): SiftExtractor::kMaxBatch of them share every launch of the pipeline -- the
// images are independent (SiftGPU keeps no state between them), so frame f's outputs are those of a single call.
int rgbdfe_sift_detect_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, int32_t rows, int32_t cols,
                             int32_t max_keypoints, int32_t out_stride, rgbdfe_keypoint* keypoints, float* desc128,
                             int32_t* n_out) {
  if (!ctx || n_frames < 0 || rows < 1 || cols < 1 || out_stride < 0 ||
      (n_frames > 0 && (!gray || !n_out || (out_stride > 0 && (!keypoints || !desc128)))))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (!frames_non_null(n_frames, gray)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "null frame");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  for (int32_t f = 0; f < n_frames; ++f) n_out[f] = 0;
  bool overflow = false;
  SiftChunkSteps steps;
  steps.after = [&](const SiftChunk& ch, std::string&) -> int {
    for (int k = 0; k < ch.nf; ++k) {
      const std::vector<SiftKey>& K = ch.keys[k];
      const int32_t f = ch.c * SiftExtractor::kMaxBatch + k;
      n_out[f] = (int32_t)K.size();
      if ((int32_t)K.size() > out_stride) { overflow = true; continue; }
      rgbdfe_keypoint* kp = keypoints + (size_t)f * out_stride;
      for (size_t i = 0; i < K.size(); ++i) kp[i] = sift_key_to_keypoint(K[i]);
      if (!K.empty()) memcpy(desc128 + (size_t)f * out_stride * 128, ch.desc[k], K.size() * 128 * sizeof(float));
    }
    return RGBDFE_OK;
  };
  static const bool timing = getenv("RGBDFE_SIFT_TIMING") && atoi(getenv("RGBDFE_SIFT_TIMING")) != 0;
  const int rc = sift_chunk_pipeline(ctx, n_frames, gray, nullptr, rows, cols, max_keypoints, steps, timing);
  if (rc != RGBDFE_OK) return rc;
  if (overflow) return fail(ctx, RGBDFE_ERR_CAPACITY, "more SIFT features in a frame than out_stride rows");
  return RGBDFE_OK;
}

// ---------------------------------------------------------------------------------------------
// SIFTGPU front end for a recorded run: detect -> projectTo3DSiftGPU -> RootSIFT -> resident node
// ---------------------------------------------------------------------------------------------
void sift_nodes_release(rgbdfe_ctx* ctx) {
  rgbdfe_ctx::SiftNodeBufs& sn = ctx->sn;
  for (void* p : {(void*)sn.d_depth, (void*)sn.d_n, (void*)sn.d_xyz_out, (void*)sn.d_feat_out, (void*)sn.d_kept_out})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)sn.h_depth, (void*)sn.h_n, (void*)sn.h_xyz_out, (void*)sn.h_feat_out, (void*)sn.h_kept_out})
    if (p) (void)hipHostFree(p);
  for (hipEvent_t e : sn.depth_done) if (e) (void)hipEventDestroy(e);
  if (sn.depth_stream) (void)hipStreamDestroy(sn.depth_stream);
  sn = rgbdfe_ctx::SiftNodeBufs{};
}

// the buffers of rgbdfe_sift_detect_batch_nodes for frames of `plane` pixels (reallocated when the size changes); the host-output
// rows are allocated with the first call that asks for them
int sift_nodes_prepare(rgbdfe_ctx* ctx, size_t plane, bool host_out) {
  rgbdfe_ctx::SiftNodeBufs& sn = ctx->sn;
  constexpr size_t S = 3 * (size_t)kSiftNodeFramesMax;
  const size_t rows = S * (size_t)ctx->cfg.max_keypoints;
  if (sn.plane != plane) {
    if (sn.depth_stream) HIP_TRY(ctx, hipStreamSynchronize(sn.depth_stream));
    if (sn.d_depth) (void)hipFree(sn.d_depth);
    if (sn.h_depth) (void)hipHostFree(sn.h_depth);
    sn.d_depth = nullptr; sn.h_depth = nullptr; sn.plane = 0;
    if (hipMalloc((void**)&sn.d_depth, S * plane * 4) != hipSuccess ||
        hipHostMalloc((void**)&sn.h_depth, S * plane * 4, hipHostMallocDefault) != hipSuccess)
      return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "SIFT node depth staging");
    sn.plane = plane;
  }
  if (!sn.d_n) {
    if (hipMalloc((void**)&sn.d_n, S * 4) != hipSuccess || hipHostMalloc((void**)&sn.h_n, S * 4, hipHostMallocDefault) != hipSuccess)
      return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "SIFT node counts");
    HIP_TRY(ctx, create_side_stream(&sn.depth_stream, -1));   // uploads: behind everything else
    for (hipEvent_t& e : sn.depth_done) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (host_out && !sn.d_xyz_out) {
    if (hipMalloc((void**)&sn.d_xyz_out, rows * 16) != hipSuccess || hipMalloc((void**)&sn.d_feat_out, rows * 512) != hipSuccess ||
        hipMalloc((void**)&sn.d_kept_out, rows * 4) != hipSuccess ||
        hipHostMalloc((void**)&sn.h_xyz_out, rows * 16, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&sn.h_feat_out, rows * 512, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&sn.h_kept_out, rows * 4, hipHostMallocDefault) != hipSuccess)
      return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "SIFT node output rows");
  }
  return RGBDFE_OK;
}

// Node::Node's SIFTGPU branch (node.cpp:147-176, 695-769, 1557-1571) for a run of frames, node by node into the slabs:
// sift_chunk_pipeline with the descriptor launch writing device memory only and one sift_nodes launch per chunk behind it
// (sift_nodes.hip).  The depth images of a chunk are staged by the pipeline's helper thread and copied on a stream of their
// own while the chunk is extracted; the node launch is ordered behind them.  The host reads the chunk's node counts (and the
// host outputs, when asked for) once, after the wait it does for the chunk's keypoints anyway.
int rgbdfe_sift_detect_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const float* const* depth,
                                   int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling,
                                   int32_t max_keypoints, int32_t use_root_sift, const int32_t* node_ids, int32_t out_stride,
                                   rgbdfe_keypoint* keypoints, float* xyz1, float* feature_descriptors, int32_t* n_out) {
  if (!ctx || n_frames < 0 || rows < 1 || cols < 1 || out_stride < 0 ||
      (n_frames > 0 && (!gray || !depth || !node_ids || !n_out)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (max_keypoints < 1 || max_keypoints > ctx->cfg.max_keypoints)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "max_keypoints must lie in [1, the context's max_keypoints (node rows)]");
  if (!frames_non_null(n_frames, gray, depth)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "null frame");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  for (int32_t f = 0; f < n_frames; ++f) n_out[f] = 0;
  if (n_frames == 0) return RGBDFE_OK;
  const bool host_out = keypoints || xyz1 || feature_descriptors;
  int rc = ensure_sift(ctx);
  if (rc == RGBDFE_OK) rc = sift_nodes_prepare(ctx, (size_t)rows * (size_t)cols, host_out);
  // the node table, all-or-nothing as rgbdfe_detect_describe_batch_nodes: every fresh id takes a slot before any work (a
  // frame without features becomes an empty node), existing nodes are rewritten in place
  std::vector<int64_t> slot_of;
  if (rc == RGBDFE_OK) rc = reserve_node_slots(ctx, n_frames, node_ids, 2u, &slot_of);
  if (rc != RGBDFE_OK) return rc;
  rgbdfe_ctx::SiftNodeBufs& sn = ctx->sn;
  constexpr int B = SiftExtractor::kMaxBatch;
  const size_t plane = sn.plane, mk = (size_t)ctx->cfg.max_keypoints;
  struct DeviceDescriptors {   // the extractors hand their descriptors to the node launch for the length of this call
    SiftExtractor* ex[3];
    DeviceDescriptors(rgbdfe_ctx* c) : ex{&c->sift, &c->sift2, &c->sift3} { for (SiftExtractor* e : ex) e->desc_device = true; }
    ~DeviceDescriptors() { for (SiftExtractor* e : ex) e->desc_device = false; }
  } device_descriptors(ctx);
  bool overflow = false;
  SiftChunkSteps steps;
  // behind chunk c's descriptor launch: its node launch, then the counts (and host outputs) on their way back
  steps.behind = [&](const SiftChunk& c, std::string& err) -> int {
    const SiftExtractor& X = *c.ex;
    SiftNodeChunk ch{};
    ch.n_frames = c.nf;
    ch.n_out = sn.d_n + (size_t)c.set * B;
    for (int k = 0; k < c.nf; ++k) {
      const int32_t f = c.c * B + k;
      const SiftExtractor::FrameState& F = X.fs[(size_t)k];
      SiftNodeFrame& o = ch.frame[k];
      o.n_keys = X.fin_grand2 > 0 ? F.total : 0;
      if (o.n_keys > 0) {
        o.keys = X.d_keys + F.base;
        o.desc = reinterpret_cast<const float2*>(X.d_desc + (size_t)F.base * 128);
      }
      o.depth = c.d_depth + (size_t)k * plane;
      if (slot_of[(size_t)f] >= 0) {
        const size_t row0 = (size_t)slot_of[(size_t)f] * mk;
        o.xyz = ctx->d_xyz + row0;
        o.feat = reinterpret_cast<float2*>(ctx->d_sift_f32 + row0 * 128);
      }
      const size_t r0 = ((size_t)c.set * B + k) * mk;
      if (xyz1) o.xyz_out = sn.d_xyz_out + r0;
      if (feature_descriptors) o.feat_out = reinterpret_cast<float2*>(sn.d_feat_out + r0 * 128);
      if (keypoints) o.kept_out = sn.d_kept_out + r0;
    }
    hipStream_t s = c.stream;
    launch_sift_nodes(ch, rows, cols, (float)(1. / fx), (float)(1. / fy), (float)cx, (float)cy, depth_scaling, max_keypoints,
                      ctx->feature_min_depth, use_root_sift != 0, s);
    hipError_t e = hipGetLastError();
    const size_t r0 = (size_t)c.set * B * mk, nr = (size_t)c.nf * mk;
    if (e == hipSuccess) e = hipMemcpyAsync(sn.h_n + (size_t)c.set * B, ch.n_out, (size_t)c.nf * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && xyz1) e = hipMemcpyAsync(sn.h_xyz_out + r0, sn.d_xyz_out + r0, nr * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && feature_descriptors)
      e = hipMemcpyAsync(sn.h_feat_out + r0 * 128, sn.d_feat_out + r0 * 128, nr * 512, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && keypoints) e = hipMemcpyAsync(sn.h_kept_out + r0, sn.d_kept_out + r0, nr * 4, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { err = std::string("SIFT node launch: ") + hipGetErrorString(e); return RGBDFE_ERR_HIP; }
    return RGBDFE_OK;
  };
  // after the chunk's wait: the node table and the caller's arrays
  steps.after = [&](const SiftChunk& c, std::string& err) -> int {
    if (hipStreamSynchronize(c.stream) != hipSuccess) { err = "hipStreamSynchronize"; return RGBDFE_ERR_HIP; }
    for (int k = 0; k < c.nf; ++k) {
      const int32_t f = c.c * B + k;
      const int32_t n = sn.h_n[(size_t)c.set * B + k];
      n_out[f] = n;
      if (node_ids[f] >= 0) ctx->nodes[node_ids[f]] = NodeEntry{(uint32_t)slot_of[(size_t)f], (uint32_t)n, 2u, 0u};
      if (!host_out) continue;
      if (n > out_stride) { overflow = true; continue; }
      const size_t r0 = ((size_t)c.set * B + k) * mk;
      if (keypoints) {
        const int32_t* kept = sn.h_kept_out + r0;
        rgbdfe_keypoint* kp = keypoints + (size_t)f * out_stride;
        for (int32_t i = 0; i < n; ++i) kp[i] = sift_key_to_keypoint(c.keys[k][(size_t)kept[i]]);
      }
      if (xyz1 && n > 0) memcpy(xyz1 + (size_t)f * out_stride * 4, sn.h_xyz_out + r0, (size_t)n * 16);
      if (feature_descriptors && n > 0)
        memcpy(feature_descriptors + (size_t)f * out_stride * 128, sn.h_feat_out + r0 * 128, (size_t)n * 512);
    }
    return RGBDFE_OK;
  };
  rc = sift_chunk_pipeline(ctx, n_frames, gray, depth, rows, cols, max_keypoints, steps);
  if (rc != RGBDFE_OK) return rc;
  if (overflow) return fail(ctx, RGBDFE_ERR_CAPACITY, "more kept SIFT features in a frame than out_stride rows");
  return RGBDFE_OK;
}

// stage access for the parity tests (tests/test_gpu_sift_extract.py): a Gaussian plane / the keypoint candidates of one
// (octave, dog level) of the latest rgbdfe_sift_detect frame
int rgbdfe_sift_debug_plane(rgbdfe_ctx* ctx, int32_t octave, int32_t level, float* out, int32_t capacity_floats, int32_t* w,
                            int32_t* h) {
  if (!ctx || !out || !w || !h) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  std::vector<float> v;
  int ww = 0, hh = 0;
  const int rc = ctx->sift.debug_plane(octave, level, v, &ww, &hh, ctx->stream);
  if (rc != RGBDFE_OK) return fail(ctx, rc, "no such SIFT pyramid plane");
  *w = ww; *h = hh;
  if ((int64_t)v.size() > (int64_t)capacity_floats) return fail(ctx, RGBDFE_ERR_CAPACITY, "plane larger than the output");
  memcpy(out, v.data(), v.size() * sizeof(float));
  return RGBDFE_OK;
}

int rgbdfe_sift_debug_candidates(rgbdfe_ctx* ctx, int32_t octave, int32_t dog_level, float* out, int32_t capacity_rows,
                                 int32_t* n) {
  if (!ctx || !n) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  std::vector<float> v;
  const int rc = ctx->sift.debug_candidates(octave, dog_level, v, ctx->stream);
  if (rc != RGBDFE_OK) return fail(ctx, rc, "no such SIFT level");
  *n = (int32_t)(v.size() / 6);
  if (*n > capacity_rows) return fail(ctx, RGBDFE_ERR_CAPACITY, "more candidates than the output holds");
  if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(float));
  return RGBDFE_OK;
}

int rgbdfe_sift_geometry(rgbdfe_ctx* ctx, int32_t* octave_min, int32_t* octave_num, int32_t* levels, int32_t* dog_levels) {
  if (!ctx || !octave_min || !octave_num || !levels || !dog_levels) return RGBDFE_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  *octave_min = ctx->sift.octave_min; *octave_num = ctx->sift.octave_num;
  *levels = SiftExtractor::kLevels; *dog_levels = SiftExtractor::kDogLevels;
  return RGBDFE_OK;
}

// hasNonZero(sub_mask) (feature_adjuster.cpp:175-183) of n cells for one frame: a sensor frame's mask, the caller's, or none
static void frame_mask_flags(const SensorRun* sensor, int sframe, const uint8_t* mask, int cols, const GridCell* cells, int n,
                             char* flags) {
  if (sensor) cell_mask_flags(cells, n, flags, [&](const GridCell& ce) { return sensor->mask_nonzero(sframe, ce.x0, ce.y0, ce.w, ce.h); });
  else if (mask) cell_mask_flags(cells, n, flags, [&](const GridCell& ce) { return mask_nonzero(mask, cols, ce); });
  else std::fill(flags, flags + n, (char)1);
}

// the batch pipelines' side streams and the events that order them, created by the first batch call
static int ensure_orb_streams(rgbdfe_ctx* ctx) {
  if (ctx->orb_upload_stream) return RGBDFE_OK;
  HIP_TRY(ctx, create_side_stream(&ctx->orb_upload_stream, -1));   // uploads + pyramids: behind everything else
  HIP_TRY(ctx, create_side_stream(&ctx->orb_compute_stream, +1));  // descriptions: short, the host waits for them
  for (hipEvent_t& e : ctx->orb_upload_done) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (hipEvent_t& e : ctx->orb_describe_done) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return RGBDFE_OK;
}

// One frame of Node::Node's feature path in three stages; the caller holds the lock.
//   detect()            detector grid + threshold adaptation (node.cpp:160) on ctx->stream: the frame's keypoints
//   describe_enqueue()  removeDepthless, retainBest, cv::ORB::compute and projectTo3D (:186-210) enqueued on a stream
//   finish()            wait for that stream, hand the results out
// A single call runs them back to back on one stream; rgbdfe_detect_describe_batch runs describe_enqueue of frame k while
// the device executes the detection pass of frame k + 1 (another stream, the other image set).
struct DetectFrame {
  rgbdfe_ctx* ctx = nullptr;
  const uint8_t* gray = nullptr; const uint8_t* mask = nullptr; const float* depth = nullptr;
  // a sensor frame in place of the three planes (rgbdfe_sensor_detect_describe*): frame `sframe` of the run; its float depth
  // plane (min-depth mode only) is ctx->sensor.d_depth[depth_set], written by the ingest launch behind the frame's upload
  const SensorRun* sensor = nullptr;
  int sframe = 0, depth_set = 0;
  int32_t rows = 0, cols = 0;
  double fx = 0, fy = 0, cx = 0, cy = 0, depth_scaling = 1;
  rgbdfe_keypoint* keypoints = nullptr; uint8_t* descriptors = nullptr; float* xyz1 = nullptr; int32_t* n_out = nullptr;
  std::vector<KpOut> kps;
  std::vector<float> zmin;
  float depth_px(int r, int c) const { return sensor ? sensor->depth_at(sframe, r, c) : depth[(size_t)r * cols + c]; }
  std::vector<uint8_t> desc;
  std::vector<int> order;  // compute(): positions, in the list handed to it, of the keypoints it keeps, in output order
  std::vector<float> xyz_in_big, xyz_out_big;
  float* xyz_out = nullptr;
  bool tm = false;
  double tq = 0;
  void lap(int slot) {
    if (!tm) return;
    const double now = orb_now_us();
    ctx->orb.timing.us[slot] += now - tq;
    tq = now;
  }

  int detect(bool uploaded, const std::function<int()>& prefetch) {
    OrbWorkspace& orb = ctx->orb;
    std::string err;
    static const bool timing_env = getenv("RGBDFE_DETECT_TIMING") && atoi(getenv("RGBDFE_DETECT_TIMING")) != 0;
    orb.timing.on = timing_env;
    tm = timing_env;
    tq = tm ? orb_now_us() : 0;
    int rc = orb.prepare(cols, rows, true, err);
    if (rc != RGBDFE_OK) return fail(ctx, rc, err);
    orb.cell_mask_nonzero.resize((size_t)orb.n_cells);
    frame_mask_flags(sensor, sframe, mask, cols, orb.cells.data(), orb.n_cells, orb.cell_mask_nonzero.data());
    // the depth image stays on the host: removeDepthless and projectTo3D look at one pixel per keypoint
    lap(0);
    if (!uploaded && sensor) {  // raw bytes up, the ingest kernel writes [gray | mask] into the pool (and the depth plane)
      sensor->stage(sframe, ctx->sensor.h_raw[0]);
      IngestParams o{};
      o.gray = orb.d_pool; o.mask = orb.d_pool + (size_t)rows * cols;
      o.depth_m = ctx->feature_min_depth ? ctx->sensor.d_depth[depth_set] : nullptr;
      rc = sensor_upload_ingest(ctx, *sensor, 0, 0, 1, o, ctx->stream);
      if (rc != RGBDFE_OK) return rc;
      rc = orb.build_uploaded(ctx->stream, err, -1, /*defer_blur=*/true);
    } else if (!uploaded) rc = orb.upload_and_build(gray, mask, ctx->stream, err, -1, /*defer_blur=*/true);
    lap(1);
    orb.before_wait = prefetch;
    const double pass_before = tm ? orb.timing.us[2] + orb.timing.us[3] + orb.timing.us[4] : 0;
    if (rc == RGBDFE_OK) rc = orb.grid_detect(kps, ctx->stream, err);  // node.cpp:160
    if (rc == RGBDFE_OK && orb.before_wait) {  // (cannot happen: a frame has at least one pass) -- never lose the hook
      std::function<int()> f = std::move(orb.before_wait);
      orb.before_wait = nullptr;
      rc = f();
    }
    orb.before_wait = nullptr;
    if (rc != RGBDFE_OK) return fail(ctx, rc, err);
    if (tm) {  // grid_detect minus its detection passes = the adjuster logic + the per-cell merge
      const double now = orb_now_us();
      orb.timing.us[5] += (now - tq) - (orb.timing.us[2] + orb.timing.us[3] + orb.timing.us[4] - pass_before);
      tq = now;
    }
    return RGBDFE_OK;
  }

  int describe_enqueue(hipStream_t st) {
    OrbWorkspace& orb = ctx->orb;
    const int max_kp = ctx->orb_max_keypoints;
    std::string err;
    int rc = RGBDFE_OK;
    if (tm) tq = orb_now_us();
    // "use_feature_min_depth" (parameter_server.cpp:90, rgbdfe_set_feature_min_depth): a keypoint's depth is the nearest
    // valid depth of its neighbourhood (getMinDepthInNeighborhood, misc.cpp:774-793) -- looked up on the device for all
    // keypoints at once (the depth image is uploaded in this mode only) and carried along with the keypoints from here on.
    const bool min_depth = ctx->feature_min_depth;
    if (min_depth && !kps.empty()) {
      const int n0 = (int)kps.size();
      DeviceLayout lay;
      const Block b_depth = lay.room((size_t)rows * cols * 4), b_kp = lay.room((size_t)n0 * 12), b_z = lay.room((size_t)n0 * 4);
      lay.room(256);
      rc = ensure_scratch(ctx, lay.total());
      if (rc != RGBDFE_OK) return rc;
      float* d_depth = sensor ? ctx->sensor.d_depth[depth_set] : at<float>(ctx->d_scratch, b_depth);
      float* d_kps3 = at<float>(ctx->d_scratch, b_kp);
      float* d_z = at<float>(ctx->d_scratch, b_z);
      std::vector<float> h3((size_t)n0 * 3);
      for (int i = 0; i < n0; ++i) { h3[3 * i] = kps[i].x; h3[3 * i + 1] = kps[i].y; h3[3 * i + 2] = kps[i].size; }
      zmin.resize((size_t)n0);
      if (!sensor) HIP_TRY(ctx, hipMemcpyAsync(d_depth, depth, (size_t)rows * cols * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(d_kps3, h3.data(), h3.size() * 4, hipMemcpyHostToDevice, st));
      launch_min_depth(d_kps3, n0, d_depth, rows, cols, d_z, st);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(zmin.data(), d_z, (size_t)n0 * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    // one scattered read of the 1.2 MB depth image per keypoint: issue them all before the first is needed (removeDepthless
    // otherwise pays a cache miss per keypoint, ~100 us per frame)
    for (const KpOut& k : kps) {
      if (min_depth || sensor) break;
      if (!(k.x >= 0 && k.x < (float)cols && k.y >= 0 && k.y < (float)rows)) continue;
      int r, c;
      depth_pixel(k, rows, cols, r, c);
      __builtin_prefetch(depth + (size_t)r * cols + c, 0, 1);
    }
    auto depth_at = [this](int r, int c) { return depth_px(r, c); };
    remove_depthless_and_cut(kps, min_depth ? &zmin : nullptr, depth_at, rows, cols, max_kp);  // node.cpp:186-191
    // cv::ORB::compute (node.cpp:202) drops border keypoints and regroups the rest by octave, so projectTo3D
    // (node.cpp:210) is enqueued from inside compute_enqueue(), once the final keypoint list exists: both ride on one
    // synchronisation.  xy (2n floats) + depth.at<float>(round(y), round(x)) (n floats, node.cpp:942): 12 bytes per
    // keypoint cross PCIe instead of the 1.2 MB image.
    auto enqueue_project = [&]() -> int {
      const int n = (int)kps.size();
      if (n == 0) return RGBDFE_OK;
      float* xyz_in = orb.h_xyz_in;
      xyz_out = orb.h_xyz_out;
      if (n > orb.pin_cap) {
        xyz_in_big.resize((size_t)n * 3); xyz_out_big.resize((size_t)n * 4);
        xyz_in = xyz_in_big.data(); xyz_out = xyz_out_big.data();
      }
      depth_lookups(kps, min_depth ? &zmin : nullptr, order, depth_at, rows, cols, xyz_in);
      if (hipMemcpyAsync(orb.d_kpxy, xyz_in, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess)
        return RGBDFE_ERR_HIP;
      launch_project_to_3d(orb.d_kpxy, n, nullptr, rows, cols, (float)(1. / fx), (float)(1. / fy), (float)cx,
                           (float)cy, depth_scaling, max_kp, orb.d_kept, orb.d_xyz, orb.d_n_proj, st, false,
                           orb.d_kpxy + (size_t)2 * n);
      if (hipGetLastError() != hipSuccess) return RGBDFE_ERR_HIP;
      if (hipMemcpyAsync(orb.h_n_proj, orb.d_n_proj, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipMemcpyAsync(xyz_out, orb.d_xyz, sizeof(float) * 4 * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess)
        return RGBDFE_ERR_HIP;
      return RGBDFE_OK;
    };
    lap(6);
    rc = orb.compute_enqueue(kps, desc, st, err, enqueue_project, &order);
    if (rc != RGBDFE_OK) return fail(ctx, rc, err);
    return RGBDFE_OK;
  }

  int finish(hipStream_t st) {
    OrbWorkspace& orb = ctx->orb;
    std::string err;
    const int rc = orb.compute_finish(desc, st, err);
    if (rc != RGBDFE_OK) return fail(ctx, rc, err);
    if (tm) tq = orb_now_us();
    const int n = (int)kps.size();
    *n_out = 0;
    if (n > 0) {
      if (*orb.h_n_proj != n) return fail(ctx, RGBDFE_ERR_HIP, "projectTo3D dropped keypoints that removeDepthless kept");
      memcpy(xyz1, xyz_out, sizeof(float) * 4 * (size_t)n);
    }
    kp_to_abi(kps, keypoints);
    if (!desc.empty()) memcpy(descriptors, desc.data(), desc.size());
    *n_out = n;
    lap(9);
    if (tm) orb.timing.frames++;
    return RGBDFE_OK;
  }

  // a single call: the three stages back to back on the context's stream (the images are set already)
  int run_alone(rgbdfe_ctx* c, double fx_, double fy_, double cx_, double cy_, double scaling, rgbdfe_keypoint* kp_out,
                uint8_t* desc_out, float* xyz_out_, int32_t* n) {
    ctx = c; fx = fx_; fy = fy_; cx = cx_; cy = cy_; depth_scaling = scaling;
    keypoints = kp_out; descriptors = desc_out; xyz1 = xyz_out_; n_out = n;
    int rc = detect(false, nullptr);
    if (rc == RGBDFE_OK) rc = describe_enqueue(ctx->stream);
    if (rc == RGBDFE_OK) rc = finish(ctx->stream);
    return rc;
  }
};

int rgbdfe_detect_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth,
                           int32_t rows, int32_t cols, double fx, double fy, double cx, double cy,
                           double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors,
                           float* xyz1, int32_t* n_out) {
  if (!ctx || !gray || !depth || rows < 1 || cols < 1 || !keypoints || !descriptors || !xyz1 || !n_out)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  if (ctx->detector_type == RGBDFE_DETECTOR_FAST)  // feature_detector_type "FAST" (api_fast.hip)
    return fast_detect_describe(ctx, 1, &gray, &mask, &depth, rows, cols, fx, fy, cx, cy, depth_scaling, ctx->orb_max_keypoints,
                                keypoints, descriptors, xyz1, n_out, nullptr);
  DetectFrame fr;
  fr.gray = gray; fr.mask = mask; fr.depth = depth; fr.rows = rows; fr.cols = cols;
  return fr.run_alone(ctx, fx, fy, cx, cy, depth_scaling, keypoints, descriptors, xyz1, n_out);
}

// rgbdfe_detect_describe on frame 0 of a sensor run (the ORB type; the caller holds the lock, has set the device, ensured
// the detector and ctx->sensor's buffers for one frame)
int detect_describe_sensor_frame(rgbdfe_ctx* ctx, const SensorRun& run, double fx, double fy, double cx, double cy,
                                 double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1,
                                 int32_t* n_out) {
  DetectFrame fr;
  fr.sensor = &run; fr.sframe = 0; fr.depth_set = 0; fr.rows = run.H; fr.cols = run.W;
  return fr.run_alone(ctx, fx, fy, cx, cy, depth_scaling, keypoints, descriptors, xyz1, n_out);
}

int detect_aggregate(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                     std::vector<KpOut>& kps) {
  if (ctx->detector_type == RGBDFE_DETECTOR_FAST)  // feature_detector_type "FAST" (api_fast.hip)
    return fast_grid_keypoints(ctx, gray, mask, rows, cols, kps);
  DetectFrame fr;
  fr.ctx = ctx; fr.gray = gray; fr.mask = mask; fr.rows = rows; fr.cols = cols;
  const int rc = fr.detect(false, nullptr);
  if (rc != RGBDFE_OK) return rc;
  kps = std::move(fr.kps);
  return RGBDFE_OK;
}

// detector->detect alone (node.cpp:160): the grid detector's aggregate (feature_adjuster.cpp:185-317) in aggregate order, with
// the per-cell thresholds advanced exactly as rgbdfe_detect_describe advances them -- its detection step, stopped before
// removeDepthless.  keepStrongest(max_total / cells) per cell bounds the aggregate by max_total, so a smaller capacity is
// refused before the detector's state changes.
int rgbdfe_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                  rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out) {
  if (!ctx || !gray || rows < 1 || cols < 1 || !keypoints || !n_out) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  if (capacity < ctx->orb.max_total)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "capacity below the aggregate's bound floor(1.5 * max_keypoints)");
  *n_out = 0;
  std::vector<KpOut> kps;
  const int rc = detect_aggregate(ctx, gray, mask, rows, cols, kps);
  if (rc != RGBDFE_OK) return rc;
  if ((int64_t)kps.size() > (int64_t)capacity) return fail(ctx, RGBDFE_ERR_INTERNAL, "aggregate larger than max_total");
  kp_to_abi(kps, keypoints);
  *n_out = (int32_t)kps.size();
  return RGBDFE_OK;
}

// ---- rgbdfe_detect_describe_batch, super-frame form -----------------------------------------------------------------
constexpr int kSuperFrames = 7;   // frames per super-frame at least (large frames)
// B = 64 / grid^2 (7 for the 3 x 3 grid) frames share every launch: one upload, one pyramid chain (7 launches), one blur,
// one detection pass (FAST score -> NMS count -> scan -> emit -> measure) over 7 x 72 images, one rBRIEF launch -- a frame
// alone is 1.7 M pixels and cannot fill 256 CUs, and its 27 dependent device operations cost 5-15 us each whatever their
// size.  Frames stay sequentially dependent through the per-cell FAST thresholds: the device pass runs at a floor threshold
// and OrbWorkspace::super_replay replays the reference's adjuster over the scored corners frame by frame (identical
// keypoints: see orb_replay.h select_cell).  The per-frame CPU work that does not touch the HIP runtime (removeDepthless, retainBest,
// cv::ORB::compute's border filter / regroup / descriptor records, the depth look-ups) runs on worker threads while the
// calling thread drives the next super-frame's pass.
namespace {

struct SuperFrameJob {  // one frame of a super-frame, between detection and copy-out
  bool deferred = false;              // the frame's keypoints are still to be selected from the pass's corners (select_frame)
  GridDetector det;                   // ... of this detector (its mask flags are the calling thread's: not read here)
  PassView pv;
  std::vector<int> thr;               // every (frame, cell)'s final threshold of the super-frame
  std::vector<KpOut> kps;
  std::vector<int> order;
  std::vector<DescKp> dk;
  std::vector<float> xyz_in;  // 2n (x, y) then n depths
  int off = 0;                // first row of this frame in the super-frame's concatenated buffers
};

// removeDepthless (node.cpp:67-97, :186) + retainBest(max_keypoints) (:188-191) + the CPU half of cv::ORB::compute +
// projectTo3D's depth look-ups (node.cpp:942) for one frame: DetectFrame::describe_enqueue's host work, no HIP calls
void super_describe_prepare(const OrbWorkspace& orb, SuperFrameJob& j, int frame_in_super, const float* depth, int rows,
                            int cols, int max_kp, const SensorRun* sensor = nullptr, int sframe = 0) {
  auto depth_px = [&](int r, int c) { return sensor ? sensor->depth_at(sframe, r, c) : depth[(size_t)r * cols + c]; };
  if (j.deferred) select_frame(j.det, j.pv, frame_in_super, j.thr.data(), j.kps);
  remove_depthless_and_cut(j.kps, nullptr, depth_px, rows, cols, max_kp);
  orb.compute_prepare(j.kps, frame_in_super, j.order, j.dk);
  j.xyz_in.resize(j.kps.size() * 3);
  depth_lookups(j.kps, nullptr, j.order, depth_px, rows, cols, j.xyz_in.data());
}

int detect_describe_batch_super(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                                const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                double cy, double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                uint8_t* descriptors, float* xyz1, int32_t* n_out, const int32_t* node_ids,
                                const SensorRun* sensor) {
  OrbWorkspace& orb = ctx->orb_super;
  const OrbWorkspace& one = ctx->orb;
  const int pc = one.grid * one.grid;
  // frames per super-frame: as many as the launches' tables hold, at most kSuperFrames (RGBDFE_SUPER_FRAMES: A/B runs)
  static const int super_frames_env = getenv("RGBDFE_SUPER_FRAMES") ? atoi(getenv("RGBDFE_SUPER_FRAMES")) : 0;
  // default: about 4.3 Mpixel of frames per launch, 7 to 28 frames -- 14 at 640 x 480 (measured 7 / 14 / 28 frames: 13.4 / 16.3 /
  // 16.6 k frames/s), 7 at 1280 x 960 (4.7 / 4.7 / 1.9 k: a 112-frame run is only four super-frames of 28)
  const int by_size = std::max(kSuperFrames, std::min(28, (int)(4300000.0 / ((double)rows * (double)cols) + 0.5)));
  const int B = std::max(1, std::min(std::min(kOrbCtlMax / pc, kProjectFramesMax), super_frames_env > 0 ? super_frames_env : by_size));
  // the detector object is one: its configuration and thresholds move into the super-frame workspace and back
  orb.grid = one.grid; orb.adjuster_iters = one.adjuster_iters; orb.cell_min = one.cell_min; orb.cell_max = one.cell_max;
  orb.max_total = one.max_total; orb.lookahead = one.lookahead;
  for (int i = 0; i < 64; ++i) orb.thresh[i] = one.thresh[i];
  if (const char* e = getenv("RGBDFE_SUPER_FLOOR")) orb.super_floor_factor = atof(e);  // experiments
  std::string err;
  int rc = orb.prepare(cols, rows, true, err, B);
  if (rc == RGBDFE_OK) rc = orb.ensure_alt(err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err);
  // sensor frames: a raw staging buffer per image staging buffer, a raw device buffer per image set
  if (sensor) {
    rc = sensor_ensure(ctx, OrbWorkspace::kStages, OrbWorkspace::kSets, sensor->frame_bytes * (size_t)B, 0, 0);
    if (rc != RGBDFE_OK) return rc;
  }
  if ((rc = ensure_orb_streams(ctx)) != RGBDFE_OK) return rc;
  hipStream_t up = ctx->orb_upload_stream, st2 = ctx->orb_compute_stream;
  const int max_kp = ctx->orb_max_keypoints;
  if (node_ids) {
    // all-or-nothing on capacity, like rgbdfe_upload_nodes: everything that can be refused is refused before the first
    // frame is detected.  Every fresh id is counted as needing a slot: a frame that ends up WITHOUT features still becomes an
    // (empty, n = 0) node -- a fresh id takes its slot, an existing node is rewritten to n = 0 (the end of this function) -- so
    // the count is exact.
    if (max_kp > ctx->cfg.max_keypoints)
      return fail(ctx, RGBDFE_ERR_CAPACITY, "the detector's max_keypoints exceeds the context's max_keypoints (node rows)");
    // The slots themselves are taken super-frame by super-frame (acquire_node_slot).
    rc = reserve_node_slots(ctx, n_frames, node_ids, 0u, nullptr);
    if (rc != RGBDFE_OK) return rc;
  }
  const int S = (n_frames + B - 1) / B;
  // D - 1 device passes are in flight ahead of the super-frame the host is replaying: D image sets / pass slots, D + 1
  // staging buffers.  A pass is a chain of ~25 dependent device operations (~1 ms from enqueue to read-back although its
  // kernels take < 0.5 ms), so one pass ahead leaves the host waiting; two hide the chain.  RGBDFE_SUPER_DEPTH=2: one ahead.
  int D = OrbWorkspace::kSets;
  if (const char* e = getenv("RGBDFE_SUPER_DEPTH")) D = std::min(std::max(atoi(e), 2), (int)OrbWorkspace::kSets);
  auto first_of = [&](int s) { return s * B; };
  auto count_of = [&](int s) { return std::min(B, n_frames - s * B); };
  // helper thread: the caller's pageable images of super-frame s -> pinned staging buffer s % NS, as soon as super-frame
  // s - NS (the buffer's previous user) has been detected (its upload from that buffer is complete then)
  const int NS = std::max(D + 1, std::min((int)OrbWorkspace::kStages,
                                          getenv("RGBDFE_SUPER_STAGES") ? atoi(getenv("RGBDFE_SUPER_STAGES")) : (int)OrbWorkspace::kStages));
  // (the frames' CPU halves: a worker per frame up to RGBDFE_DETECT_WORKERS workers, the frames queue behind them)
  static const int max_workers = getenv("RGBDFE_DETECT_WORKERS") ? std::max(1, atoi(getenv("RGBDFE_DETECT_WORKERS"))) : 14;   // (a worker per frame of a 14-frame super-frame; 7 / 12 / 14 workers: 20.6 / 20.3 / 21.2 k frames/s, four alternating runs each)
  const int n_workers = std::min(B, max_workers);
  if (!ctx->detect_pool || ctx->detect_pool->size() != n_workers) ctx->detect_pool.reset(new TaskPool(n_workers));
  TaskPool& copy_pool = stage_pool(ctx);
  TaskPool& pool = *ctx->detect_pool;
  pool.failed_ = false;
  StagingRing ring(S, NS, [&](int s) {
    // (2 W H bytes per frame through one core's memcpy would bound the whole pipeline: 75 us per 640 x 480 frame)
    for (int k = 0; k < count_of(s); ++k) {
      const int f = first_of(s) + k;
      if (sensor) {  // the raw bytes, nothing else: the ingest kernel behind the upload makes the planes
        uint8_t* dst = ctx->sensor.h_raw[s % NS] + (size_t)k * sensor->frame_bytes;
        copy_pool.submit([sensor, f, dst] { sensor->stage(f, dst); });
        continue;
      }
      copy_pool.submit([&orb, &gray, &mask, f, s, k, NS] { orb.stage_image_at(gray[f], mask ? mask[f] : nullptr, s % NS, k); });
    }
    copy_pool.wait_all();
  });
  std::vector<SuperFrameJob> jobs[2];
  jobs[0].resize((size_t)B); jobs[1].resize((size_t)B);
  int n_tot[2] = {0, 0};
  auto enqueue_upload = [&](int s) -> int {
    ring.wait_staged(s);
    if (s >= D && hipStreamWaitEvent(up, ctx->orb_describe_done[s % D], 0) != hipSuccess) { err = "hipStreamWaitEvent"; return RGBDFE_ERR_HIP; }
    int r;
    if (sensor) {  // frame k's [gray | mask] pair at k * 2WH of the set's pool (orb_host.hip enqueue_staged_super)
      IngestParams o{};
      o.gray = orb.pool_set[s % D]; o.mask = o.gray + (size_t)rows * cols;
      o.gray_stride = o.mask_stride = (size_t)2 * rows * cols;
      r = sensor_upload_ingest(ctx, *sensor, s % NS, s % D, count_of(s), o, up);
      if (r != RGBDFE_OK) { err.clear(); return r; }
      r = orb.build_uploaded(up, err, s % D, false);
    } else r = orb.enqueue_staged_super(count_of(s), up, err, s % D, s % NS);
    if (r != RGBDFE_OK) return r;
    if (hipEventRecord(ctx->orb_upload_done[s % D], up) != hipSuccess) { err = "hipEventRecord"; return RGBDFE_ERR_HIP; }
    return RGBDFE_OK;
  };
  // the CPU halves of super-frame s's descriptions: worker threads, no HIP calls
  auto start_prepare = [&](int s) {
    std::vector<SuperFrameJob>& J = jobs[s & 1];
    for (int k = 0; k < count_of(s); ++k) {
      const int sf = first_of(s) + k;
      const float* dp = sensor ? nullptr : depth[sf];
      SuperFrameJob* j = &J[(size_t)k];
      pool.submit([&orb, j, k, dp, rows, cols, max_kp, sensor, sf] { super_describe_prepare(orb, *j, k, dp, rows, cols, max_kp, sensor, sf); });
    }
  };
  // device half: one descriptor-record upload, one rBRIEF launch, one projectTo3D launch per frame, three read-backs
  auto enqueue_describe = [&](int s) -> int {
    pool.wait_all();
    if (pool.failed_) { err = "describe preparation failed"; return RGBDFE_ERR_INTERNAL; }
    std::vector<SuperFrameJob>& J = jobs[s & 1];
    const int nf = count_of(s);
    int tot = 0;
    for (int k = 0; k < nf; ++k) { J[(size_t)k].off = tot; tot += (int)J[(size_t)k].kps.size(); }
    n_tot[s & 1] = tot;
    if (hipStreamWaitEvent(st2, ctx->orb_upload_done[s % D], 0) != hipSuccess) return RGBDFE_ERR_HIP;
    if (tot > orb.pin_cap || tot > orb.kp_cap) { err = "super-frame: more keypoints than the staging buffers hold"; return RGBDFE_ERR_CAPACITY; }
    if (tot > 0) {
      for (int k = 0; k < nf; ++k) {
        const SuperFrameJob& j = J[(size_t)k];
        const size_t n = j.kps.size();
        if (n == 0) continue;
        memcpy(orb.h_desckp + j.off, j.dk.data(), sizeof(DescKp) * n);
        memcpy(orb.h_xyz_in + (size_t)3 * j.off, j.xyz_in.data(), sizeof(float) * 3 * n);
      }
      uint8_t* const pool_dev = orb.pool_set[s % D];
      uint8_t* const blur_dev = orb.blur_set[s % D];
      if (hipMemcpyAsync(orb.d_desckp, orb.h_desckp, sizeof(DescKp) * (size_t)tot, hipMemcpyHostToDevice, st2) != hipSuccess ||
          hipMemcpyAsync(orb.d_kpxy, orb.h_xyz_in, sizeof(float) * 3 * (size_t)tot, hipMemcpyHostToDevice, st2) != hipSuccess)
        return RGBDFE_ERR_HIP;
      launch_orb_brief(pool_dev, blur_dev, orb.d_frame_imgs, orb.d_desckp, tot, orb.d_desc, st2);
      ProjectFrames pf{};
      pf.n_frames = nf;
      for (int k = 0; k < nf; ++k) { pf.off[k] = J[(size_t)k].off; pf.n[k] = (int)J[(size_t)k].kps.size(); }
      launch_project_to_3d_frames(pf, orb.d_kpxy, rows, cols, (float)(1. / fx), (float)(1. / fy), (float)cx, (float)cy,
                                  depth_scaling, max_kp, orb.d_kept, orb.d_xyz, orb.d_n_proj, st2);
      if (hipGetLastError() != hipSuccess) return RGBDFE_ERR_HIP;
      // node_ids: the frames' features become resident nodes straight from the description's device buffers (no trip
      // through the host and back: what Node::Node + GraphManager::addNode + rgbdfe_upload_node would do)
      if (node_ids)
        for (int k = 0; k < nf; ++k) {
          const int32_t id = node_ids[first_of(s) + k];
          const int n = (int)J[(size_t)k].kps.size();
          if (id < 0 || n == 0) continue;
          if (n > ctx->cfg.max_keypoints) { err = "node has more rows than max_keypoints"; return RGBDFE_ERR_CAPACITY; }
          uint32_t slot;
          const int rc_slot = acquire_node_slot(ctx, id, 0u, &slot, true);   // (the lanes: waited for before the first frame)
          if (rc_slot != RGBDFE_OK) return rc_slot;
          const size_t row0 = (size_t)slot * (size_t)ctx->cfg.max_keypoints;
          const size_t off = (size_t)J[(size_t)k].off;
          if (hipMemcpyAsync(ctx->d_desc + row0 * 8, orb.d_desc + off * 32, (size_t)n * 32, hipMemcpyDeviceToDevice, st2) != hipSuccess ||
              hipMemcpyAsync(ctx->d_xyz + row0, orb.d_xyz + off, (size_t)n * 16, hipMemcpyDeviceToDevice, st2) != hipSuccess)
            return RGBDFE_ERR_HIP;
          launch_hamming_expand(ctx->d_desc + row0 * 8, ctx->d_desc4, slot, (uint32_t)ctx->cfg.max_keypoints, (uint32_t)n, st2);
          ctx->nodes[id] = NodeEntry{slot, (uint32_t)n, 0u, 0u};
        }
      if (hipMemcpyAsync(orb.h_desc, orb.d_desc, (size_t)32 * tot, hipMemcpyDeviceToHost, st2) != hipSuccess ||
          hipMemcpyAsync(orb.h_xyz_out, orb.d_xyz, sizeof(float) * 4 * (size_t)tot, hipMemcpyDeviceToHost, st2) != hipSuccess ||
          hipMemcpyAsync(orb.h_n_proj, orb.d_n_proj, sizeof(int32_t) * (size_t)nf, hipMemcpyDeviceToHost, st2) != hipSuccess)
        return RGBDFE_ERR_HIP;
    }
    return hipEventRecord(ctx->orb_describe_done[s % D], st2) == hipSuccess ? RGBDFE_OK : RGBDFE_ERR_HIP;
  };
  auto finish = [&](int s) -> int {
    if (hipStreamSynchronize(st2) != hipSuccess) return RGBDFE_ERR_HIP;
    std::vector<SuperFrameJob>& J = jobs[s & 1];
    for (int k = 0; k < count_of(s); ++k) {
      const SuperFrameJob& j = J[(size_t)k];
      const int f = first_of(s) + k;
      const int n = (int)j.kps.size();
      n_out[f] = 0;
      if (n > 0) {
        if (orb.h_n_proj[k] != n) { err = "projectTo3D dropped keypoints that removeDepthless kept"; return RGBDFE_ERR_HIP; }
        memcpy(xyz1 + (size_t)f * out_stride * 4, orb.h_xyz_out + (size_t)4 * j.off, sizeof(float) * 4 * (size_t)n);
        memcpy(descriptors + (size_t)f * out_stride * 32, orb.h_desc + (size_t)32 * j.off, (size_t)32 * n);
      }
      kp_to_abi(j.kps, keypoints + (size_t)f * out_stride);
      n_out[f] = n;
    }
    return RGBDFE_OK;
  };
  static const bool tm = getenv("RGBDFE_DETECT_TIMING") && atoi(getenv("RGBDFE_DETECT_TIMING")) != 0;
  double t_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // mask scan, replay, hook: describe enqueue, hook: upload enqueue, finish, prepare start, pool wait
  double tq = tm ? orb_now_us() : 0;
  auto lap = [&](int i) { if (tm) { const double now = orb_now_us(); t_us[i] += now - tq; tq = now; } };
  orb.timing.on = tm;
  const long passes0 = orb.device_passes;
  // Software pipeline: the device pass of super-frame s + 1 is enqueued BEFORE the host replays the adjuster over
  // super-frame s (its floors come from the thresholds of that moment; a cell that falls below its floor is re-run by
  // super_replay), so the device works on s + 1 while the host selects keypoints of s; description of s - 1 and the
  // upload of s + 1 are enqueued in between, the CPU halves of the descriptions run on the worker threads.
  auto pass_enqueue = [&](int s) -> int {
    if (hipStreamWaitEvent(ctx->stream, ctx->orb_upload_done[s % D], 0) != hipSuccess) { err = "hipStreamWaitEvent"; return RGBDFE_ERR_HIP; }
    return orb.super_pass_enqueue(count_of(s), s % D, s % D, ctx->stream, err);
  };
  for (int s = 0; s < D - 1 && s < S && rc == RGBDFE_OK; ++s) {
    rc = enqueue_upload(s);
    if (rc == RGBDFE_OK) rc = pass_enqueue(s);
  }
  lap(6);
  for (int s = 0; s < S && rc == RGBDFE_OK; ++s) {
    const int nf = count_of(s);
    if (tm) tq = orb_now_us();
    if (s > 0) { rc = enqueue_describe(s - 1); if (rc != RGBDFE_OK) break; }
    lap(2);
    if (s + D - 1 < S) {
      rc = enqueue_upload(s + D - 1);
      if (rc == RGBDFE_OK) rc = pass_enqueue(s + D - 1);
      if (rc != RGBDFE_OK) break;
    }
    lap(3);
    orb.cell_mask_nonzero.assign((size_t)orb.n_cells, 1);
    for (int k = 0; k < nf; ++k)
      frame_mask_flags(sensor, first_of(s) + k, mask ? mask[first_of(s) + k] : nullptr, cols, orb.cells.data() + (size_t)k * pc, pc,
                       orb.cell_mask_nonzero.data() + (size_t)k * pc);
    lap(0);
    std::vector<std::vector<KpOut>> kps;
    OrbWorkspace::Deferred def;
    rc = orb.super_replay(nf, s % D, s % D, kps, ctx->stream, err, def);
    if (rc != RGBDFE_OK) break;
    ring.mark_consumed(s);   // (its upload from the staging buffer is complete)
    lap(1);
    if (s > 0) { rc = finish(s - 1); if (rc != RGBDFE_OK) break; }
    lap(4);
    for (int k = 0; k < nf; ++k) {
      SuperFrameJob& j = jobs[s & 1][(size_t)k];
      j.deferred = def.valid;
      if (def.valid) { j.det = orb.detector(); j.pv = def.pv; j.thr = def.thr_final; j.kps.clear(); }
      else j.kps.swap(kps[(size_t)k]);
    }
    start_prepare(s);
    lap(5);
  }
  if (tm) {
    fprintf(stderr, "[rgbdfe super-frame timing] depth %d (sequential fallbacks: %ld); ", D, orb.replay_fallbacks);
    fprintf(stderr, "[rgbdfe super-frame timing] %d frames in %d super-frames, %ld device passes; per frame (us): mask scan %.1f, "
            "replay incl. wait for its pass %.1f, describe enqueue %.1f, upload + next pass enqueue %.1f (re-passes: enqueue %.1f, "
            "wait %.1f; selections %.1f), finish %.1f, prepare start %.1f\n", (int)n_frames, S, orb.device_passes - passes0,
            t_us[0] / n_frames, t_us[1] / n_frames, t_us[2] / n_frames, t_us[3] / n_frames, orb.timing.us[2] / n_frames,
            orb.timing.us[3] / n_frames, orb.timing.us[4] / n_frames, t_us[4] / n_frames, t_us[5] / n_frames);
    for (double& u : orb.timing.us) u = 0;
    orb.timing.frames = 0; orb.timing.passes = 0;
    tq = orb_now_us();
  }
  if (rc == RGBDFE_OK) rc = enqueue_describe(S - 1);
  if (rc == RGBDFE_OK) rc = finish(S - 1);
  pool.wait_all();
  (void)hipStreamSynchronize(st2);
  lap(7);
  if (tm) fprintf(stderr, "[rgbdfe super-frame timing] whole call (us): filling the pipeline (staging + upload + pass enqueue of the first "
                          "%d super-frames) %.0f, draining it (the last super-frame's description) %.0f\n", D - 1, t_us[6], t_us[7]);
  ring.stop();
  (void)hipStreamSynchronize(up);
  (void)hipStreamSynchronize(ctx->stream);
  orb.use_set(0);
  for (int i = 0; i < 64; ++i) ctx->orb.thresh[i] = orb.thresh[i];   // the detector's state goes back
  if (rc != RGBDFE_OK) return err.empty() ? rc : fail(ctx, rc, err);
  if (node_ids)   // frames without features: empty nodes (n = 0), as rgbdfe_upload_node(id, ..., 0) would leave them
    for (int32_t f = 0; f < n_frames; ++f)
      if (node_ids[f] >= 0 && n_out[f] == 0) {
        uint32_t slot;
        rc = acquire_node_slot(ctx, node_ids[f], 0u, &slot, true);
        if (rc != RGBDFE_OK) return rc;
        ctx->nodes[node_ids[f]].n = 0;
      }
  return RGBDFE_OK;
}

}  // namespace

// A run of frames through the same detector state, in order (the per-cell thresholds of frame k+1 start from frame k's,
// as in a sequence of single calls -- same keypoints, bit for bit).  What the batch adds is overlap, three deep: frame
// k+2's images are staged, uploaded and turned into their pyramid by a helper thread (own stream, the free image set)
// while frame k+1's detection pass runs on the device and the calling thread prepares and enqueues frame k's description
// (third stream) instead of sitting in hipStreamSynchronize.  Outputs: frame f's keypoints /
// descriptors / points at offset f * out_stride (rows), n_out[f] of them.
static int detect_describe_batch_frames(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                                        const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                        double cy, double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                        uint8_t* descriptors, float* xyz1, int32_t* n_out, const SensorRun* sensor);
// node_ids (may be NULL): frame f's features also become the resident node node_ids[f] (>= 0), see
// rgbdfe_detect_describe_batch_nodes
int rgbdfe_detect_describe_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                                 const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                 double cy, double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                 uint8_t* descriptors, float* xyz1, int32_t* n_out, const int32_t* node_ids,
                                 const SensorRun* sensor) {
  // (sensor: a validated run of sensor frames in place of the three plane arrays, which are NULL then; api_sensor.hip)
  if (!ctx || n_frames < 0 || (n_frames > 0 && ((!sensor && (!gray || !depth)) || !n_out)) || rows < 1 || cols < 1)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (node_ids && node_id_twice(n_frames, node_ids)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "a node id appears twice");
  std::lock_guard<std::mutex> g(ctx->mu);
  // (the host outputs may be NULL only where the nodes are the outputs: FAST with node_ids)
  const bool fast = ctx->detector_type == RGBDFE_DETECTOR_FAST;
  if (n_frames > 0 && !(fast && node_ids) && (!keypoints || !descriptors || !xyz1))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  if (n_frames > 0 && out_stride < ctx->orb_max_keypoints)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "out_stride must be at least the configured max_keypoints");
  if (!sensor && !frames_non_null(n_frames, gray, depth)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "null frame");
  if (n_frames == 0) return RGBDFE_OK;
  if (sensor) {
    const int rc_dev = sensor_run_device(ctx, const_cast<SensorRun&>(*sensor));   // the resampling tables
    if (rc_dev != RGBDFE_OK) return rc_dev;
  }
  if (fast)  // feature_detector_type "FAST" (api_fast.hip): its own chunked pipeline, nodes written by its kernels
    return fast_detect_describe(ctx, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy, depth_scaling, out_stride, keypoints,
                                descriptors, xyz1, n_out, node_ids, sensor);
  {  // several frames per launch chain (above) unless switched off or the detector is in a mode only the frame path has
    static const bool super_env = !(getenv("RGBDFE_DETECT_SUPER") && atoi(getenv("RGBDFE_DETECT_SUPER")) == 0);
    if (super_env && n_frames >= 2 && !ctx->feature_min_depth && ctx->orb.grid * ctx->orb.grid * 2 <= 64)
      return detect_describe_batch_super(ctx, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy, depth_scaling, out_stride,
                                         keypoints, descriptors, xyz1, n_out, node_ids, sensor);
  }
  const int rc_frames = detect_describe_batch_frames(ctx, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                                    out_stride, keypoints, descriptors, xyz1, n_out, sensor);
  if (rc_frames != RGBDFE_OK || !node_ids) return rc_frames;
  // the frame-by-frame pipeline hands its nodes over from the host outputs
  std::vector<int32_t> ids, cnt;
  std::vector<const uint8_t*> dp;
  std::vector<const float*> xp;
  for (int32_t f = 0; f < n_frames; ++f)
    if (node_ids[f] >= 0) {
      ids.push_back(node_ids[f]); cnt.push_back(n_out[f]);
      dp.push_back(descriptors + (size_t)f * out_stride * 32); xp.push_back(xyz1 + (size_t)f * out_stride * 4);
    }
  return upload_nodes_locked(ctx, (int32_t)ids.size(), ids.data(), dp.data(), xp.data(), cnt.data());
}

static int detect_describe_batch_frames(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                                        const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                        double cy, double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                        uint8_t* descriptors, float* xyz1, int32_t* n_out, const SensorRun* sensor) {
  OrbWorkspace& orb = ctx->orb;
  std::string err;
  int rc = orb.prepare(cols, rows, true, err);
  if (rc == RGBDFE_OK) rc = orb.ensure_alt(err);
  if (rc != RGBDFE_OK) return fail(ctx, rc, err);
  if ((rc = ensure_orb_streams(ctx)) != RGBDFE_OK) return rc;
  hipStream_t up = ctx->orb_upload_stream;
  if (sensor) {  // frame f's raw bytes and float depth plane live in set f & 1 too
    rc = sensor_ensure(ctx, 2, 2, sensor->frame_bytes, ctx->feature_min_depth ? 2 : 0, (size_t)rows * cols);
    if (rc != RGBDFE_OK) return rc;
  }
  // Frame f lives in image set f & 1 (device pyramid + pinned staging buffer).  A helper thread copies the caller's
  // pageable images of frame f into the set's staging buffer as soon as frame f - 2 has been detected (its upload from that
  // buffer is complete then) -- CPU work only: two host threads inside the HIP runtime at once serialise on its locks, and
  // the calling thread's launches are the critical path.  The calling thread enqueues the device half of frame f + 2's
  // upload (one copy + the pyramid launches, on a second stream) from the hook of frame f + 1's detection pass, behind
  // frame f's description, which reads the same set.
  StagingRing ring(n_frames, 2, [&](int f) {
    if (sensor) sensor->stage(f, ctx->sensor.h_raw[f & 1]);
    else orb.stage_images(gray[f], mask ? mask[f] : nullptr, f & 1);
  });
  // The calling thread: frame f + 1 is detected on ctx->stream (set (f + 1) & 1) while frame f is described on the second
  // stream (set f & 1) -- describe_enqueue(f) runs as the `before_wait` hook of frame f + 1's first detection pass, i.e.
  // its host work (removeDepthless, retainBest, the descriptor records) overlaps that pass's device time.
  hipStream_t st2 = ctx->orb_compute_stream;
  std::vector<DetectFrame> fr((size_t)2);
  auto init = [&](DetectFrame& d, int32_t f) {
    d = DetectFrame();
    d.ctx = ctx; d.rows = rows; d.cols = cols;
    if (sensor) { d.sensor = sensor; d.sframe = f; d.depth_set = f & 1; }
    else { d.gray = gray[f]; d.mask = mask ? mask[f] : nullptr; d.depth = depth[f]; }
    d.fx = fx; d.fy = fy; d.cx = cx; d.cy = cy; d.depth_scaling = depth_scaling;
    d.keypoints = keypoints + (size_t)f * out_stride; d.descriptors = descriptors + (size_t)f * out_stride * 32;
    d.xyz1 = xyz1 + (size_t)f * out_stride * 4; d.n_out = n_out + f;
  };
  auto enqueue_upload = [&](int32_t f) -> int {  // the device half of frame f's upload, on `up`
    ring.wait_staged(f);
    // the set was frame f - 2's: its description (second stream) reads the pyramid this upload overwrites
    if (f >= 2 && hipStreamWaitEvent(up, ctx->orb_describe_done[f & 1], 0) != hipSuccess) { err = "hipStreamWaitEvent"; return RGBDFE_ERR_HIP; }
    int r;
    if (sensor) {
      IngestParams o{};
      o.gray = orb.pool_set[f & 1]; o.mask = o.gray + (size_t)rows * cols;
      o.depth_m = ctx->feature_min_depth ? ctx->sensor.d_depth[f & 1] : nullptr;
      r = sensor_upload_ingest(ctx, *sensor, f & 1, f & 1, 1, o, up);
      if (r != RGBDFE_OK) { err.clear(); return r; }
      r = orb.build_uploaded(up, err, f & 1, false);
    } else r = orb.enqueue_staged(mask != nullptr && mask[f] != nullptr, up, err, f & 1);
    if (r != RGBDFE_OK) return r;
    if (hipEventRecord(ctx->orb_upload_done[f & 1], up) != hipSuccess) { err = "hipEventRecord"; return RGBDFE_ERR_HIP; }
    return RGBDFE_OK;
  };
  auto wait_upload = [&](int32_t f) -> int {  // order ctx->stream behind frame f's upload and pyramid
    if (hipStreamWaitEvent(ctx->stream, ctx->orb_upload_done[f & 1], 0) != hipSuccess) { err = "hipStreamWaitEvent"; return RGBDFE_ERR_HIP; }
    return RGBDFE_OK;
  };
  auto describe = [&](int32_t f) -> int {  // enqueue frame f's description on the second stream, from its own image set
    orb.use_set(f & 1);
    if (hipStreamWaitEvent(st2, ctx->orb_upload_done[f & 1], 0) != hipSuccess) return RGBDFE_ERR_HIP;
    const int r = fr[(size_t)(f & 1)].describe_enqueue(st2);
    if (r != RGBDFE_OK) return r;
    return hipEventRecord(ctx->orb_describe_done[f & 1], st2) == hipSuccess ? RGBDFE_OK : RGBDFE_ERR_HIP;
  };
  rc = enqueue_upload(0);
  if (rc == RGBDFE_OK) rc = wait_upload(0);
  if (rc == RGBDFE_OK) {
    init(fr[0], 0);
    orb.use_set(0);
    int rc_up = RGBDFE_OK;
    rc = fr[0].detect(true, n_frames > 1 ? std::function<int()>([&]() -> int { rc_up = enqueue_upload(1); return rc_up; })
                                         : std::function<int()>());
    if (rc != RGBDFE_OK && rc_up == RGBDFE_OK) err.clear();  // reported through fail()
    if (rc == RGBDFE_OK) ring.mark_consumed(0);
  }
  for (int32_t f = 0; f < n_frames && rc == RGBDFE_OK; ++f) {
    if (f + 1 < n_frames) {
      rc = wait_upload(f + 1);
      if (rc != RGBDFE_OK) break;
      init(fr[(size_t)((f + 1) & 1)], f + 1);
      orb.use_set((f + 1) & 1);
      int rc_hook = RGBDFE_OK;
      bool hook_err_is_mine = false;
      rc = fr[(size_t)((f + 1) & 1)].detect(true, [&, f]() -> int {
        rc_hook = describe(f);
        if (rc_hook == RGBDFE_OK && f + 2 < n_frames) {
          rc_hook = enqueue_upload(f + 2);
          hook_err_is_mine = rc_hook != RGBDFE_OK;
        }
        orb.use_set((f + 1) & 1);  // the rest of the pass (a second read-back of a crowded frame) is frame f + 1's
        return rc_hook;
      });
      if (rc != RGBDFE_OK) { if (!hook_err_is_mine) err.clear(); break; }
      ring.mark_consumed(f + 1);
    } else {
      rc = describe(f);
      if (rc != RGBDFE_OK) { err.clear(); break; }
    }
    rc = fr[(size_t)(f & 1)].finish(st2);
    if (rc != RGBDFE_OK) { err.clear(); break; }
  }
  (void)hipStreamSynchronize(st2);
  ring.stop();
  (void)hipStreamSynchronize(up);
  orb.use_set(0);
  if (rc != RGBDFE_OK) return err.empty() ? rc : fail(ctx, rc, err);
  return RGBDFE_OK;
}


}  // namespace impl
