// api_sift_behind.hip -- feature_extractor_type "SIFTGPU" behind the ORB or FAST grid detector (node.cpp:160, 165-176), one
// frame or a run of frames into resident float nodes.  (one of the host-side translation units of librgbdfe.so; rgbdfe_host.h)
//
// A chunk of up to 8 frames, under the context's lock from the first detection to the last output:
//   1. detector->detect per frame, in order (the per-cell thresholds carry over): the aggregate, on the host after the
//      detector's own read-back (ORB: the host replay; FAST: the select kernel's list)
//   2. the aggregates and depth images go up; sift_keys_from_detector (sift_keys.hip) runs projectTo3D's walk, the cut and the
//      wrapper's conversions for every frame in one launch; the counts and the SiftGPU keys (16 bytes a keypoint) come back
//   3. frames with no kept keypoint take the wrapper's empty-list path: SiftGPU's own detection (rare: no depth anywhere a
//      corner is); the others share one pyramid chain and ONE descriptor launch (SiftExtractor::describe_frames), whose rows
//      are gathered into the callers' order on the device
//   4. sift_nodes.hip: projectTo3DSiftGPU + RootSIFT into the node slabs and the output rows, one launch for the chunk
//   5. the counts (and the host outputs, when asked for) come back once
// With NULL host outputs no descriptor crosses PCIe, except those of empty-list frames.
#include "rgbdfe_host.h"

namespace impl {

namespace {

constexpr int B = kSiftNodeFramesMax;

// the layout of rgbdfe_ctx::sb for frames of `plane` pixels, R kept rows and A aggregate rows per frame
struct Layout {
  size_t d_agg, d_depth, d_keys, d_rec, d_nkeys, d_rows, d_map, d_n1, d_n, d_xyz, d_feat, d_raw, d_kept, dev_bytes;
  size_t h_agg, h_depth, h_keys, h_rec, h_map, h_n1, h_n, h_xyz, h_feat, h_raw, h_kept, pin_bytes;
  Layout(size_t plane, size_t R, size_t A) {
    Arena d, h;
    d_agg = d.carve(B * A * sizeof(rgbdfe_keypoint)); d_depth = d.carve(B * plane * 4); d_keys = d.carve(B * R * 16);
    d_rec = d.carve(B * R * sizeof(rgbdfe_keypoint)); d_nkeys = d.carve(B * R * 16); d_rows = d.carve(B * R * 512);
    d_map = d.carve(B * R * 4); d_n1 = d.carve(B * 4); d_n = d.carve(B * 4); d_xyz = d.carve(B * R * 16);
    d_feat = d.carve(B * R * 512); d_raw = d.carve(B * R * 512); d_kept = d.carve(B * R * 4);
    dev_bytes = d.size;
    h_agg = h.carve(B * A * sizeof(rgbdfe_keypoint)); h_depth = h.carve(B * plane * 4); h_keys = h.carve(B * R * 16);
    h_rec = h.carve(B * R * sizeof(rgbdfe_keypoint)); h_map = h.carve(B * R * 4); h_n1 = h.carve(B * 4); h_n = h.carve(B * 4);
    h_xyz = h.carve(B * R * 16); h_feat = h.carve(B * R * 512); h_raw = h.carve(B * R * 512); h_kept = h.carve(B * R * 4);
    pin_bytes = h.size;
  }
};

int prepare_bufs(rgbdfe_ctx* ctx, size_t plane, int R, int A) {
  rgbdfe_ctx::SiftBehindBufs& sb = ctx->sb;
  if (sb.dev && sb.plane == plane && sb.rows_per_frame == R && sb.agg_per_frame == A) return RGBDFE_OK;
  if (sb.dev) (void)hipFree(sb.dev);
  if (sb.pin) (void)hipHostFree(sb.pin);
  sb.dev = sb.pin = nullptr; sb.plane = 0;
  const Layout L(plane, (size_t)R, (size_t)A);
  if (hipMalloc(&sb.dev, L.dev_bytes) != hipSuccess || hipHostMalloc(&sb.pin, L.pin_bytes, hipHostMallocDefault) != hipSuccess)
    return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "SIFT-behind-detector buffers");
  sb.plane = plane; sb.rows_per_frame = R; sb.agg_per_frame = A;
  return RGBDFE_OK;
}

// where a call's outputs go (every pointer may be NULL); row f of the call starts at f * stride
struct Outputs {
  int32_t stride = 0;
  rgbdfe_keypoint* keypoints = nullptr; float* xyz1 = nullptr; float* raw = nullptr; float* feat = nullptr;
  int32_t* n_out = nullptr;
};

// the whole pipeline for n_frames frames; ctx->mu is held.  node_ids: NULL (no nodes) or one id per frame (slots reserved by
// the caller, slot_of[f] >= 0 for a frame with a node)
int run_frames(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask, const float* const* depth,
               int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, bool root,
               const int32_t* node_ids, const std::vector<int64_t>& slot_of, const Outputs& out) {
  ensure_detector(ctx);
  const int R = ctx->orb_max_keypoints, A = ctx->orb.max_total;
  const bool min_depth = ctx->feature_min_depth;
  const size_t plane = (size_t)rows * (size_t)cols, mk = (size_t)ctx->cfg.max_keypoints;
  int rc = prepare_bufs(ctx, plane, R, A);
  if (rc != RGBDFE_OK) return rc;
  rgbdfe_ctx::SiftBehindBufs& sb = ctx->sb;
  const Layout L(plane, (size_t)R, (size_t)A);
  void* D = sb.dev;
  void* P = sb.pin;
  hipStream_t st = ctx->stream;
  const bool host_out = out.keypoints || out.xyz1 || out.raw || out.feat;
  std::string err;
  for (int32_t f0 = 0; f0 < n_frames; f0 += B) {
    const int nf = std::min<int32_t>(B, n_frames - f0);
    // 1. detection, frame by frame
    for (int k = 0; k < nf; ++k) {
      std::vector<KpOut> kps;
      rc = detect_aggregate(ctx, gray[f0 + k], mask ? mask[f0 + k] : nullptr, rows, cols, kps);
      if (rc != RGBDFE_OK) return rc;
      if ((int)kps.size() > A) return fail(ctx, RGBDFE_ERR_INTERNAL, "aggregate larger than max_total");
      kp_to_abi(kps, at<rgbdfe_keypoint>(P, L.h_agg) + (size_t)k * A);
      at<int32_t>(P, L.h_n)[k] = (int32_t)kps.size();   // (staging of the aggregate counts)
      memcpy(at<float>(P, L.h_depth) + (size_t)k * plane, depth[f0 + k], plane * 4);
    }
    // 2. projectTo3D's kept keypoints and the wrapper's conversions, every frame in one launch
    SiftKeysChunk kc{};
    kc.n_frames = nf;
    kc.n_out = at<int32_t>(D, L.d_n1);
    for (int k = 0; k < nf; ++k) {
      SiftKeysFrame& o = kc.frame[k];
      o.agg = at<rgbdfe_keypoint>(D, L.d_agg) + (size_t)k * A;
      o.n_agg = at<int32_t>(P, L.h_n)[k];
      o.depth = at<float>(D, L.d_depth) + (size_t)k * plane;
      o.keys = at<float4>(D, L.d_keys) + (size_t)k * R;
      o.rebuilt = at<rgbdfe_keypoint>(D, L.d_rec) + (size_t)k * R;
      o.node_keys = at<float4>(D, L.d_nkeys) + (size_t)k * R;
    }
    HIP_TRY(ctx, hipMemcpyAsync(at<void>(D, L.d_agg), at<void>(P, L.h_agg), (size_t)nf * A * sizeof(rgbdfe_keypoint),
                                hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(at<void>(D, L.d_depth), at<void>(P, L.h_depth), (size_t)nf * plane * 4, hipMemcpyHostToDevice, st));
    launch_sift_keys_from_detector(kc, rows, cols, depth_scaling, R, min_depth, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_n1), at<void>(D, L.d_n1), (size_t)nf * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_keys), at<void>(D, L.d_keys), (size_t)nf * R * 16, hipMemcpyDeviceToHost, st));
    if (out.keypoints)
      HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_rec), at<void>(D, L.d_rec), (size_t)nf * R * sizeof(rgbdfe_keypoint),
                                  hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const int32_t* n1 = at<int32_t>(P, L.h_n1);
    // 3a. the wrapper's empty-list path: SiftGPU's own features (keys rebuilt as rgbdfe_sift_detect reports them)
    std::vector<std::vector<rgbdfe_keypoint>> qrec((size_t)nf);
    std::vector<size_t> qoff((size_t)nf, 0);
    std::vector<int> qn((size_t)nf, 0);
    {
      std::vector<std::vector<SiftKey>> qkeys((size_t)nf);
      std::vector<std::vector<float>> qdesc((size_t)nf);
      size_t qtot = 0;
      for (int k = 0; k < nf; ++k) {
        if (n1[k] > 0) continue;
        const float* d = nullptr;
        rc = ctx->sift.run(gray[f0 + k], rows, cols, R, qkeys[(size_t)k], d, st, err);
        if (rc != RGBDFE_OK) return fail(ctx, rc, err);
        const size_t n = qkeys[(size_t)k].size();
        qdesc[(size_t)k].assign(d, d + n * 128);
        qoff[(size_t)k] = qtot;
        qn[(size_t)k] = (int)n;
        qtot += n;
      }
      if (qtot > sb.q_cap) {
        if (sb.d_qdesc) (void)hipFree(sb.d_qdesc);
        if (sb.d_qkeys) (void)hipFree(sb.d_qkeys);
        sb.d_qdesc = nullptr; sb.d_qkeys = nullptr; sb.q_cap = 0;
        if (hipMalloc((void**)&sb.d_qdesc, qtot * 512) != hipSuccess || hipMalloc((void**)&sb.d_qkeys, qtot * 16) != hipSuccess)
          return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "SIFT features of empty-list frames");
        sb.q_cap = qtot;
      }
      std::vector<float4> k4;
      for (int k = 0; k < nf; ++k) {
        if (n1[k] > 0 || qn[(size_t)k] == 0) continue;
        const std::vector<SiftKey>& K = qkeys[(size_t)k];
        k4.resize(K.size());
        qrec[(size_t)k].resize(K.size());
        for (size_t i = 0; i < K.size(); ++i) {
          qrec[(size_t)k][i] = sift_key_to_keypoint(K[i]);
          k4[i] = make_float4(K[i].x, K[i].y, qrec[(size_t)k][i].size, 0.f);
        }
        HIP_TRY(ctx, hipMemcpyAsync(sb.d_qkeys + qoff[(size_t)k], k4.data(), K.size() * 16, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(sb.d_qdesc + qoff[(size_t)k] * 128, qdesc[(size_t)k].data(), K.size() * 512,
                                    hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));   // (the host vectors are reused)
      }
    }
    // 3b. the others: one pyramid chain and one descriptor launch, rows gathered into the callers' order
    std::vector<const uint8_t*> dg;
    std::vector<const SiftKey*> dk;
    std::vector<int> dn, slot_in_desc((size_t)nf, -1);
    for (int k = 0; k < nf; ++k) {
      if (n1[k] == 0) continue;
      slot_in_desc[(size_t)k] = (int)dg.size();
      dg.push_back(gray[f0 + k]);
      dk.push_back(reinterpret_cast<const SiftKey*>(at<float4>(P, L.h_keys) + (size_t)k * R));
      dn.push_back(n1[k]);
    }
    if (!dg.empty()) {
      rc = ctx->sift.describe_frames(dg.data(), (int)dg.size(), rows, cols, dk.data(), dn.data(), at<float>(D, L.d_rows),
                                     (size_t)R, at<int32_t>(D, L.d_map), at<int32_t>(P, L.h_map), st, err);
      if (rc != RGBDFE_OK) { (void)hipStreamSynchronize(st); return fail(ctx, rc, err); }
    }
    // 4. projectTo3DSiftGPU + RootSIFT into the nodes and the output rows
    auto node_launch = [&](bool root_sift, bool raw_rows) {
      SiftNodeChunk ch{};
      ch.n_frames = nf;
      ch.n_out = at<int32_t>(D, L.d_n);
      for (int k = 0; k < nf; ++k) {
        SiftNodeFrame& o = ch.frame[k];
        const int j = slot_in_desc[(size_t)k];
        if (j >= 0) {
          o.keys = at<float4>(D, L.d_nkeys) + (size_t)k * R;
          o.desc = reinterpret_cast<const float2*>(at<float>(D, L.d_rows) + (size_t)j * R * 128);
          o.n_keys = n1[k];
        } else if (qn[(size_t)k] > 0) {
          o.keys = sb.d_qkeys + qoff[(size_t)k];
          o.desc = reinterpret_cast<const float2*>(sb.d_qdesc + qoff[(size_t)k] * 128);
          o.n_keys = qn[(size_t)k];
        }
        o.depth = at<float>(D, L.d_depth) + (size_t)k * plane;
        const int32_t f = f0 + k;
        if (!raw_rows && node_ids && slot_of[(size_t)f] >= 0) {
          const size_t row0 = (size_t)slot_of[(size_t)f] * mk;
          o.xyz = ctx->d_xyz + row0;
          o.feat = reinterpret_cast<float2*>(ctx->d_sift_f32 + row0 * 128);
        }
        const size_t r0 = (size_t)k * R;
        if (raw_rows) {
          o.feat_out = reinterpret_cast<float2*>(at<float>(D, L.d_raw) + r0 * 128);
        } else {
          if (out.xyz1) o.xyz_out = at<float4>(D, L.d_xyz) + r0;
          if (out.feat) o.feat_out = reinterpret_cast<float2*>(at<float>(D, L.d_feat) + r0 * 128);
          if (out.keypoints) o.kept_out = at<int32_t>(D, L.d_kept) + r0;
        }
      }
      launch_sift_nodes(ch, rows, cols, (float)(1. / fx), (float)(1. / fy), (float)cx, (float)cy, depth_scaling, R, min_depth,
                        root_sift, st);
    };
    if (out.raw) node_launch(false, true);   // siftgpu_descriptors: the same rows without RootSIFT
    node_launch(root, false);
    HIP_TRY(ctx, hipGetLastError());
    const size_t nr = (size_t)nf * R;
    HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_n), at<void>(D, L.d_n), (size_t)nf * 4, hipMemcpyDeviceToHost, st));
    if (out.xyz1) HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_xyz), at<void>(D, L.d_xyz), nr * 16, hipMemcpyDeviceToHost, st));
    if (out.feat) HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_feat), at<void>(D, L.d_feat), nr * 512, hipMemcpyDeviceToHost, st));
    if (out.raw) HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_raw), at<void>(D, L.d_raw), nr * 512, hipMemcpyDeviceToHost, st));
    if (out.keypoints) HIP_TRY(ctx, hipMemcpyAsync(at<void>(P, L.h_kept), at<void>(D, L.d_kept), nr * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // 5. the node table and the caller's rows
    for (int k = 0; k < nf; ++k) {
      const int32_t f = f0 + k;
      const int32_t n = at<int32_t>(P, L.h_n)[k];
      out.n_out[f] = n;
      if (node_ids && node_ids[f] >= 0) ctx->nodes[node_ids[f]] = NodeEntry{(uint32_t)slot_of[(size_t)f], (uint32_t)n, 2u, 0u};
      if (!host_out || n == 0) continue;
      const size_t r0 = (size_t)k * R, o = (size_t)f * (size_t)out.stride;
      if (out.keypoints) {
        const int32_t* kept = at<int32_t>(P, L.h_kept) + r0;
        const rgbdfe_keypoint* rec = n1[k] > 0 ? at<rgbdfe_keypoint>(P, L.h_rec) + r0 : qrec[(size_t)k].data();
        for (int32_t i = 0; i < n; ++i) out.keypoints[o + i] = rec[kept[i]];
      }
      if (out.xyz1) memcpy(out.xyz1 + o * 4, at<float4>(P, L.h_xyz) + r0, (size_t)n * 16);
      if (out.feat) memcpy(out.feat + o * 128, at<float>(P, L.h_feat) + r0 * 128, (size_t)n * 512);
      if (out.raw) memcpy(out.raw + o * 128, at<float>(P, L.h_raw) + r0 * 128, (size_t)n * 512);
    }
  }
  return RGBDFE_OK;
}

}  // namespace

void sift_behind_release(rgbdfe_ctx* ctx) {
  rgbdfe_ctx::SiftBehindBufs& sb = ctx->sb;
  if (sb.dev) (void)hipFree(sb.dev);
  if (sb.pin) (void)hipHostFree(sb.pin);
  if (sb.d_qdesc) (void)hipFree(sb.d_qdesc);
  if (sb.d_qkeys) (void)hipFree(sb.d_qkeys);
  sb = rgbdfe_ctx::SiftBehindBufs{};
}

// Node::Node for feature_detector_type ORB / FAST and feature_extractor_type SIFTGPU (node.cpp:160, 165-176), one frame:
// detector->detect, projectTo3D (:900-965), SiftGPUWrapper::detect with the kept list (sift_gpu_wrapper.cpp:132-165) -- or with
// an EMPTY list when projectTo3D kept nothing: the wrapper skips SetKeypointList (:133) and SiftGPU detects on its own
// (SiftPyramid.cpp:154-156 clears any earlier list) -- then projectTo3DSiftGPU (+ RootSIFT) (:175, 695-769, 1557-1571).
// The same bits as rgbdfe_detect -> rgbdfe_project_to_3d(_min_depth) -> rgbdfe_sift_describe (or rgbdfe_sift_detect) ->
// rgbdfe_sift_node_features(_min_depth).  Outputs hold the detector's max_keypoints rows; feature_descriptors may be NULL.
int rgbdfe_detect_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth, int32_t rows,
                                int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling,
                                int32_t use_root_sift, rgbdfe_keypoint* keypoints, float* xyz1, float* siftgpu_descriptors,
                                float* feature_descriptors, int32_t* n_out) {
  if (!ctx || !gray || !depth || rows < 1 || cols < 1 || !keypoints || !xyz1 || !siftgpu_descriptors || !n_out)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  *n_out = 0;
  Outputs out;
  out.stride = 0; out.keypoints = keypoints; out.xyz1 = xyz1; out.raw = siftgpu_descriptors; out.feat = feature_descriptors;
  out.n_out = n_out;
  const uint8_t* m[1] = {mask};
  return run_frames(ctx, 1, &gray, m, &depth, rows, cols, fx, fy, cx, cy, depth_scaling, use_root_sift != 0, nullptr, {}, out);
}

// A run of frames through the same detector state: the results of n_frames calls of rgbdfe_detect_sift_describe, frame f's
// features becoming the float node node_ids[f] (rgbdfe_upload_float_node(id, feature_descriptors, 128, xyz1, n)).  The node
// table follows rgbdfe_sift_detect_batch_nodes: free slots are checked and reserved for the whole batch before any work (every
// fresh id takes one; a frame without features becomes an empty node), an existing id is rewritten in place after the pair
// lanes that may read it have finished.
int rgbdfe_detect_sift_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                            const uint8_t* const* mask, const float* const* depth, int32_t rows, int32_t cols,
                                            double fx, double fy, double cx, double cy, double depth_scaling,
                                            int32_t use_root_sift, const int32_t* node_ids, int32_t out_stride,
                                            rgbdfe_keypoint* keypoints, float* xyz1, float* feature_descriptors, int32_t* n_out) {
  if (!ctx || n_frames < 0 || rows < 1 || cols < 1 || (n_frames > 0 && (!gray || !depth || !node_ids || !n_out)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (!frames_non_null(n_frames, gray, depth)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "null frame");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  ensure_detector(ctx);
  const int32_t R = ctx->orb_max_keypoints;
  if (n_frames > 0 && out_stride < R) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "out_stride below the detector's max_keypoints");
  if (R > ctx->cfg.max_keypoints)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "the detector's max_keypoints exceeds the context's max_keypoints (node rows)");
  for (int32_t f = 0; f < n_frames; ++f) n_out[f] = 0;
  if (n_frames == 0) return RGBDFE_OK;
  int rc = ensure_sift(ctx);
  std::vector<int64_t> slot_of;   // all-or-nothing; fresh ids are registered (as empty float nodes) before any work
  if (rc == RGBDFE_OK) rc = reserve_node_slots(ctx, n_frames, node_ids, 2u, &slot_of);
  if (rc != RGBDFE_OK) return rc;
  Outputs out;
  out.stride = out_stride; out.keypoints = keypoints; out.xyz1 = xyz1; out.feat = feature_descriptors; out.n_out = n_out;
  return run_frames(ctx, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy, depth_scaling, use_root_sift != 0, node_ids,
                    slot_of, out);
}

int detector_max_keypoints(rgbdfe_ctx* ctx) {
  std::lock_guard<std::mutex> g(ctx->mu);
  ensure_detector(ctx);
  return ctx->orb_max_keypoints;
}

}  // namespace impl
