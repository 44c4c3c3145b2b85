// rgbdfe_api.hip -- the extern "C" layer of include/rgbdfe.h: every entry point behind an exception barrier, dispatched to the
// single-device implementation (namespace impl) or to the multi-device group.  There is no CPU fallback: without a HIP device
// every entry point reports RGBDFE_ERR_NO_DEVICE.
#include "rgbdfe_host.h"
#include "session_format.h"

extern "C" {

void rgbdfe_default_config(rgbdfe_config* cfg) { impl::rgbdfe_default_config(cfg); }

int rgbdfe_create(const rgbdfe_config* cfg, rgbdfe_ctx** out) {
  return guarded(nullptr, [&]() -> int { return impl::rgbdfe_create(cfg, out); });
}

int rgbdfe_create_multi(const rgbdfe_config* cfg, const int32_t* device_ids, int32_t n_devices, rgbdfe_ctx** out) {
  return guarded(nullptr, [&]() -> int { return group_create(cfg, device_ids, n_devices, out); });
}

void rgbdfe_destroy(rgbdfe_ctx* ctx) {
  if (!ctx) return;
  try {
    if (ctx->group) group_destroy(ctx);
    else impl::rgbdfe_destroy(ctx);
  } catch (...) {
  }
}

int rgbdfe_device_count(rgbdfe_ctx* ctx) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return ctx->group ? (int)ctx->group->children.size() : 1;
}

rgbdfe_ctx* rgbdfe_device_context(rgbdfe_ctx* ctx, int32_t i) {
  if (!ctx) return nullptr;
  if (!ctx->group) return i == 0 ? ctx : nullptr;
  return i >= 0 && (size_t)i < ctx->group->children.size() ? ctx->group->children[(size_t)i] : nullptr;
}

int rgbdfe_group_submit_us(rgbdfe_ctx* ctx, double* us) {
  if (!ctx || !us) return RGBDFE_ERR_INVALID_ARG;
  *us = 0.0;
  if (ctx->group) {
    std::lock_guard<std::recursive_mutex> call_lock(ctx->group->mu);
    *us = ctx->group->last_submit_us;
  }
  return RGBDFE_OK;
}

const char* rgbdfe_gather_transport(rgbdfe_ctx* ctx) {
  static thread_local std::string buf;
  if (ctx && ctx->group) {
    std::lock_guard<std::recursive_mutex> call_lock(ctx->group->mu);
    buf = ctx->group->transport;
  } else buf = "none";
  return buf.c_str();
}

int rgbdfe_gather_exchanges(rgbdfe_ctx* ctx) {
  if (!ctx || !ctx->group) return 0;
  std::lock_guard<std::recursive_mutex> call_lock(ctx->group->mu);
  return ctx->group->inl_exchanges;
}

int rgbdfe_set_params(rgbdfe_ctx* ctx, const rgbdfe_params* p) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (RGBDFE_IS_GROUP(ctx) && p) {
    std::lock_guard<std::recursive_mutex> call_lock(ctx->group->mu);
    ctx->cfg.params = *p;
    return RGBDFE_ALL(ctx, impl::rgbdfe_set_params(c, p));
  }
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_params(c, p));
}

const char* rgbdfe_status_string(int status) { return impl::rgbdfe_status_string(status); }

// a copy per calling thread: the context's string may be rewritten by another thread at any time
const char* rgbdfe_last_error(rgbdfe_ctx* ctx) {
  static thread_local std::string buf;
  try {
    buf.clear();
    if (ctx) {
      std::lock_guard<std::mutex> g(ctx->err_mu);
      buf = ctx->last_error;
    } else {
      buf = rgbdfe_session::contextless_error();   // pose-graph / slam byte strings: calls without a context
    }
    return buf.c_str();
  } catch (...) {
    return "";
  }
}

int rgbdfe_upload_node(rgbdfe_ctx* ctx, int32_t node_id, const uint8_t* desc, const float* xyz1, int32_t n) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_upload_node(c, node_id, desc, xyz1, n));
}

int rgbdfe_upload_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const uint8_t* const* desc,
                        const float* const* xyz1, const int32_t* counts) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_upload_nodes(c, n_nodes, node_ids, desc, xyz1, counts));
}

int rgbdfe_upload_node_device(rgbdfe_ctx* ctx, int32_t node_id, const void* d_desc, const void* d_xyz1, int32_t n,
                              void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_upload_node_device");
    return impl::rgbdfe_upload_node_device(ctx, node_id, d_desc, d_xyz1, n, stream);
  });
}

int rgbdfe_upload_node_keypoints(rgbdfe_ctx* ctx, int32_t node_id, const float* kp_xy, int32_t n) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_upload_node_keypoints(c, node_id, kp_xy, n));
}

int rgbdfe_release_node(rgbdfe_ctx* ctx, int32_t node_id) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_release_node(c, node_id));
}

int rgbdfe_node_count(rgbdfe_ctx* ctx, int32_t node_id) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    return impl::rgbdfe_node_count(RGBDFE_IS_GROUP(ctx) ? ctx->group->children[0] : ctx, node_id);
  });
}

int rgbdfe_match_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                           rgbdfe_match_result* out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_match(ctx, query_ids, train_ids, n_pairs, out, false, nullptr);
    return impl::rgbdfe_match_pair_list(ctx, query_ids, train_ids, n_pairs, out);
  });
}

int rgbdfe_match_node_pairs(rgbdfe_ctx* ctx, int32_t new_node_id, const int32_t* candidate_ids, int32_t n_pairs,
                            rgbdfe_match_result* out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (n_pairs < 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad match arguments");
    std::vector<int32_t> q((size_t)n_pairs, new_node_id);
    if (RGBDFE_IS_GROUP(ctx)) return group_match(ctx, q.data(), candidate_ids, n_pairs, out, false, nullptr);
    return impl::rgbdfe_match_pair_list(ctx, q.data(), candidate_ids, n_pairs, out);
  });
}

int rgbdfe_match_pair_list_allgather(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                     int32_t n_pairs, void* const* d_out, int32_t* records_per_device) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!RGBDFE_IS_GROUP(ctx))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "rgbdfe_match_pair_list_allgather needs a context made by rgbdfe_create_multi");
    return group_match_allgather(ctx, query_ids, train_ids, n_pairs, d_out, records_per_device);
  });
}

int rgbdfe_match_pair_list_allgather_compact(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                             int32_t n_pairs, void* const* d_out, int32_t* records_per_device) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!RGBDFE_IS_GROUP(ctx))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "rgbdfe_match_pair_list_allgather_compact needs a context made by rgbdfe_create_multi");
    return group_match_allgather(ctx, query_ids, train_ids, n_pairs, d_out, records_per_device, true);
  });
}

int rgbdfe_pack_compact(rgbdfe_ctx* ctx, const void* d_records, int32_t n, void* d_compact, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_pack_compact");
    return impl::rgbdfe_pack_compact(ctx, d_records, n, d_compact, stream);
  });
}

int rgbdfe_set_graph_capture(rgbdfe_ctx* ctx, int enable) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_graph_capture(c, enable));
}

int rgbdfe_pack_inliers(rgbdfe_ctx* ctx, const void* d_records, int32_t n, int32_t n_headers, void* d_stream, int32_t* d_total,
                        void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_pack_inliers");
    return impl::rgbdfe_pack_inliers(ctx, d_records, n, n_headers, d_stream, d_total, stream);
  });
}
int rgbdfe_sizeof_inlier_header(void) { return impl::rgbdfe_sizeof_inlier_header(); }

int rgbdfe_match_pair_list_allgather_edges(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                           int32_t n_pairs, void* const* d_out, int32_t* const* d_index,
                                           int32_t* edges_per_device, int32_t* stride) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!RGBDFE_IS_GROUP(ctx))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG,
                  "rgbdfe_match_pair_list_allgather_edges needs a context made by rgbdfe_create_multi");
    return group_match_allgather_edges(ctx, query_ids, train_ids, n_pairs, d_out, d_index, edges_per_device, stride);
  });
}

int rgbdfe_match_pair_list_allgather_inliers(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                             int32_t n_pairs, void* const* d_out, int32_t* records_per_device,
                                             int32_t* list_entries, int64_t* stride_bytes) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!RGBDFE_IS_GROUP(ctx))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG,
                  "rgbdfe_match_pair_list_allgather_inliers needs a context made by rgbdfe_create_multi");
    return group_match_allgather_inliers(ctx, query_ids, train_ids, n_pairs, d_out, records_per_device, list_entries, stride_bytes);
  });
}

int rgbdfe_submit_pair_list_host(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                                 void* out, size_t out_bytes, int payload, int64_t* ticket) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_submit_pair_list_host");
    return impl::rgbdfe_submit_pair_list_host(ctx, query_ids, train_ids, n_pairs, out, out_bytes, payload, ticket);
  });
}
int rgbdfe_wait_host(rgbdfe_ctx* ctx, int64_t ticket, int64_t* bytes_written) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_wait_host");
    return impl::rgbdfe_wait_host(ctx, ticket, bytes_written);
  });
}

int rgbdfe_wait_host_into(rgbdfe_ctx* ctx, int64_t ticket, void* out, size_t out_bytes, int64_t* bytes_written) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_wait_host_into");
    return impl::rgbdfe_wait_host_into(ctx, ticket, out, out_bytes, bytes_written);
  });
}

int rgbdfe_match_pair_list_device(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                                  void* d_out, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_match_pair_list_device");
    return impl::rgbdfe_match_pair_list_device(ctx, query_ids, train_ids, n_pairs, d_out, stream);
  });
}

int rgbdfe_submit_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                            void* d_out, int64_t* ticket) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_submit_pair_list");
    return impl::rgbdfe_submit_pair_list(ctx, query_ids, train_ids, n_pairs, d_out, ticket);
  });
}

int rgbdfe_wait_ticket(rgbdfe_ctx* ctx, int64_t ticket, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_wait_ticket");
    return impl::rgbdfe_wait_ticket(ctx, ticket, stream);
  });
}

int rgbdfe_synchronize(rgbdfe_ctx* ctx) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_synchronize(c));
}

int rgbdfe_upload_sift_node(rgbdfe_ctx* ctx, int32_t node_id, const float* desc128, const float* xyz1, int32_t n) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_upload_sift_node(c, node_id, desc128, xyz1, n));
}

int rgbdfe_match_sift_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                                rgbdfe_match_result* out, float* out_dist) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_match(ctx, query_ids, train_ids, n_pairs, out, true, out_dist);
    return impl::rgbdfe_match_sift_pair_list(ctx, query_ids, train_ids, n_pairs, out, out_dist);
  });
}

int rgbdfe_upload_float_node(rgbdfe_ctx* ctx, int32_t node_id, const float* desc, int32_t dim, const float* xyz1,
                             int32_t n) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_upload_float_node(c, node_id, desc, dim, xyz1, n));
}

int rgbdfe_match_flann_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                                 double nn_distance_ratio, rgbdfe_match_result* out, float* out_dist) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!(nn_distance_ratio > 0.0)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "nn_distance_ratio must be > 0");
    if (RGBDFE_IS_GROUP(ctx)) {
      if (n_pairs < 0 || (n_pairs > 0 && (!query_ids || !train_ids || !out)))
        return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad match arguments");
      Group& g = *ctx->group;
      const int G = (int)g.children.size();
      return group_run(ctx, [&](int i) -> int {
        std::vector<int32_t> qs, ts;
        for (int32_t k = i; k < n_pairs; k += G) { qs.push_back(query_ids[k]); ts.push_back(train_ids[k]); }
        if (qs.empty()) return RGBDFE_OK;
        return impl::rgbdfe_match_sift_pair_list(g.children[(size_t)i], qs.data(), ts.data(), (int32_t)qs.size(), out + i,
                                                 out_dist ? out_dist + (size_t)i * RGBDFE_MAX_MATCHES : nullptr, G, 2,
                                                 nn_distance_ratio);
      });
    }
    return impl::rgbdfe_match_sift_pair_list(ctx, query_ids, train_ids, n_pairs, out, out_dist, 1, 2, nn_distance_ratio);
  });
}

int rgbdfe_submit_sift_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                                 void* d_out, void* d_out_dist, int64_t* ticket) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_submit_sift_pair_list");
    return impl::rgbdfe_submit_sift_pair_list(ctx, query_ids, train_ids, n_pairs, d_out, d_out_dist, ticket);
  });
}

int rgbdfe_sift_match_nodes(rgbdfe_ctx* ctx, int32_t query_id, int32_t train_id, int32_t* match_q, int32_t* match_t,
                            float* match_dist, int32_t* n_matches) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_match_nodes(c, query_id, train_id, match_q, match_t, match_dist, n_matches));
}

int rgbdfe_detector_configure(rgbdfe_ctx* ctx, int32_t max_keypoints, int32_t grid_resolution,
                              int32_t adjuster_max_iterations) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detector_configure(c, max_keypoints, grid_resolution, adjuster_max_iterations));
}

int rgbdfe_set_detector_type(rgbdfe_ctx* ctx, int32_t type) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_set_detector_type(c, type));
}

int rgbdfe_fast_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols, int32_t threshold,
                       rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_fast_detect(c, gray, mask, rows, cols, threshold, keypoints, capacity, n_out));
}

int rgbdfe_detector_thresholds(rgbdfe_ctx* ctx, double* thresholds, int32_t* n_cells) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detector_thresholds(c, thresholds, n_cells));
}

int rgbdfe_orb_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                      int32_t fast_threshold, rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_orb_detect(c, gray, mask, rows, cols, fast_threshold, keypoints, capacity, n_out));
}

int rgbdfe_orb_compute(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols, rgbdfe_keypoint* keypoints,
                       int32_t n, uint8_t* descriptors, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_orb_compute(c, gray, rows, cols, keypoints, n, descriptors, n_out));
}

int rgbdfe_detect_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth, int32_t rows,
                           int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling,
                           rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detect_describe(c, gray, mask, depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                                        keypoints, descriptors, xyz1, n_out));
}

int rgbdfe_set_feature_min_depth(rgbdfe_ctx* ctx, int32_t on) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_feature_min_depth(c, on));
}

int rgbdfe_project_to_3d_min_depth(rgbdfe_ctx* ctx, const float* kp_xy, const float* kp_size, int32_t n_kp,
                                   const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                   double cy, double depth_scaling, int32_t max_keypoints, int32_t* kept_idx,
                                   float* xyz1, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_project_to_3d_min_depth(c, kp_xy, kp_size, n_kp, depth, rows, cols, fx, fy, cx, cy,
                                                                depth_scaling, max_keypoints, kept_idx, xyz1, n_out));
}

int rgbdfe_detect_describe_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                                 const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                 double cy, double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                 uint8_t* descriptors, float* xyz1, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detect_describe_batch(c, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy,
                                                              depth_scaling, out_stride, keypoints, descriptors, xyz1,
                                                              n_out));
}

int rgbdfe_detect_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                                       const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                       double cy, double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                       uint8_t* descriptors, float* xyz1, int32_t* n_out, const int32_t* node_ids) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (!node_ids) return guarded(ctx, [&]() -> int { return fail(ctx, RGBDFE_ERR_INVALID_ARG, "node_ids is required"); });
  if (!RGBDFE_IS_GROUP(ctx))
    return RGBDFE_FIRST(ctx, impl::rgbdfe_detect_describe_batch(c, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy,
                                                                depth_scaling, out_stride, keypoints, descriptors, xyz1, n_out,
                                                                node_ids));
  // several devices behind the handle: the frames are processed on the first one, the nodes go to all of them from the host
  // outputs (every device holds every node).  FAST takes NULL host outputs: the rows then pass through arrays of this call.
  std::vector<rgbdfe_keypoint> kp_tmp;
  std::vector<uint8_t> desc_tmp;
  std::vector<float> xyz_tmp;
  if (n_frames > 0 && out_stride > 0 && rgbdfe_device_context(ctx, 0)->detector_type == RGBDFE_DETECTOR_FAST &&
      (!keypoints || !descriptors || !xyz1)) {
    const size_t rows_all = (size_t)n_frames * (size_t)out_stride;
    if (!keypoints) { kp_tmp.resize(rows_all); keypoints = kp_tmp.data(); }
    if (!descriptors) { desc_tmp.resize(rows_all * 32); descriptors = desc_tmp.data(); }
    if (!xyz1) { xyz_tmp.resize(rows_all * 4); xyz1 = xyz_tmp.data(); }
  }
  int rc = RGBDFE_FIRST(ctx, impl::rgbdfe_detect_describe_batch(c, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy,
                                                                depth_scaling, out_stride, keypoints, descriptors, xyz1, n_out));
  if (rc != RGBDFE_OK) return rc;
  std::vector<int32_t> ids, cnt;
  std::vector<const uint8_t*> dp;
  std::vector<const float*> xp;
  for (int32_t f = 0; f < n_frames; ++f)
    if (node_ids[f] >= 0) {
      ids.push_back(node_ids[f]); cnt.push_back(n_out[f]);
      dp.push_back(descriptors + (size_t)f * out_stride * 32); xp.push_back(xyz1 + (size_t)f * out_stride * 4);
    }
  return RGBDFE_ALL(ctx, impl::rgbdfe_upload_nodes(c, (int32_t)ids.size(), ids.data(), dp.data(), xp.data(), cnt.data()));
}

// ---- sensor frames (api_sensor.hip)
int rgbdfe_sizeof_sensor_frame(void) { return (int)sizeof(rgbdfe_sensor_frame); }

int rgbdfe_ingest_frame(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, uint8_t* gray, uint8_t* mono8, float* depth_m) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_ingest_frame(c, frame, gray, mono8, depth_m));
}

int rgbdfe_sensor_detect_describe(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, double fx, double fy, double cx, double cy,
                                  double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1,
                                  int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sensor_detect_describe(c, frame, fx, fy, cx, cy, depth_scaling, keypoints, descriptors,
                                                               xyz1, n_out));
}

int rgbdfe_sensor_detect_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, double fx,
                                              double fy, double cx, double cy, double depth_scaling, int32_t out_stride,
                                              rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out,
                                              const int32_t* node_ids, const rgbdfe_sensor_cloud* cloud) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  // everything about the frames and the cloud request that can be refused, before any detector state changes
  int rc = guarded(ctx, [&]() -> int {
    SensorRun run;
    return impl::sensor_batch_validate(ctx, n_frames, frames, node_ids, cloud, run);
  });
  if (rc != RGBDFE_OK) return rc;
  if (!RGBDFE_IS_GROUP(ctx)) {
    rc = RGBDFE_FIRST(ctx, impl::rgbdfe_sensor_detect_describe_batch(c, n_frames, frames, fx, fy, cx, cy, depth_scaling, out_stride,
                                                                     keypoints, descriptors, xyz1, n_out, node_ids));
  } else {
    // several devices behind the handle, as rgbdfe_detect_describe_batch_nodes: the frames are processed on the first one,
    // the nodes go to all of them from the host outputs
    std::vector<rgbdfe_keypoint> kp_tmp;
    std::vector<uint8_t> desc_tmp;
    std::vector<float> xyz_tmp;
    if (node_ids && n_frames > 0 && out_stride > 0 && rgbdfe_device_context(ctx, 0)->detector_type == RGBDFE_DETECTOR_FAST &&
        (!keypoints || !descriptors || !xyz1)) {
      const size_t rows_all = (size_t)n_frames * (size_t)out_stride;
      if (!keypoints) { kp_tmp.resize(rows_all); keypoints = kp_tmp.data(); }
      if (!descriptors) { desc_tmp.resize(rows_all * 32); descriptors = desc_tmp.data(); }
      if (!xyz1) { xyz_tmp.resize(rows_all * 4); xyz1 = xyz_tmp.data(); }
    }
    rc = RGBDFE_FIRST(ctx, impl::rgbdfe_sensor_detect_describe_batch(c, n_frames, frames, fx, fy, cx, cy, depth_scaling, out_stride,
                                                                     keypoints, descriptors, xyz1, n_out, nullptr));
    if (rc == RGBDFE_OK && node_ids) {
      std::vector<int32_t> ids, cnt;
      std::vector<const uint8_t*> dp;
      std::vector<const float*> xp;
      for (int32_t f = 0; f < n_frames; ++f)
        if (node_ids[f] >= 0) {
          ids.push_back(node_ids[f]); cnt.push_back(n_out[f]);
          dp.push_back(descriptors + (size_t)f * out_stride * 32); xp.push_back(xyz1 + (size_t)f * out_stride * 4);
        }
      rc = RGBDFE_ALL(ctx, impl::rgbdfe_upload_nodes(c, (int32_t)ids.size(), ids.data(), dp.data(), xp.data(), cnt.data()));
    }
  }
  if (rc != RGBDFE_OK || !cloud) return rc;
  return RGBDFE_ALL(ctx, impl::rgbdfe_sensor_clouds(c, n_frames, frames, fx, fy, cx, cy, depth_scaling, node_ids, cloud));
}

int rgbdfe_sift_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                       int32_t max_keypoints, rgbdfe_keypoint* keypoints, float* desc128, int32_t capacity, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_detect(c, gray, mask, rows, cols, max_keypoints, keypoints, desc128, capacity,
                                                    n_out));
}

int rgbdfe_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols, rgbdfe_keypoint* keypoints, int32_t n,
                         float* desc128) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_describe(c, gray, rows, cols, keypoints, n, desc128));
}

int rgbdfe_sift_detect_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, int32_t rows, int32_t cols,
                             int32_t max_keypoints, int32_t out_stride, rgbdfe_keypoint* keypoints, float* desc128,
                             int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_detect_batch(c, n_frames, gray, rows, cols, max_keypoints, out_stride, keypoints,
                                                          desc128, n_out));
}

int rgbdfe_sift_detect_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const float* const* depth,
                                   int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling,
                                   int32_t max_keypoints, int32_t use_root_sift, const int32_t* node_ids, int32_t out_stride,
                                   rgbdfe_keypoint* keypoints, float* xyz1, float* feature_descriptors, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (!node_ids && n_frames > 0)
    return guarded(ctx, [&]() -> int { return fail(ctx, RGBDFE_ERR_INVALID_ARG, "node_ids is required"); });
  if (!RGBDFE_IS_GROUP(ctx))
    return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_detect_batch_nodes(c, n_frames, gray, depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                                                  max_keypoints, use_root_sift, node_ids, out_stride, keypoints,
                                                                  xyz1, feature_descriptors, n_out));
  // several devices behind the handle: the frames are processed on the first one, into its nodes and into host rows of
  // max_keypoints per frame (a frame keeps no more); the other devices get the nodes from those rows (every device holds
  // every node), the caller's arrays get them at out_stride
  if (n_frames < 0 || out_stride < 0 || max_keypoints < 1)
    return guarded(ctx, [&]() -> int { return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments"); });
  const size_t mk = (size_t)max_keypoints, nf = (size_t)n_frames;
  std::vector<rgbdfe_keypoint> kp(keypoints ? nf * mk : 0);
  std::vector<float> xyz(nf * mk * 4), feat(nf * mk * 128);
  int rc = RGBDFE_FIRST(ctx, impl::rgbdfe_sift_detect_batch_nodes(c, n_frames, gray, depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                                                  max_keypoints, use_root_sift, node_ids, max_keypoints,
                                                                  keypoints ? kp.data() : nullptr, xyz.data(), feat.data(), n_out));
  if (rc != RGBDFE_OK) return rc;
  rc = guarded(ctx, [&]() -> int {
    return group_run(ctx, [&](int i) -> int {
      if (i == 0) return RGBDFE_OK;
      rgbdfe_ctx* c = ctx->group->children[(size_t)i];
      for (size_t f = 0; f < nf; ++f) {
        if (node_ids[f] < 0) continue;
        const int r = impl::rgbdfe_upload_float_node(c, node_ids[f], feat.data() + f * mk * 128, 128, xyz.data() + f * mk * 4, n_out[f]);
        if (r != RGBDFE_OK) return r;
      }
      return RGBDFE_OK;
    });
  });
  if (rc != RGBDFE_OK) return rc;
  bool overflow = false;
  for (size_t f = 0; f < nf; ++f) {
    const size_t n = (size_t)n_out[f];
    if (!(keypoints || xyz1 || feature_descriptors)) break;
    if (n > (size_t)out_stride) { overflow = true; continue; }
    if (keypoints && n) memcpy(keypoints + f * out_stride, kp.data() + f * mk, n * sizeof(rgbdfe_keypoint));
    if (xyz1 && n) memcpy(xyz1 + f * out_stride * 4, xyz.data() + f * mk * 4, n * 16);
    if (feature_descriptors && n) memcpy(feature_descriptors + f * out_stride * 128, feat.data() + f * mk * 128, n * 512);
  }
  if (overflow)
    return guarded(ctx, [&]() -> int { return fail(ctx, RGBDFE_ERR_CAPACITY, "more kept SIFT features in a frame than out_stride rows"); });
  return RGBDFE_OK;
}

int rgbdfe_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                  rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detect(c, gray, mask, rows, cols, keypoints, capacity, n_out));
}

int rgbdfe_detect_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth, int32_t rows,
                                int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling,
                                int32_t use_root_sift, rgbdfe_keypoint* keypoints, float* xyz1, float* siftgpu_descriptors,
                                float* feature_descriptors, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detect_sift_describe(c, gray, mask, depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                                             use_root_sift, keypoints, xyz1, siftgpu_descriptors,
                                                             feature_descriptors, n_out));
}

int rgbdfe_detect_sift_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                            const uint8_t* const* mask, const float* const* depth, int32_t rows, int32_t cols,
                                            double fx, double fy, double cx, double cy, double depth_scaling,
                                            int32_t use_root_sift, const int32_t* node_ids, int32_t out_stride,
                                            rgbdfe_keypoint* keypoints, float* xyz1, float* feature_descriptors, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (!RGBDFE_IS_GROUP(ctx))
    return RGBDFE_FIRST(ctx, impl::rgbdfe_detect_sift_describe_batch_nodes(c, n_frames, gray, mask, depth, rows, cols, fx, fy, cx,
                                                                           cy, depth_scaling, use_root_sift, node_ids, out_stride,
                                                                           keypoints, xyz1, feature_descriptors, n_out));
  // several devices behind the handle: the frames are processed on the first one, into its nodes and into host rows of the
  // detector's max_keypoints per frame (a frame keeps no more); the other devices get the nodes from those rows (every device
  // holds every node), the caller's arrays get them at out_stride
  if (n_frames < 0 || (n_frames > 0 && (!node_ids || !n_out)))
    return guarded(ctx, [&]() -> int { return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments"); });
  int R = 0;
  int rc = guarded(ctx, [&]() -> int { R = impl::detector_max_keypoints(ctx->group->children[0]); return RGBDFE_OK; });
  if (rc != RGBDFE_OK) return rc;
  if (n_frames > 0 && out_stride < R)
    return guarded(ctx, [&]() -> int { return fail(ctx, RGBDFE_ERR_INVALID_ARG, "out_stride below the detector's max_keypoints"); });
  const size_t mk = (size_t)R, nf = (size_t)n_frames;
  std::vector<rgbdfe_keypoint> kp(keypoints ? nf * mk : 0);
  std::vector<float> xyz(nf * mk * 4), feat(nf * mk * 128);
  rc = RGBDFE_FIRST(ctx, impl::rgbdfe_detect_sift_describe_batch_nodes(c, n_frames, gray, mask, depth, rows, cols, fx, fy, cx, cy,
                                                                      depth_scaling, use_root_sift, node_ids, R,
                                                                      keypoints ? kp.data() : nullptr, xyz.data(), feat.data(),
                                                                      n_out));
  if (rc != RGBDFE_OK) return rc;
  rc = guarded(ctx, [&]() -> int {
    return group_run(ctx, [&](int i) -> int {
      if (i == 0) return RGBDFE_OK;
      rgbdfe_ctx* c = ctx->group->children[(size_t)i];
      for (size_t f = 0; f < nf; ++f) {
        if (node_ids[f] < 0) continue;
        const int r = impl::rgbdfe_upload_float_node(c, node_ids[f], feat.data() + f * mk * 128, 128, xyz.data() + f * mk * 4, n_out[f]);
        if (r != RGBDFE_OK) return r;
      }
      return RGBDFE_OK;
    });
  });
  if (rc != RGBDFE_OK) return rc;
  for (size_t f = 0; f < nf; ++f) {
    const size_t n = (size_t)n_out[f], o = f * (size_t)out_stride;
    if (keypoints && n) memcpy(keypoints + o, kp.data() + f * mk, n * sizeof(rgbdfe_keypoint));
    if (xyz1 && n) memcpy(xyz1 + o * 4, xyz.data() + f * mk * 4, n * 16);
    if (feature_descriptors && n) memcpy(feature_descriptors + o * 128, feat.data() + f * mk * 128, n * 512);
  }
  return RGBDFE_OK;
}

int rgbdfe_sift_detect_orb_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const float* depth, int32_t rows, int32_t cols, double fx,
                                    double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                    rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_detect_orb_describe(c, gray, depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                                                 max_keypoints, keypoints, descriptors, xyz1, n_out));
}

int rgbdfe_sift_detect_orb_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                                const float* const* depth, int32_t rows, int32_t cols, double fx, double fy,
                                                double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                                const int32_t* node_ids, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                                uint8_t* descriptors, float* xyz1, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (!RGBDFE_IS_GROUP(ctx))
    return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_detect_orb_describe_batch_nodes(c, n_frames, gray, depth, rows, cols, fx, fy, cx, cy,
                                                                               depth_scaling, max_keypoints, node_ids, out_stride,
                                                                               keypoints, descriptors, xyz1, n_out));
  // several devices behind the handle: the frames are processed on the first one, into its nodes and into host rows of
  // max_keypoints per frame (a frame keeps no more); the other devices get the nodes from those rows (every device holds
  // every node), the caller's arrays get them at out_stride
  if (n_frames < 0 || out_stride < 0 || max_keypoints < 1 || (n_frames > 0 && (!node_ids || !n_out)))
    return guarded(ctx, [&]() -> int { return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments"); });
  if (n_frames > 0 && (keypoints || descriptors || xyz1) && out_stride < max_keypoints)
    return guarded(ctx, [&]() -> int {
      return fail(ctx, RGBDFE_ERR_CAPACITY, "out_stride below max_keypoints while a host output is asked for");
    });
  const size_t mk = (size_t)max_keypoints, nf = (size_t)n_frames;
  std::vector<rgbdfe_keypoint> kp(keypoints ? nf * mk : 0);
  std::vector<uint8_t> desc(nf * mk * 32);
  std::vector<float> xyz(nf * mk * 4);
  int rc = RGBDFE_FIRST(ctx, impl::rgbdfe_sift_detect_orb_describe_batch_nodes(c, n_frames, gray, depth, rows, cols, fx, fy, cx, cy,
                                                                               depth_scaling, max_keypoints, node_ids, max_keypoints,
                                                                               keypoints ? kp.data() : nullptr, desc.data(),
                                                                               xyz.data(), n_out));
  if (rc != RGBDFE_OK) return rc;
  std::vector<int32_t> ids, cnt;
  std::vector<const uint8_t*> dp;
  std::vector<const float*> xp;
  for (size_t f = 0; f < nf; ++f)
    if (node_ids[f] >= 0) {
      ids.push_back(node_ids[f]); cnt.push_back(n_out[f]);
      dp.push_back(desc.data() + f * mk * 32); xp.push_back(xyz.data() + f * mk * 4);
    }
  rc = guarded(ctx, [&]() -> int {
    return group_run(ctx, [&](int i) -> int {
      if (i == 0) return RGBDFE_OK;
      return impl::rgbdfe_upload_nodes(ctx->group->children[(size_t)i], (int32_t)ids.size(), ids.data(), dp.data(), xp.data(),
                                       cnt.data());
    });
  });
  if (rc != RGBDFE_OK) return rc;
  for (size_t f = 0; f < nf; ++f) {
    const size_t n = (size_t)n_out[f], o = f * (size_t)out_stride;
    if (keypoints && n) memcpy(keypoints + o, kp.data() + f * mk, n * sizeof(rgbdfe_keypoint));
    if (descriptors && n) memcpy(descriptors + o * 32, desc.data() + f * mk * 32, n * 32);
    if (xyz1 && n) memcpy(xyz1 + o * 4, xyz.data() + f * mk * 4, n * 16);
  }
  return RGBDFE_OK;
}

int rgbdfe_sift_debug_plane(rgbdfe_ctx* ctx, int32_t octave, int32_t level, float* out, int32_t capacity_floats, int32_t* w,
                            int32_t* h) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_debug_plane(c, octave, level, out, capacity_floats, w, h));
}

int rgbdfe_sift_debug_candidates(rgbdfe_ctx* ctx, int32_t octave, int32_t dog_level, float* out, int32_t capacity_rows,
                                 int32_t* n) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_debug_candidates(c, octave, dog_level, out, capacity_rows, n));
}

int rgbdfe_sift_geometry(rgbdfe_ctx* ctx, int32_t* octave_min, int32_t* octave_num, int32_t* levels, int32_t* dog_levels) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_geometry(c, octave_min, octave_num, levels, dog_levels));
}

int rgbdfe_hamming_nn_nodes(rgbdfe_ctx* ctx, int32_t query_id, int32_t train_id, int32_t* out_hd, int32_t* out_idx) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_hamming_nn_nodes(c, query_id, train_id, out_hd, out_idx));
}

int rgbdfe_place_recognition(rgbdfe_ctx* ctx, int32_t query_id, const int32_t* candidate_ids, int32_t n_candidates,
                             int32_t k_neighbours, int32_t max_hd, int32_t max_out, int32_t* out_ids, float* out_scores,
                             int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_place_recognition(c, query_id, candidate_ids, n_candidates, k_neighbours, max_hd,
                                                          max_out, out_ids, out_scores, n_out));
}

int rgbdfe_place_recognition_batch(rgbdfe_ctx* ctx, const int32_t* query_ids, int32_t n_queries,
                                   const int32_t* candidate_offsets, const int32_t* candidate_ids, int32_t k_neighbours,
                                   int32_t max_hd, int32_t max_out, int32_t* out_ids, float* out_scores,
                                   int32_t* out_counts) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_place_recognition_batch(c, query_ids, n_queries, candidate_offsets, candidate_ids,
                                                                k_neighbours, max_hd, max_out, out_ids, out_scores,
                                                                out_counts));
}

int rgbdfe_hamming_nn_host(rgbdfe_ctx* ctx, const uint8_t* qdesc, int32_t nq, const uint8_t* tdesc, int32_t nt,
                           int32_t* out_hd, int32_t* out_idx) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_hamming_nn_host(c, qdesc, nq, tdesc, nt, out_hd, out_idx));
}

int rgbdfe_project_to_3d(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* depth, int32_t rows,
                         int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling,
                         int32_t max_keypoints, int32_t* kept_idx, float* xyz1, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_project_to_3d(c, kp_xy, n_kp, depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                                      max_keypoints, kept_idx, xyz1, n_out));
}

int rgbdfe_project_to_3d_cloud(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* cloud, int32_t rows,
                               int32_t cols, double maximum_depth, int32_t max_keypoints, int32_t* kept_idx, float* xyz1,
                               int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_project_to_3d_cloud(c, kp_xy, n_kp, cloud, rows, cols, maximum_depth,
                                                            max_keypoints, kept_idx, xyz1, n_out));
}

int rgbdfe_detect_describe_cloud(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* cloud,
                                 int32_t rows, int32_t cols, double maximum_depth, rgbdfe_keypoint* keypoints,
                                 uint8_t* descriptors, float* xyz1, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detect_describe_cloud(c, gray, mask, cloud, rows, cols, maximum_depth, keypoints,
                                                              descriptors, xyz1, n_out));
}

int rgbdfe_sift_node_features(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* desc_in,
                              const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy,
                              double depth_scaling, int32_t max_keypoints, int32_t use_root_sift, int32_t* kept_idx,
                              float* xyz1, float* siftgpu_descriptors, float* feature_descriptors, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_node_features(c, kp_xy, nullptr, n_kp, desc_in, depth, rows, cols, fx, fy, cx, cy,
                                                           depth_scaling, max_keypoints, use_root_sift, kept_idx, xyz1,
                                                           siftgpu_descriptors, feature_descriptors, n_out));
}

int rgbdfe_sift_node_features_min_depth(rgbdfe_ctx* ctx, const float* kp_xy, const float* kp_size, int32_t n_kp,
                                        const float* desc_in, const float* depth, int32_t rows, int32_t cols, double fx,
                                        double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                        int32_t use_root_sift, int32_t* kept_idx, float* xyz1, float* siftgpu_descriptors,
                                        float* feature_descriptors, int32_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (n_kp > 0 && !kp_size) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "kp_size is required");
  return RGBDFE_FIRST(ctx, impl::rgbdfe_sift_node_features(c, kp_xy, kp_size, n_kp, desc_in, depth, rows, cols, fx, fy, cx,
                                                           cy, depth_scaling, max_keypoints, use_root_sift, kept_idx, xyz1,
                                                           siftgpu_descriptors, feature_descriptors, n_out));
}

int rgbdfe_host_register(rgbdfe_ctx* ctx, void* ptr, size_t bytes) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!ptr || bytes == 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
    if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, RGBDFE_ERR_HIP, "hipHostRegister failed (already registered, or not host memory)");
    }
    return RGBDFE_OK;
  });
}

int rgbdfe_host_unregister(rgbdfe_ctx* ctx, void* ptr) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!ptr) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
    if (hipHostUnregister(ptr) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, RGBDFE_ERR_HIP, "hipHostUnregister failed (not a registered range)");
    }
    return RGBDFE_OK;
  });
}

int rgbdfe_depth_to_mono8(rgbdfe_ctx* ctx, const void* depth, int32_t depth_is_u16, int32_t rows, int32_t cols,
                          uint8_t* mono8, float* depth_m) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_depth_to_mono8(c, depth, depth_is_u16, rows, cols, mono8, depth_m));
}

int rgbdfe_upload_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, const float* depth, int32_t rows, int32_t cols,
                             const uint8_t* rgb, int32_t rgb_channels, int32_t encoding_bgr, double fx, double fy,
                             double cx, double cy, double depth_scaling, double min_depth, int32_t cloud_skip,
                             float* cloud_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  // replicated like the node features, so that the measurement-model jobs can be sharded; the copy comes from device 0
  return RGBDFE_ALL(ctx, impl::rgbdfe_upload_node_cloud(c, node_id, depth, rows, cols, rgb, rgb_channels, encoding_bgr, fx,
                                                        fy, cx, cy, depth_scaling, min_depth, cloud_skip,
                                                        (!RGBDFE_IS_GROUP(ctx) || c == ctx->group->children[0]) ? cloud_out
                                                                                                               : nullptr));
}

int rgbdfe_release_node_cloud(rgbdfe_ctx* ctx, int32_t node_id) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_release_node_cloud(c, node_id));
}

// the clouds are replicated on every device of a group: served from the first one, like the other read-only frame-level calls
int rgbdfe_assemble_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth,
                        int32_t preserve_raster, float* out, int64_t capacity, int64_t* n_out, int64_t* node_offsets) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_assemble_map(c, n_nodes, node_ids, transforms, maximum_depth, preserve_raster, out, capacity,
                                                     n_out, node_offsets));
}

int rgbdfe_assemble_map_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                               double maximum_depth, int32_t preserve_raster, void* d_out, int64_t capacity, int64_t* n_out,
                               int64_t* node_offsets, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_assemble_map_device(c, n_nodes, node_ids, transforms, maximum_depth, preserve_raster, d_out,
                                                            capacity, n_out, node_offsets, stream));
}

int rgbdfe_download_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, float* cloud_out, int64_t capacity_points, int32_t* rows,
                               int32_t* cols) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_download_node_cloud(c, node_id, cloud_out, capacity_points, rows, cols));
}

int rgbdfe_voxel_filter(rgbdfe_ctx* ctx, const float* points, int64_t n_in, double voxelfilter_size, float* out, int64_t capacity,
                        int64_t* n_out, int32_t* flags) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_voxel_filter(c, points, n_in, voxelfilter_size, out, capacity, n_out, flags));
}

int rgbdfe_voxel_filter_device(rgbdfe_ctx* ctx, const void* d_points, int64_t n_in, double voxelfilter_size, void* d_out,
                               int64_t capacity, int64_t* n_out, int32_t* flags, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_voxel_filter_device(c, d_points, n_in, voxelfilter_size, d_out, capacity, n_out, flags,
                                                            stream));
}

// every device of a group reduces its replica of the cloud: the same kernels on the same bytes; n_out / flags from the first
int rgbdfe_reduce_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, double voxelfilter_size, int64_t* n_out, int32_t* flags) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (!n_out) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  return RGBDFE_ALL(ctx, [&]() -> int {
    int64_t n = 0;
    int32_t f = 0;
    const int rc = impl::rgbdfe_reduce_node_cloud(c, node_id, voxelfilter_size, &n, &f);
    if (!RGBDFE_IS_GROUP(ctx) || c == ctx->group->children[0]) {
      *n_out = n;
      if (flags) *flags = f;
    }
    return rc;
  }());
}

// the occupancy map lives on one device (the first of a group, where the clouds are replicated): every call goes there
void rgbdfe_octomap_default_params(rgbdfe_octomap_params* params) { impl::rgbdfe_octomap_default_params(params); }

int rgbdfe_octomap_create(rgbdfe_ctx* ctx, const rgbdfe_octomap_params* params, int64_t capacity_cells, rgbdfe_octomap** map) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_octomap_create(c, ctx, params, capacity_cells, map));
}

void rgbdfe_octomap_destroy(rgbdfe_octomap* map) {
  try {
    impl::rgbdfe_octomap_destroy(map);
  } catch (...) {
  }
}

#define RGBDFE_ON_MAP(map, call)                       \
  do {                                                 \
    if (!(map)) return RGBDFE_ERR_INVALID_ARG;         \
    rgbdfe_ctx* ctx = impl::octomap_owner(map);        \
    return RGBDFE_FIRST(ctx, ((void)c, (call)));       \
  } while (0)

int rgbdfe_octomap_reset(rgbdfe_octomap* map) { RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_reset(map)); }

int rgbdfe_octomap_reserve(rgbdfe_octomap* map, int64_t capacity_cells) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_reserve(map, capacity_cells));
}

int rgbdfe_octomap_insert_nodes(rgbdfe_octomap* map, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                                double max_range, int32_t* n_done) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_insert_nodes(map, n_nodes, node_ids, transforms, max_range, n_done));
}

int rgbdfe_octomap_insert_cloud(rgbdfe_octomap* map, const float* points, int64_t n, const float* transform, double max_range) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_insert_cloud(map, points, n, transform, max_range));
}

int rgbdfe_octomap_size(rgbdfe_octomap* map, int64_t* n_leaves) { RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_size(map, n_leaves)); }

int rgbdfe_octomap_leaves(rgbdfe_octomap* map, rgbdfe_octomap_leaf* out, int64_t capacity, int64_t* n_out) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_leaves(map, out, capacity, n_out));
}

int rgbdfe_octomap_stats(rgbdfe_octomap* map, int64_t* out, int32_t n_out) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_stats(map, out, n_out));
}

int rgbdfe_octomap_tree(rgbdfe_octomap* map, rgbdfe_octomap_node* out, int64_t capacity, int64_t* n_nodes) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_tree(map, out, capacity, n_nodes));
}

int rgbdfe_octomap_tree_device(rgbdfe_octomap* map, void* d_out, int64_t capacity, int64_t* n_nodes, void* stream) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_tree_device(map, d_out, capacity, n_nodes, stream));
}

int rgbdfe_octomap_nodes_at_depth(rgbdfe_octomap* map, int32_t depth, float min_log_odds, rgbdfe_octomap_leaf* out,
                                  int64_t capacity, int64_t* n_out) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_nodes_at_depth(map, depth, min_log_odds, out, capacity, n_out));
}

int rgbdfe_octomap_write(rgbdfe_octomap* map, const char* path) { RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_write(map, path)); }

int rgbdfe_octomap_set_leaves(rgbdfe_octomap* map, const rgbdfe_octomap_leaf* leaves, int64_t n) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_set_leaves(map, leaves, n));
}

int rgbdfe_octomap_read(rgbdfe_octomap* map, const char* path) { RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_read(map, path)); }

int rgbdfe_sizeof_octomap_ray_hit(void) { return (int)sizeof(rgbdfe_octomap_ray_hit); }

int rgbdfe_octomap_occupied_log_odds(rgbdfe_octomap* map, float* out) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_occupied_log_odds(map, out));
}

int rgbdfe_octomap_search(rgbdfe_octomap* map, const float* points, int64_t n, int32_t* found, rgbdfe_octomap_leaf* leaves) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_search(map, points, n, found, leaves));
}

int rgbdfe_octomap_cast_rays(rgbdfe_octomap* map, const float* origins, const float* directions, int64_t n, int32_t ignore_unknown,
                             double max_range, float occupied_log_odds, rgbdfe_octomap_ray_hit* hits) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_cast_rays(map, origins, directions, n, ignore_unknown, max_range, occupied_log_odds, hits));
}

int rgbdfe_octomap_view_cloud(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy, int32_t rows,
                              int32_t cols, int32_t ignore_unknown, double max_range, float occupied_log_odds, float* out,
                              uint8_t* status) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_view_cloud(map, transform, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range,
                                                     occupied_log_odds, out, status));
}

int rgbdfe_octomap_view_cloud_device(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy,
                                     int32_t rows, int32_t cols, int32_t ignore_unknown, double max_range, float occupied_log_odds,
                                     void* d_out, void* d_status, void* stream) {
  RGBDFE_ON_MAP(map, impl::rgbdfe_octomap_view_cloud_device(map, transform, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range,
                                                            occupied_log_odds, d_out, d_status, stream));
}
#undef RGBDFE_ON_MAP

// pose-graph optimisation runs on one device (the first of a group)
int rgbdfe_pose_graph_chi2(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_pose_graph_chi2(c, g, chi2));
}

int rgbdfe_pose_graph_linearize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* errors, double* weights, int32_t edge_capacity,
                                int32_t* n_edges, int32_t* free_ids, double* h_diag, double* b, int32_t vertex_capacity,
                                int32_t* n_free, int32_t* off_rows, int32_t* off_cols, double* h_off, int32_t block_capacity,
                                int32_t* n_blocks, double* chi2) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_pose_graph_linearize(c, g, errors, weights, edge_capacity, n_edges, free_ids, h_diag, b,
                                                             vertex_capacity, n_free, off_rows, off_cols, h_off, block_capacity,
                                                             n_blocks, chi2));
}

int rgbdfe_pose_graph_optimize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, int32_t iterations, rgbdfe_pose_graph_report* report) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_pose_graph_optimize(c, g, iterations, report));
}

int rgbdfe_pose_graph_optimize_graph(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double break_criterion,
                                     rgbdfe_pose_graph_report* report) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_pose_graph_optimize_graph(c, g, break_criterion, report));
}

int rgbdfe_pose_graph_edge_errors(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2, double* err_sq, int32_t* active,
                                  int32_t capacity, int32_t* n_edges) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_pose_graph_edge_errors(c, g, chi2, err_sq, active, capacity, n_edges));
}

int rgbdfe_pose_graph_prune_edges(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, float thresh, uint8_t* verdicts, int32_t capacity,
                                  int32_t* n_pruned) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_pose_graph_prune_edges(c, g, thresh, verdicts, capacity, n_pruned));
}

int rgbdfe_pose_graph_evaluate(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double optimizer_iterations,
                               rgbdfe_pose_graph_evaluation* out, double* estimates, int32_t capacity_nodes) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_pose_graph_evaluate(c, g, optimizer_iterations, out, estimates, capacity_nodes));
}

// the ICP fallback runs on one device (the first of a group)
void rgbdfe_icp_default_params(rgbdfe_icp_params* p) { impl::rgbdfe_icp_default_params(p); }

int rgbdfe_icp_align_nodes(rgbdfe_ctx* ctx, int32_t n_jobs, const int32_t* source_ids, const int32_t* target_ids,
                           const float* guesses, const rgbdfe_icp_params* params, float* transforms_out,
                           rgbdfe_icp_report* reports_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_icp_align_nodes(c, n_jobs, source_ids, target_ids, guesses, params, transforms_out,
                                                        reports_out));
}

int rgbdfe_icp_align_clouds(rgbdfe_ctx* ctx, const float* source, int64_t n_source, const float* target, int64_t n_target,
                            const float* guess, const rgbdfe_icp_params* params, float* transform_out,
                            rgbdfe_icp_report* report_out, int32_t* nn_index_out, float* nn_d2_out, int64_t debug_capacity) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_icp_align_clouds(c, source, n_source, target, n_target, guess, params, transform_out,
                                                         report_out, nn_index_out, nn_d2_out, debug_capacity));
}

int rgbdfe_filter_cloud(rgbdfe_ctx* ctx, const float* cloud, int64_t n, int32_t desired_size, int32_t* indices_out,
                        float* rows_out, int64_t capacity, int64_t* n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_filter_cloud(c, cloud, n, desired_size, indices_out, rows_out, capacity, n_out));
}

void rgbdfe_display_default_params(rgbdfe_display_params* p) { impl::rgbdfe_display_default_params(p); }

// the clouds are replicated on every device of a group: served from the first one, like map assembly
int rgbdfe_display_geometry(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                            const rgbdfe_display_params* params, float* vertices, int64_t vertex_capacity, int64_t* n_vertices,
                            int64_t* node_offsets, int64_t* strips, int64_t strip_capacity, int64_t* n_strips,
                            int64_t* node_strip_offsets, int32_t* node_types) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_display_geometry(c, n_nodes, node_ids, transforms, params, vertices, vertex_capacity,
                                                         n_vertices, node_offsets, strips, strip_capacity, n_strips,
                                                         node_strip_offsets, node_types));
}

int rgbdfe_display_geometry_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                                   const rgbdfe_display_params* params, void* d_vertices, int64_t vertex_capacity,
                                   int64_t* n_vertices, int64_t* node_offsets, void* d_strips, int64_t strip_capacity,
                                   int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_display_geometry_device(c, n_nodes, node_ids, transforms, params, d_vertices,
                                                                vertex_capacity, n_vertices, node_offsets, d_strips,
                                                                strip_capacity, n_strips, node_strip_offsets, node_types, stream));
}

void rgbdfe_render_default_params(rgbdfe_render_params* p) { impl::rgbdfe_render_default_params(p); }

// served from the first device of a group, like display geometry
int rgbdfe_render_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                        const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params, uint8_t* rgba,
                        float* depth, int64_t* ids, int32_t* node_index) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_render_nodes(c, n_nodes, node_ids, transforms, display_params, render_params, rgba, depth,
                                                     ids, node_index));
}

int rgbdfe_render_nodes_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                               const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params,
                               void* d_rgba, void* d_depth, void* d_ids, void* d_node_index, void* stream) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_render_nodes_device(c, n_nodes, node_ids, transforms, display_params, render_params, d_rgba,
                                                            d_depth, d_ids, d_node_index, stream));
}

void rgbdfe_render_perspective(double fovy, double aspect, double z_near, double z_far, double* out16) {
  impl::rgbdfe_render_perspective(fovy, aspect, z_near, z_far, out16);
}

void rgbdfe_render_viewer_view(double x_tra, double y_tra, double z_tra, double x_rot, double y_rot, double z_rot,
                               double rotation_stepping, const double* viewpoint, double* out16) {
  impl::rgbdfe_render_viewer_view(x_tra, y_tra, z_tra, x_rot, y_rot, z_rot, rotation_stepping, viewpoint, out16);
}

void rgbdfe_render_sensor_camera(double fx, double fy, double cx, double cy, int32_t width, int32_t height, double z_near,
                                 double z_far, const double* pose, double* view_out16, double* projection_out16) {
  impl::rgbdfe_render_sensor_camera(fx, fy, cx, cy, width, height, z_near, z_far, pose, view_out16, projection_out16);
}

int rgbdfe_render_unproject(double x, double y, double depth, const double* view, const double* projection, int32_t width,
                            int32_t height, double* out3) {
  return impl::rgbdfe_render_unproject(x, y, depth, view, projection, width, height, out3);
}

int rgbdfe_render_fragment_stats(rgbdfe_ctx* ctx, int32_t enable, int64_t* out2) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_render_fragment_stats(c, enable, out2));
}

int rgbdfe_observation_likelihood(rgbdfe_ctx* ctx, int32_t n, const int32_t* new_ids, const int32_t* old_ids,
                                  const float* transforms, int32_t emm_skip_step, rgbdfe_emm_counts* out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!RGBDFE_IS_GROUP(ctx))
      return impl::rgbdfe_observation_likelihood(ctx, n, new_ids, old_ids, transforms, emm_skip_step, out);
    if (n < 0 || (n > 0 && (!new_ids || !old_ids || !transforms || !out)))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
    Group& g = *ctx->group;
    const int G = (int)g.children.size();
    return group_run(ctx, [&](int i) -> int {  // job k -> device k mod G
      std::vector<int32_t> a, b;
      std::vector<float> T;
      for (int32_t k = i; k < n; k += G) {
        a.push_back(new_ids[k]); b.push_back(old_ids[k]);
        T.insert(T.end(), transforms + (size_t)k * 16, transforms + (size_t)k * 16 + 16);
      }
      if (a.empty()) return RGBDFE_OK;
      std::vector<rgbdfe_emm_counts> o(a.size());
      const int rc = impl::rgbdfe_observation_likelihood(g.children[(size_t)i], (int32_t)a.size(), a.data(), b.data(),
                                                         T.data(), emm_skip_step, o.data());
      if (rc != RGBDFE_OK) return rc;
      for (size_t m = 0; m < o.size(); ++m) out[(size_t)i + m * (size_t)G] = o[m];
      return RGBDFE_OK;
    });
  });
}

int rgbdfe_observation_criterion_met(uint32_t inliers, uint32_t outliers, uint32_t all, double observability_threshold,
                                     double* quality) {
  return impl::rgbdfe_observation_criterion_met(inliers, outliers, all, observability_threshold, quality);
}

int rgbdfe_set_latency_mode(rgbdfe_ctx* ctx, int32_t max_pairs, int32_t chunk_iterations) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_latency_mode(c, max_pairs, chunk_iterations));
}

int rgbdfe_set_hamming_mode(rgbdfe_ctx* ctx, int32_t mode) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_hamming_mode(c, mode));
}

int rgbdfe_hamming_wide_last(rgbdfe_ctx* ctx) {
  if (!ctx) return -1;
  return impl::rgbdfe_hamming_wide_last(RGBDFE_IS_GROUP(ctx) ? ctx->group->children[0] : ctx);   // (a value, not a status)
}

int rgbdfe_set_hamming_shape(rgbdfe_ctx* ctx, int32_t shape) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_hamming_shape(c, shape));
}

int rgbdfe_hamming_shape_last(rgbdfe_ctx* ctx) {
  if (!ctx) return -1;
  return impl::rgbdfe_hamming_shape_last(RGBDFE_IS_GROUP(ctx) ? ctx->group->children[0] : ctx);   // (a value, not a status)
}

int rgbdfe_set_profiling(rgbdfe_ctx* ctx, int enable) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_profiling(c, enable));
}

// group: the sum over the devices
int rgbdfe_get_kernel_time(rgbdfe_ctx* ctx, int which, double* total_ms, int64_t* launches, int64_t* pairs) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (!RGBDFE_IS_GROUP(ctx)) return impl::rgbdfe_get_kernel_time(ctx, which, total_ms, launches, pairs);
    double ms = 0; int64_t nl = 0, np = 0;
    for (rgbdfe_ctx* c : ctx->group->children) {
      double a = 0; int64_t b = 0, d = 0;
      const int rc = impl::rgbdfe_get_kernel_time(c, which, &a, &b, &d);
      if (rc != RGBDFE_OK) return rc;
      ms += a; nl += b; np += d;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = nl;
    if (pairs) *pairs = np;
    return RGBDFE_OK;
  });
}

int rgbdfe_reset_kernel_time(rgbdfe_ctx* ctx) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_reset_kernel_time(c));
}

// group: the sum over the devices
int rgbdfe_graph_stats(rgbdfe_ctx* ctx, int64_t* out, int32_t n_out) {
  if (!ctx || !out || n_out < 0) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    for (int32_t i = 0; i < n_out; ++i) out[i] = 0;
    if (!RGBDFE_IS_GROUP(ctx)) return impl::rgbdfe_graph_stats(ctx, out, n_out);
    for (rgbdfe_ctx* c : ctx->group->children) {
      const int rc = impl::rgbdfe_graph_stats(c, out, n_out);
      if (rc != RGBDFE_OK) return rc;
    }
    return RGBDFE_OK;
  });
}

int rgbdfe_sizeof_match_result(void) { return impl::rgbdfe_sizeof_match_result(); }
int rgbdfe_sizeof_compact_result(void) { return impl::rgbdfe_sizeof_compact_result(); }
int rgbdfe_update_inlier_features(rgbdfe_ctx* ctx, const void* d_records, const int32_t* query_ids, const int32_t* train_ids,
                                  const uint8_t* accept, int32_t n, int32_t* launched) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  if (RGBDFE_IS_GROUP(ctx)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "rgbdfe_update_inlier_features takes device pointers: single-device contexts only");
  return guarded(ctx, [&]() -> int { return impl::rgbdfe_update_inlier_features(ctx, d_records, query_ids, train_ids, accept, n, launched); });
}

int rgbdfe_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, uint8_t* out, int32_t capacity) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_node_feature_stats(c, node_id, out, capacity));
}

// a multi-device handle answers from its first device: every node is resident on all of them
int rgbdfe_download_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc,
                          float* xyz1, float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_download_nodes(c, n_nodes, node_ids, capacity_rows, desc, xyz1, kp_xy, stats, row_offsets, kinds));
}

int rgbdfe_debug_download_nodes_copy_loop(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc,
                                          float* xyz1, float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_debug_download_nodes_copy_loop(c, n_nodes, node_ids, capacity_rows, desc, xyz1, kp_xy, stats, row_offsets, kinds));
}

int rgbdfe_download_node(rgbdfe_ctx* ctx, int32_t node_id, int32_t capacity_rows, void* desc, float* xyz1, float* kp_xy,
                         uint8_t* stats, int32_t* kind, int32_t* has_keypoints) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {   // (the return value is a row count: not through RGBDFE_FIRST, which reads it as a status)
    return impl::rgbdfe_download_node(RGBDFE_IS_GROUP(ctx) ? ctx->group->children[0] : ctx, node_id, capacity_rows, desc, xyz1,
                                      kp_xy, stats, kind, has_keypoints);
  });
}

int rgbdfe_download_nodes_stats(rgbdfe_ctx* ctx, int64_t* out, int32_t n_out) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_download_nodes_stats(c, out, n_out));
}

int rgbdfe_set_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, const uint8_t* stats, int32_t n) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_set_node_feature_stats(c, node_id, stats, n));
}

int rgbdfe_detector_set_thresholds(rgbdfe_ctx* ctx, const double* thresholds, int32_t n_cells) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_detector_set_thresholds(c, thresholds, n_cells));
}

int rgbdfe_node_cloud_info(rgbdfe_ctx* ctx, int32_t node_id, double* out8) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_node_cloud_info(c, node_id, out8));
}

int rgbdfe_restore_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, const float* points, int32_t rows, int32_t cols, double fx, double fy,
                              double cx, double cy, int32_t cloud_skip) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_ALL(ctx, impl::rgbdfe_restore_node_cloud(c, node_id, points, rows, cols, fx, fy, cx, cy, cloud_skip));
}

int rgbdfe_session_save(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, uint32_t flags, const char* path) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_session_save");
    return impl::rgbdfe_session_save(ctx, slam, graph, flags, path);
  });
}

int rgbdfe_session_load(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, const char* path) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return guarded(ctx, [&]() -> int {
    if (RGBDFE_IS_GROUP(ctx)) return group_only_single(ctx, "rgbdfe_session_load");
    return impl::rgbdfe_session_load(ctx, slam, graph, path);
  });
}

// (the host-only calls of the map files -- rgbdfe_save_cloud_file, rgbdfe_cloud_file_info, rgbdfe_load_cloud_file,
// rgbdfe_cloud_file_path -- take no context: api_map_files.hip defines them behind a barrier of their own)
int rgbdfe_save_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth,
                    int32_t preserve_raster, const char* path, int64_t chunk_points, char* path_written, int64_t path_capacity,
                    rgbdfe_map_file_stats* stats) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_save_map(c, n_nodes, node_ids, transforms, maximum_depth, preserve_raster, path, chunk_points,
                                                 path_written, path_capacity, stats));
}

int rgbdfe_save_node_clouds(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const int32_t* graph_ids, const double* poses,
                            int32_t transform_individual_clouds, const char* basename, int32_t* n_written) {
  if (!ctx) return RGBDFE_ERR_INVALID_ARG;
  return RGBDFE_FIRST(ctx, impl::rgbdfe_save_node_clouds(c, n_nodes, node_ids, graph_ids, poses, transform_individual_clouds, basename,
                                                         n_written));
}

int rgbdfe_abi_version(void) { return impl::rgbdfe_abi_version(); }

}  // extern "C"

