// api_slam.hip -- the SLAM step (include/rgbdfe.h, "the SLAM step"): the decision machine of slam_machine.h behind the C
// ABI, rgbdfe_slam_add_node = that machine plus the device calls, and feature_matching_stats_ on the resident nodes
// (the kernel: slam_step.hip).
#include <chrono>
#include <new>

#include "rgbdfe_host.h"
#include "session_format.h"
#include "slam_machine.h"
#include "slam_step.h"

namespace impl {

// the counters of every slot, allocated zeroed on first use (rgbdfe_host.h: d_feat_stats); ctx->mu is held
int ensure_feature_stats(rgbdfe_ctx* ctx) {
  if (ctx->d_feat_stats) return RGBDFE_OK;
  const size_t bytes = (size_t)ctx->cfg.max_nodes * ctx->feat_stats_stride();
  if (hipMalloc((void**)&ctx->d_feat_stats, bytes) != hipSuccess) {
    (void)hipGetLastError();
    ctx->d_feat_stats = nullptr;
    return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "feature statistics");
  }
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_feat_stats, 0, bytes, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return RGBDFE_OK;
}

int rgbdfe_update_inlier_features(rgbdfe_ctx* ctx, const void* d_records, const int32_t* query_ids, const int32_t* train_ids,
                                  const uint8_t* accept, int32_t n, int32_t* launched) {
  if (launched) *launched = 0;
  if (!ctx || n < 0 || (n > 0 && (!d_records || !query_ids || !train_ids || !accept)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::vector<rgbdfe::SlamStatsPair> pairs((size_t)n);
  bool any = false;
  std::lock_guard<std::mutex> g(ctx->mu);
  for (int32_t k = 0; k < n; ++k) {
    pairs[(size_t)k] = rgbdfe::SlamStatsPair{0u, 0u, 0u};
    if (!accept[k]) continue;
    const auto q = ctx->nodes.find(query_ids[k]), t = ctx->nodes.find(train_ids[k]);
    if (q == ctx->nodes.end() || t == ctx->nodes.end())
      return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "an accepted pair names a node that is not resident");
    pairs[(size_t)k] = rgbdfe::SlamStatsPair{q->second.slot, t->second.slot, 1u};
    any = true;
  }
  if (!any) return RGBDFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  if (const int rc = ensure_feature_stats(ctx)) return rc;
  if (const int rc = ensure_scratch(ctx, sizeof(rgbdfe::SlamStatsPair) * (size_t)n)) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_scratch, pairs.data(), sizeof(rgbdfe::SlamStatsPair) * (size_t)n, hipMemcpyHostToDevice,
                              ctx->stream));
  const int launches = rgbdfe::launch_inlier_stats(static_cast<const rgbdfe_match_result*>(d_records),
                                                   static_cast<const rgbdfe::SlamStatsPair*>(ctx->d_scratch), (uint32_t)n,
                                                   ctx->d_feat_stats, (uint32_t)ctx->feat_stats_stride(),
                                                   (uint32_t)ctx->cfg.max_keypoints, ctx->stream);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // `pairs` and the scratch are this call's
  if (launched) *launched = launches;
  return RGBDFE_OK;
}

int rgbdfe_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, uint8_t* out, int32_t capacity) {
  if (!ctx || capacity < 0 || (capacity > 0 && !out)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const auto it = ctx->nodes.find(node_id);
  if (it == ctx->nodes.end()) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "feature statistics of a node that is not resident");
  const uint32_t n = it->second.n;
  if ((uint32_t)capacity < n) return fail(ctx, RGBDFE_ERR_CAPACITY, "feature statistics: capacity below the node's rows");
  if (n == 0) return 0;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  if (const int rc = ensure_feature_stats(ctx)) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_feat_stats + (size_t)it->second.slot * ctx->feat_stats_stride(), n,
                              hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return (int)n;
}

}  // namespace impl

// ---- the rgbdfe_slam object
struct rgbdfe_slam {
  rgbdfe_slam_machine::Machine m;
  rgbdfe_ctx* ctx = nullptr;
  int device_id = 0;               // of ctx (the buffers below are freed without it)
  std::mutex mu;
  void* d_records = nullptr;       // RGBDFE_SLAM_MAX_CANDIDATES records: where add_node's batches leave their results
  rgbdfe_match_result* h_records = nullptr;   // pinned
  bool defer_apply = false;        // add_node applies a finished step itself, behind its statistics launch
};

namespace {

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// what a finished step leaves to the device: slots and clouds to release, the optimisation
int apply_step(rgbdfe_slam* s, rgbdfe_slam_step* st) {
  if (!s->ctx || s->defer_apply) return RGBDFE_OK;
  for (int32_t slot : s->m.to_release) {
    const int rc = rgbdfe_release_node(s->ctx, slot);   // (drops the node's cloud too)
    if (rc != RGBDFE_OK && rc != RGBDFE_ERR_UNKNOWN_NODE) return rc;
  }
  s->m.to_release.clear();
  if (st->cloud_released) {
    const int rc = rgbdfe_release_node_cloud(s->ctx, s->m.slot_of[(size_t)st->id]);
    if (rc != RGBDFE_OK && rc != RGBDFE_ERR_UNKNOWN_NODE) return rc;   // a node without a cloud has none to release
  }
  if (st->optimize_due) {
    const auto t0 = std::chrono::steady_clock::now();
    rgbdfe_pose_graph_report rep;
    const int rc = rgbdfe_pose_graph_optimize_graph(s->ctx, s->m.g, s->m.prm.optimizer_iterations, &rep);
    if (rc != RGBDFE_OK) return rc;
    st->optimized = 1;
    st->lm_iterations = rep.iterations;
    st->chi2 = rep.chi2;
    st->seconds[3] = seconds_since(t0);
  }
  return RGBDFE_OK;
}

// the inverse of a column-major Matrix4f through Gauss-Jordan in double with partial pivoting (final_trafo.inverse(),
// node.cpp:1532; the same arithmetic as include/rgbdfe.hpp's inverse4)
void inverse4(const float* T, float* out) {
  double a[4][8];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { a[r][c] = T[c * 4 + r]; a[r][c + 4] = r == c ? 1.0 : 0.0; }
  for (int i = 0; i < 4; ++i) {
    int p = i;
    for (int r = i + 1; r < 4; ++r) if (std::fabs(a[r][i]) > std::fabs(a[p][i])) p = r;
    for (int c = 0; c < 8; ++c) std::swap(a[i][c], a[p][c]);
    const double d = a[i][i];
    for (int c = 0; c < 8; ++c) a[i][c] /= d;
    for (int r = 0; r < 4; ++r)
      if (r != i) { const double f = a[r][i]; for (int c = 0; c < 8; ++c) a[r][c] -= f * a[i][c]; }
  }
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[c * 4 + r] = (float)a[r][c + 4];
}

// What follows the pair op in Node::matchNodePair for the n results of one list (ids[k]: the candidate's graph id, at[k]:
// its record's position or -1, slots[at[k]]: its slot): the ICP fallback (node.cpp:1356-1377) and the pairwise observation
// likelihood (:1340-1345).  compact[k] / flags[k] become what rgbdfe_slam_feed takes.
int matchnodepair_tail(rgbdfe_slam* s, int32_t new_slot, const int32_t* ids, const int32_t* at, int32_t n, const int32_t* slots,
                       rgbdfe_compact_result* compact, uint8_t* flags) {
  const rgbdfe_slam_params& p = s->m.prm;
  std::vector<int32_t> icp_k, emm_k;
  for (int32_t k = 0; k < n; ++k) {
    if (at[k] < 0) continue;
    if (compact[k].id1 >= 0) { if (p.observability_threshold > 0) emm_k.push_back(k); }
    else if (p.use_icp && s->m.new_id - ids[k] <= 1) icp_k.push_back(k);
  }
  if (!icp_k.empty()) {
    std::vector<int32_t> source, target(icp_k.size(), new_slot);   // the OLDER node's cloud onto the new node's (:1362-1364)
    for (int32_t k : icp_k) source.push_back(slots[at[k]]);
    std::vector<float> T(16 * icp_k.size());
    std::vector<rgbdfe_icp_report> rep(icp_k.size());
    rgbdfe_icp_params ip;
    rgbdfe_icp_default_params(&ip);
    const int rc = rgbdfe_icp_align_nodes(s->ctx, (int32_t)icp_k.size(), source.data(), target.data(), nullptr, &ip, T.data(), rep.data());
    if (rc != RGBDFE_OK) return rc;
    for (size_t j = 0; j < icp_k.size(); ++j) {
      if (!rep[j].converged) continue;
      rgbdfe_compact_result& c = compact[icp_k[j]];
      c.id1 = slots[at[icp_k[j]]]; c.id2 = new_slot;   // final_trafo = icp_trafo, the literal assignment (:1370-1373)
      memcpy(c.trafo, T.data() + 16 * j, sizeof(c.trafo));
      flags[icp_k[j]] |= RGBDFE_SLAM_RESULT_ICP;
    }
  }
  if (!emm_k.empty()) {
    std::vector<int32_t> new_ids, old_ids;
    std::vector<float> T;
    for (int32_t k : emm_k) {
      float inv[16];
      inverse4(compact[k].trafo, inv);
      new_ids.push_back(new_slot); old_ids.push_back(slots[at[k]]); T.insert(T.end(), compact[k].trafo, compact[k].trafo + 16);
      new_ids.push_back(slots[at[k]]); old_ids.push_back(new_slot); T.insert(T.end(), inv, inv + 16);
    }
    std::vector<rgbdfe_emm_counts> c(new_ids.size());
    const int rc = rgbdfe_observation_likelihood(s->ctx, (int32_t)new_ids.size(), new_ids.data(), old_ids.data(), T.data(),
                                                 p.emm__skip_step, c.data());
    if (rc != RGBDFE_OK) return rc;
    for (size_t j = 0; j < emm_k.size(); ++j) {
      const rgbdfe_emm_counts &a = c[2 * j], &b = c[2 * j + 1];   // node.cpp:1548-1551
      const uint32_t inl = a.inliers + b.inliers, outl = a.outliers + b.outliers, occ = a.occluded + b.occluded;
      double quality = 0.0;
      if (!rgbdfe_observation_criterion_met(inl, outl, occ + inl + outl, p.observability_threshold, &quality))
        flags[emm_k[j]] |= RGBDFE_SLAM_RESULT_WITHDRAWN;
    }
  }
  return RGBDFE_OK;
}

}  // namespace
namespace rgbdfe_host { int slam_fail(rgbdfe_slam* s, int code, const std::string& msg); }
namespace {

template <class F>
int slam_guarded(F&& f) noexcept {
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

void rgbdfe_slam_default_params(rgbdfe_slam_params* p) {
  if (!p) return;
  *p = rgbdfe_slam_params{};
  p->min_matches = 20;
  p->predecessor_candidates = 4;
  p->neighbor_candidates = 4;
  p->min_sampled_candidates = 4;
  p->geodesic_depth = 3;
  p->create_cloud_every_nth_node = 1;
  p->optimizer_skip_step = 1;
  p->emm__skip_step = 8;
  p->max_translation_meter = 1e10;
  p->max_rotation_degree = 360;
  p->optimizer_iterations = 0.01;
  p->observability_threshold = -0.6;
  for (int k = 0; k < 16; ++k) p->init_base_pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

int rgbdfe_slam_create(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, const rgbdfe_slam_params* p, rgbdfe_slam** out) {
  return slam_guarded([&]() -> int {
    if (!g || !p || !out || p->min_matches < 0 || p->predecessor_candidates < 1 || p->neighbor_candidates < 0 ||
        p->min_sampled_candidates < 0 || p->create_cloud_every_nth_node < 1)
      return RGBDFE_ERR_INVALID_ARG;
    if (ctx && RGBDFE_IS_GROUP(ctx)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "rgbdfe_slam: single-device contexts only");
    // the longest list candidate selection can hand out must fit one batch: refused here, before any step can be half done
    const int64_t longest = (int64_t)p->predecessor_candidates + p->neighbor_candidates + p->min_sampled_candidates;
    if (longest > RGBDFE_SLAM_MAX_CANDIDATES || (ctx && longest > ctx->cfg.max_pairs_per_batch))
      return fail(ctx, RGBDFE_ERR_CAPACITY, "rgbdfe_slam: predecessor + neighbor + sampled candidates exceed a batch (max_pairs_per_batch, RGBDFE_SLAM_MAX_CANDIDATES)");
    rgbdfe_slam* s = new rgbdfe_slam();
    s->ctx = ctx;
    if (ctx) s->device_id = ctx->cfg.device_id;
    s->m.prm = *p;
    s->m.g = g;
    *out = s;
    return RGBDFE_OK;
  });
}

void rgbdfe_slam_destroy(rgbdfe_slam* s) {
  if (!s) return;
  if (s->d_records || s->h_records) {
    (void)hipSetDevice(s->device_id);
    if (s->d_records) (void)hipFree(s->d_records);
    if (s->h_records) (void)hipHostFree(s->h_records);
  }
  delete s;
}

int rgbdfe_slam_reset(rgbdfe_slam* s) {
  return slam_guarded([&]() -> int {
    if (!s) return RGBDFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> l(s->mu);
    s->m.reset();
    s->m.calls = 0;
    s->m.to_release.clear();
    return RGBDFE_OK;
  });
}

int rgbdfe_slam_set_rand(rgbdfe_slam* s, rgbdfe_rand_fn rand_fn, void* rand_state) {
  if (!s) return RGBDFE_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> l(s->mu);
  s->m.rand_fn = rand_fn;
  s->m.rand_state = rand_state;
  return RGBDFE_OK;
}

int rgbdfe_slam_begin(rgbdfe_slam* s, int32_t slot, int32_t n_rows, int64_t stamp_sec, int32_t stamp_nsec, int32_t* ids,
                      int32_t capacity, int32_t* n_ids, rgbdfe_slam_step* step) {
  return slam_guarded([&]() -> int {
    if (!s || !step) return RGBDFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> l(s->mu);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = s->m.begin(slot, n_rows, stamp_sec, stamp_nsec, ids, capacity, n_ids, step);
    if (rc != RGBDFE_OK) return rc;
    s->m.st.seconds[0] += seconds_since(t0);
    if (*n_ids > 0) return RGBDFE_OK;
    step->seconds[0] = s->m.st.seconds[0];
    return apply_step(s, step);
  });
}

int rgbdfe_slam_feed(rgbdfe_slam* s, const rgbdfe_compact_result* results, const uint8_t* flags, int32_t n, int32_t* ids,
                     int32_t capacity, int32_t* n_ids, rgbdfe_slam_step* step) {
  return slam_guarded([&]() -> int {
    if (!s || !step) return RGBDFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> l(s->mu);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = s->m.feed(results, flags, n, ids, capacity, n_ids, step);
    if (rc != RGBDFE_OK) return rc;
    if (*n_ids > 0) {   // the initial comparison is behind us: what followed was candidate selection
      s->m.st.seconds[0] += seconds_since(t0);
      return RGBDFE_OK;
    }
    step->seconds[0] = s->m.st.seconds[0];
    step->seconds[2] = seconds_since(t0);
    return apply_step(s, step);
  });
}

int rgbdfe_slam_add_node(rgbdfe_slam* s, int32_t slot, int64_t stamp_sec, int32_t stamp_nsec, rgbdfe_slam_step* out) {
  return slam_guarded([&]() -> int {
    if (!s || !out) return RGBDFE_ERR_INVALID_ARG;
    rgbdfe_ctx* ctx = s->ctx;
    if (!ctx) return RGBDFE_ERR_NO_DEVICE;   // the machine alone: rgbdfe_slam_begin / rgbdfe_slam_feed
    const int n_rows = rgbdfe_node_count(ctx, slot);
    if (n_rows < 0) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "rgbdfe_slam_add_node: the slot holds no node");
    if (!s->d_records) {
      HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
      HIP_TRY(ctx, hipMalloc(&s->d_records, sizeof(rgbdfe_match_result) * (RGBDFE_SLAM_MAX_CANDIDATES + 1)));
      HIP_TRY(ctx, hipHostMalloc((void**)&s->h_records, sizeof(rgbdfe_match_result) * (RGBDFE_SLAM_MAX_CANDIDATES + 1), hipHostMallocDefault));
    }
    int32_t ids[RGBDFE_SLAM_MAX_CANDIDATES], n_ids = 0;
    { std::lock_guard<std::mutex> l(s->mu); s->defer_apply = true; }
    int rc = rgbdfe_slam_begin(s, slot, n_rows, stamp_sec, stamp_nsec, ids, RGBDFE_SLAM_MAX_CANDIDATES, &n_ids, out);
    if (rc != RGBDFE_OK) { std::lock_guard<std::mutex> l(s->mu); s->defer_apply = false; return rc; }
    // The step's records stay in device memory until its one statistics launch: record 0 is the initial comparison's,
    // records 1 .. the main batch's.
    double compare_seconds = 0.0;
    int32_t q[RGBDFE_SLAM_MAX_CANDIDATES + 1], t[RGBDFE_SLAM_MAX_CANDIDATES + 1], n_rec = 1;
    uint8_t accept[RGBDFE_SLAM_MAX_CANDIDATES + 1];
    memset(accept, 0, sizeof(accept));
    q[0] = slot; t[0] = slot;
    bool any = false;
    auto abandon = [&](int code) { std::lock_guard<std::mutex> l(s->mu); s->m.phase = rgbdfe_slam_machine::Machine::kIdle; s->defer_apply = false; return code; };
    while (n_ids > 0) {
      const auto t0 = std::chrono::steady_clock::now();
      if (n_ids > ctx->cfg.max_pairs_per_batch)
        return abandon(fail(ctx, RGBDFE_ERR_CAPACITY, "rgbdfe_slam_add_node: more candidates than max_pairs_per_batch"));
      const bool initial = s->m.phase == rgbdfe_slam_machine::Machine::kInitial;
      const int32_t base = initial ? 0 : 1;
      // the candidates that still have features, as one batch; a released node gives no edge
      int32_t at[RGBDFE_SLAM_MAX_CANDIDATES], nb = 0;
      for (int32_t k = 0; k < n_ids; ++k) {
        const int32_t cs = rgbdfe_slam_slot_of(s, ids[k]);
        at[k] = -1;
        if (cs < 0) continue;
        q[base + nb] = slot; t[base + nb] = cs; at[k] = base + nb++;
      }
      if (nb > 0) {
        rgbdfe_match_result* d = static_cast<rgbdfe_match_result*>(s->d_records) + base;
        rc = rgbdfe_match_pair_list_device(ctx, q + base, t + base, nb, d, nullptr);
        if (rc != RGBDFE_OK) return abandon(rc);
        hipError_t he = hipSetDevice(ctx->cfg.device_id);
        if (he == hipSuccess) he = hipMemcpyAsync(s->h_records + base, d, sizeof(rgbdfe_match_result) * (size_t)nb, hipMemcpyDeviceToHost, ctx->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
        if (he != hipSuccess) return abandon(fail(ctx, RGBDFE_ERR_HIP, std::string("rgbdfe_slam_add_node: ") + hipGetErrorString(he)));
      }
      if (!initial) n_rec = 1 + nb;
      rgbdfe_compact_result compact[RGBDFE_SLAM_MAX_CANDIDATES];
      for (int32_t k = 0; k < n_ids; ++k) {
        rgbdfe_compact_result& c = compact[k];
        memset(&c, 0, sizeof(c));
        c.id1 = -1; c.id2 = -1;
        if (at[k] < 0) continue;
        const rgbdfe_match_result& r = s->h_records[at[k]];
        c.id1 = r.id1; c.id2 = r.id2; c.n_all = r.n_all; c.n_inl = r.n_inl; c.rmse = r.rmse;
        memcpy(c.trafo, r.trafo, sizeof(c.trafo));
        c.info_scale = r.info_scale;
        c.valid_iterations = r.valid_iterations; c.real_iterations = r.real_iterations;
        memcpy(c.inlier_mask, r.inlier_mask, sizeof(c.inlier_mask));
      }
      // the rest of matchNodePair's chain (node.cpp:1340-1377), each stage one batch.  Who is served is settled on the
      // RANSAC results: the ICP fallback takes the candidates WITHOUT a RANSAC transformation that are adjacent to the new
      // node, the measurement model the RANSAC edges only -- an edge it withdraws is not offered to ICP.
      uint8_t flags[RGBDFE_SLAM_MAX_CANDIDATES];
      memset(flags, 0, sizeof(flags));
      rc = matchnodepair_tail(s, slot, ids, at, n_ids, t, compact, flags);
      if (rc != RGBDFE_OK) return abandon(rc);
      compare_seconds += seconds_since(t0);
      const int32_t n_fed = n_ids;
      rc = rgbdfe_slam_feed(s, compact, flags, n_fed, ids, RGBDFE_SLAM_MAX_CANDIDATES, &n_ids, out);
      if (rc != RGBDFE_OK) return abandon(rc);
      std::lock_guard<std::mutex> l(s->mu);
      const rgbdfe_slam_step& st = s->m.st;   // (kept by the machine until the next step begins)
      for (int32_t k = 0; k < n_fed; ++k) {
        const int v = initial ? st.initial_verdict : st.verdicts[k];
        if (at[k] >= 0 && v == RGBDFE_SLAM_VERDICT_ACCEPTED && s->h_records[at[k]].n_inl > 0) { accept[at[k]] = 1; any = true; }
      }
    }
    // updateInlierFeatures for what the machine accepted, from the records where they lie -- before the step releases a slot
    int32_t launched = 0;
    if (any) {
      const int32_t first = accept[0] ? 0 : 1;
      rc = rgbdfe_update_inlier_features(ctx, static_cast<rgbdfe_match_result*>(s->d_records) + first, q + first, t + first,
                                         accept + first, n_rec - first, &launched);
      if (rc != RGBDFE_OK) return abandon(rc);
    }
    {
      std::lock_guard<std::mutex> l(s->mu);
      s->defer_apply = false;
      rc = apply_step(s, out);
      if (rc != RGBDFE_OK) return rc;
    }
    out->seconds[1] = compare_seconds;
    out->stats_launches = launched;
    return RGBDFE_OK;
  });
}

int rgbdfe_slam_node_count(const rgbdfe_slam* s) { return s ? (int)s->m.slot_of.size() : RGBDFE_ERR_INVALID_ARG; }

int rgbdfe_slam_slot_of(const rgbdfe_slam* s, int32_t id) {
  if (!s) return RGBDFE_ERR_UNKNOWN_NODE;
  if (id < 0 || (size_t)id >= s->m.slot_of.size()) return RGBDFE_ERR_UNKNOWN_NODE;
  return s->m.slot_of[(size_t)id];
}

int rgbdfe_slam_valid_tf(const rgbdfe_slam* s, int32_t id) {
  if (!s) return RGBDFE_ERR_INVALID_ARG;
  if (id < 0 || (size_t)id >= s->m.valid_tf.size()) return RGBDFE_ERR_UNKNOWN_NODE;
  return s->m.valid_tf[(size_t)id];
}

int rgbdfe_slam_keyframes(const rgbdfe_slam* s, int32_t* ids, int32_t capacity, int32_t* n_out) {
  if (!s || !n_out || capacity < 0 || (capacity > 0 && !ids)) return RGBDFE_ERR_INVALID_ARG;
  *n_out = (int32_t)s->m.keyframes.size();
  if (*n_out > capacity) return RGBDFE_ERR_CAPACITY;
  for (int32_t k = 0; k < *n_out; ++k) ids[k] = s->m.keyframes[(size_t)k];
  return RGBDFE_OK;
}

int rgbdfe_sizeof_slam_step(void) { return (int)sizeof(rgbdfe_slam_step); }

int rgbdfe_slam_serialize(rgbdfe_slam* s, uint8_t* out, int64_t capacity, int64_t* bytes) {
  return slam_guarded([&]() -> int {
    if (!s || !bytes || capacity < 0 || (capacity > 0 && !out)) return slam_fail(s, RGBDFE_ERR_INVALID_ARG, "slam state: bad arguments");
    std::vector<uint8_t> b;
    {
      std::lock_guard<std::mutex> l(s->mu);
      if (s->m.phase != rgbdfe_slam_machine::Machine::kIdle)
        return slam_fail(s, RGBDFE_ERR_INVALID_ARG, "slam state: busy: a step is in flight (between rgbdfe_slam_begin and the last rgbdfe_slam_feed)");
      rgbdfe_session::slam_serialize(s->m, b);
    }
    *bytes = (int64_t)b.size();
    if ((int64_t)b.size() > capacity) return slam_fail(s, RGBDFE_ERR_CAPACITY, "slam state: capacity below the string's length (*bytes holds it)");
    std::copy(b.begin(), b.end(), out);
    return RGBDFE_OK;
  });
}

int rgbdfe_slam_deserialize(rgbdfe_slam* s, const uint8_t* in, int64_t bytes) {
  return slam_guarded([&]() -> int { return rgbdfe_host::slam_deserialize(s, in, bytes, true); });
}

}  // extern "C"

namespace rgbdfe_host {
int slam_fail(rgbdfe_slam* s, int code, const std::string& msg) {
  rgbdfe_session::contextless_error() = msg;
  return (s && s->ctx) ? fail(s->ctx, code, msg) : code;
}
// everything rgbdfe_slam_deserialize checks; the object changes only with `commit` and only when nothing was wrong
int slam_deserialize(rgbdfe_slam* s, const uint8_t* in, int64_t bytes, bool commit) {
  if (!s || !in || bytes < 0) return slam_fail(s, RGBDFE_ERR_INVALID_ARG, "slam state: bad arguments");
  rgbdfe_session::SlamImage img;
  const std::string err = rgbdfe_session::slam_parse(in, (size_t)bytes, img);
  if (!err.empty()) return slam_fail(s, RGBDFE_ERR_INVALID_ARG, err);
  std::lock_guard<std::mutex> l(s->mu);
  if (!rgbdfe_session::slam_is_fresh(s->m))
    return slam_fail(s, RGBDFE_ERR_INVALID_ARG, "slam state: the target of a deserialise must be fresh or reset (rgbdfe_slam_reset)");
  if (const char* field = rgbdfe_session::slam_params_differ(s->m.prm, img.prm))
    return slam_fail(s, RGBDFE_ERR_INVALID_ARG, std::string("slam state: the object's parameters differ from the stored ones: ") + field);
  if (commit) rgbdfe_session::slam_commit(s->m, img);
  return RGBDFE_OK;
}
rgbdfe_ctx* slam_context(rgbdfe_slam* s) { return s->ctx; }
rgbdfe_pose_graph* slam_graph(rgbdfe_slam* s) { return s->m.g; }
}  // namespace rgbdfe_host
