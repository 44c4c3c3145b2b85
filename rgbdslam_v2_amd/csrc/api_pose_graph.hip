// api_pose_graph.hip -- pose-graph optimisation, host side: GraphManager::optimizeGraphImpl (graph_manager.cpp:938-1066)
// over the kernels of pose_graph.hip.  Per call the host builds the plan (free-vertex map, incidence and block lists, all in
// insertion order), uploads it with the estimates and the edges in one copy, drives Levenberg-Marquardt (the scalars of a
// trial come back in one small record per chunk of PCG iterations) and reads the estimates back once at the end.
// Then the reference's last stage on the same graph (include/rgbdfe.h, "fixation strategies, pruning and the evaluation rounds"):
// the pose_relative_to flags around optimize_graph, per-edge figures, pruneEdgesWithErrorAbove (one launch and one read-back
// per call; the host owns the topology and mirrors the verdicts into its edges) and the rounds of OpenNIListener::evaluation.
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"
#include "pose_graph.h"
#include "pose_graph_host.h"

#include <cfloat>
#include <chrono>
#include <map>

namespace impl {

namespace {

struct PgDevice {  // belongs to the graph object: one allocation, grown when a call needs more
  int device_id = 0;
  void* blob = nullptr;
  size_t bytes = 0;
};

void pg_device_free(void* p) {
  PgDevice* d = static_cast<PgDevice*>(p);
  if (d->blob) {
    (void)hipSetDevice(d->device_id);
    (void)hipFree(d->blob);
  }
  delete d;
}

constexpr int32_t kPcgFirstChunk = 8, kPcgMaxChunk = 64;  // PCG iterations enqueued before the first / any read-back
constexpr int kMaxTrials = 10;

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

struct PgRun {  // one call's problem on the device; ctx->mu is held while it lives
  rgbdfe_ctx* ctx = nullptr;
  rgbdfe_pose_graph* g = nullptr;
  hipStream_t st = nullptr;
  PgProblem P{};
  double* est[2] = {nullptr, nullptr};
  int cur = 0;
  std::vector<int32_t> node_of;              // vertex -> node id
  std::vector<int32_t> free_of, vert_of, blk_rc;
  PgScalars hs{};
  const std::vector<uint8_t>* topo = nullptr;  // a prune call's topology bits: uploaded with room for its results
  uint8_t* d_topo = nullptr;
  double* d_edge_in = nullptr;
  int32_t* d_active = nullptr;
  int32_t* d_prune_out = nullptr;              // the count, then a verdict byte per edge
  int32_t n_active = 0;                        // measured edges that still take part
  int64_t launches = 0, readbacks = 0;
  double upload_seconds = 0;

  int read_scalars() {
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&hs, P.s, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ++readbacks;
    return RGBDFE_OK;
  }

  // the plan, the edges and the estimates onto the device
  int setup() {
    const auto t0 = std::chrono::steady_clock::now();
    std::map<int32_t, int32_t> vertex_of;  // node id -> vertex
    std::vector<double> est_h;
    for (const auto& kv : g->nodes) {
      vertex_of[kv.first] = (int32_t)node_of.size();
      node_of.push_back(kv.first);
      free_of.push_back(kv.second.fixed ? -1 : (int32_t)vert_of.size());
      if (!kv.second.fixed) vert_of.push_back((int32_t)node_of.size() - 1);
      est_h.insert(est_h.end(), kv.second.est, kv.second.est + 12);
    }
    const size_t nv = node_of.size(), nf = vert_of.size(), ne = g->edges.size();
    std::vector<int32_t> edge_ij(2 * ne), edge_active(ne);
    std::vector<double> edge_in((size_t)kPgEdgeIn * ne);
    std::vector<std::vector<int32_t>> vert_list(nf), blk_list, vb_list(nf);
    std::map<std::pair<int32_t, int32_t>, int32_t> block_at;
    for (size_t e = 0; e < ne; ++e) {
      const rgbdfe_pose_graph::MeasuredEdge& m = g->edges[e];
      const int32_t vi = vertex_of.at(m.id1), vj = vertex_of.at(m.id2);
      edge_ij[2 * e] = vi;
      edge_ij[2 * e + 1] = vj;
      std::copy(m.z, m.z + 12, edge_in.begin() + kPgEdgeIn * e);
      std::copy(m.info, m.info + 36, edge_in.begin() + kPgEdgeIn * e + kPgPose);
      edge_active[e] = m.active ? 1 : 0;
      if (!m.active) continue;  // a pruned edge is in no list
      ++n_active;
      const int32_t fi = free_of[vi], fj = free_of[vj];
      if (fi >= 0) vert_list[fi].push_back((int32_t)(2 * e));
      if (fj >= 0) vert_list[fj].push_back((int32_t)(2 * e + 1));
      if (fi < 0 || fj < 0) continue;
      const std::pair<int32_t, int32_t> key(std::min(fi, fj), std::max(fi, fj));
      auto at = block_at.find(key);
      if (at == block_at.end()) {
        at = block_at.emplace(key, (int32_t)blk_list.size()).first;
        blk_rc.push_back(key.first);
        blk_rc.push_back(key.second);
        vb_list[key.first].push_back(2 * (int32_t)blk_list.size());
        vb_list[key.second].push_back(2 * (int32_t)blk_list.size() + 1);
        blk_list.emplace_back();
      }
      blk_list[at->second].push_back((int32_t)(2 * e) + (fi > fj ? 1 : 0));
    }
    const size_t nb = blk_list.size();
    auto csr = [](const std::vector<std::vector<int32_t>>& lists, std::vector<int32_t>* ptr, std::vector<int32_t>* items) {
      ptr->assign(1, 0);
      for (const auto& l : lists) {
        items->insert(items->end(), l.begin(), l.end());
        ptr->push_back((int32_t)items->size());
      }
    };
    std::vector<int32_t> vert_ptr, vert_items, blk_ptr, blk_items, vb_ptr, vb_items;
    csr(vert_list, &vert_ptr, &vert_items);
    csr(blk_list, &blk_ptr, &blk_items);
    csr(vb_list, &vb_ptr, &vb_items);

    // the layout: the uploaded part first (one copy), then the working arrays
    DeviceLayout lay;
    auto put = [&lay](const void* src, size_t bytes) { return lay.put(src, bytes); };
    auto room = [&lay](size_t bytes) { return lay.room(bytes); };
    const Block o_est = put(est_h.data(), 8 * est_h.size()), o_free = put(free_of.data(), 4 * nv),
                 o_vert = put(vert_of.data(), 4 * nf), o_ij = put(edge_ij.data(), 4 * edge_ij.size()),
                 o_in = put(edge_in.data(), 8 * edge_in.size()), o_vp = put(vert_ptr.data(), 4 * vert_ptr.size()),
                 o_vi = put(vert_items.data(), 4 * vert_items.size()), o_bp = put(blk_ptr.data(), 4 * blk_ptr.size()),
                 o_bi = put(blk_items.data(), 4 * blk_items.size()), o_vbp = put(vb_ptr.data(), 4 * vb_ptr.size()),
                 o_vbi = put(vb_items.data(), 4 * vb_items.size()), o_rc = put(blk_rc.data(), 4 * blk_rc.size());
    PgScalars zero{};
    const Block o_s = put(&zero, sizeof(zero)), o_act = put(edge_active.data(), 4 * ne);
    const Block o_topo = put(topo ? topo->data() : nullptr, topo ? ne : 0), o_po = put(nullptr, topo ? 4 + ne : 0);
    const size_t leaves = std::max((ne + kPgTile - 1) / kPgTile, (nf + kPgTile - 1) / kPgTile) + 1;
    const Block o_est1 = room(8 * est_h.size()), o_out = room(8 * (size_t)kPgEdgeOut * ne), o_Hd = room(8 * 36 * nf),
                 o_B = room(8 * 36 * nb), o_b = room(8 * 6 * nf), o_L = room(8 * 36 * nf), o_x = room(8 * 6 * nf),
                 o_r = room(8 * 6 * nf), o_z = room(8 * 6 * nf), o_p = room(8 * 6 * nf), o_q = room(8 * 6 * nf),
                 o_pa = room(8 * leaves), o_pb = room(8 * leaves);
    const size_t total = lay.total();

    PgDevice* d = static_cast<PgDevice*>(g->device);
    if (!d) {
      d = new PgDevice();
      g->device = d;
      g->device_free = pg_device_free;
    }
    if (d->bytes < total || d->device_id != ctx->cfg.device_id) {
      if (d->blob) {
        (void)hipSetDevice(d->device_id);
        (void)hipFree(d->blob);
        HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
      }
      d->blob = nullptr;
      d->bytes = 0;
      d->device_id = ctx->cfg.device_id;
      if (hipMalloc(&d->blob, total) != hipSuccess) {
        (void)hipGetLastError();
        d->blob = nullptr;
        return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "pose graph: device allocation failed");
      }
      d->bytes = total;
    }
    void* base = d->blob;
    auto f64 = [base](Block b) { return at<double>(base, b); };
    auto i32 = [base](Block b) { return at<int32_t>(base, b); };
    est[0] = f64(o_est);
    est[1] = f64(o_est1);
    HIP_TRY(ctx, hipMemcpyAsync(base, lay.staged(), lay.staged_bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(est[1], est[0], 8 * est_h.size(), hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));  // the staging vector goes out of scope; and the upload's share is timed
    P.n_vert = (int32_t)nv; P.n_free = (int32_t)nf; P.n_edge = (int32_t)ne; P.n_block = (int32_t)nb;
    P.free_of = i32(o_free); P.vert_of = i32(o_vert);
    P.edge_ij = i32(o_ij); P.edge_in = f64(o_in);
    P.edge_out = f64(o_out);
    d_edge_in = f64(o_in); d_active = i32(o_act); P.edge_active = d_active;
    d_topo = at<uint8_t>(base, o_topo); d_prune_out = i32(o_po);
    P.vert_ptr = i32(o_vp); P.vert_items = i32(o_vi);
    P.blk_ptr = i32(o_bp); P.blk_items = i32(o_bi);
    P.vb_ptr = i32(o_vbp); P.vb_items = i32(o_vbi);
    P.blk_rc = i32(o_rc);
    P.Hd = f64(o_Hd); P.B = f64(o_B); P.b = f64(o_b); P.L = f64(o_L);
    P.x = f64(o_x); P.r = f64(o_r); P.z = f64(o_z); P.p = f64(o_p);
    P.q = f64(o_q); P.part_a = f64(o_pa); P.part_b = f64(o_pb);
    P.s = at<PgScalars>(base, o_s);
    upload_seconds = seconds_since(t0);
    return RGBDFE_OK;
  }

  int chi2_now(double* out) {
    if (P.n_edge == 0) { *out = 0.0; return RGBDFE_OK; }
    launches += launch_pg_edges(P, est[cur], false, st);
    launches += launch_pg_chi2(P, st);
    const int rc = read_scalars();
    *out = hs.chi2;
    return rc;
  }

  // the estimates back into the graph object
  int finish() {
    std::vector<double> h((size_t)kPgPose * node_of.size());
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), est[cur], 8 * h.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ++readbacks;
    size_t v = 0;
    for (auto& kv : g->nodes) {
      std::copy(h.begin() + kPgPose * v, h.begin() + kPgPose * (v + 1), kv.second.est);
      ++v;
    }
    return RGBDFE_OK;
  }
};

void append(rgbdfe_pose_graph_report* rep, const rgbdfe_pose_graph_iteration& it) {
  if (rep->recorded < RGBDFE_POSE_GRAPH_REPORT_ITERATIONS) rep->it[rep->recorded++] = it;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg on the set-up problem; *done = iterations run
int optimize_run(PgRun& run, int32_t iterations, rgbdfe_pose_graph_report* rep, int32_t* done) {
  const PgProblem& P = run.P;
  *done = 0;
  if (run.n_active == 0 || P.n_free == 0) return run.chi2_now(&rep->chi2);
  const int32_t max_iter = 6 * P.n_free;
  double lambda = 0.0, ni = 2.0;
  for (int32_t it = 0; it < iterations; ++it) {
    run.launches += launch_pg_edges(P, run.est[run.cur], true, run.st);
    run.launches += launch_pg_gather(P, run.st);
    int rc = run.read_scalars();
    if (rc != RGBDFE_OK) return rc;
    double cur = run.hs.chi2;
    if (it == 0) {
      lambda = 1e-5 * run.hs.max_diag;
      ni = 2.0;
    }
    rgbdfe_pose_graph_iteration rec{};
    rec.chi2_before = cur;
    double rho = 0.0;
    int qmax = 0;
    do {
      run.launches += launch_pg_pcg_begin(P, lambda, max_iter, run.st);
      int32_t next = 0, chunk = kPcgFirstChunk;
      for (;;) {
        run.launches += launch_pg_pcg_iterations(P, lambda, next, chunk, max_iter, run.st);
        next += chunk;
        run.launches += launch_pg_trial(P, lambda, next, run.est[run.cur], run.est[1 - run.cur], run.st);
        rc = run.read_scalars();
        if (rc != RGBDFE_OK) return rc;
        if (run.hs.applied) break;
        if (next > max_iter) return fail(run.ctx, RGBDFE_ERR_INTERNAL, "pose graph: PCG did not report its stop");
        chunk = std::min(2 * chunk, kPcgMaxChunk);
      }
      const double trial = run.hs.trial_chi2;
      const double scale = run.hs.scale + 1e-3;
      rho = (cur - trial) / scale;
      rec.pcg_iterations[rec.trials++] = run.hs.iters;
      if (rho > 0 && std::isfinite(trial)) {
        run.cur = 1 - run.cur;
        double a = 2.0 * rho - 1.0;
        a = 1.0 - (a * a) * a;
        a = std::min(a, 2.0 / 3.0);
        a = std::max(1.0 / 3.0, a);
        lambda = lambda * a;
        ni = 2.0;
        cur = trial;
      } else {
        lambda = lambda * ni;  // the trial's estimates stay in the other buffer, unused: nothing to restore
        ni = ni * 2.0;
      }
      ++qmax;
    } while (rho < 0 && qmax < kMaxTrials);
    rec.chi2_after = cur;
    rec.lambda = lambda;
    append(rep, rec);
    ++*done;
    if (qmax == kMaxTrials || rho == 0) break;
  }
  rep->iterations += *done;
  return run.chi2_now(&rep->chi2);
}

int begin(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, PgRun* run) {
  run->ctx = ctx;
  run->g = g;
  run->st = ctx->stream;
  return run->setup();
}

void close_report(const PgRun& run, rgbdfe_pose_graph_report* rep, std::chrono::steady_clock::time_point t0) {
  rep->launches = run.launches;
  rep->readbacks = run.readbacks;
  rep->upload_seconds = run.upload_seconds;
  rep->total_seconds = seconds_since(t0);
}

// fixationOfVertices (graph_manager.cpp:911-937), at the start of optimizeGraphImpl
void apply_fixation(rgbdfe_pose_graph* g) {
  auto clear_all = [&]() { for (auto& kv : g->nodes) kv.second.fixed = false; };
  switch (g->strategy) {
    case RGBDFE_POSE_RELATIVE_TO_FIRST:  // the reference indexes graph[0]; here: the node of lowest id
      clear_all();
      if (!g->nodes.empty()) g->nodes.begin()->second.fixed = true;
      break;
    case RGBDFE_POSE_RELATIVE_TO_PREVIOUS:  // graph[size - 2]: the node of second-highest id
      if (g->nodes.size() > 2) {
        clear_all();
        std::next(g->nodes.rbegin())->second.fixed = true;
      }
      break;
    case RGBDFE_POSE_RELATIVE_TO_LARGEST_LOOP:
      for (auto& kv : g->nodes) kv.second.fixed = kv.first < g->earliest_loop_closure_node;
      break;
    default:
      break;  // NONE, INAFFECTED: the flags as they stand
  }
}

// after the optimisation (:1031-1036)
void release_fixation(rgbdfe_pose_graph* g) {
  if (g->strategy == RGBDFE_POSE_RELATIVE_TO_NONE) return;
  const bool fixed = g->strategy == RGBDFE_POSE_RELATIVE_TO_INAFFECTED;
  for (auto& kv : g->nodes) kv.second.fixed = fixed;
}

}  // namespace

int rgbdfe_pose_graph_chi2(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2) {
  if (!ctx || !g || !chi2) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (g->edges.empty()) { *chi2 = 0.0; return RGBDFE_OK; }
  std::lock_guard<std::mutex> lock(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  PgRun run;
  const int rc = begin(ctx, g, &run);
  if (rc != RGBDFE_OK) return rc;
  return run.chi2_now(chi2);
}

int rgbdfe_pose_graph_linearize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* errors, double* weights, int32_t edge_capacity,
                                int32_t* n_edges, int32_t* free_ids, double* h_diag, double* b, int32_t vertex_capacity,
                                int32_t* n_free, int32_t* off_rows, int32_t* off_cols, double* h_off, int32_t block_capacity,
                                int32_t* n_blocks, double* chi2) {
  if (!ctx || !g || !n_edges || !n_free || !n_blocks || edge_capacity < 0 || vertex_capacity < 0 || block_capacity < 0)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> lock(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  PgRun run;
  int rc = begin(ctx, g, &run);
  if (rc != RGBDFE_OK) return rc;
  const PgProblem& P = run.P;
  *n_edges = P.n_edge;
  *n_free = P.n_free;
  *n_blocks = P.n_block;
  if (P.n_edge > edge_capacity || P.n_free > vertex_capacity || P.n_block > block_capacity)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "pose graph: the output arrays are too small (the needed sizes are set)");
  if (chi2) *chi2 = 0.0;
  if (P.n_edge > 0) {
    run.launches += launch_pg_edges(P, run.est[0], true, run.st);
    run.launches += launch_pg_gather(P, run.st);
    rc = run.read_scalars();
    if (rc != RGBDFE_OK) return rc;
    if (chi2) *chi2 = run.hs.chi2;
    std::vector<double> out((size_t)kPgEdgeOut * P.n_edge);
    HIP_TRY(ctx, hipMemcpyAsync(out.data(), P.edge_out, 8 * out.size(), hipMemcpyDeviceToHost, run.st));
    if (h_diag && P.n_free) HIP_TRY(ctx, hipMemcpyAsync(h_diag, P.Hd, 8 * 36 * (size_t)P.n_free, hipMemcpyDeviceToHost, run.st));
    if (b && P.n_free) HIP_TRY(ctx, hipMemcpyAsync(b, P.b, 8 * 6 * (size_t)P.n_free, hipMemcpyDeviceToHost, run.st));
    if (h_off && P.n_block) HIP_TRY(ctx, hipMemcpyAsync(h_off, P.B, 8 * 36 * (size_t)P.n_block, hipMemcpyDeviceToHost, run.st));
    HIP_TRY(ctx, hipStreamSynchronize(run.st));
    for (int32_t e = 0; e < P.n_edge; ++e) {
      if (errors) std::copy(out.begin() + (size_t)kPgEdgeOut * e, out.begin() + (size_t)kPgEdgeOut * e + 6, errors + 6 * (size_t)e);
      if (weights) weights[e] = out[(size_t)kPgEdgeOut * e + kPgW];
      if (!g->edges[(size_t)e].active) {  // a pruned edge wrote no record: error 0, weight 0
        if (errors) std::fill(errors + 6 * (size_t)e, errors + 6 * (size_t)e + 6, 0.0);
        if (weights) weights[e] = 0.0;
      }
    }
  } else {
    if (h_diag) std::fill(h_diag, h_diag + 36 * (size_t)P.n_free, 0.0);
    if (b) std::fill(b, b + 6 * (size_t)P.n_free, 0.0);
  }
  for (int32_t f = 0; f < P.n_free; ++f)
    if (free_ids) free_ids[f] = run.node_of[(size_t)run.vert_of[(size_t)f]];
  for (int32_t n = 0; n < P.n_block; ++n) {
    if (off_rows) off_rows[n] = run.blk_rc[2 * (size_t)n];
    if (off_cols) off_cols[n] = run.blk_rc[2 * (size_t)n + 1];
  }
  return RGBDFE_OK;
}

int rgbdfe_pose_graph_optimize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, int32_t iterations, rgbdfe_pose_graph_report* report) {
  if (!ctx || !g || iterations < 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  const auto t0 = std::chrono::steady_clock::now();
  rgbdfe_pose_graph_report local;
  rgbdfe_pose_graph_report* rep = report ? report : &local;
  memset(rep, 0, sizeof(*rep));
  if (g->edges.empty()) return RGBDFE_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  PgRun run;
  int rc = begin(ctx, g, &run);
  if (rc != RGBDFE_OK) return rc;
  int32_t done = 0;
  rc = optimize_run(run, iterations, rep, &done);
  if (rc != RGBDFE_OK) return rc;
  rc = run.finish();
  close_report(run, rep, t0);
  return rc;
}

int rgbdfe_pose_graph_optimize_graph(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double break_criterion,
                                     rgbdfe_pose_graph_report* report) {
  if (!ctx || !g || !std::isfinite(break_criterion) || break_criterion > 1e9)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  const auto t0 = std::chrono::steady_clock::now();
  rgbdfe_pose_graph_report local;
  rgbdfe_pose_graph_report* rep = report ? report : &local;
  memset(rep, 0, sizeof(*rep));
  apply_fixation(g);
  struct Release {  // the flags after the optimisation, on every way out
    rgbdfe_pose_graph* g;
    ~Release() { release_fixation(g); }
  } release{g};
  if (g->edges.empty()) return RGBDFE_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  PgRun run;
  int rc = begin(ctx, g, &run);  // one upload: the calls of the loop go on from the estimates on the device
  if (rc != RGBDFE_OK) return rc;
  int32_t done = 0;
  if (break_criterion >= 1.0) {  // a number of iterations, in at most ten steps (graph_manager.cpp:998-1003)
    const int32_t step = (int32_t)std::ceil(break_criterion / 10.0);
    int64_t total = 0;
    do {
      rc = optimize_run(run, step, rep, &done);
      if (rc != RGBDFE_OK) return rc;
      total += done;
    } while ((double)total < break_criterion && done > 0);
  } else {                       // to convergence (:1006-1013)
    double value = DBL_MAX, prev;
    do {
      prev = value;
      rc = optimize_run(run, 5, rep, &done);
      if (rc != RGBDFE_OK) return rc;
      value = rep->chi2;
    } while (done > 0 && value / prev < (1.0 - break_criterion));
  }
  rc = run.finish();
  close_report(run, rep, t0);
  return rc;
}

int rgbdfe_pose_graph_edge_errors(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2, double* err_sq, int32_t* active,
                                  int32_t capacity, int32_t* n_edges) {
  if (!ctx || !g || !n_edges || capacity < 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  const size_t ne = g->edges.size();
  *n_edges = (int32_t)ne;
  if (ne > (size_t)capacity) return fail(ctx, RGBDFE_ERR_CAPACITY, "pose graph: the output arrays are too small (the count is set)");
  if (ne == 0) return RGBDFE_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  PgRun run;
  const int rc = begin(ctx, g, &run);
  if (rc != RGBDFE_OK) return rc;
  run.launches += launch_pg_edges(run.P, run.est[0], false, run.st);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> head(7 * ne);  // e[6], chi2 of every record
  HIP_TRY(ctx, hipMemcpy2DAsync(head.data(), 7 * sizeof(double), run.P.edge_out, kPgEdgeOut * sizeof(double), 7 * sizeof(double), ne,
                                hipMemcpyDeviceToHost, run.st));
  HIP_TRY(ctx, hipStreamSynchronize(run.st));
  for (size_t e = 0; e < ne; ++e) {
    const bool on = g->edges[e].active;
    const double* h = head.data() + 7 * e;
    double sq = h[0] * h[0];
    for (int k = 1; k < 6; ++k) sq = sq + h[k] * h[k];
    if (chi2) chi2[e] = on ? h[kPgChi2] : 0.0;
    if (err_sq) err_sq[e] = on ? sq : 0.0;
    if (active) active[e] = on ? 1 : 0;
  }
  return RGBDFE_OK;
}

namespace {

// one prune call; stats (may be NULL) takes its launches, read-backs and upload time
int prune_run(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, float thresh, uint8_t* verdicts, int32_t* n_pruned, PgRun* stats) {
  const size_t ne = g->edges.size();
  *n_pruned = 0;
  if (ne == 0) return RGBDFE_OK;
  // the topology is the host's: the degree counts every measured edge ever added, pruned ones included (the reference erases
  // an edge from cam_cam_edges_ only, never from the optimiser: v->edges().size() does not shrink)
  std::map<int32_t, int32_t> degree;
  for (const auto& m : g->edges) { ++degree[m.id1]; ++degree[m.id2]; }
  std::vector<uint8_t> topo(ne);
  for (size_t e = 0; e < ne; ++e) {
    const auto& m = g->edges[e];
    const int64_t d = (int64_t)m.id1 - (int64_t)m.id2;
    topo[e] = (uint8_t)(((d == 1 || d == -1) ? kPgTopoSequential : 0) |
                        ((degree[m.id1] > 1 && degree[m.id2] > 1) ? kPgTopoBothJoined : 0));
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  PgRun run;
  run.topo = &topo;
  const int rc = begin(ctx, g, &run);
  if (rc != RGBDFE_OK) return rc;
  run.launches += launch_pg_prune(run.P, run.est[0], (double)thresh, run.d_topo, run.d_edge_in, run.d_active,
                                  (uint8_t*)(run.d_prune_out + 1), run.d_prune_out, run.st);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<uint8_t> back(4 + ne);  // the one read-back: the count and the verdict bytes
  HIP_TRY(ctx, hipMemcpyAsync(back.data(), run.d_prune_out, back.size(), hipMemcpyDeviceToHost, run.st));
  HIP_TRY(ctx, hipStreamSynchronize(run.st));
  ++run.readbacks;
  memcpy(n_pruned, back.data(), 4);
  for (size_t e = 0; e < ne; ++e) {  // the host's copy of the edges follows the device's
    const uint8_t v = back[4 + e];
    verdicts[e] = v;
    if (v == kPgPruneKept) continue;
    auto& m = g->edges[e];
    for (int k = 0; k < kPgPose; ++k) m.z[k] = (k < 9 && k % 4 == 0) ? 1.0 : 0.0;
    if (v == kPgPruneRemoved) {
      m.active = false;
    } else {
      const double diag = v == kPgPruneDiscounted ? 1e-100 : 1.0;
      for (int k = 0; k < 36; ++k) m.info[k] = (k % 7 == 0) ? diag : 0.0;
    }
  }
  if (stats) {
    stats->launches = run.launches;
    stats->readbacks = run.readbacks;
    stats->upload_seconds = run.upload_seconds;
  }
  return RGBDFE_OK;
}

}  // namespace

int rgbdfe_pose_graph_prune_edges(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, float thresh, uint8_t* verdicts, int32_t capacity,
                                  int32_t* n_pruned) {
  if (!ctx || !g || !n_pruned || capacity < 0 || thresh != thresh) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (g->edges.size() > (size_t)capacity) {
    *n_pruned = (int32_t)g->edges.size();
    return fail(ctx, RGBDFE_ERR_CAPACITY, "pose graph: the verdict array is too small (the edge count is set)");
  }
  std::vector<uint8_t> local(verdicts ? 0 : g->edges.size());
  return prune_run(ctx, g, thresh, verdicts ? verdicts : local.data(), n_pruned, nullptr);
}

int rgbdfe_pose_graph_evaluate(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double optimizer_iterations,
                               rgbdfe_pose_graph_evaluation* out, double* estimates, int32_t capacity_nodes) {
  if (!ctx || !g || !std::isfinite(optimizer_iterations) || optimizer_iterations > 1e9 || capacity_nodes < 0)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  const size_t nn = g->nodes.size();
  if (estimates && nn > (size_t)capacity_nodes)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "pose graph: the estimates array is too small");
  rgbdfe_pose_graph_evaluation local;
  rgbdfe_pose_graph_evaluation* ev = out ? out : &local;
  memset(ev, 0, sizeof(*ev));
  static const float kThresh[RGBDFE_POSE_GRAPH_EVALUATION_ROUNDS] = {0.f, 0.f, 5.0f, 1.0f, 0.25f};
  std::vector<uint8_t> verdicts(g->edges.size());
  for (int r = 0; r < RGBDFE_POSE_GRAPH_EVALUATION_ROUNDS; ++r) {  // the calls of OpenNIListener::evaluation, one after another
    const auto t0 = std::chrono::steady_clock::now();
    rgbdfe_pose_graph_round& rd = ev->round[r];
    double criterion = optimizer_iterations;
    if (r == 1) g->strategy = RGBDFE_POSE_RELATIVE_TO_FIRST;  // and it stays
    if (r >= 2) {
      PgRun stats;
      const int rc = prune_run(ctx, g, kThresh[r], verdicts.data(), &rd.pruned, &stats);
      if (rc != RGBDFE_OK) return rc;
      rd.launches = stats.launches;
      rd.readbacks = stats.readbacks;
      rd.upload_seconds = stats.upload_seconds;
      if (rd.pruned == 0) criterion = 1.0;
    }
    rgbdfe_pose_graph_report rep;
    const int rc = impl::rgbdfe_pose_graph_optimize_graph(ctx, g, criterion, &rep);
    if (rc != RGBDFE_OK) return rc;
    rd.chi2 = rep.chi2;
    rd.iterations = rep.iterations;
    rd.launches += rep.launches;
    rd.readbacks += rep.readbacks;
    rd.upload_seconds += rep.upload_seconds;
    rd.seconds = seconds_since(t0);
    if (estimates) {
      double* dst = estimates + 16 * nn * (size_t)r;
      for (const auto& kv : g->nodes) {
        const double* est = kv.second.est;
        for (int a = 0; a < 3; ++a) {
          for (int c = 0; c < 3; ++c) dst[4 * c + a] = est[3 * a + c];
          dst[12 + a] = est[9 + a];
          dst[4 * a + 3] = 0.0;
        }
        dst[15] = 1.0;
        dst += 16;
      }
    }
  }
  return RGBDFE_OK;
}

}  // namespace impl
