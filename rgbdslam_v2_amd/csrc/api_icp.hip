// api_icp.hip -- the ICP fallback, host side: filterCloud and icpAlignment (icp.cpp:20-89) over the kernels of icp.hip.
// A call counts and scans the valid rows of every distinct cloud it names (one read-back: the counts), computes the sample
// positions with filterCloud's float recurrence, gathers the samples, and then drives all jobs together: two launches per
// iteration, enqueued in chunks of 2, 4, 8, 16, 16 ... with one read of the jobs' records per chunk.
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"
#include "icp.h"

#include <cfloat>

namespace impl {

namespace {

constexpr int32_t kIcpFirstChunk = 2, kIcpMaxChunk = 16;  // iterations enqueued before the first / any read-back
constexpr int64_t kIcpMaxRows = 1ll << 24;                // filterCloud's float index is exact up to here
constexpr int32_t kIcpMaxJobs = 65535;                    // the jobs are a grid dimension

struct CloudRef {   // a cloud on the device
  const float4* d;
  uint32_t n;
};
struct JobRef {
  int source, target;   // indices into the call's cloud list
  float G[16];
};

int ensure_icp(rgbdfe_ctx* ctx, size_t bytes) { return ctx->icp.ensure(ctx, bytes, "icp: device allocation failed"); }

// the events of a profiled chunk: back in the context's pool when the chunk ends, however it ends
struct ChunkEvents {
  rgbdfe_ctx* ctx;
  std::vector<hipEvent_t> ev;
  explicit ChunkEvents(rgbdfe_ctx* c) : ctx(c) {}
  ~ChunkEvents() { ctx->event_pool.insert(ctx->event_pool.end(), ev.begin(), ev.end()); }
  ChunkEvents(const ChunkEvents&) = delete;
  ChunkEvents& operator=(const ChunkEvents&) = delete;
};

// filterCloud's loop (icp.cpp:34-38): the positions in the list of valid rows
std::vector<uint32_t> sample_positions(uint32_t n_valid, int32_t desired_size) {
  std::vector<uint32_t> pos;
  float step = (float)n_valid / static_cast<float>(desired_size);
  step = step < 1.0 ? 1.0 : step;
  for (float i = 0; i < (float)n_valid; i += step) pos.push_back(static_cast<unsigned int>(i));
  return pos;
}

int check_params(rgbdfe_ctx* ctx, const rgbdfe_icp_params* p) {
  if (!p) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "icp: params is NULL");
  if (std::isnan(p->max_correspondence_distance) || std::isnan(p->transformation_epsilon) ||
      std::isnan(p->euclidean_fitness_epsilon) || p->max_correspondence_distance < 0.0)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "icp: a NaN parameter or a negative max_correspondence_distance");
  if (p->max_iterations < 1 || p->max_iterations > 1000)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "icp: max_iterations outside 1 .. 1000");
  if (p->desired_size <= 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "icp: desired_size <= 0");
  return RGBDFE_OK;
}

// One call on the device.  ctx->mu is held.  `host_clouds` (may be empty) are uploaded behind the table and take the
// place of the entries of `clouds` whose pointer is NULL, in order.  filter() stops behind the gather
// (rgbdfe_filter_cloud): the samples of cloud 0 go to rows_out / indices_out.
struct IcpCall {
  rgbdfe_ctx* ctx = nullptr;
  hipStream_t st = nullptr;
  std::vector<CloudRef> clouds;
  std::vector<const float*> host_clouds;
  std::vector<JobRef> jobs;
  int32_t desired_size = 0;
  int64_t launches = 0, readbacks = 0;
  // after compact()
  std::vector<IcpCloud> table;
  std::vector<std::vector<uint32_t>> pos;
  IcpCloud* d_table = nullptr;
  uint32_t* d_tile_first = nullptr;

  // phase 1, in the context's scratch: the table, the tile counts and offsets; uploaded host clouds behind them
  int compact() {
    const size_t nc = clouds.size();
    table.assign(nc, IcpCloud{});
    size_t tiles = 0, host_rows = 0;
    uint32_t max_tiles = 0;
    for (size_t c = 0; c < nc; ++c) {
      const uint32_t t = (clouds[c].n + (uint32_t)kIcpScanTile - 1u) / (uint32_t)kIcpScanTile;
      table[c].n = clouds[c].n;
      table[c].first_tile = (uint32_t)tiles;
      tiles += t;
      if (!clouds[c].d) host_rows += clouds[c].n;
      max_tiles = std::max(max_tiles, t);
    }
    DeviceLayout lay;
    const Block o_table = lay.room(sizeof(IcpCloud) * nc), o_count = lay.room(4 * tiles), o_first = lay.room(4 * tiles),
                o_nvalid = lay.room(4 * nc), o_host = lay.room(16 * host_rows);
    int rc = ensure_scratch(ctx, lay.total());
    if (rc != RGBDFE_OK) return rc;
    void* base = ctx->d_scratch;
    size_t at_host = 0, h = 0;
    for (size_t c = 0; c < nc; ++c) {
      if (clouds[c].d) {
        table[c].d = clouds[c].d;
      } else {
        float4* d = at<float4>(base, o_host) + at_host;
        table[c].d = d;
        if (clouds[c].n) HIP_TRY(ctx, hipMemcpyAsync(d, host_clouds[h], 16 * (size_t)clouds[c].n, hipMemcpyHostToDevice, st));
        at_host += clouds[c].n;
        ++h;
      }
    }
    d_table = at<IcpCloud>(base, o_table);
    HIP_TRY(ctx, hipMemcpyAsync(d_table, table.data(), sizeof(IcpCloud) * nc, hipMemcpyHostToDevice, st));
    uint32_t* d_nvalid = at<uint32_t>(base, o_nvalid);
    d_tile_first = at<uint32_t>(base, o_first);
    launches += launch_icp_compact(d_table, (uint32_t)nc, max_tiles, at<uint32_t>(base, o_count), d_tile_first, d_nvalid, st);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint32_t> n_valid(nc);
    HIP_TRY(ctx, hipMemcpyAsync(n_valid.data(), d_nvalid, 4 * nc, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ++readbacks;
    pos.resize(nc);
    for (size_t c = 0; c < nc; ++c) {
      if (n_valid[c] > clouds[c].n) return fail(ctx, RGBDFE_ERR_INTERNAL, "icp: more valid rows than rows");
      pos[c] = sample_positions(n_valid[c], desired_size);
      table[c].n_samples = (uint32_t)pos[c].size();
    }
    return RGBDFE_OK;
  }

  int filter(int32_t* indices_out, float* rows_out, int64_t capacity, int64_t* n_out) {
    int rc = compact();
    if (rc != RGBDFE_OK) return rc;
    const size_t ns = pos[0].size();
    *n_out = (int64_t)ns;
    if ((int64_t)ns > capacity) return fail(ctx, RGBDFE_ERR_CAPACITY, "filter_cloud: the outputs are too small (*n_out rows are needed)");
    if (ns == 0) return RGBDFE_OK;
    DeviceLayout lay;
    const Block o_pos = lay.room(4 * ns), o_rows = lay.room(16 * ns), o_idx = lay.room(4 * ns);
    rc = ensure_icp(ctx, lay.total());
    if (rc != RGBDFE_OK) return rc;
    void* base = ctx->icp.p;
    table[0].pos = at<uint32_t>(base, o_pos);
    table[0].samples = at<float4>(base, o_rows);
    table[0].sample_index = at<uint32_t>(base, o_idx);
    table[0].poison = 0;
    HIP_TRY(ctx, hipMemcpyAsync(at<uint32_t>(base, o_pos), pos[0].data(), 4 * ns, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_table, table.data(), sizeof(IcpCloud), hipMemcpyHostToDevice, st));
    launches += launch_icp_gather(d_table, 1, (uint32_t)ns, d_tile_first, st);
    HIP_TRY(ctx, hipGetLastError());
    if (rows_out) HIP_TRY(ctx, hipMemcpyAsync(rows_out, table[0].samples, 16 * ns, hipMemcpyDeviceToHost, st));
    if (indices_out) HIP_TRY(ctx, hipMemcpyAsync(indices_out, table[0].sample_index, 4 * ns, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ++readbacks;
    return RGBDFE_OK;
  }

  int align(const rgbdfe_icp_params& prm, float* transforms_out, rgbdfe_icp_report* reports_out, int32_t* nn_index_out,
            float* nn_d2_out, int64_t debug_capacity) {
    int rc = compact();
    if (rc != RGBDFE_OK) return rc;
    const size_t nc = clouds.size(), nj = jobs.size();
    if ((nn_index_out || nn_d2_out) && (int64_t)pos[(size_t)jobs[0].source].size() > debug_capacity)
      return fail(ctx, RGBDFE_ERR_CAPACITY, "icp: debug_capacity is below the sampled source count");
    // phase 2: the uploaded part first (positions, jobs, records: one copy), then the working arrays
    DeviceLayout lay;
    std::vector<Block> o_pos(nc), o_samples(nc);
    for (size_t c = 0; c < nc; ++c) o_pos[c] = lay.put(pos[c].data(), 4 * pos[c].size());
    std::vector<IcpJob> job_h(nj);
    std::vector<IcpRecord> rec_h(2 * nj);
    memset(rec_h.data(), 0, sizeof(IcpRecord) * rec_h.size());
    uint32_t max_ns = 0, max_samples = 0;
    for (size_t j = 0; j < nj; ++j) {
      IcpJob& jb = job_h[j];
      memset(&jb, 0, sizeof(jb));
      rigid_of_matrix4f(jobs[j].G, jb.GR, jb.Gt);
      jb.ns = (int32_t)pos[(size_t)jobs[j].source].size();
      jb.nt = (int32_t)pos[(size_t)jobs[j].target].size();
      max_ns = std::max(max_ns, (uint32_t)jb.ns);
      IcpRecord& r0 = rec_h[2 * j];
      r0.mse = DBL_MAX;
      for (int a = 0; a < 9; ++a) {
        r0.R[a] = (a % 4 == 0) ? 1.0f : 0.0f;
        r0.FR[a] = jb.GR[a];
      }
      for (int a = 0; a < 3; ++a) r0.Ft[a] = jb.Gt[a];
    }
    const Block o_jobs = lay.put(job_h.data(), sizeof(IcpJob) * nj), o_rec = lay.put(rec_h.data(), sizeof(IcpRecord) * 2 * nj);
    for (size_t c = 0; c < nc; ++c) {
      o_samples[c] = lay.room(16 * pos[c].size());
      max_samples = std::max(max_samples, (uint32_t)pos[c].size());
    }
    std::vector<Block> o_P(nj), o_nnj(nj), o_nnd(nj), o_part(nj);
    for (size_t j = 0; j < nj; ++j) {
      const size_t ns = (size_t)job_h[j].ns, leaves = (ns + kIcpLeaf - 1) / kIcpLeaf;
      o_P[j] = lay.room(16 * ns);
      o_nnj[j] = lay.room(4 * ns);
      o_nnd[j] = lay.room(4 * ns);
      o_part[j] = lay.room(8 * (size_t)kIcpSums * leaves);
    }
    rc = ensure_icp(ctx, lay.total());
    if (rc != RGBDFE_OK) return rc;
    void* base = ctx->icp.p;
    for (size_t c = 0; c < nc; ++c) {
      table[c].pos = at<uint32_t>(base, o_pos[c]);
      table[c].samples = at<float4>(base, o_samples[c]);
      table[c].sample_index = nullptr;
      table[c].poison = 1;
    }
    IcpRecord* d_rec = at<IcpRecord>(base, o_rec);
    IcpJob* jp = lay.staged<IcpJob>(o_jobs);
    for (size_t j = 0; j < nj; ++j) {
      jp[j].S = table[(size_t)jobs[j].source].samples;
      jp[j].T = table[(size_t)jobs[j].target].samples;
      jp[j].P = at<float4>(base, o_P[j]);
      jp[j].nn_j = at<int32_t>(base, o_nnj[j]);
      jp[j].nn_d2 = at<float>(base, o_nnd[j]);
      jp[j].part = at<double>(base, o_part[j]);
      jp[j].rec = d_rec + 2 * j;
    }
    HIP_TRY(ctx, hipMemcpyAsync(base, lay.staged(), lay.staged_bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_table, table.data(), sizeof(IcpCloud) * nc, hipMemcpyHostToDevice, st));
    launches += launch_icp_gather(d_table, (uint32_t)nc, max_samples, d_tile_first, st);
    HIP_TRY(ctx, hipGetLastError());

    IcpStop stop{};
    stop.maxdist2 = prm.max_correspondence_distance * prm.max_correspondence_distance;
    stop.transformation_epsilon = prm.transformation_epsilon;
    stop.euclidean_fitness_epsilon = prm.euclidean_fitness_epsilon;
    stop.max_iterations = prm.max_iterations;
    const IcpJob* d_jobs = at<IcpJob>(base, o_jobs);
    int32_t next = 1, chunk = kIcpFirstChunk;
    for (;;) {
      const int32_t count = std::min(chunk, prm.max_iterations - next + 1);
      ChunkEvents events(ctx);   // rgbdfe_set_profiling: the nearest-neighbour launches bracketed one by one
      std::vector<hipEvent_t>& ev = events.ev;
      if (ctx->profiling) {
        for (int32_t k = next; k < next + count; ++k) {
          ev.push_back(get_event(ctx));
          ev.push_back(get_event(ctx));
          (void)hipEventRecord(ev[ev.size() - 2], st);
          launches += launch_icp_nn(d_jobs, (uint32_t)nj, max_ns, stop, k, st);
          (void)hipEventRecord(ev.back(), st);
          launches += launch_icp_finish(d_jobs, (uint32_t)nj, stop, k, st);
        }
      } else {
        launches += launch_icp_iterations(d_jobs, (uint32_t)nj, max_ns, stop, next, count, st);
      }
      next += count;
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(rec_h.data(), d_rec, sizeof(IcpRecord) * 2 * nj, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));  // (the first one also covers the staging vector's copy)
      ++readbacks;
      for (size_t e = 0; e + 1 < ev.size(); e += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[e], ev[e + 1]) == hipSuccess) {
          ctx->k_ms[RGBDFE_KERNEL_ICP_NN] += ms;
          ctx->k_launches[RGBDFE_KERNEL_ICP_NN]++;
          ctx->k_pairs[RGBDFE_KERNEL_ICP_NN] += (int64_t)nj;
        }
      }
      bool all = true;
      for (size_t j = 0; j < nj; ++j) all = all && rec_h[2 * j + (size_t)((next - 1) & 1)].done != 0;
      if (all) break;
      if (next > prm.max_iterations) return fail(ctx, RGBDFE_ERR_INTERNAL, "icp: a job did not report its stop");
      chunk = std::min(2 * chunk, kIcpMaxChunk);
    }
    if (nn_index_out || nn_d2_out) {
      const size_t ns = (size_t)job_h[0].ns;
      if (ns && nn_index_out) HIP_TRY(ctx, hipMemcpyAsync(nn_index_out, at<int32_t>(base, o_nnj[0]), 4 * ns, hipMemcpyDeviceToHost, st));
      if (ns && nn_d2_out) HIP_TRY(ctx, hipMemcpyAsync(nn_d2_out, at<float>(base, o_nnd[0]), 4 * ns, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
      ++readbacks;
    }
    for (size_t j = 0; j < nj; ++j) {
      const IcpRecord& r = rec_h[2 * j + (size_t)((next - 1) & 1)];
      const bool converged = r.state != kIcpNoCorrespondences;
      float* out = transforms_out + 16 * j;
      if (converged) {
        for (int a = 0; a < 3; ++a) {
          for (int b = 0; b < 3; ++b) out[b * 4 + a] = r.FR[a * 3 + b];
          out[12 + a] = r.Ft[a];
          out[4 * a + 3] = 0.0f;
        }
        out[15] = 1.0f;
      } else {
        memcpy(out, jobs[j].G, 16 * sizeof(float));
      }
      if (reports_out) {
        rgbdfe_icp_report& rep = reports_out[j];
        memset(&rep, 0, sizeof(rep));
        rep.converged = converged ? 1 : 0;
        rep.state = r.state;
        rep.iterations = r.k;
        rep.correspondences = r.c;
        rep.mse = r.mse;
        rep.n_source = job_h[j].ns;
        rep.n_target = job_h[j].nt;
        rep.launches = launches;
        rep.readbacks = readbacks;
      }
    }
    return RGBDFE_OK;
  }
};

const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

}  // namespace

void rgbdfe_icp_default_params(rgbdfe_icp_params* p) {
  if (!p) return;
  p->max_correspondence_distance = 0.05;   // icp.cpp:68
  p->max_iterations = 50;                  // :70
  p->transformation_epsilon = 1e-8;        // :72
  p->euclidean_fitness_epsilon = 1.0;      // :74
  p->desired_size = 10000;                 // gicp_max_cloud_size, parameter_server.cpp:111
}

int rgbdfe_icp_align_nodes(rgbdfe_ctx* ctx, int32_t n_jobs, const int32_t* source_ids, const int32_t* target_ids,
                           const float* guesses, const rgbdfe_icp_params* params, float* transforms_out,
                           rgbdfe_icp_report* reports_out) {
  if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!source_ids || !target_ids || !transforms_out)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad icp arguments");
  int rc = check_params(ctx, params);
  if (rc != RGBDFE_OK) return rc;
  if (n_jobs == 0) return RGBDFE_OK;
  if (n_jobs > kIcpMaxJobs) return fail(ctx, RGBDFE_ERR_CAPACITY, "icp: more than 65535 jobs in one call");
  std::lock_guard<std::mutex> lock(ctx->mu);
  IcpCall call;
  call.ctx = ctx;
  call.st = ctx->stream;
  call.desired_size = params->desired_size;
  std::unordered_map<int32_t, int> cloud_of;  // node id -> index in the call's cloud list
  auto cloud_index = [&](int32_t id, int* out) -> int {
    auto at = cloud_of.find(id);
    if (at != cloud_of.end()) { *out = at->second; return RGBDFE_OK; }
    const CloudEntry* ce = resident_cloud(ctx, id);
    if (!ce) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "icp: no cloud for a listed node");
    const int64_t n = (int64_t)ce->ch * (int64_t)ce->cw;
    if (n > kIcpMaxRows) return fail(ctx, RGBDFE_ERR_CAPACITY, "icp: a cloud of more than 2^24 rows");
    *out = (int)call.clouds.size();
    cloud_of[id] = *out;
    call.clouds.push_back(CloudRef{ce->d, (uint32_t)n});
    return RGBDFE_OK;
  };
  call.jobs.resize((size_t)n_jobs);
  for (int32_t j = 0; j < n_jobs; ++j) {
    JobRef& jr = call.jobs[(size_t)j];
    if ((rc = cloud_index(source_ids[j], &jr.source)) != RGBDFE_OK) return rc;
    if ((rc = cloud_index(target_ids[j], &jr.target)) != RGBDFE_OK) return rc;
    memcpy(jr.G, guesses ? guesses + 16 * (size_t)j : kIdentity, sizeof(jr.G));
  }
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  return call.align(*params, transforms_out, reports_out, nullptr, nullptr, 0);
}

int rgbdfe_icp_align_clouds(rgbdfe_ctx* ctx, const float* source, int64_t n_source, const float* target, int64_t n_target,
                            const float* guess, const rgbdfe_icp_params* params, float* transform_out,
                            rgbdfe_icp_report* report_out, int32_t* nn_index_out, float* nn_d2_out, int64_t debug_capacity) {
  if (!ctx || n_source < 0 || n_target < 0 || (n_source > 0 && !source) || (n_target > 0 && !target) || !transform_out ||
      debug_capacity < 0)
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad icp arguments");
  const int rc = check_params(ctx, params);
  if (rc != RGBDFE_OK) return rc;
  if (n_source > kIcpMaxRows || n_target > kIcpMaxRows) return fail(ctx, RGBDFE_ERR_CAPACITY, "icp: a cloud of more than 2^24 rows");
  std::lock_guard<std::mutex> lock(ctx->mu);
  IcpCall call;
  call.ctx = ctx;
  call.st = ctx->stream;
  call.desired_size = params->desired_size;
  call.clouds = {CloudRef{nullptr, (uint32_t)n_source}, CloudRef{nullptr, (uint32_t)n_target}};
  call.host_clouds = {source, target};
  call.jobs.resize(1);
  call.jobs[0].source = 0;
  call.jobs[0].target = 1;
  memcpy(call.jobs[0].G, guess ? guess : kIdentity, sizeof(call.jobs[0].G));
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  return call.align(*params, transform_out, report_out, nn_index_out, nn_d2_out, debug_capacity);
}

int rgbdfe_filter_cloud(rgbdfe_ctx* ctx, const float* cloud, int64_t n, int32_t desired_size, int32_t* indices_out,
                        float* rows_out, int64_t capacity, int64_t* n_out) {
  if (!ctx || n < 0 || (n > 0 && !cloud) || capacity < 0 || !n_out) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad filter_cloud arguments");
  if (desired_size <= 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "filter_cloud: desired_size <= 0");
  if (n > kIcpMaxRows) return fail(ctx, RGBDFE_ERR_CAPACITY, "filter_cloud: a cloud of more than 2^24 rows");
  std::lock_guard<std::mutex> lock(ctx->mu);
  IcpCall call;
  call.ctx = ctx;
  call.st = ctx->stream;
  call.desired_size = desired_size;
  call.clouds = {CloudRef{nullptr, (uint32_t)n}};
  call.host_clouds = {cloud};
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  return call.filter(indices_out, rows_out, capacity, n_out);
}

}  // namespace impl
