// tests/emu/emu_icp.cpp -- TEST INFRASTRUCTURE ONLY: csrc/icp.hip compiled as host C++ over tests/emu/hip/hip_runtime.h
// (tests/test_emu_icp_kernels.py builds it: the kernel SOURCE of the product runs, one OS thread per HIP thread).  The
// kernels use workgroup barriers only, so every one of them runs here.  Jobs are driven as api_icp.hip drives them:
// iterations enqueued in chunks of 2, 4, 8, 16, 16 ..., the records looked at once per chunk.
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include <float.h>

#include <algorithm>

#include "icp.hip"

// filterCloud's device part: the count and the scan of one cloud's valid rows, then -- with positions -- the rows of those
// ranks.  Returns the number of valid rows.
extern "C" int emu_icp_filter(const float* cloud, uint32_t n, const uint32_t* pos, uint32_t n_pos, int32_t poison,
                              float* samples, uint32_t* sample_index) {
  using namespace rgbdfe;
  const uint32_t tiles = (n + kIcpScanTile - 1) / kIcpScanTile;
  std::vector<uint32_t> count(tiles + 1), first(tiles + 1);
  uint32_t n_valid = 0;
  IcpCloud c{};
  c.d = reinterpret_cast<const float4*>(cloud);
  c.n = n;
  launch_icp_compact(&c, 1, tiles, count.data(), first.data(), &n_valid, nullptr);
  if (pos) {
    c.pos = pos;
    c.n_samples = n_pos;
    c.poison = (uint32_t)poison;
    c.samples = reinterpret_cast<float4*>(samples);
    c.sample_index = sample_index;
    launch_icp_gather(&c, 1, n_pos, first.data(), nullptr);
  }
  return (int)n_valid;
}

// One job over two sampled clouds.  G12: the guess's rotation (row-major) and translation.  At most `limit` iterations are
// enqueued (1: a single iteration).  rec_out: the last record as doubles: mse, R[9], t[3], FR[9], Ft[3], done, state, k, c.
// P_out: the working copy as the last iteration that ran left it (its increment is applied by the next one).
// Returns the kernel launches; *chunks = the record reads.
extern "C" int emu_icp_job(const float* S, int32_t ns, const float* T, int32_t nt, const float* G12, double maxdist,
                           double transformation_epsilon, double euclidean_fitness_epsilon, int32_t max_iterations,
                           int32_t limit, double* rec_out, int32_t* nn_j, float* nn_d2, float* P_out, int32_t* chunks) {
  using namespace rgbdfe;
  const size_t leaves = ((size_t)ns + kIcpLeaf - 1) / kIcpLeaf;
  std::vector<double> part(kIcpSums * leaves + 1);
  IcpRecord rec[2];
  memset(rec, 0, sizeof(rec));
  IcpJob job{};
  job.S = reinterpret_cast<const float4*>(S);
  job.T = reinterpret_cast<const float4*>(T);
  job.P = reinterpret_cast<float4*>(P_out);
  job.ns = ns;
  job.nt = nt;
  job.nn_j = nn_j;
  job.nn_d2 = nn_d2;
  job.part = part.data();
  job.rec = rec;
  for (int a = 0; a < 9; ++a) {
    job.GR[a] = G12[a];
    rec[0].R[a] = (a % 4 == 0) ? 1.0f : 0.0f;
    rec[0].FR[a] = G12[a];
  }
  for (int a = 0; a < 3; ++a) job.Gt[a] = rec[0].Ft[a] = G12[9 + a];
  rec[0].mse = DBL_MAX;
  IcpStop stop{};
  stop.maxdist2 = maxdist * maxdist;
  stop.transformation_epsilon = transformation_epsilon;
  stop.euclidean_fitness_epsilon = euclidean_fitness_epsilon;
  stop.max_iterations = max_iterations;
  const int32_t last = std::min(limit, max_iterations);
  int launches = 0;
  int32_t next = 1, chunk = 2;
  *chunks = 0;
  for (;;) {
    const int32_t count = std::min(chunk, last - next + 1);
    launches += launch_icp_iterations(&job, 1, (uint32_t)ns, stop, next, count, nullptr);
    next += count;
    ++*chunks;
    if (rec[(next - 1) & 1].done || next > last) break;
    chunk = std::min(2 * chunk, 16);
  }
  const IcpRecord& r = rec[(next - 1) & 1];
  double* o = rec_out;
  *o++ = r.mse;
  for (int a = 0; a < 9; ++a) *o++ = r.R[a];
  for (int a = 0; a < 3; ++a) *o++ = r.t[a];
  for (int a = 0; a < 9; ++a) *o++ = r.FR[a];
  for (int a = 0; a < 3; ++a) *o++ = r.Ft[a];
  *o++ = r.done; *o++ = r.state; *o++ = r.k; *o++ = r.c;
  return launches;
}
