// tests/emu/emu_pose_graph.cpp -- TEST INFRASTRUCTURE ONLY: csrc/pose_graph.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_pose_graph_kernels.py builds it: the kernel SOURCE of the product runs, one OS
// thread per HIP thread).  The kernels use workgroup barriers only, so every one of them runs here.  The plan (the lists
// api_pose_graph.hip builds) comes from the test; one call is one linearisation and one Levenberg-Marquardt trial at the
// given lambda, driven as api_pose_graph.hip drives it: PCG iterations in chunks, the trial's tail gated on the stop.
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include "pose_graph.hip"

// edge_head: the first nine values of every edge record after the linearisation.  scal_out: chi2, max_diag, trial_chi2, scale.  Returns the kernel launches, -1 when the stop was never reported.
extern "C" int emu_pose_graph(int32_t n_vert, int32_t n_free, int32_t n_edge, int32_t n_block, const int32_t* free_of,
                              const int32_t* vert_of, const int32_t* edge_ij, const double* edge_in, const int32_t* vert_ptr,
                              const int32_t* vert_items, const int32_t* blk_ptr, const int32_t* blk_items, const int32_t* vb_ptr,
                              const int32_t* vb_items, const int32_t* blk_rc, const double* est_in, double lambda, int32_t chunk,
                              double* edge_out, double* edge_head, double* Hd, double* B, double* b, double* scal_out, double* x, double* est_out,
                              int32_t* iters, int32_t* chunks) {
  using namespace rgbdfe;
  const size_t nf = (size_t)n_free, leaves = (size_t)std::max(n_edge, n_free) / kPgTile + 2;
  std::vector<double> L(36 * nf), r(6 * nf), z(6 * nf), p(6 * nf), q(6 * nf), pa(leaves), pb(leaves);
  PgScalars s{};
  PgProblem P{};
  P.n_vert = n_vert; P.n_free = n_free; P.n_edge = n_edge; P.n_block = n_block;
  P.free_of = free_of; P.vert_of = vert_of; P.edge_ij = edge_ij; P.edge_in = edge_in; P.edge_out = edge_out;
  P.vert_ptr = vert_ptr; P.vert_items = vert_items; P.blk_ptr = blk_ptr; P.blk_items = blk_items;
  P.vb_ptr = vb_ptr; P.vb_items = vb_items; P.blk_rc = blk_rc;
  P.Hd = Hd; P.B = B; P.b = b; P.L = L.data(); P.x = x; P.r = r.data(); P.z = z.data(); P.p = p.data(); P.q = q.data();
  P.part_a = pa.data(); P.part_b = pb.data(); P.s = &s;
  int launches = launch_pg_edges(P, est_in, true, nullptr);
  launches += launch_pg_gather(P, nullptr);
  for (int32_t e = 0; e < n_edge; ++e)  // e, chi2, rho, w of the linearisation: the trial writes its own over them
    memcpy(edge_head + 9 * (size_t)e, edge_out + (size_t)kPgEdgeOut * e, 9 * sizeof(double));
  const int32_t max_iter = 6 * n_free;
  launches += launch_pg_pcg_begin(P, lambda, max_iter, nullptr);
  int32_t next = 0;
  *chunks = 0;
  for (;;) {
    launches += launch_pg_pcg_iterations(P, lambda, next, chunk, max_iter, nullptr);
    next += chunk;
    launches += launch_pg_trial(P, lambda, next, est_in, est_out, nullptr);
    ++*chunks;
    if (s.applied) break;
    if (next > max_iter) return -1;
  }
  scal_out[0] = s.chi2; scal_out[1] = s.max_diag; scal_out[2] = s.trial_chi2; scal_out[3] = s.scale;
  *iters = s.iters;
  return launches;
}
