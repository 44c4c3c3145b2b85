// tests/emu/emu_pose_graph_prune.cpp -- TEST INFRASTRUCTURE ONLY: csrc/pose_graph.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_pose_graph_prune.py builds it: the kernel SOURCE of the product runs, one OS
// thread per HIP thread).  One call is one prune launch as api_pose_graph.hip issues it, followed by the per-edge kernel
// without Jacobians on the patched arrays, so that the active gate of pg_edges_kernel and the chi2 tree are covered too.
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

#include "pose_graph.hip"

// edge_in and edge_active are patched in place.  edge_head: the first nine values of every edge record after the
// second launch (an inactive edge's stay as they came in).  Returns the kernel launches.
extern "C" int emu_pose_graph_prune(int32_t n_vert, int32_t n_edge, const int32_t* edge_ij, double* edge_in, int32_t* edge_active,
                                    const uint8_t* topo, const double* est, double thresh, uint8_t* verdict, int32_t* count,
                                    double* edge_head, double* chi2_out) {
  using namespace rgbdfe;
  std::vector<double> out((size_t)kPgEdgeOut * n_edge), pa((size_t)n_edge / kPgTile + 2);
  for (int32_t e = 0; e < n_edge; ++e) memcpy(out.data() + (size_t)kPgEdgeOut * e, edge_head + 9 * (size_t)e, 9 * sizeof(double));
  PgScalars s{};
  PgProblem P{};
  P.n_vert = n_vert; P.n_edge = n_edge;
  P.edge_ij = edge_ij; P.edge_in = edge_in; P.edge_out = out.data(); P.edge_active = edge_active;
  P.part_a = pa.data(); P.s = &s;
  *count = 0;
  int launches = launch_pg_prune(P, est, thresh, topo, edge_in, edge_active, verdict, count, nullptr);
  launches += launch_pg_edges(P, est, false, nullptr);
  launches += launch_pg_chi2(P, nullptr);
  for (int32_t e = 0; e < n_edge; ++e) memcpy(edge_head + 9 * (size_t)e, out.data() + (size_t)kPgEdgeOut * e, 9 * sizeof(double));
  *chi2_out = s.chi2;
  return launches;
}
