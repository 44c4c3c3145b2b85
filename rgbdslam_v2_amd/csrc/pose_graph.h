// pose_graph.h -- what pose_graph.hip (kernels) and api_pose_graph.hip (host side) share: the device view of one
// optimisation problem and the launch functions.  The contract is the "pose-graph optimisation" block of include/rgbdfe.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbdfe {

constexpr int kPgTile = 64;          // values per leaf of the reduction tree = threads of the per-edge / per-vertex kernels
constexpr int kPgSpmvThreads = 6 * kPgTile;  // the product's workgroup: 64 vertices x 6 rows
// a pose: rotation row-major [0..8], translation [9..11]
constexpr int kPgPose = 12;
// an edge's input record: measurement pose [0..11], information row-major [12..47]
constexpr int kPgEdgeIn = 48;
// an edge's output record (doubles): e[6], chi2, rho, w, Hii[36], Hij[36], Hjj[36], bi[6], bj[6]
constexpr int kPgE = 0, kPgChi2 = 6, kPgRho = 7, kPgW = 8, kPgHii = 9, kPgHij = 45, kPgHjj = 81, kPgBi = 117, kPgBj = 123,
              kPgEdgeOut = 129;

struct PgScalars {        // the one small record the host reads back
  double chi2;            // of the last linearisation (sum of rho)
  double max_diag;        // max |diag H| of the last linearisation
  double trial_chi2;      // of the last applied trial
  double scale;           // dx' (lambda dx + b) of the last applied trial
  double alpha;
  double rz[2];           // r' M^-1 r entering iteration k at [k & 1]
  int32_t done[2];        // PCG has stopped, as iteration k sees it at [k & 1]
  int32_t iters;          // PCG iterations done
  int32_t applied;        // the trial's tail ran (PCG had stopped when it was reached)
};

struct PgProblem {
  int32_t n_vert, n_free, n_edge, n_block;
  const int32_t* free_of;      // [n_vert]: free index or -1
  const int32_t* vert_of;      // [n_free]
  const int32_t* edge_ij;      // [2 n_edge]: vertex indices
  const double* edge_in;       // [n_edge][kPgEdgeIn]
  double* edge_out;            // [n_edge][kPgEdgeOut]
  const int32_t* edge_active;  // [n_edge]: 0 = a pruned edge: rho 0 in its slot, no record, in no list; nullptr: all active
  // lists, all in insertion order: per free vertex its incident edges (edge * 2 + side), per block its edges
  // (edge * 2 + transposed), per free vertex its blocks (block * 2 + the vertex is the block's column)
  const int32_t *vert_ptr, *vert_items, *blk_ptr, *blk_items, *vb_ptr, *vb_items;
  const int32_t* blk_rc;       // [2 n_block]: row, column (free indices, row < column)
  double *Hd, *B, *b;          // [n_free][36], [n_block][36], [n_free][6]
  double* L;                   // [n_free][36]: the Cholesky factors of the damped diagonal blocks
  double *x, *r, *z, *p, *q;   // [n_free][6]
  double *part_a, *part_b;     // the tree's leaf sums: max(leaves of the edges, leaves of the vertices) each
  PgScalars* s;
};

// each returns its number of kernel launches
// est -> edge_out (errors, rho, w; with the products when jacobians), part_a = the leaf sums of rho
int launch_pg_edges(const PgProblem& P, const double* est, bool jacobians, hipStream_t st);
// edge_out -> Hd, b, B; s->chi2, s->max_diag (after launch_pg_edges with jacobians)
int launch_pg_gather(const PgProblem& P, hipStream_t st);
// s->chi2 alone from part_a (after launch_pg_edges)
int launch_pg_chi2(const PgProblem& P, hipStream_t st);
// L from Hd + lambda I; x = 0, r = b, z, p; s->rz[0], s->done[0], s->iters = 0, s->applied = 0
int launch_pg_pcg_begin(const PgProblem& P, double lambda, int32_t max_iter, hipStream_t st);
// iterations first .. first + count - 1, each a no-op once s->done
int launch_pg_pcg_iterations(const PgProblem& P, double lambda, int32_t first, int32_t count, int32_t max_iter, hipStream_t st);
// when PCG has stopped as iteration `next` sees it: est_out = est_in (+) x, its chi2 into s->trial_chi2, s->scale, s->applied = 1
int launch_pg_trial(const PgProblem& P, double lambda, int32_t next, const double* est_in, double* est_out, hipStream_t st);

// pruneEdgesWithErrorAbove (graph_manager.cpp:1106-1246), a lane per edge, in place in the uploaded edge arrays.  topo[e]:
// bit 0 = |id1 - id2| == 1, bit 1 = both vertices have more than one measured edge (the host owns the topology).
// An active edge with chi2 > thresh at est: *count += 1, Z = identity, and verdict / information / gate as kPgPrune*.
constexpr uint8_t kPgPruneKept = 0, kPgPruneRemoved = 1, kPgPruneDiscounted = 2, kPgPruneZeroMotion = 3;
constexpr uint8_t kPgTopoSequential = 1, kPgTopoBothJoined = 2;
int launch_pg_prune(const PgProblem& P, const double* est, double thresh, const uint8_t* topo, double* edge_in,
                    int32_t* edge_active, uint8_t* verdict, int32_t* count, hipStream_t st);

}  // namespace rgbdfe
