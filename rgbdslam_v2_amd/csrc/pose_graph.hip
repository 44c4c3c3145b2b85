// pose_graph.hip -- pose-graph optimisation on the device, gfx950: the kernels of GraphManager::optimizeGraphImpl's work
// (graph_manager.cpp:938-1066): Levenberg-Marquardt over SE(3) edges with a Huber kernel, solved by block-Jacobi
// preconditioned conjugate gradients.  The contract is the "pose-graph optimisation" block of include/rgbdfe.h
// (DESIGN.md 4.21); tests/pose_graph_oracle.py restates it literally and the bytes must agree.
//
//   edges    a lane per edge: e = toVectorMQT(Z^-1 Xi^-1 Xj), chi2 = e'Oe, Huber rho and w = rho'; with jacobians also
//            Ji, Jj (analytic, at a zero update) and w J'OJ (three blocks), -w J'Oe (two vectors) into the edge's record
//   gather   a lane per element of a diagonal block / of b / of an off-diagonal block: the records of the edges that feed it,
//            added in list order (the lists are built by the host in insertion order)
//   pcg      begin (factor H_ff + lambda I = L L', x = 0, r = b, z, p), then per iteration four launches: q = A p with the
//            leaves of p'q; alpha; x, r, z with the leaves of r'z; beta and p.  The scalars live in PgScalars; an iteration
//            enqueued after the stop returns at once, so the host enqueues chunks and reads one record per chunk.
//   prune    a lane per edge: pruneEdgesWithErrorAbove (:1106-1246) on the uploaded edge arrays, in place
//   trial    gated on the stop: the update applied to a second set of estimates, their chi2, dx'(lambda dx + b)
//
// Double throughout; + - * / sqrt and comparisons only (-ffp-contract=off).  Every sum has one order: the terms of a small
// product left to right, list entries in list order, and one reduction tree (leaves of 64 values halved 32 .. 1, the leaf
// sums round-robin into 64 accumulators, those halved again) whose shape depends on the element count alone.  No atomics,
// no workgroup waits for another: hand-offs are kernel boundaries.
#include "pose_graph.h"

namespace rgbdfe {

namespace {

constexpr double kPcgTol = 1e-6;

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// the sum of the workgroup's first 64 values (one per thread t < 64; every thread of the workgroup calls)
__device__ __forceinline__ double pg_tree_leaf(double v, double* lds) {
  const unsigned t = threadIdx.x;
  if (t < (unsigned)kPgTile) lds[t] = v;
  __syncthreads();
  for (unsigned s = kPgTile / 2; s >= 1; s >>= 1) {
    if (t < s) lds[t] = lds[t] + lds[t + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// the tree's second level over m leaf sums (a 64-thread workgroup)
__device__ __forceinline__ double pg_tree_finish(const double* part, int m, double* lds) {
  double acc = 0.0;
  for (int k = (int)threadIdx.x; k < m; k += kPgTile) acc = acc + part[k];
  return pg_tree_leaf(acc, lds);
}

__device__ __forceinline__ int pg_leaves(int n) { return n > 0 ? (n + kPgTile - 1) / kPgTile : 1; }

// (x, y, z, w) of a rotation matrix (row-major): the four-branch conversion, normalised, w >= 0
__device__ __forceinline__ void quat_from_rot(const double* R, double* q) {
  const double tr = (R[0] + R[4]) + R[8];
  double x, y, z, w;
  if (tr > 0.0) {
    double s = sqrt(tr + 1.0);
    w = 0.5 * s;
    s = 0.5 / s;
    x = (R[7] - R[5]) * s;
    y = (R[2] - R[6]) * s;
    z = (R[3] - R[1]) * s;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0);
    double v[3];
    v[i] = 0.5 * s;
    s = 0.5 / s;
    w = (R[3 * k + j] - R[3 * j + k]) * s;
    v[j] = (R[3 * j + i] + R[3 * i + j]) * s;
    v[k] = (R[3 * k + i] + R[3 * i + k]) * s;
    x = v[0]; y = v[1]; z = v[2];
  }
  const double n = sqrt(((x * x + y * y) + z * z) + w * w);
  x = x / n; y = y / n; z = z / n; w = w / n;
  if (w < 0.0) { x = -x; y = -y; z = -z; w = -w; }
  q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

// e = toVectorMQT(Z^-1 Xi^-1 Xj) into err, and chi2 = e'Oe; Ra, ta, RD, q and Oe stay for the jacobians
__device__ __forceinline__ double pg_edge_error(const double* Xi, const double* Xj, const double* Z, const double* Om, double* Ra,
                                                double* ta, double* RD, double* q, double* err, double* Oe) {
  double d[3];
  for (int k = 0; k < 3; ++k) d[k] = Xj[9 + k] - Xi[9 + k];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) Ra[3 * a + b] = dot3(Xi[a], Xi[3 + a], Xi[6 + a], Xj[b], Xj[3 + b], Xj[6 + b]);
    ta[a] = dot3(Xi[a], Xi[3 + a], Xi[6 + a], d[0], d[1], d[2]);
  }
  for (int k = 0; k < 3; ++k) d[k] = ta[k] - Z[9 + k];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) RD[3 * a + b] = dot3(Z[a], Z[3 + a], Z[6 + a], Ra[b], Ra[3 + b], Ra[6 + b]);
    err[a] = dot3(Z[a], Z[3 + a], Z[6 + a], d[0], d[1], d[2]);
  }
  quat_from_rot(RD, q);
  err[3] = q[0]; err[4] = q[1]; err[5] = q[2];
  for (int a = 0; a < 6; ++a) {
    double acc = Om[6 * a] * err[0];
    for (int k = 1; k < 6; ++k) acc = acc + Om[6 * a + k] * err[k];
    Oe[a] = acc;
  }
  double chi2 = err[0] * Oe[0];
  for (int k = 1; k < 6; ++k) chi2 = chi2 + err[k] * Oe[k];
  return chi2;
}

// a 64-thread workgroup may use the whole register file of a wave: the 6 x 6 products stay in registers.  A pruned edge
// (edge_active 0) keeps rho 0 in its place in the tree and writes no record.
template <bool kJac>
__global__ void __launch_bounds__(kPgTile) pg_edges_kernel(PgProblem P, const double* est, const int32_t* gate) {
  __shared__ double lds[kPgTile];
  if (gate && !*gate) return;
  const int e = (int)(blockIdx.x * kPgTile + threadIdx.x);
  double rho = 0.0;
  if (e < P.n_edge && (!P.edge_active || P.edge_active[e])) {
    const double* Xi = est + (size_t)kPgPose * P.edge_ij[2 * e];
    const double* Xj = est + (size_t)kPgPose * P.edge_ij[2 * e + 1];
    const double* Z = P.edge_in + (size_t)kPgEdgeIn * e;
    const double* Om = Z + kPgPose;
    double* out = P.edge_out + (size_t)kPgEdgeOut * e;
    double Ra[9], ta[3], RD[9], err[6], q[4], Oe[6];
    const double chi2 = pg_edge_error(Xi, Xj, Z, Om, Ra, ta, RD, q, err, Oe);
    double w = 1.0;
    rho = chi2;
    if (!(chi2 <= 1.0)) {  // Huber, delta = 1
      const double sq = sqrt(chi2);
      rho = 2.0 * sq - 1.0;
      w = 1.0 / sq;
    }
    for (int k = 0; k < 6; ++k) out[kPgE + k] = err[k];
    out[kPgChi2] = chi2;
    out[kPgRho] = rho;
    out[kPgW] = w;
    if (kJac) {
      double Ji[36], Jj[36], Q[9], S[9];
      for (int k = 0; k < 36; ++k) { Ji[k] = 0.0; Jj[k] = 0.0; }
      // Q = w I + [u]x of the error quaternion (u, w); S = 2 [ta]x
      Q[0] = q[3]; Q[1] = -q[2]; Q[2] = q[1];
      Q[3] = q[2]; Q[4] = q[3]; Q[5] = -q[0];
      Q[6] = -q[1]; Q[7] = q[0]; Q[8] = q[3];
      const double a0 = 2.0 * ta[0], a1 = 2.0 * ta[1], a2 = 2.0 * ta[2];
      S[0] = 0.0; S[1] = -a2; S[2] = a1;
      S[3] = a2; S[4] = 0.0; S[5] = -a0;
      S[6] = -a1; S[7] = a0; S[8] = 0.0;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          Jj[6 * a + b] = RD[3 * a + b];
          Jj[6 * (3 + a) + 3 + b] = Q[3 * a + b];
          Ji[6 * a + b] = -Z[3 * b + a];
          Ji[6 * a + 3 + b] = dot3(Z[a], Z[3 + a], Z[6 + a], S[b], S[3 + b], S[6 + b]);
          Ji[6 * (3 + a) + 3 + b] = -dot3(Q[3 * a], Q[3 * a + 1], Q[3 * a + 2], Ra[3 * b], Ra[3 * b + 1], Ra[3 * b + 2]);
        }
      double Wi[36], Wj[36];
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
          double ai = Om[6 * a] * Ji[b], aj = Om[6 * a] * Jj[b];
          for (int k = 1; k < 6; ++k) {
            ai = ai + Om[6 * a + k] * Ji[6 * k + b];
            aj = aj + Om[6 * a + k] * Jj[6 * k + b];
          }
          Wi[6 * a + b] = ai;
          Wj[6 * a + b] = aj;
        }
      for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) {
          double hii = Ji[a] * Wi[b], hij = Ji[a] * Wj[b], hjj = Jj[a] * Wj[b];
          for (int k = 1; k < 6; ++k) {
            hii = hii + Ji[6 * k + a] * Wi[6 * k + b];
            hij = hij + Ji[6 * k + a] * Wj[6 * k + b];
            hjj = hjj + Jj[6 * k + a] * Wj[6 * k + b];
          }
          out[kPgHii + 6 * a + b] = w * hii;
          out[kPgHij + 6 * a + b] = w * hij;
          out[kPgHjj + 6 * a + b] = w * hjj;
        }
        double bi = Ji[a] * Oe[0], bj = Jj[a] * Oe[0];
        for (int k = 1; k < 6; ++k) {
          bi = bi + Ji[6 * k + a] * Oe[k];
          bj = bj + Jj[6 * k + a] * Oe[k];
        }
        out[kPgBi + a] = -(w * bi);
        out[kPgBj + a] = -(w * bj);
      }
    }
  }
  const double leaf = pg_tree_leaf(rho, lds);
  if (threadIdx.x == 0) P.part_a[blockIdx.x] = leaf;
}

// a lane per output element: 42 per free vertex (its diagonal block, its part of b), then 36 per off-diagonal block
__global__ void pg_gather_kernel(PgProblem P) {
  const long long idx = (long long)blockIdx.x * kPgTile + threadIdx.x;
  const long long n_diag = 42ll * P.n_free;
  if (idx < n_diag) {
    const int f = (int)(idx / 42), el = (int)(idx % 42);
    double acc = 0.0;
    for (int it = P.vert_ptr[f]; it < P.vert_ptr[f + 1]; ++it) {
      const int item = P.vert_items[it], e = item >> 1, side = item & 1;
      const int off = el < 36 ? (side ? kPgHjj : kPgHii) + el : (side ? kPgBj : kPgBi) + (el - 36);
      acc = acc + P.edge_out[(size_t)kPgEdgeOut * e + off];
    }
    if (el < 36) P.Hd[36 * (size_t)f + el] = acc; else P.b[6 * (size_t)f + (el - 36)] = acc;
  } else if (idx < n_diag + 36ll * P.n_block) {
    const long long k = idx - n_diag;
    const int n = (int)(k / 36), el = (int)(k % 36);
    const int tel = (el % 6) * 6 + el / 6;
    double acc = 0.0;
    for (int it = P.blk_ptr[n]; it < P.blk_ptr[n + 1]; ++it) {
      const int item = P.blk_items[it], e = item >> 1;
      acc = acc + P.edge_out[(size_t)kPgEdgeOut * e + kPgHij + ((item & 1) ? tel : el)];
    }
    P.B[36 * (size_t)n + el] = acc;
  }
}

// one workgroup: chi2 from the edges' leaf sums; with_diag: max |diag H| too (a maximum has no order)
__global__ void pg_lin_finish_kernel(PgProblem P, int with_diag) {
  __shared__ double lds[kPgTile];
  const double chi2 = pg_tree_finish(P.part_a, pg_leaves(P.n_edge), lds);
  double mx = 0.0;
  if (with_diag) {
    for (int k = (int)threadIdx.x; k < 6 * P.n_free; k += kPgTile) {
      double v = P.Hd[36 * (size_t)(k / 6) + 7 * (k % 6)];
      if (v < 0.0) v = -v;
      if (v > mx) mx = v;
    }
    lds[threadIdx.x] = mx;
    __syncthreads();
    for (unsigned s = kPgTile / 2; s >= 1; s >>= 1) {
      if (threadIdx.x < s && lds[threadIdx.x + s] > lds[threadIdx.x]) lds[threadIdx.x] = lds[threadIdx.x + s];
      __syncthreads();
    }
    mx = lds[0];
  }
  if (threadIdx.x == 0) {
    P.s->chi2 = chi2;
    if (with_diag) P.s->max_diag = mx;
  }
}

// z = (L L')^-1 r for one vertex
__device__ __forceinline__ void chol_solve(const double* L, const double* r, double* z) {
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = r[i];
    for (int k = 0; k < i; ++k) s = s - L[6 * i + k] * y[k];
    y[i] = s / L[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s = s - L[6 * k + i] * z[k];
    z[i] = s / L[6 * i + i];
  }
}

__device__ __forceinline__ double dot6(const double* a, const double* b) {
  double d = a[0] * b[0];
  for (int k = 1; k < 6; ++k) d = d + a[k] * b[k];
  return d;
}

// a lane per free vertex: the factor of its damped diagonal block, x = 0, r = b, z; the leaves of r'z
__global__ void __launch_bounds__(kPgTile) pg_pcg_factor_kernel(PgProblem P, double lambda) {
  __shared__ double lds[kPgTile];
  const int f = (int)(blockIdx.x * kPgTile + threadIdx.x);
  double d = 0.0;
  if (f < P.n_free) {
    double A[36], L[36], r[6], z[6];
    for (int k = 0; k < 36; ++k) { A[k] = P.Hd[36 * (size_t)f + k]; L[k] = 0.0; }
    for (int a = 0; a < 6; ++a) A[7 * a] = A[7 * a] + lambda;
    for (int j = 0; j < 6; ++j) {
      double s = A[7 * j];
      for (int k = 0; k < j; ++k) s = s - L[6 * j + k] * L[6 * j + k];
      L[7 * j] = sqrt(s);
      for (int i = j + 1; i < 6; ++i) {
        s = A[6 * i + j];
        for (int k = 0; k < j; ++k) s = s - L[6 * i + k] * L[6 * j + k];
        L[6 * i + j] = s / L[7 * j];
      }
    }
    for (int k = 0; k < 36; ++k) P.L[36 * (size_t)f + k] = L[k];
    for (int k = 0; k < 6; ++k) r[k] = P.b[6 * (size_t)f + k];
    chol_solve(L, r, z);
    for (int k = 0; k < 6; ++k) {
      P.x[6 * (size_t)f + k] = 0.0;
      P.r[6 * (size_t)f + k] = r[k];
      P.z[6 * (size_t)f + k] = z[k];
    }
    d = dot6(r, z);
  }
  const double leaf = pg_tree_leaf(d, lds);
  if (threadIdx.x == 0) P.part_b[blockIdx.x] = leaf;
}

// a lane per free vertex, every workgroup finishing the tree for itself: p = z; workgroup 0 writes the scalars
__global__ void pg_pcg_start_kernel(PgProblem P, int32_t max_iter) {
  __shared__ double lds[kPgTile];
  const double rz = pg_tree_finish(P.part_b, pg_leaves(P.n_free), lds);
  const int f = (int)(blockIdx.x * kPgTile + threadIdx.x);
  if (f < P.n_free)
    for (int k = 0; k < 6; ++k) P.p[6 * (size_t)f + k] = P.z[6 * (size_t)f + k];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    P.s->rz[0] = rz;
    P.s->done[0] = (rz <= kPcgTol || max_iter <= 0) ? 1 : 0;
    P.s->iters = 0;
    P.s->applied = 0;
  }
}

// q = (H + lambda I) p, a lane per row (64 vertices x 6 rows a workgroup): the diagonal block's six terms, then the vertex's
// off-diagonal blocks in list order, six terms each (a stored block serves its row vertex as is, its column vertex
// transposed); then the leaves of p'q
__global__ void __launch_bounds__(kPgSpmvThreads) pg_pcg_spmv_kernel(PgProblem P, double lambda, int32_t k) {
  __shared__ double prod[kPgSpmvThreads];
  __shared__ double lds[kPgTile];
  if (P.s->done[k & 1]) return;
  const int t = (int)threadIdx.x, a = t % 6;
  const int f = (int)(blockIdx.x * kPgTile) + t / 6;
  double pq = 0.0;
  if (f < P.n_free) {
    const double* H = P.Hd + 36 * (size_t)f + 6 * a;
    const double* p = P.p + 6 * (size_t)f;
    double acc = (a == 0 ? H[0] + lambda : H[0]) * p[0];
    for (int c = 1; c < 6; ++c) acc = acc + (a == c ? H[c] + lambda : H[c]) * p[c];
    for (int it = P.vb_ptr[f]; it < P.vb_ptr[f + 1]; ++it) {
      const int item = P.vb_items[it], n = item >> 1;
      const double* B = P.B + 36 * (size_t)n;
      if (item & 1) {  // this vertex is the block's column: the transposed block times the row vertex's p
        const double* po = P.p + 6 * (size_t)P.blk_rc[2 * n];
        for (int c = 0; c < 6; ++c) acc = acc + B[6 * c + a] * po[c];
      } else {
        const double* po = P.p + 6 * (size_t)P.blk_rc[2 * n + 1];
        for (int c = 0; c < 6; ++c) acc = acc + B[6 * a + c] * po[c];
      }
    }
    P.q[6 * (size_t)f + a] = acc;
    pq = p[a] * acc;
  }
  prod[t] = pq;
  __syncthreads();
  double d = 0.0;
  if (t < kPgTile) {
    d = prod[6 * t];
    for (int c = 1; c < 6; ++c) d = d + prod[6 * t + c];
  }
  const double leaf = pg_tree_leaf(d, lds);
  if (t == 0) P.part_b[blockIdx.x] = leaf;
}

__global__ void pg_pcg_alpha_kernel(PgProblem P, int32_t k) {
  __shared__ double lds[kPgTile];
  if (P.s->done[k & 1]) return;
  const double pq = pg_tree_finish(P.part_b, pg_leaves(P.n_free), lds);
  if (threadIdx.x == 0) P.s->alpha = P.s->rz[k & 1] / pq;
}

// a lane per free vertex: x += alpha p, r -= alpha q, z = M^-1 r; the leaves of r'z
__global__ void __launch_bounds__(kPgTile) pg_pcg_update_kernel(PgProblem P, int32_t k) {
  __shared__ double lds[kPgTile];
  if (P.s->done[k & 1]) return;
  const double alpha = P.s->alpha;
  const int f = (int)(blockIdx.x * kPgTile + threadIdx.x);
  double d = 0.0;
  if (f < P.n_free) {
    double r[6], z[6];
    for (int c = 0; c < 6; ++c) {
      const size_t at = 6 * (size_t)f + c;
      P.x[at] = P.x[at] + alpha * P.p[at];
      r[c] = P.r[at] - alpha * P.q[at];
      P.r[at] = r[c];
    }
    chol_solve(P.L + 36 * (size_t)f, r, z);
    for (int c = 0; c < 6; ++c) P.z[6 * (size_t)f + c] = z[c];
    d = dot6(r, z);
  }
  const double leaf = pg_tree_leaf(d, lds);
  if (threadIdx.x == 0) P.part_b[blockIdx.x] = leaf;
}

// a lane per free vertex, every workgroup finishing the tree for itself: beta, p = z + beta p; workgroup 0 writes what
// iteration k + 1 reads (the other parity: nothing read in this launch is written in it)
__global__ void pg_pcg_beta_kernel(PgProblem P, int32_t k, int32_t max_iter) {
  __shared__ double lds[kPgTile];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (P.s->done[k & 1]) {
    if (first) P.s->done[(k + 1) & 1] = 1;
    return;
  }
  const double rz_new = pg_tree_finish(P.part_b, pg_leaves(P.n_free), lds);
  const double beta = rz_new / P.s->rz[k & 1];
  const int f = (int)(blockIdx.x * kPgTile + threadIdx.x);
  if (f < P.n_free)
    for (int c = 0; c < 6; ++c) {
      const size_t at = 6 * (size_t)f + c;
      P.p[at] = P.z[at] + beta * P.p[at];
    }
  if (first) {
    P.s->rz[(k + 1) & 1] = rz_new;
    P.s->iters = k + 1;
    P.s->done[(k + 1) & 1] = (rz_new <= kPcgTol || k + 1 >= max_iter) ? 1 : 0;
  }
}

// a lane per free vertex: X <- X * fromVectorMQT(dx) from est_in into est_out (no re-orthogonalisation), and the leaves of
// dx'(lambda dx + b)
__global__ void pg_trial_apply_kernel(PgProblem P, double lambda, const int32_t* gate, const double* est_in, double* est_out) {
  __shared__ double lds[kPgTile];
  if (!*gate) return;
  const int f = (int)(blockIdx.x * kPgTile + threadIdx.x);
  double sc = 0.0;
  if (f < P.n_free) {
    const double* x = P.x + 6 * (size_t)f;
    const double* b = P.b + 6 * (size_t)f;
    const double* X = est_in + (size_t)kPgPose * P.vert_of[f];
    double* Y = est_out + (size_t)kPgPose * P.vert_of[f];
    const double v0 = x[3], v1 = x[4], v2 = x[5];
    double w = 1.0 - ((v0 * v0 + v1 * v1) + v2 * v2);
    double Rd[9];
    if (w < 0.0) {
      for (int k = 0; k < 9; ++k) Rd[k] = (k % 4 == 0) ? 1.0 : 0.0;
    } else {
      w = sqrt(w);
      const double tx = 2.0 * v0, ty = 2.0 * v1, tz = 2.0 * v2;
      const double twx = tx * w, twy = ty * w, twz = tz * w;
      const double txx = tx * v0, txy = tx * v1, txz = tx * v2;
      const double tyy = ty * v1, tyz = ty * v2, tzz = tz * v2;
      Rd[0] = 1.0 - (tyy + tzz); Rd[1] = txy - twz; Rd[2] = txz + twy;
      Rd[3] = txy + twz; Rd[4] = 1.0 - (txx + tzz); Rd[5] = tyz - twx;
      Rd[6] = txz - twy; Rd[7] = tyz + twx; Rd[8] = 1.0 - (txx + tyy);
    }
    for (int a = 0; a < 3; ++a) {
      for (int c = 0; c < 3; ++c) Y[3 * a + c] = dot3(X[3 * a], X[3 * a + 1], X[3 * a + 2], Rd[c], Rd[3 + c], Rd[6 + c]);
      Y[9 + a] = dot3(X[3 * a], X[3 * a + 1], X[3 * a + 2], x[0], x[1], x[2]) + X[9 + a];
    }
    sc = x[0] * (lambda * x[0] + b[0]);
    for (int c = 1; c < 6; ++c) sc = sc + x[c] * (lambda * x[c] + b[c]);
  }
  const double leaf = pg_tree_leaf(sc, lds);
  if (threadIdx.x == 0) P.part_b[blockIdx.x] = leaf;
}

__global__ void pg_trial_finish_kernel(PgProblem P, const int32_t* gate) {
  __shared__ double lds[kPgTile];
  if (!*gate) return;
  const double chi2 = pg_tree_finish(P.part_a, pg_leaves(P.n_edge), lds);
  const double scale = pg_tree_finish(P.part_b, pg_leaves(P.n_free), lds);
  if (threadIdx.x == 0) {
    P.s->trial_chi2 = chi2;
    P.s->scale = scale;
    P.s->applied = 1;
  }
}

// pruneEdgesWithErrorAbove, a lane per edge (one wave a workgroup): the error code of pg_edges_kernel, then the verdict from
// the host's topology bits.  The patched measurement and information, the gate and the verdict go in place; the count is an
// integer (one atomic per wave: any order gives the same number).  NaN compares false: the edge is kept.
__global__ void __launch_bounds__(kPgTile) pg_prune_kernel(PgProblem P, const double* est, double thresh, const uint8_t* topo,
                                                           double* edge_in, int32_t* edge_active, uint8_t* verdict, int32_t* count) {
  const int e = (int)(blockIdx.x * kPgTile + threadIdx.x);
  bool pruned = false;
  if (e < P.n_edge) {
    uint8_t v = kPgPruneKept;
    if (edge_active[e]) {
      const double* Xi = est + (size_t)kPgPose * P.edge_ij[2 * e];
      const double* Xj = est + (size_t)kPgPose * P.edge_ij[2 * e + 1];
      double* Z = edge_in + (size_t)kPgEdgeIn * e;
      double* Om = Z + kPgPose;
      double Ra[9], ta[3], RD[9], err[6], q[4], Oe[6];
      const double chi2 = pg_edge_error(Xi, Xj, Z, Om, Ra, ta, RD, q, err, Oe);
      if (chi2 > thresh) {
        pruned = true;
        for (int k = 0; k < kPgPose; ++k) Z[k] = (k < 9 && k % 4 == 0) ? 1.0 : 0.0;
        const uint8_t tp = topo[e];
        double diag = 1.0;
        if (tp & kPgTopoSequential) {
          v = kPgPruneZeroMotion;
        } else if (tp & kPgTopoBothJoined) {
          v = kPgPruneRemoved;
          edge_active[e] = 0;
        } else {
          v = kPgPruneDiscounted;
          diag = 1e-100;
        }
        if (v != kPgPruneRemoved)
          for (int k = 0; k < 36; ++k) Om[k] = (k % 7 == 0) ? diag : 0.0;
      }
    }
    verdict[e] = v;
  }
  const int n = __popcll(__ballot(pruned ? 1 : 0));
  if (threadIdx.x == 0 && n > 0) atomicAdd(count, n);
}

inline unsigned grid_for(long long n) { return (unsigned)(n > 0 ? (n + kPgTile - 1) / kPgTile : 1); }

}  // namespace

int launch_pg_edges(const PgProblem& P, const double* est, bool jacobians, hipStream_t st) {
  const int32_t* gate = nullptr;
  if (jacobians)
    hipLaunchKernelGGL((pg_edges_kernel<true>), dim3(grid_for(P.n_edge)), dim3(kPgTile), 0, st, P, est, gate);
  else
    hipLaunchKernelGGL((pg_edges_kernel<false>), dim3(grid_for(P.n_edge)), dim3(kPgTile), 0, st, P, est, gate);
  return 1;
}

int launch_pg_prune(const PgProblem& P, const double* est, double thresh, const uint8_t* topo, double* edge_in,
                    int32_t* edge_active, uint8_t* verdict, int32_t* count, hipStream_t st) {
  hipLaunchKernelGGL(pg_prune_kernel, dim3(grid_for(P.n_edge)), dim3(kPgTile), 0, st, P, est, thresh, topo, edge_in, edge_active,
                     verdict, count);
  return 1;
}

int launch_pg_gather(const PgProblem& P, hipStream_t st) {
  hipLaunchKernelGGL(pg_gather_kernel, dim3(grid_for(42ll * P.n_free + 36ll * P.n_block)), dim3(kPgTile), 0, st, P);
  hipLaunchKernelGGL(pg_lin_finish_kernel, dim3(1), dim3(kPgTile), 0, st, P, 1);
  return 2;
}

int launch_pg_chi2(const PgProblem& P, hipStream_t st) {
  hipLaunchKernelGGL(pg_lin_finish_kernel, dim3(1), dim3(kPgTile), 0, st, P, 0);
  return 1;
}

int launch_pg_pcg_begin(const PgProblem& P, double lambda, int32_t max_iter, hipStream_t st) {
  hipLaunchKernelGGL(pg_pcg_factor_kernel, dim3(grid_for(P.n_free)), dim3(kPgTile), 0, st, P, lambda);
  hipLaunchKernelGGL(pg_pcg_start_kernel, dim3(grid_for(P.n_free)), dim3(kPgTile), 0, st, P, max_iter);
  return 2;
}

int launch_pg_pcg_iterations(const PgProblem& P, double lambda, int32_t first, int32_t count, int32_t max_iter, hipStream_t st) {
  const dim3 grid(grid_for(P.n_free));
  for (int32_t k = first; k < first + count; ++k) {
    hipLaunchKernelGGL(pg_pcg_spmv_kernel, grid, dim3(kPgSpmvThreads), 0, st, P, lambda, k);
    hipLaunchKernelGGL(pg_pcg_alpha_kernel, dim3(1), dim3(kPgTile), 0, st, P, k);
    hipLaunchKernelGGL(pg_pcg_update_kernel, grid, dim3(kPgTile), 0, st, P, k);
    hipLaunchKernelGGL(pg_pcg_beta_kernel, grid, dim3(kPgTile), 0, st, P, k, max_iter);
  }
  return 4 * count;
}

int launch_pg_trial(const PgProblem& P, double lambda, int32_t next, const double* est_in, double* est_out, hipStream_t st) {
  const int32_t* gate = &P.s->done[next & 1];
  hipLaunchKernelGGL(pg_trial_apply_kernel, dim3(grid_for(P.n_free)), dim3(kPgTile), 0, st, P, lambda, gate, est_in, est_out);
  hipLaunchKernelGGL((pg_edges_kernel<false>), dim3(grid_for(P.n_edge)), dim3(kPgTile), 0, st, P, (const double*)est_out, gate);
  hipLaunchKernelGGL(pg_trial_finish_kernel, dim3(1), dim3(kPgTile), 0, st, P, gate);
  return 3;
}

}  // namespace rgbdfe
