/*
 * oracle/rgbd_oracle.c -- TEST INFRASTRUCTURE ONLY (see rgbd_oracle.h).
 *
 * Plain-C restatement of the reference's pair path.  Every function cites the
 * reference file:line (relative to the rgbdslam_v2 tree) it follows.  Build with
 * -ffp-contract=off and without -ffast-math: the float/double operation ORDER
 * written here is the specification the HIP kernels reproduce bit-for-bit.
 *
 * Deliberate, documented deviations from the reference (all "define away a race
 * or UB"):
 *   D1  rand()/srand(clock()) is replaced by a counter-based generator
 *       orc_rand31(seed, pair_uid, iteration, k)              (node.cpp:1033-1034,1102)
 *   D2  the distance jitter rand()/(1000*RAND_MAX) is dropped; ties in hd are
 *       broken by queryIdx (stable)                            (node.cpp:573, 520-531, 1127)
 *   D3  depth_covariance()'s function-local static is an explicit parameter
 *       depth_cov                                              (misc2.h:30-35)
 *   D4  size==0 in bruteForceSearchORB (unsigned wrap -> OOB walk) returns (257,-1)
 *                                                              (features.cpp:174)
 *   D5  a non-positive LLT pivot yields DBL_MAX (Eigen would continue with a
 *       partially factored matrix)                             (misc.cpp:763)
 *
 * PINNING.  oracle/Makefile compiles the reference's own first-party code from the sources where they lie
 * (/root/reference) into oracle/_ref/ (.so files) and the tests hold this file against it bit for bit:
 *   libref_bforb.so   bruteForceSearchORB                                   tests/test_oracle_hamming.py
 *   libref_node.so    sampling, keepStrongestMatches, depth_covariance, backProject   tests/test_oracle_ransac.py
 *   libref_ransac.so  matchNodePair, featureMatching (ORB), getRelativeTransformationTo, computeInliersAndError,
 *                     errorFunction2, getTransformFromMatches                tests/test_oracle_ransac.py
 *   libref_siftmatch.so  the SiftGPU matcher kernels + SiftMatchCU + SiftGPUWrapper::match   tests/test_oracle_sift.py
 *   libref_frame.so   removeDepthless, projectTo3D, projectTo3DSiftGPU, squareroot_descriptor_space,
 *                     createXYZRGBPointCloud, observationLikelihood          tests/test_oracle_reference_frame.py
 * Third-party arithmetic those functions call (Eigen products / LLT / JacobiSVD, pcl::TransformationFromCorrespondences,
 * pcl::transformPointCloud, cv::reduce / convertTo) is absent from the tree and enters the pins through stand-ins that
 * carry THIS file's restatement: for that arithmetic alone the status remains "parity unpinned".
 */
#include "rgbd_oracle.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ------------------------------------------------------------------------- */
/* A.1 Hamming nearest neighbour -- src/features.cpp:163-182                   */
/* ------------------------------------------------------------------------- */
static inline int orc_hd256(const uint64_t* a, const uint64_t* b) {
  /* features.cpp:163-166: four 64-bit xor+popcount, little-endian words of the 32 bytes */
  return (__builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1])) +
         (__builtin_popcountll(a[2] ^ b[2]) + __builtin_popcountll(a[3] ^ b[3]));
}

int orc_hamming_nn(const uint64_t* v, const uint64_t* search_array, uint32_t size,
                   int* result_index) {
  int best = 1 + 256; /* features.cpp:173 */
  *result_index = -1; /* features.cpp:172 */
  if (size == 0) return best; /* D4 */
  /* features.cpp:174: `i < size-1` -- the LAST train row is never visited */
  for (uint32_t i = 0; i + 1 < size; ++i, search_array += 4) {
    int d = orc_hd256(v, search_array);
    if (d < best) { /* strict: first minimum wins, features.cpp:176 */
      best = d;
      *result_index = (int)i;
    }
  }
  return best;
}

void orc_hamming_nn_batch(const uint8_t* qdesc, uint32_t nq, const uint8_t* tdesc,
                          uint32_t nt, int32_t* out_hd, int32_t* out_idx) {
  /* node.cpp:567-571: descriptors are reinterpreted as uint64_t rows of 4 words */
  for (uint32_t i = 0; i < nq; ++i) {
    uint64_t q[4];
    memcpy(q, qdesc + 32u * i, 32);
    int idx;
    /* train rows are 32-byte aligned copies to keep the cast legal */
    int best = 257;
    idx = -1;
    if (nt > 0) {
      for (uint32_t t = 0; t + 1 < nt; ++t) {
        uint64_t r[4];
        memcpy(r, tdesc + 32u * t, 32);
        int d = orc_hd256(q, r);
        if (d < best) { best = d; idx = (int)t; }
      }
    }
    out_hd[i] = best;
    out_idx[i] = idx;
  }
}

/* ------------------------------------------------------------------------- */
/* A.2 featureMatching, ORB branch -- src/node.cpp:561-576, 520-531, 674       */
/* ------------------------------------------------------------------------- */
int orc_feature_matching_orb(const uint8_t* qdesc, uint32_t nq, const uint8_t* tdesc,
                             uint32_t nt, int max_matches,
                             int32_t* mq, int32_t* mt, int32_t* mhd) {
  int32_t* hd = (int32_t*)malloc(sizeof(int32_t) * (nq ? nq : 1));
  int32_t* idx = (int32_t*)malloc(sizeof(int32_t) * (nq ? nq : 1));
  orc_hamming_nn_batch(qdesc, nq, tdesc, nt, hd, idx);
  /* node.cpp:572: `if(hd >= 128) continue;` then keepStrongestMatches(max_matches)
   * (node.cpp:674) and the later std::sort by distance (node.cpp:1127).  With D2 the
   * order is (hd, queryIdx): a stable counting sort over hd in query order. */
  int n = 0;
  for (int h = 0; h < 128 && n < max_matches; ++h)
    for (uint32_t i = 0; i < nq && n < max_matches; ++i)
      if (hd[i] == h) {
        mq[n] = (int32_t)i;
        mt[n] = idx[i];
        mhd[n] = h;
        ++n;
      }
  free(hd);
  free(idx);
  return n;
}

/* ------------------------------------------------------------------------- */
/* D1: counter-based replacement for rand() -- node.cpp:1033-1034               */
/* ------------------------------------------------------------------------- */
static inline uint32_t orc_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

uint32_t orc_rand31(uint32_t seed, uint32_t uid, uint32_t iter, uint32_t k) {
  uint32_t h = orc_mix32(seed ^ 0x9E3779B9u);
  h = orc_mix32(h + uid * 0x85EBCA6Bu);
  h = orc_mix32(h ^ (iter * 0xC2B2AE35u + 0x165667B1u));
  h = orc_mix32(h + k * 0x27D4EB2Fu);
  return h >> 1; /* rand() range [0, RAND_MAX = 2^31-1] */
}

uint32_t orc_pair_uid(int32_t query_id, int32_t train_id) {
  return orc_mix32((uint32_t)query_id * 0x9E3779B1u ^ ((uint32_t)train_id + 0x7F4A7C15u));
}

/* sample_matches_prefer_by_distance -- node.cpp:1024-1047.  Returns #ids (ascending). */
int orc_sample4(uint32_t seed, uint32_t uid, uint32_t iter, uint32_t n, uint32_t ids[4]) {
  int cnt = 0;
  int safety_net = 0;
  uint32_t k = 0;
  while (cnt < 4 && n >= 4) { /* node.cpp:1031 */
    uint32_t id1 = orc_rand31(seed, uid, iter, k) % n; /* :1033 */
    uint32_t id2 = orc_rand31(seed, uid, iter, k + 1) % n; /* :1034 */
    k += 2;
    if (id1 > id2) id1 = id2; /* :1035 */
    /* std::set insert: keep ascending, ignore duplicates (:1036) */
    int pos = 0, dup = 0;
    while (pos < cnt && ids[pos] < id1) ++pos;
    if (pos < cnt && ids[pos] == id1) dup = 1;
    if (!dup) {
      for (int j = cnt; j > pos; --j) ids[j] = ids[j - 1];
      ids[pos] = id1;
      ++cnt;
    }
    if (++safety_net > 10000) break; /* :1037 */
  }
  return cnt;
}

/* ------------------------------------------------------------------------- */
/* Sensitivity harness (tests/test_oracle_sensitivity.py).       */
/* The arithmetic INSIDE Eigen 3.2 / PCL 1.7 is restated here from the published */
/* algorithms and cannot be pinned on this machine (the libraries are absent).  */
/* Every place where a plausible implementation could round differently has a   */
/* switchable alternative; the harness runs whole bench steps under each and    */
/* measures what changes.  0 = the restatement the kernels follow.              */
/* ------------------------------------------------------------------------- */
static unsigned g_variant = 0u;
void orc_set_variant(unsigned flags) { g_variant = flags; }
unsigned orc_get_variant(void) { return g_variant; }

/* ------------------------------------------------------------------------- */
/* 3x3 float SVD (two-sided Jacobi, Eigen::JacobiSVD<Matrix3f> as published)   */
/* Matrices are ROW-major here: A[i*3+j].                                      */
/* ------------------------------------------------------------------------- */
void orc_svd3(const float C[9], float U[9], float S[3], float V[9]) {
  float W[9];
  float scale = 0.0f;
  for (int i = 0; i < 9; ++i) {
    float a = fabsf(C[i]);
    if (a > scale) scale = a;
  }
  if (scale == 0.0f) scale = 1.0f;
  if (g_variant & ORC_VAR_SVD_NO_PRESCALE) scale = 1.0f;
  for (int i = 0; i < 9; ++i) W[i] = C[i] / scale;
  for (int i = 0; i < 9; ++i) U[i] = V[i] = (i % 4 == 0) ? 1.0f : 0.0f;

  const float precision = 2.0f * FLT_EPSILON;
  const float consider_as_zero = FLT_MIN;
  float max_diag = fabsf(W[0]);
  if (fabsf(W[4]) > max_diag) max_diag = fabsf(W[4]);
  if (fabsf(W[8]) > max_diag) max_diag = fabsf(W[8]);

  for (int sweep = 0; sweep < 30; ++sweep) {
    int finished = 1;
    for (int pi = 0; pi < 3; ++pi) {
      {
        /* Eigen: for p = 1..2, for q = 0..p-1 -> (1,0) (2,0) (2,1); variant: (2,1) (2,0) (1,0) */
        static const int kP[2][3] = {{1, 2, 2}, {2, 2, 1}}, kQ[2][3] = {{0, 0, 1}, {1, 0, 0}};
        const int ord = (g_variant & ORC_VAR_SVD_SWEEP_ORDER) ? 1 : 0;
        const int p = kP[ord][pi], q = kQ[ord][pi];
        float threshold = precision * max_diag;
        if (g_variant & ORC_VAR_SVD_PAIR_THRESHOLD) { /* older Eigen: relative to the pair's own diagonal */
          float dp = fabsf(W[p * 3 + p]), dq = fabsf(W[q * 3 + q]);
          threshold = precision * (dp > dq ? dp : dq);
        }
        if (consider_as_zero > threshold) threshold = consider_as_zero;
        if (!(fabsf(W[p * 3 + q]) > threshold || fabsf(W[q * 3 + p]) > threshold)) continue;
        finished = 0;
        /* real_2x2_jacobi_svd on m = [W(p,p) W(p,q); W(q,p) W(q,q)] */
        float m00 = W[p * 3 + p], m01 = W[p * 3 + q], m10 = W[q * 3 + p], m11 = W[q * 3 + q];
        float t = m00 + m11;
        float d = m10 - m01;
        float c1, s1;
        if (fabsf(d) < FLT_MIN) {
          c1 = 1.0f; s1 = 0.0f;
        } else {
          float u = t / d;
          float tmp = sqrtf(1.0f + u * u);
          s1 = 1.0f / tmp;
          c1 = u / tmp;
        }
        /* m.applyOnTheLeft(0,1,rot1) */
        float n00 = c1 * m00 + s1 * m10;
        float n01 = c1 * m01 + s1 * m11;
        float n11 = (-s1) * m01 + c1 * m11;
        /* j_right.makeJacobi(n00, n01, n11) */
        float cr, sr;
        float deno = 2.0f * fabsf(n01);
        if (deno < FLT_MIN) {
          cr = 1.0f; sr = 0.0f;
        } else {
          float tau = (n00 - n11) / deno;
          float w = sqrtf(tau * tau + 1.0f);
          float tt = (tau > 0.0f) ? 1.0f / (tau + w) : 1.0f / (tau - w);
          float sign_t = (tt > 0.0f) ? 1.0f : -1.0f;
          float nn = 1.0f / sqrtf(tt * tt + 1.0f);
          sr = -sign_t * (n01 / fabsf(n01)) * fabsf(tt) * nn;
          cr = nn;
        }
        /* j_left = rot1 * j_right.transpose() */
        float cl = c1 * cr + s1 * sr;
        float sl = s1 * cr - c1 * sr;
        /* W.applyOnTheLeft(p,q,j_left) ; U.applyOnTheRight(p,q,j_left^T) */
        for (int k = 0; k < 3; ++k) {
          float x = W[p * 3 + k], y = W[q * 3 + k];
          W[p * 3 + k] = cl * x + sl * y;
          W[q * 3 + k] = (-sl) * x + cl * y;
        }
        for (int k = 0; k < 3; ++k) {
          float x = U[k * 3 + p], y = U[k * 3 + q];
          U[k * 3 + p] = cl * x + sl * y;
          U[k * 3 + q] = (-sl) * x + cl * y;
        }
        /* W.applyOnTheRight(p,q,j_right) ; V.applyOnTheRight(p,q,j_right) */
        for (int k = 0; k < 3; ++k) {
          float x = W[k * 3 + p], y = W[k * 3 + q];
          W[k * 3 + p] = cr * x - sr * y;
          W[k * 3 + q] = sr * x + cr * y;
        }
        for (int k = 0; k < 3; ++k) {
          float x = V[k * 3 + p], y = V[k * 3 + q];
          V[k * 3 + p] = cr * x - sr * y;
          V[k * 3 + q] = sr * x + cr * y;
        }
        float a = fabsf(W[p * 3 + p]), b = fabsf(W[q * 3 + q]);
        if (b > a) a = b;
        if (a > max_diag) max_diag = a;
      }
    }
    if (finished) break;
  }
  /* positive singular values, then sort descending (columns of U,V follow) */
  for (int i = 0; i < 3; ++i) {
    float w = W[i * 3 + i];
    S[i] = fabsf(w);
    if (w < 0.0f)
      for (int k = 0; k < 3; ++k) U[k * 3 + i] = -U[k * 3 + i];
    S[i] = S[i] * scale;
  }
  for (int i = 0; i < 3; ++i) {
    int pos = i;
    float best = S[i];
    for (int j = i + 1; j < 3; ++j)
      if (S[j] > best) { best = S[j]; pos = j; }
    if (best == 0.0f) break;
    if (pos != i) {
      float ts = S[i]; S[i] = S[pos]; S[pos] = ts;
      for (int k = 0; k < 3; ++k) {
        float tu = U[k * 3 + i]; U[k * 3 + i] = U[k * 3 + pos]; U[k * 3 + pos] = tu;
        float tv = V[k * 3 + i]; V[k * 3 + i] = V[k * 3 + pos]; V[k * 3 + pos] = tv;
      }
    }
  }
}

static inline float orc_det3(const float* m) {
  /* Eigen bruteforce_det3_helper */
  float h0 = m[0] * (m[4] * m[8] - m[5] * m[7]);
  float h1 = m[1] * (m[3] * m[8] - m[5] * m[6]);
  float h2 = m[2] * (m[3] * m[7] - m[4] * m[6]);
  return h0 - h1 + h2;
}

/* ------------------------------------------------------------------------- */
/* A.4 getTransformFromMatches -- transformation_estimation_euclidean.cpp:7-61 */
/*     + pcl::TransformationFromCorrespondences (PCL 1.7, not in tree)          */
/* T is column-major (Eigen::Matrix4f storage): T[c*4+r].                       */
/* ------------------------------------------------------------------------- */
void orc_fit_transform(const float* qxyz1, const float* txyz1, const int32_t* mq,
                       const int32_t* mt, const int32_t* sel, int nsel, float T[16]) {
  float W = 0.0f;
  float mean1[3] = {0, 0, 0}, mean2[3] = {0, 0, 0};
  float C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = 0; s < nsel; ++s) {
    const int m = sel[s];
    const float* from = qxyz1 + 4 * mq[m]; /* newer node, queryIdx (:20) */
    const float* to = txyz1 + 4 * mt[m];   /* earlier node, trainIdx (:21) */
    if (isnan(from[2]) || isnan(to[2])) continue; /* :22-23 */
    /* :25  weight = 1.0/(from(2)*to(2)) : float product, double divide, float store */
    float w = (float)(1.0 / (double)(from[2] * to[2]));
    /* tfc.add(from, to, w) */
    if (w == 0.0f) continue;
    W += w;
    float alpha = w / W;
    float d1[3], d2[3];
    for (int j = 0; j < 3; ++j) d1[j] = from[j] - mean1[j];
    for (int i = 0; i < 3; ++i) d2[i] = to[i] - mean2[i];
    float oma = 1.0f - alpha;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        float outer = d2[i] * d1[j];
        if (g_variant & ORC_VAR_PCL_COV_ASSOC) { /* (1-a)*C + ((1-a)*a)*outer */
          C[i * 3 + j] = oma * C[i * 3 + j] + (oma * alpha) * outer;
          continue;
        }
        float scaled = alpha * outer;
        float sum = C[i * 3 + j] + scaled;
        C[i * 3 + j] = oma * sum;
      }
    for (int j = 0; j < 3; ++j) {
      float a1 = alpha * d1[j];
      mean1[j] = mean1[j] + a1;
    }
    for (int i = 0; i < 3; ++i) {
      float a2 = alpha * d2[i];
      mean2[i] = mean2[i] + a2;
    }
  }
  /* tfc.getTransformation() */
  float U[9], S[3], V[9];
  orc_svd3(C, U, S, V);
  float s22 = 1.0f;
  if (orc_det3(U) * orc_det3(V) < 0.0f) s22 = -1.0f;
  float R[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      float us2 = U[i * 3 + 2] * s22;
      if (g_variant & ORC_VAR_ROT_ASSOC) /* U * (S * V^T), summed from the last term */
        R[i * 3 + j] = U[i * 3 + 0] * V[j * 3 + 0] + (U[i * 3 + 1] * V[j * 3 + 1] + U[i * 3 + 2] * (s22 * V[j * 3 + 2]));
      else
      R[i * 3 + j] = (U[i * 3 + 0] * V[j * 3 + 0] + U[i * 3 + 1] * V[j * 3 + 1]) + us2 * V[j * 3 + 2];
    }
  float t[3];
  for (int i = 0; i < 3; ++i) {
    float rm = (R[i * 3 + 0] * mean1[0] + R[i * 3 + 1] * mean1[1]) + R[i * 3 + 2] * mean1[2];
    t[i] = mean2[i] - rm;
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[j * 4 + i] = R[i * 3 + j];
    T[12 + i] = t[i];
    T[i * 4 + 3] = 0.0f;
  }
  T[15] = 1.0f;
}

/* ------------------------------------------------------------------------- */
/* A.5 errorFunction2 -- src/misc.cpp:697-770 (all double)                      */
/* ------------------------------------------------------------------------- */
static double g_raster_cov_x, g_raster_cov_y;
static int g_raster_init = 0;
static void orc_raster_init(void) {
  if (g_raster_init) return;
  const double cam_angle_x = 58.0 / 180.0 * M_PI; /* misc.cpp:702 */
  const double cam_angle_y = 45.0 / 180.0 * M_PI; /* :703 */
  const double cam_resol_x = 640;                 /* :704 */
  const double cam_resol_y = 480;                 /* :705 */
  const double sx = 3 * tan(cam_angle_x / cam_resol_x); /* :706 */
  const double sy = 3 * tan(cam_angle_y / cam_resol_y); /* :707 */
  g_raster_cov_x = sx * sx; /* :708 */
  g_raster_cov_y = sy * sy; /* :709 */
  g_raster_init = 1;
}
void orc_raster_cov(double* cx, double* cy) {
  orc_raster_init();
  *cx = g_raster_cov_x;
  *cy = g_raster_cov_y;
}

double orc_error_function2(const float x1[4], const float x2[4], const double T[16],
                           double depth_cov) {
  orc_raster_init();
  const double rcx = g_raster_cov_x, rcy = g_raster_cov_y;
  if (isnan(x1[2]) || isnan(x2[2])) return DBL_MAX; /* :712-717 */
  double a[4], b[4];
  for (int i = 0; i < 4; ++i) { a[i] = (double)x1[i]; b[i] = (double)x2[i]; } /* :718-719 */
  /* mu_1_in_frame_2 = (tf_12 * x_1).head<3>()  (:724), T column-major */
  double m12[3];
  for (int i = 0; i < 3; ++i)
    m12[i] = ((T[0 * 4 + i] * a[0] + T[1 * 4 + i] * a[1]) + T[2 * 4 + i] * a[2]) + T[3 * 4 + i] * a[3];
  double d[3];
  for (int i = 0; i < 3; ++i) d[i] = m12[i] - b[i];
  /* shortcut :726-735 */
  {
    double dsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    double smax1 = rcx > depth_cov ? rcx : depth_cov;
    double smax2 = rcx > depth_cov ? rcx : depth_cov;
    if (dsq > 2.0 * (smax1 + smax2)) return DBL_MAX;
  }
  /* cov1, cov2 :740-749 */
  double c1[3] = {rcx * a[2], rcy * a[2], depth_cov};
  double c2[3] = {rcx * b[2], rcy * b[2], depth_cov};
  /* cov1_in_frame_2 = R^T * cov1 * R (:751, sic).  R(k,i) = T[i*4+k]. */
  double S[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      if (g_variant & ORC_VAR_COV_ASSOC) { /* R^T * (cov1 * R) */
        S[i * 3 + j] = (T[i * 4 + 0] * (c1[0] * T[j * 4 + 0]) + T[i * 4 + 1] * (c1[1] * T[j * 4 + 1])) +
                       T[i * 4 + 2] * (c1[2] * T[j * 4 + 2]);
        continue;
      }
      double a0 = T[i * 4 + 0] * c1[0]; /* (R^T cov1)(i,0) = R(0,i)*c1_0 */
      double a1 = T[i * 4 + 1] * c1[1];
      double a2 = T[i * 4 + 2] * c1[2];
      S[i * 3 + j] = (a0 * T[j * 4 + 0] + a1 * T[j * 4 + 1]) + a2 * T[j * 4 + 2];
    }
  if (isnan(d[2])) return DBL_MAX; /* :755-758 */
  S[0] += c2[0]; S[4] += c2[1]; S[8] += c2[2]; /* :760 */
  /* d^T * S.llt().solve(d) (:763): unblocked Cholesky on the lower triangle */
  double l00, l10, l20, l11, l21, l22, x;
  x = S[0];
  if (!(x > 0.0)) return DBL_MAX; /* D5 */
  l00 = sqrt(x);
  if (g_variant & ORC_VAR_LLT_RECIPROCAL) { /* A21 *= 1/x instead of A21 /= x */
    const double r = 1.0 / l00;
    l10 = S[3] * r;
    l20 = S[6] * r;
  } else {
    l10 = S[3] / l00;
    l20 = S[6] / l00;
  }
  x = S[4] - l10 * l10;
  if (!(x > 0.0)) return DBL_MAX;
  l11 = sqrt(x);
  if (g_variant & ORC_VAR_LLT_RECIPROCAL) l21 = (S[7] - l20 * l10) * (1.0 / l11);
  else
  l21 = (S[7] - l20 * l10) / l11;
  x = S[8] - (l20 * l20 + l21 * l21);
  if (!(x > 0.0)) return DBL_MAX;
  l22 = sqrt(x);
  /* forward: L y = d ; backward: L^T z = y */
  double y0, y1, y2, z0, z1, z2;
  if (g_variant & ORC_VAR_SOLVE_ORDER) { /* triangular solves that subtract term by term, reciprocal pivots */
    const double r0 = 1.0 / l00, r1 = 1.0 / l11, r2 = 1.0 / l22;
    y0 = d[0] * r0;
    y1 = (d[1] - l10 * y0) * r1;
    y2 = ((d[2] - l20 * y0) - l21 * y1) * r2;
    z2 = y2 * r2;
    z1 = (y1 - l21 * z2) * r1;
    z0 = ((y0 - l20 * z2) - l10 * z1) * r0;
  } else {
  y0 = d[0] / l00;
  y1 = (d[1] - l10 * y0) / l11;
  y2 = (d[2] - (l20 * y0 + l21 * y1)) / l22;
  z2 = y2 / l22;
  z1 = (y1 - l21 * z2) / l11;
  z0 = (y0 - (l10 * z1 + l20 * z2)) / l00;
  }
  double e = (d[0] * z0 + d[1] * z1) + d[2] * z2;
  if (!(e >= 0.0)) return DBL_MAX; /* :765-768 */
  return e;
}

/* ------------------------------------------------------------------------- */
/* computeInliersAndError -- src/node.cpp:968-1020                              */
/* ------------------------------------------------------------------------- */
int orc_compute_inliers_and_error(const float* qxyz1, const float* txyz1,
                                  const int32_t* mq, const int32_t* mt, int n,
                                  const float T[16], double sq_max_dist, double depth_cov,
                                  int32_t* inl, double* mean_error_out) {
  double Td[16];
  for (int i = 0; i < 16; ++i) Td[i] = (double)T[i]; /* :984 */
  double mean_error = 0.0;
  int cnt = 0;
  for (int i = 0; i < n; ++i) { /* :988 */
    const float* origin = qxyz1 + 4 * mq[i];
    const float* target = txyz1 + 4 * mt[i];
    if (origin[2] == 0.0f || target[2] == 0.0f) continue; /* :994 */
    double e = orc_error_function2(origin, target, Td, depth_cov); /* :997 */
    if (e > sq_max_dist) continue; /* :998 */
    if (!(e >= 0.0)) continue;     /* :1001 */
    mean_error += e;               /* :1006 */
    inl[cnt++] = i;                /* :1008 */
  }
  if (cnt < 3) { /* :1012 */
    *mean_error_out = 1e9;
  } else {
    mean_error /= cnt;              /* :1016 */
    *mean_error_out = sqrt(mean_error); /* :1017 */
  }
  return cnt;
}

static int orc_has_nan16(const float* T) {
  for (int i = 0; i < 16; ++i)
    if (T[i] != T[i]) return 1;
  return 0;
}

/* ------------------------------------------------------------------------- */
/* A.3 getRelativeTransformationTo -- src/node.cpp:1074-1277                    */
/* matches (mq,mt) must already be sorted ascending by distance (:1127, D2).    */
/* ------------------------------------------------------------------------- */
/* ------------------------------------------------------------------------- */
/* a21  getTransformFromMatchesG2O -- src/transformation_estimation.cpp:37-170                                  */
/* Two-view bundle adjustment: camera 2 = the newer node, fixed at the identity (:70-81); camera 1 = the        */
/* earlier node, free, initialised with the RANSAC estimate (:83-91); one free point vertex per match,           */
/* initialised with the newer node's 3-D position (:95-125, the second edgeToFeature call overwrites the first);  */
/* two EdgeSE3PointXYZDepth edges per match with measurement (u, v, depth) and information diag(1, 1,             */
/* 1/depth_covariance) (misc2.h:37-47); camera K = (521, 521, 319.5, 239.5) hard-coded (:56); Gauss-Newton for     */
/* `iterations` steps (:44, :164); result = float(estimate of camera 1).inverse() (:169).                          */
/* g2o (felixendres/g2o, branch c++03) is NOT in the reference tree: the optimiser is restated from the published  */
/* algorithm -- the normal equations of exactly this cost with the point blocks eliminated (Schur complement, as   */
/* g2o's BlockSolver does), the 3x3 point blocks inverted by cofactors, the 6x6 reduced system solved by Cholesky, */
/* VertexSE3's update estimate = estimate * (dt, quaternion(dq)) -- "parity unpinned" against a g2o build; the     */
/* per-match partial sums are reduced in the order the kernel uses (64 lanes, xor butterfly) so that kernel and    */
/* oracle agree to the bit.                                                                                        */
/* sel: positions (into mq/mt) of the matches to use.  qkp/tkp: pixel coordinates (x, y) per keypoint.              */
/* ------------------------------------------------------------------------- */
/* returns the branch taken: ORC_G2O_QUAT_TRACE, or the largest diagonal element 0, 1 or 2 */
static int gn_rot_from_matrix_via_quaternion(const double Rin[9], double Rout[9]) {
  /* Eigen::Quaterniond(Matrix3d) (Shoemake), normalised by g2o::SE3Quat, back to a rotation matrix */
  double q[4]; /* x y z w */
  int branch = ORC_G2O_QUAT_TRACE;
  const double t = Rin[0] + Rin[4] + Rin[8];
  if (t > 0.0) {
    double tt = sqrt(t + 1.0);
    q[3] = 0.5 * tt;
    tt = 0.5 / tt;
    q[0] = (Rin[7] - Rin[5]) * tt;
    q[1] = (Rin[2] - Rin[6]) * tt;
    q[2] = (Rin[3] - Rin[1]) * tt;
  } else {
    int i = 0;
    if (Rin[4] > Rin[0]) i = 1;
    if (Rin[8] > Rin[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double tt = sqrt(Rin[i * 3 + i] - Rin[j * 3 + j] - Rin[k * 3 + k] + 1.0);
    q[i] = 0.5 * tt;
    tt = 0.5 / tt;
    q[3] = (Rin[k * 3 + j] - Rin[j * 3 + k]) * tt;
    q[j] = (Rin[j * 3 + i] + Rin[i * 3 + j]) * tt;
    q[k] = (Rin[k * 3 + i] + Rin[i * 3 + k]) * tt;
    branch = i;
  }
  const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] = q[i] / nrm;
  /* Quaternion::toRotationMatrix */
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  Rout[0] = 1.0 - (tyy + tzz); Rout[1] = txy - twz;          Rout[2] = txz + twy;
  Rout[3] = txy + twz;          Rout[4] = 1.0 - (txx + tzz); Rout[5] = tyz - twx;
  Rout[6] = txz - twy;          Rout[7] = tyz + twx;          Rout[8] = 1.0 - (txx + tyy);
  return branch;
}

/* projection Jacobian d(u, v, depth)/dY at camera coordinates Y, K = (fx, fy) */
static void gn_proj(const double Y[3], double fx, double fy, double cx, double cy, double e[3], double J[9]) {
  const double iz = 1.0 / Y[2];
  e[0] = fx * (Y[0] * iz) + cx;
  e[1] = fy * (Y[1] * iz) + cy;
  e[2] = Y[2];
  J[0] = fx * iz; J[1] = 0.0;     J[2] = -(fx * (Y[0] * iz)) * iz;
  J[3] = 0.0;     J[4] = fy * iz; J[5] = -(fy * (Y[1] * iz)) * iz;
  J[6] = 0.0;     J[7] = 0.0;     J[8] = 1.0;
}

#define GN_LANES 64
/* the 27 reduced quantities of one Gauss-Newton step: upper triangle of S (21) then g (6) */
static void gn_match_terms(const double X[3], const double R1[9], const double t1[3], const double m1[3],
                           const double m2[3], double wz, double acc[27], double Hpp_inv[9], double bp[3],
                           double Hcp[18]) {
  const double fx = 521.0, fy = 521.0, cx = 319.5, cy = 239.5; /* :56 */
  double e2[3], J2[9], e1[3], Jp1[9];
  gn_proj(X, fx, fy, cx, cy, e2, J2); /* camera 2 = identity */
  for (int i = 0; i < 3; ++i) e2[i] = e2[i] - m2[i];
  const double dX[3] = {X[0] - t1[0], X[1] - t1[1], X[2] - t1[2]};
  double Y[3];
  for (int i = 0; i < 3; ++i) Y[i] = (R1[0 * 3 + i] * dX[0] + R1[1 * 3 + i] * dX[1]) + R1[2 * 3 + i] * dX[2]; /* R1^T dX */
  gn_proj(Y, fx, fy, cx, cy, e1, Jp1);
  for (int i = 0; i < 3; ++i) e1[i] = e1[i] - m1[i];
  /* J1p = Jp1 * R1^T (3x3) ; J1c = Jp1 * [ -I | 2 [Y]x ] (3x6) */
  double J1p[9], J1c[18];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      J1p[r * 3 + c] = (Jp1[r * 3 + 0] * R1[c * 3 + 0] + Jp1[r * 3 + 1] * R1[c * 3 + 1]) + Jp1[r * 3 + 2] * R1[c * 3 + 2];
  const double Yx[9] = {0.0, -Y[2], Y[1], Y[2], 0.0, -Y[0], -Y[1], Y[0], 0.0};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) J1c[r * 6 + c] = -Jp1[r * 3 + c];
    for (int c = 0; c < 3; ++c)
      J1c[r * 6 + 3 + c] = 2.0 * ((Jp1[r * 3 + 0] * Yx[0 * 3 + c] + Jp1[r * 3 + 1] * Yx[1 * 3 + c]) + Jp1[r * 3 + 2] * Yx[2 * 3 + c]);
  }
  const double w[3] = {1.0, 1.0, wz};
  double Hpp[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s2 = 0.0, s1 = 0.0;
      for (int r = 0; r < 3; ++r) { s2 += (J2[r * 3 + a] * w[r]) * J2[r * 3 + b]; s1 += (J1p[r * 3 + a] * w[r]) * J1p[r * 3 + b]; }
      Hpp[a * 3 + b] = s2 + s1;
    }
  for (int a = 0; a < 3; ++a) {
    double s2 = 0.0, s1 = 0.0;
    for (int r = 0; r < 3; ++r) { s2 += (J2[r * 3 + a] * w[r]) * e2[r]; s1 += (J1p[r * 3 + a] * w[r]) * e1[r]; }
    bp[a] = s2 + s1;
  }
  double Hcc[36], bc[6];
  for (int a = 0; a < 6; ++a) {
    for (int b = 0; b < 6; ++b) {
      double s = 0.0;
      for (int r = 0; r < 3; ++r) s += (J1c[r * 6 + a] * w[r]) * J1c[r * 6 + b];
      Hcc[a * 6 + b] = s;
    }
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int r = 0; r < 3; ++r) s += (J1c[r * 6 + a] * w[r]) * J1p[r * 3 + b];
      Hcp[a * 3 + b] = s;
    }
    double s = 0.0;
    for (int r = 0; r < 3; ++r) s += (J1c[r * 6 + a] * w[r]) * e1[r];
    bc[a] = s;
  }
  /* Hpp^-1 by cofactors (Eigen's 3x3 inverse) */
  {
    const double c00 = Hpp[4] * Hpp[8] - Hpp[5] * Hpp[7], c01 = Hpp[5] * Hpp[6] - Hpp[3] * Hpp[8], c02 = Hpp[3] * Hpp[7] - Hpp[4] * Hpp[6];
    const double det = (Hpp[0] * c00 + Hpp[1] * c01) + Hpp[2] * c02;
    const double id = 1.0 / det;
    Hpp_inv[0] = c00 * id; Hpp_inv[3] = c01 * id; Hpp_inv[6] = c02 * id;
    Hpp_inv[1] = (Hpp[2] * Hpp[7] - Hpp[1] * Hpp[8]) * id;
    Hpp_inv[4] = (Hpp[0] * Hpp[8] - Hpp[2] * Hpp[6]) * id;
    Hpp_inv[7] = (Hpp[1] * Hpp[6] - Hpp[0] * Hpp[7]) * id;
    Hpp_inv[2] = (Hpp[1] * Hpp[5] - Hpp[2] * Hpp[4]) * id;
    Hpp_inv[5] = (Hpp[2] * Hpp[3] - Hpp[0] * Hpp[5]) * id;
    Hpp_inv[8] = (Hpp[0] * Hpp[4] - Hpp[1] * Hpp[3]) * id;
  }
  /* W = Hcp * Hpp^-1 (6x3) ; S_i = Hcc - W Hcp^T ; g_i = bc - W bp */
  double W[18];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 3; ++b)
      W[a * 3 + b] = (Hcp[a * 3 + 0] * Hpp_inv[0 * 3 + b] + Hcp[a * 3 + 1] * Hpp_inv[1 * 3 + b]) + Hcp[a * 3 + 2] * Hpp_inv[2 * 3 + b];
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b)
      acc[k++] += Hcc[a * 6 + b] - ((W[a * 3 + 0] * Hcp[b * 3 + 0] + W[a * 3 + 1] * Hcp[b * 3 + 1]) + W[a * 3 + 2] * Hcp[b * 3 + 2]);
  for (int a = 0; a < 6; ++a) acc[21 + a] += bc[a] - ((W[a * 3 + 0] * bp[0] + W[a * 3 + 1] * bp[1]) + W[a * 3 + 2] * bp[2]);
}

/* returns 1 when every step solved (positive pivots), 0 when the solver stopped early; tr (may be NULL): which path */
int orc_g2o_refine_traced(const float* qxyz1, const float* txyz1, const float* qkp, const float* tkp, const int32_t* mq,
                          const int32_t* mt, const int32_t* sel, int nsel, float T[16], int iterations, double depth_cov,
                          orc_g2o_trace* tr) {
  if (tr) { tr->quat_branch = -1; tr->pivot_failed_at = -1; tr->ww_negative = 0; tr->nsel = nsel; }
  if (nsel <= 0 || nsel > ORC_MAX_MATCHES) return 0;
  const double wz = 1.0 / depth_cov; /* misc2.h:44 with the frozen depth_covariance (D3) */
  double (*X)[3] = malloc(sizeof(double) * 3 * (size_t)nsel);
  double (*M1)[3] = malloc(sizeof(double) * 3 * (size_t)nsel);
  double (*M2)[3] = malloc(sizeof(double) * 3 * (size_t)nsel);
  for (int s = 0; s < nsel; ++s) {
    const int m = sel[s];
    const float* pq = qxyz1 + 4 * mq[m]; /* newer node: camera 2 */
    const float* pt = txyz1 + 4 * mt[m]; /* earlier node: camera 1 */
    /* edgeToFeature(earlier_node, trainIdx, cam1, v) then edgeToFeature(newer_node, queryIdx, cam2, v) (:152-156) */
    if (!isnan(pt[2])) { M1[s][0] = (double)tkp[2 * mt[m]]; M1[s][1] = (double)tkp[2 * mt[m] + 1]; M1[s][2] = (double)pt[2]; }
    else { M1[s][0] = (double)tkp[2 * mt[m]]; M1[s][1] = (double)tkp[2 * mt[m] + 1]; M1[s][2] = 10.0; }
    if (!isnan(pq[2])) {
      M2[s][0] = (double)qkp[2 * mq[m]]; M2[s][1] = (double)qkp[2 * mq[m] + 1]; M2[s][2] = (double)pq[2];
      X[s][0] = (double)pq[0]; X[s][1] = (double)pq[1]; X[s][2] = (double)pq[2];
    } else {
      M2[s][0] = (double)qkp[2 * mq[m]]; M2[s][1] = (double)qkp[2 * mq[m] + 1]; M2[s][2] = 10.0;
      X[s][0] = (double)(pq[0] * 10); X[s][1] = (double)(pq[1] * 10); X[s][2] = 10.0; /* :118 (float products) */
    }
  }
  double Rin[9], R1[9], t1[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rin[r * 3 + c] = (double)T[c * 4 + r];
    t1[r] = (double)T[12 + r];
  }
  const int branch = gn_rot_from_matrix_via_quaternion(Rin, R1);
  if (tr) tr->quat_branch = branch;
  int ok = 1;
  for (int it = 0; it < iterations; ++it) {
    /* lane l accumulates its matches l, l+64, ...; then the xor butterfly */
    double part[GN_LANES][27];
    memset(part, 0, sizeof(part));
    double Hinv[9], bp[3], Hcp[18];
    for (int s = 0; s < nsel; ++s) gn_match_terms(X[s], R1, t1, M1[s], M2[s], wz, part[s % GN_LANES], Hinv, bp, Hcp);
    for (int d = GN_LANES / 2; d >= 1; d >>= 1) {
      double nxt[GN_LANES][27];
      for (int l = 0; l < GN_LANES; ++l)
        for (int k = 0; k < 27; ++k) nxt[l][k] = part[l][k] + part[l ^ d][k];
      memcpy(part, nxt, sizeof(part));
    }
    /* S dc = -g by Cholesky (lower) */
    double S[36], g[6], L[36], y[6], dc[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) { S[a * 6 + b] = S[b * 6 + a] = part[0][k]; ++k; }
    for (int a = 0; a < 6; ++a) g[a] = part[0][21 + a];
    memset(L, 0, sizeof(L));
    for (int j = 0; j < 6 && ok; ++j) {
      double d = S[j * 6 + j];
      for (int kk = 0; kk < j; ++kk) d -= L[j * 6 + kk] * L[j * 6 + kk];
      if (!(d > 0.0)) { ok = 0; break; }
      L[j * 6 + j] = sqrt(d);
      for (int i = j + 1; i < 6; ++i) {
        double v = S[i * 6 + j];
        for (int kk = 0; kk < j; ++kk) v -= L[i * 6 + kk] * L[j * 6 + kk];
        L[i * 6 + j] = v / L[j * 6 + j];
      }
    }
    if (!ok) { /* the linear solver failed: g2o stops optimising */
      if (tr) tr->pivot_failed_at = it;
      break;
    }
    for (int i = 0; i < 6; ++i) {
      double v = -g[i];
      for (int kk = 0; kk < i; ++kk) v -= L[i * 6 + kk] * y[kk];
      y[i] = v / L[i * 6 + i];
    }
    for (int i = 5; i >= 0; --i) {
      double v = y[i];
      for (int kk = i + 1; kk < 6; ++kk) v -= L[kk * 6 + i] * dc[kk];
      dc[i] = v / L[i * 6 + i];
    }
    /* points: dp = -Hpp^-1 (bp + Hcp^T dc), from the state BEFORE the update */
    for (int s = 0; s < nsel; ++s) {
      double dummy[27];
      memset(dummy, 0, sizeof(dummy));
      gn_match_terms(X[s], R1, t1, M1[s], M2[s], wz, dummy, Hinv, bp, Hcp);
      double r[3];
      for (int b = 0; b < 3; ++b) {
        double v = bp[b];
        for (int a = 0; a < 6; ++a) v += Hcp[a * 3 + b] * dc[a];
        r[b] = v;
      }
      double dp[3];
      for (int a = 0; a < 3; ++a) dp[a] = -((Hinv[a * 3 + 0] * r[0] + Hinv[a * 3 + 1] * r[1]) + Hinv[a * 3 + 2] * r[2]);
      for (int a = 0; a < 3; ++a) X[s][a] = X[s][a] + dp[a];
    }
    /* pose: estimate = estimate * (dt, q(dq)) (VertexSE3::oplusImpl, fromVectorMQT / fromCompactQuaternion) */
    {
      double Rd[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      const double qx = dc[3], qy = dc[4], qz = dc[5];
      double ww = 1.0 - ((qx * qx + qy * qy) + qz * qz);
      if (!(ww < 0.0)) {
        ww = sqrt(ww);
        const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
        const double twx = tx * ww, twy = ty * ww, twz = tz * ww;
        const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
        const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
        Rd[0] = 1.0 - (tyy + tzz); Rd[1] = txy - twz;          Rd[2] = txz + twy;
        Rd[3] = txy + twz;          Rd[4] = 1.0 - (txx + tzz); Rd[5] = tyz - twx;
        Rd[6] = txz - twy;          Rd[7] = tyz + twx;          Rd[8] = 1.0 - (txx + tyy);
      } else if (tr) {
        tr->ww_negative++;
      }
      double tn[3], Rn[9];
      for (int r = 0; r < 3; ++r) tn[r] = t1[r] + ((R1[r * 3 + 0] * dc[0] + R1[r * 3 + 1] * dc[1]) + R1[r * 3 + 2] * dc[2]);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = (R1[r * 3 + 0] * Rd[0 * 3 + c] + R1[r * 3 + 1] * Rd[1 * 3 + c]) + R1[r * 3 + 2] * Rd[2 * 3 + c];
      memcpy(R1, Rn, sizeof(Rn));
      memcpy(t1, tn, sizeof(tn));
    }
  }
  /* transformation_estimate = estimate.cast<float>().inverse().matrix() (:169): R^T, -(R^T t) in float */
  float Rf[9], tf[3];
  for (int i = 0; i < 9; ++i) Rf[i] = (float)R1[i];
  for (int i = 0; i < 3; ++i) tf[i] = (float)t1[i];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = Rf[c * 3 + r];
    const float v = (Rf[0 * 3 + r] * tf[0] + Rf[1 * 3 + r] * tf[1]) + Rf[2 * 3 + r] * tf[2];
    T[12 + r] = -v;
    T[r * 4 + 3] = 0.0f;
  }
  T[15] = 1.0f;
  free(X); free(M1); free(M2);
  return ok;
}

int orc_g2o_refine(const float* qxyz1, const float* txyz1, const float* qkp, const float* tkp, const int32_t* mq,
                   const int32_t* mt, const int32_t* sel, int nsel, float T[16], int iterations, double depth_cov) {
  return orc_g2o_refine_traced(qxyz1, txyz1, qkp, tkp, mq, mt, sel, nsel, T, iterations, depth_cov, NULL);
}

/* Sensitivity harness: which inlier set the adopted transform was FITTED from (the final inlier set is what that
 * transform then scores; two runs can agree on the latter and still have fitted from different sets). */
static _Thread_local uint64_t tl_fit_source = 0;
static uint64_t* g_trace = NULL; /* orc_match_pairs_mt: one word per pair */
void orc_set_trace(uint64_t* per_pair) { g_trace = per_pair; }
static uint64_t orc_hash_set(const int32_t* v, int n) {
  uint64_t h = 0xcbf29ce484222325ull ^ (uint64_t)n;
  for (int i = 0; i < n; ++i) h = (h ^ (uint64_t)(uint32_t)v[i]) * 0x100000001b3ull;
  return h;
}

int orc_ransac(const float* qxyz1, const float* txyz1, const int32_t* mq,
               const int32_t* mt, int n, const orc_params* prm, uint32_t uid,
               float T[16], float* rmse_out, int32_t* matches, int* n_matches_out,
               int* valid_iterations_out, int* real_iterations_out) {
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  memcpy(T, I16, sizeof(I16));
  *n_matches_out = 0;
  *valid_iterations_out = 0;
  *real_iterations_out = 0;
  if (n <= prm->min_matches) { /* :1087 -- rmse is left untouched by the reference */
    return 0;
  }
  tl_fit_source = 0;
  unsigned int min_inlier_threshold = (unsigned int)prm->min_matches; /* :1094 */
  if ((double)min_inlier_threshold > 0.75 * (double)n)                 /* :1095 */
    min_inlier_threshold = (unsigned int)(0.75 * (double)n);           /* :1098 */

  double inlier_error;
  const float max_dist_m = (float)(double)prm->max_dist_for_inliers; /* :1105 */
  const double sq_max = (double)(max_dist_m * max_dist_m);           /* float product, :1152 */
  const int ransac_iterations = prm->ransac_iterations;

  float rmse = 1e6f; /* :1112 */
  int n_matches = 0;
  unsigned int valid_iterations = 0;
  int real_iterations = 0;

  int32_t inlier[ORC_MAX_MATCHES], refined[ORC_MAX_MATCHES];
  for (int it = 0; (it < ransac_iterations && n >= 4); it++) { /* :1130 */
    double refined_error = 1e6;  /* :1133 */
    int n_refined = 0;           /* :1134 */
    float refined_T[16];
    memcpy(refined_T, I16, sizeof(I16)); /* :1137 */
    uint32_t ids[4];
    int n_inl = orc_sample4(prm->seed, uid, (uint32_t)real_iterations, (uint32_t)n, ids); /* :1135 */
    for (int i = 0; i < n_inl; ++i) inlier[i] = (int32_t)ids[i];
    real_iterations++; /* :1139 */
    uint64_t refined_src = 0;
    for (int refinements = 1; refinements < 20; refinements++) { /* :1140 */
      float Tn[16];
      const uint64_t src = g_trace ? orc_hash_set(inlier, n_inl) : 0;
      orc_fit_transform(qxyz1, txyz1, mq, mt, inlier, n_inl, Tn); /* :1142 */
      if (orc_has_nan16(Tn)) break;                                /* :1144 */
      n_inl = orc_compute_inliers_and_error(qxyz1, txyz1, mq, mt, n, Tn, sq_max,
                                            prm->depth_cov, inlier, &inlier_error); /* :1148 */
      if ((unsigned int)n_inl < min_inlier_threshold || inlier_error > (double)max_dist_m) /* :1154 */
        break;
      if (n_inl >= n_refined && inlier_error <= refined_error) { /* :1160 */
        int prev = n_refined;
        memcpy(refined_T, Tn, sizeof(Tn));
        memcpy(refined, inlier, sizeof(int32_t) * (size_t)n_inl);
        n_refined = n_inl;
        refined_error = inlier_error;
        refined_src = src;
        if (n_inl == prev) break; /* :1166 */
      } else
        break;
    }
    if (n_refined > 0) { /* :1171 */
      valid_iterations++;
      if (refined_error <= (double)rmse && n_refined >= n_matches &&
          (unsigned int)n_refined >= min_inlier_threshold) { /* :1177-1179 */
        rmse = (float)refined_error; /* :1182 double -> float */
        tl_fit_source = refined_src;
        memcpy(T, refined_T, sizeof(refined_T));
        memcpy(matches, refined, sizeof(int32_t) * (size_t)n_refined);
        n_matches = n_refined;
        if ((double)n_refined > (double)n * 0.5) it += 10;  /* :1186 */
        if ((double)n_refined > (double)n * 0.75) it += 10; /* :1187 */
        if ((double)n_refined > (double)n * 0.8) break;     /* :1188 */
      }
    }
  }
  if (valid_iterations == 0) { /* :1192 identity hypothesis */
    int n_inl = orc_compute_inliers_and_error(qxyz1, txyz1, mq, mt, n, I16, sq_max,
                                              prm->depth_cov, inlier, &inlier_error);
    if ((unsigned int)n_inl > min_inlier_threshold && inlier_error < (double)max_dist_m) { /* :1206 */
      memcpy(T, I16, sizeof(I16));
      memcpy(matches, inlier, sizeof(int32_t) * (size_t)n_inl);
      n_matches = n_inl;
      rmse = (float)inlier_error;
      valid_iterations++;
    }
  }
  /* g2o refinement (:1225-1268) is off by default (g2o_transformation_refinement = 0). */
  *rmse_out = rmse;
  *n_matches_out = n_matches;
  *valid_iterations_out = (int)valid_iterations;
  *real_iterations_out = real_iterations;
  return (unsigned int)n_matches >= min_inlier_threshold; /* :1275 */
}

/* ------------------------------------------------------------------------- */
/* The "G2O Refinement" block of getRelativeTransformationTo (node.cpp:1222-1268), applied to what the RANSAC loop    */
/* left (T, rmse, the inlier list `matches`): refine with the inliers, re-score ALL matches, keep the result when it    */
/* is superior (:1239), refine once more when it gained inliers (:1241-1249), adopt when it has at least as many        */
/* inliers as before (:1252-1260).  Runs only for g2o_iterations > 0 and more inliers than min_inlier_threshold (:1226). */
/* Returns the new `found` (:1275).                                                                                      */
/* ------------------------------------------------------------------------- */
int orc_g2o_block_traced(const float* qxyz1, const float* txyz1, const float* qkp, const float* tkp, const int32_t* mq,
                         const int32_t* mt, int n, const orc_params* prm, int g2o_iterations, float T[16], float* rmse_io,
                         int32_t* matches, int* n_matches_io, int* valid_iterations_io, orc_g2o_block_trace* tr) {
  if (tr) { memset(tr, 0, sizeof(*tr)); tr->outcome = ORC_G2O_NOT_RUN; }
  unsigned int min_inlier_threshold = (unsigned int)prm->min_matches;
  if ((double)min_inlier_threshold > 0.75 * (double)n) min_inlier_threshold = (unsigned int)(0.75 * (double)n);
  const float max_dist_m = (float)(double)prm->max_dist_for_inliers;
  const double sq_max = (double)(max_dist_m * max_dist_m); /* :1235 */
  int n_matches = *n_matches_io;
  float rmse = *rmse_io;
  if (g2o_iterations > 0 && (unsigned int)n_matches > min_inlier_threshold) { /* :1226 */
    float Tn[16];
    memcpy(Tn, T, sizeof(Tn)); /* :1228 */
    orc_g2o_refine_traced(qxyz1, txyz1, qkp, tkp, mq, mt, matches, n_matches, Tn, g2o_iterations, prm->depth_cov,
                          tr ? &tr->call[0] : NULL); /* :1229 */
    int32_t inlier[ORC_MAX_MATCHES];
    double inlier_error;
    int n_inl = orc_compute_inliers_and_error(qxyz1, txyz1, mq, mt, n, Tn, sq_max, prm->depth_cov, inlier, &inlier_error); /* :1233 */
    if (tr) {
      tr->n_calls = 1;
      tr->n_inl_first = n_inl;
      tr->outcome = ORC_G2O_REJECTED;
    }
    if (n_inl >= n_matches || ((unsigned int)n_inl >= min_inlier_threshold && inlier_error < (double)rmse)) { /* :1239 */
      if (tr) {
        tr->outcome = ORC_G2O_ENTERED_NOT_ADOPTED;
        tr->entered_by_error = !(n_inl >= n_matches);
      }
      if (n_inl > n_matches) { /* :1241 */
        orc_g2o_refine_traced(qxyz1, txyz1, qkp, tkp, mq, mt, inlier, n_inl, Tn, g2o_iterations, prm->depth_cov,
                              tr ? &tr->call[1] : NULL); /* :1243 */
        n_inl = orc_compute_inliers_and_error(qxyz1, txyz1, mq, mt, n, Tn, sq_max, prm->depth_cov, inlier, &inlier_error); /* :1244 */
        if (tr) tr->n_calls = 2;
      }
      if (n_inl >= n_matches) { /* :1252 */
        if (tr) tr->outcome = tr->n_calls == 2 ? ORC_G2O_ADOPTED_AFTER_SECOND : ORC_G2O_ADOPTED;
        memcpy(T, Tn, sizeof(Tn));                                   /* :1256 */
        memcpy(matches, inlier, sizeof(int32_t) * (size_t)n_inl);    /* :1257 */
        n_matches = n_inl;
        rmse = (float)inlier_error;                                  /* :1258 */
        (*valid_iterations_io)++;                                    /* :1259 */
      }
    }
  }
  *n_matches_io = n_matches;
  *rmse_io = rmse;
  return (unsigned int)n_matches >= min_inlier_threshold; /* :1275 */
}

int orc_g2o_block(const float* qxyz1, const float* txyz1, const float* qkp, const float* tkp, const int32_t* mq,
                  const int32_t* mt, int n, const orc_params* prm, int g2o_iterations, float T[16], float* rmse_io,
                  int32_t* matches, int* n_matches_io, int* valid_iterations_io) {
  return orc_g2o_block_traced(qxyz1, txyz1, qkp, tkp, mq, mt, n, prm, g2o_iterations, T, rmse_io, matches, n_matches_io,
                              valid_iterations_io, NULL);
}

/* the refinement block on a finished pair record (ORB or float matcher): what matchNodePair does after :1324 */
static void orc_result_g2o(const float* qxyz1, const float* qkp, int32_t qid, const float* txyz1, const float* tkp,
                           int32_t tid, const orc_params* prm, int g2o_iterations, orc_result* out,
                           orc_g2o_block_trace* tr) {
  if (tr) { memset(tr, 0, sizeof(*tr)); tr->outcome = ORC_G2O_NOT_RUN; }
  if (g2o_iterations <= 0 || out->n_all < prm->min_matches || out->n_all <= prm->min_matches) return; /* no RANSAC ran (:1319, :1087) */
  if (tr) { /* what the RANSAC loop left, for the threshold edges of :1226 */
    unsigned int thr = (unsigned int)prm->min_matches;
    if ((double)thr > 0.75 * (double)out->n_all) thr = (unsigned int)(0.75 * (double)out->n_all);
    tr->thr = (int32_t)thr;
    tr->thr_clipped = thr != (unsigned int)prm->min_matches;
    tr->n_inl_ransac = out->n_inl;
  }
  orc_g2o_block_trace blk;
  const int found = orc_g2o_block_traced(qxyz1, txyz1, qkp, tkp, out->all_q, out->all_t, out->n_all, prm, g2o_iterations,
                                         out->T, &out->rmse, out->inl_idx, &out->n_inl, &out->valid_iterations,
                                         tr ? &blk : NULL);
  if (tr) {
    const int32_t thr = tr->thr, clipped = tr->thr_clipped, n0 = tr->n_inl_ransac;
    *tr = blk;
    tr->thr = thr; tr->thr_clipped = clipped; tr->n_inl_ransac = n0;
  }
  if (found) {
    out->info_scale = (double)((float)out->n_inl / (out->rmse * out->rmse)); /* node.cpp:1335 */
    out->id1 = tid;
    out->id2 = qid;
  } else {
    out->id1 = out->id2 = -1;
    out->info_scale = 0.0;
  }
}

/* matchNodePair with g2o_transformation_refinement = g2o_iterations; qkp / tkp: KeyPoint.pt of the two nodes */
void orc_match_node_pair_g2o_traced(const uint8_t* qdesc, const float* qxyz1, const float* qkp, uint32_t nq, int32_t qid,
                                    const uint8_t* tdesc, const float* txyz1, const float* tkp, uint32_t nt, int32_t tid,
                                    const orc_params* prm, int g2o_iterations, orc_result* out, orc_g2o_block_trace* tr) {
  orc_match_node_pair(qdesc, qxyz1, nq, qid, tdesc, txyz1, nt, tid, prm, out);
  orc_result_g2o(qxyz1, qkp, qid, txyz1, tkp, tid, prm, g2o_iterations, out, tr);
}

/* the same behind the float matchers: matcher 1 = SiftGPU (orc_match_sift_node_pair), 2 = FLANN (orc_match_float_node_pair) */
void orc_match_float_node_pair_g2o(int matcher, const float* qdesc, const float* qxyz1, const float* qkp, int nq, int32_t qid,
                                   const float* tdesc, const float* txyz1, const float* tkp, int nt, int32_t tid, int dim,
                                   double nn_distance_ratio, const orc_params* prm, int g2o_iterations, orc_result* out,
                                   float* all_dist, orc_g2o_block_trace* tr) {
  if (matcher == 1) orc_match_sift_node_pair(qdesc, qxyz1, nq, qid, tdesc, txyz1, nt, tid, prm, out, all_dist);
  else orc_match_float_node_pair(qdesc, qxyz1, nq, qid, tdesc, txyz1, nt, tid, dim, nn_distance_ratio, prm, out, all_dist);
  orc_result_g2o(qxyz1, qkp, qid, txyz1, tkp, tid, prm, g2o_iterations, out, tr);
}

void orc_match_node_pair_g2o(const uint8_t* qdesc, const float* qxyz1, const float* qkp, uint32_t nq, int32_t qid,
                             const uint8_t* tdesc, const float* txyz1, const float* tkp, uint32_t nt, int32_t tid,
                             const orc_params* prm, int g2o_iterations, orc_result* out) {
  orc_match_node_pair_g2o_traced(qdesc, qxyz1, qkp, nq, qid, tdesc, txyz1, tkp, nt, tid, prm, g2o_iterations, out, NULL);
}

/* ------------------------------------------------------------------------- */
/* matchNodePair -- src/node.cpp:1305-1429 ; MatchingResult matching_result.h   */
/* ------------------------------------------------------------------------- */
void orc_match_node_pair(const uint8_t* qdesc, const float* qxyz1, uint32_t nq, int32_t qid,
                         const uint8_t* tdesc, const float* txyz1, uint32_t nt, int32_t tid,
                         const orc_params* prm, orc_result* out) {
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  memset(out, 0, sizeof(*out));
  out->id1 = out->id2 = -1;       /* matching_result.h:33 */
  out->rmse = 0.0f;               /* matching_result.h:27 */
  memcpy(out->T, I16, sizeof(I16));
  int maxm = prm->max_matches;
  if (maxm > ORC_MAX_MATCHES) maxm = ORC_MAX_MATCHES;
  out->n_all = orc_feature_matching_orb(qdesc, nq, tdesc, nt, maxm, out->all_q, out->all_t,
                                        out->all_hd); /* :1315 */
  int found = 0;
  if (out->n_all < prm->min_matches) { /* :1319 */
    found = 0;
  } else {
    found = orc_ransac(qxyz1, txyz1, out->all_q, out->all_t, out->n_all, prm,
                       orc_pair_uid(qid, tid), out->T, &out->rmse, out->inl_idx, &out->n_inl,
                       &out->valid_iterations, &out->real_iterations); /* :1324 */
    if (out->n_all <= prm->min_matches) out->rmse = 0.0f; /* early return leaves mr.rmse */
  }
  if (found) {
    /* :1335 informationMatrix = I * (inlier_matches.size()/(rmse*rmse)) : float arithmetic */
    out->info_scale = (double)((float)out->n_inl / (out->rmse * out->rmse));
    out->id1 = tid; /* older node, :1337 */
    out->id2 = qid; /* this,       :1338 */
  } else {
    out->id1 = out->id2 = -1; /* :1419-1422 */
    out->info_scale = 0.0;
  }
}

void orc_match_pairs_mt(const uint8_t* const* desc, const float* const* xyz1,
                        const uint32_t* counts, const int32_t* node_ids,
                        const int32_t* pair_q, const int32_t* pair_t, int n_pairs,
                        const orc_params* prm, orc_result* out, int n_threads) {
  /* graph_manager.cpp:541-548: one task per (new, candidate) pair on a pool of
   * one thread per core. */
#ifdef _OPENMP
  if (n_threads > 0) omp_set_num_threads(n_threads);
#pragma omp parallel for schedule(dynamic, 1)
#endif
  for (int p = 0; p < n_pairs; ++p) {
    int q = pair_q[p], t = pair_t[p];
    tl_fit_source = 0;
    orc_match_node_pair(desc[q], xyz1[q], counts[q], node_ids[q], desc[t], xyz1[t], counts[t],
                        node_ids[t], prm, &out[p]);
    if (g_trace) g_trace[p] = tl_fit_source;
  }
}

int orc_num_cores(void) {
#ifdef _OPENMP
  return omp_get_num_procs();
#else
  return 1;
#endif
}

/* ------------------------------------------------------------------------- */
/* A.7 removeDepthless + projectTo3D -- node.cpp:67-97, 900-965; misc2.h:49-65  */
/* kp_xy: n_kp x 2 float (pt.x, pt.y).  depth: rows x cols float32 (metres).    */
/* ------------------------------------------------------------------------- */
int orc_project_to_3d(const float* kp_xy, int n_kp, const float* depth, int rows, int cols,
                      double fx, double fy, double cx_d, double cy_d, double depth_scaling,
                      int max_keypoints, int32_t* kept_idx, float* xyz1) {
  const float fxinv = (float)(1. / fx); /* :913 */
  const float fyinv = (float)(1. / fy); /* :914 */
  const float cx = (float)cx_d;         /* :915 */
  const float cy = (float)cy_d;         /* :916 */
  int n = 0;
  for (int i = 0; i < n_kp; ++i) {
    float px = kp_xy[2 * i], py = kp_xy[2 * i + 1];
    if (px >= (float)cols || px < 0 || py >= (float)rows || py < 0 || isnan(px) || isnan(py))
      continue; /* :931-937 */
    /* :942 depth.at<float>(round(y), round(x)) * depth_scaling : round = half away
     * from zero; the product is float*double -> double -> float Z. */
    int r = (int)roundf(py), c = (int)roundf(px);
    if (r >= rows) r = rows - 1; /* reference reads out of bounds here; clamp */
    if (c >= cols) c = cols - 1;
    float Z = (float)((double)depth[(size_t)r * (size_t)cols + (size_t)c] * depth_scaling);
    if (isnan(Z)) continue; /* :947 */
    /* backProject, misc2.h:62-64 */
    xyz1[4 * n + 0] = (px - cx) * Z * fxinv;
    xyz1[4 * n + 1] = (py - cy) * Z * fyinv;
    xyz1[4 * n + 2] = Z;
    xyz1[4 * n + 3] = 1.0f; /* :955 */
    kept_idx[n] = i;
    ++n;
    if (n >= max_keypoints) break; /* :957 */
  }
  return n;
}

/* ------------------------------------------------------------------------- */
/* "use_feature_min_depth" (parameter_server.cpp:90, default false): the depth of   */
/* a keypoint is the nearest valid depth in its neighbourhood,                       */
/* getMinDepthInNeighborhood (misc.cpp:774-793), in removeDepthless (node.cpp:82),    */
/* projectTo3D (:940) and projectTo3DSiftGPU (:730).                                  */
/*   radius = (diameter - 1) / 2 in float, truncated; the window is                   */
/*   rows [int(y - radius), int(y + radius)) x cols [int(x - radius), int(x + radius))*/
/*   clamped to the image (cv::Range is half open: the last row / column of the       */
/*   symmetric window is NOT part of it); cv::minMaxLoc skips NaN (its `val < min`     */
/*   never holds for NaN) and reports 0 for a window without a comparable value       */
/*   (OpenCV 3.3 minMaxIdx: minidx == 0 -> 0; "parity unpinned", OpenCV is absent);    */
/*   a minimum of 0 becomes NaN (:786-789).                                            */
/* ------------------------------------------------------------------------- */
float orc_min_depth_in_neighborhood(const float* depth, int rows, int cols, float cx, float cy, float diameter) {
  const int radius = (int)((diameter - 1) / 2);
  int top = (int)(cy - (float)radius); top = top < 0 ? 0 : top;
  int left = (int)(cx - (float)radius); left = left < 0 ? 0 : left;
  int bot = (int)(cy + (float)radius); bot = bot > rows ? rows : bot;
  int right = (int)(cx + (float)radius); right = right > cols ? cols : right;
  float minv = FLT_MAX;
  int found = 0;
  for (int r = top; r < bot; ++r)
    for (int c = left; c < right; ++c) {
      const float v = depth[(size_t)r * (size_t)cols + (size_t)c];
      if (v < minv) { minv = v; found = 1; }
    }
  double minZ = found ? (double)minv : 0.0;
  if (minZ == 0.0) minZ = (double)NAN;
  return (float)minZ;
}

/* removeDepthless with use_feature_min_depth (node.cpp:66-97): kept input positions */
int orc_remove_depthless_min_depth(const float* kp_xy, const float* kp_size, int n_kp, const float* depth, int rows,
                                   int cols, int32_t* kept_idx) {
  int n = 0;
  for (int i = 0; i < n_kp; ++i) {
    const float px = kp_xy[2 * i], py = kp_xy[2 * i + 1];
    if (px >= (float)cols || px < 0 || py >= (float)rows || py < 0 || isnan(px) || isnan(py)) continue;
    const float Z = orc_min_depth_in_neighborhood(depth, rows, cols, px, py, kp_size[i]);
    if (isnan(Z)) continue;
    kept_idx[n++] = i;
  }
  return n;
}

/* projectTo3D with use_feature_min_depth (node.cpp:900-965, :940) */
int orc_project_to_3d_min_depth(const float* kp_xy, const float* kp_size, int n_kp, const float* depth, int rows,
                                int cols, double fx, double fy, double cx_d, double cy_d, double depth_scaling,
                                int max_keypoints, int32_t* kept_idx, float* xyz1) {
  const float fxinv = (float)(1. / fx), fyinv = (float)(1. / fy), cx = (float)cx_d, cy = (float)cy_d;
  int n = 0;
  for (int i = 0; i < n_kp; ++i) {
    const float px = kp_xy[2 * i], py = kp_xy[2 * i + 1];
    if (px >= (float)cols || px < 0 || py >= (float)rows || py < 0 || isnan(px) || isnan(py)) continue;
    /* :941 getMinDepthInNeighborhood(...) * depth_scaling: float * double -> double -> float Z */
    const float Z = (float)((double)orc_min_depth_in_neighborhood(depth, rows, cols, px, py, kp_size[i]) * depth_scaling);
    if (isnan(Z)) continue;
    xyz1[4 * n + 0] = (px - cx) * Z * fxinv;
    xyz1[4 * n + 1] = (py - cy) * Z * fyinv;
    xyz1[4 * n + 2] = Z;
    xyz1[4 * n + 3] = 1.0f;
    kept_idx[n] = i;
    ++n;
    if (n >= max_keypoints) break;
  }
  return n;
}

/* ------------------------------------------------------------------------- */
/* a22(i)  Node::projectTo3D, point-cloud overload -- node.cpp:855-898 (the ctor   */
/* that receives the sensor's organised cloud, node.cpp:252-369: detect ->         */
/* projectTo3D(cloud) -> compute, no retainBest).  The lookup truncates the        */
/* coordinates, point_cloud->at((int)x, (int)y) (:877); a point is dropped when     */
/* z > maximum_depth (float promoted to double) or any coordinate is NaN (:880);    */
/* the stored point is the cloud's own (x, y, z, 1) (:887); cut at max_keypoints.   */
/* cloud: rows x cols x 4 float (x, y, z, rgb).                                    */
/* ------------------------------------------------------------------------- */
int orc_project_to_3d_cloud(const float* kp_xy, int n_kp, const float* cloud, int rows, int cols,
                            double maximum_depth, int max_keypoints, int32_t* kept_idx, float* xyz1) {
  int n = 0;
  for (int i = 0; i < n_kp; ++i) {
    float px = kp_xy[2 * i], py = kp_xy[2 * i + 1];
    if (px >= (float)cols || px < 0 || py >= (float)rows || py < 0 || isnan(px) || isnan(py))
      continue; /* :868-875 (width/height are uint32: the comparison is done in float) */
    const float* p3 = cloud + 4 * ((size_t)(int)py * (size_t)cols + (size_t)(int)px); /* :877 */
    if (((double)p3[2] > maximum_depth) || isnan(p3[0]) || isnan(p3[1]) || isnan(p3[2])) continue; /* :880 */
    xyz1[4 * n + 0] = p3[0];
    xyz1[4 * n + 1] = p3[1];
    xyz1[4 * n + 2] = p3[2];
    xyz1[4 * n + 3] = 1.0f; /* :887 */
    kept_idx[n] = i;
    ++n;
    if (n >= max_keypoints) break; /* :889 */
  }
  return n;
}

/* ------------------------------------------------------------------------- */
/* a20  Node::projectTo3DSiftGPU -- node.cpp:695-769 (SIFTGPU feature path)     */
/* Differences to orc_project_to_3d: the depth lookup is depth.at<float>(p2d.y,  */
/* p2d.x), i.e. the float coordinates are converted to int by TRUNCATION (:733),  */
/* and there is no inside-the-image test (SiftGPU keypoints lie inside; an index   */
/* outside is undefined behaviour in the reference -- clamped to the image here).  */
/* The used descriptors are then re-packed densely (:752-766).                     */
/* ------------------------------------------------------------------------- */
static int orc_trunc_clamp(float v, int hi) {
  int i = isnan(v) ? 0 : (v <= -2147483648.0f ? INT32_MIN : (v >= 2147483648.0f ? INT32_MAX : (int)v));
  if (i < 0) i = 0;
  if (i > hi) i = hi;
  return i;
}
int orc_project_to_3d_sift(const float* kp_xy, int n_kp, const float* depth, int rows, int cols,
                           double fx, double fy, double cx_d, double cy_d, double depth_scaling,
                           int max_keypoints, int32_t* kept_idx, float* xyz1) {
  const float fxinv = (float)(1. / fx); /* :709 */
  const float fyinv = (float)(1. / fy); /* :710 */
  const float cx = (float)cx_d;         /* :711 */
  const float cy = (float)cy_d;         /* :712 */
  int n = 0;
  for (int i = 0; i < n_kp && n < max_keypoints; ++i) { /* :748 break once max_keyp are kept */
    const float px = kp_xy[2 * i], py = kp_xy[2 * i + 1];
    const int r = orc_trunc_clamp(py, rows - 1), c = orc_trunc_clamp(px, cols - 1);
    const float Z = (float)((double)depth[(size_t)r * (size_t)cols + (size_t)c] * depth_scaling); /* :733 */
    if (isnan(Z)) continue; /* :736-740 */
    xyz1[4 * n + 0] = (px - cx) * Z * fxinv; /* backProject, misc2.h:62-64 */
    xyz1[4 * n + 1] = (py - cy) * Z * fyinv;
    xyz1[4 * n + 2] = Z;
    xyz1[4 * n + 3] = 1.0f; /* :745 */
    kept_idx[n] = i;        /* featuresUsed, :746 */
    ++n;
  }
  return n;
}

/* projectTo3DSiftGPU with use_feature_min_depth (node.cpp:727-731): Z = getMinDepthInNeighborhood(depth, p2d, size) *
 * depth_scaling, everything else as above (no inside-the-image test either: the neighbourhood is clamped, :781-784) */
int orc_project_to_3d_sift_min_depth(const float* kp_xy, const float* kp_size, int n_kp, const float* depth, int rows,
                                     int cols, double fx, double fy, double cx_d, double cy_d, double depth_scaling,
                                     int max_keypoints, int32_t* kept_idx, float* xyz1) {
  const float fxinv = (float)(1. / fx), fyinv = (float)(1. / fy), cx = (float)cx_d, cy = (float)cy_d;
  int n = 0;
  for (int i = 0; i < n_kp && n < max_keypoints; ++i) {
    const float px = kp_xy[2 * i], py = kp_xy[2 * i + 1];
    const float Z = (float)((double)orc_min_depth_in_neighborhood(depth, rows, cols, px, py, kp_size[i]) * depth_scaling); /* :731 */
    if (isnan(Z)) continue;
    xyz1[4 * n + 0] = (px - cx) * Z * fxinv;
    xyz1[4 * n + 1] = (py - cy) * Z * fyinv;
    xyz1[4 * n + 2] = Z;
    xyz1[4 * n + 3] = 1.0f;
    kept_idx[n] = i;
    ++n;
  }
  return n;
}

/* descriptors_out / siftgpu_descriptors (:752-766): row y <- descriptors_in[featuresUsed[y]] */
void orc_gather_rows_f32(const float* in, const int32_t* kept_idx, int n, int dim, float* out) {
  for (int y = 0; y < n; ++y)
    for (int x = 0; x < dim; ++x) out[(size_t)y * dim + x] = in[(size_t)kept_idx[y] * dim + x];
}

/* squareroot_descriptor_space -- node.cpp:1557-1571 (RootSIFT), in place.
 * cv::abs, then cv::reduce(..., 1, CV_REDUCE_SUM, CV_32FC1): OpenCV 3.3 reduceC_<float,float,OpAdd>
 * keeps two float accumulators, a0 over columns 0,2,4,... and a1 over 1,3,5,... in steps of four, adds the
 * leftover columns to a0 and returns a0 + a1 (modules/core/src/matrix.cpp, "parity unpinned": OpenCV is
 * not in the tree).  Rows whose sum is 0 stay as they are (:1565); else d <- sqrt(d / sum) (:1569). */
void orc_root_sift(float* desc, int n_rows, int dim) {
  for (int r = 0; r < n_rows; ++r) {
    float* d = desc + (size_t)r * dim;
    for (int c = 0; c < dim; ++c) d[c] = fabsf(d[c]);
    float sum;
    if (dim == 1) {
      sum = d[0];
    } else {
      float a0 = d[0], a1 = d[1];
      int i = 2;
      for (; i <= dim - 4; i += 4) {
        a0 = a0 + d[i];
        a1 = a1 + d[i + 1];
        a0 = a0 + d[i + 2];
        a1 = a1 + d[i + 3];
      }
      for (; i < dim; ++i) a0 = a0 + d[i];
      sum = a0 + a1;
    }
    if (sum == 0.0f) continue;
    for (int c = 0; c < dim; ++c) d[c] = sqrtf(d[c] / sum);
  }
}

/* ========================================================================= */
/* SURVEY 8(f) "next" rows 3 and 2: the data either side of the pair path        */
/*   depthToCV8UC1            misc.cpp:414-430  (detection mask from depth)       */
/*   createXYZRGBPointCloud   misc.cpp:467-556  (structured cloud of a frame)      */
/*   observationLikelihood    misc.cpp:814-969  (environment measurement model,    */
/*                            called from matchNodePair, node.cpp:1340-1343, when  */
/*                            observability_threshold > 0)                          */
/*   observation_criterion_met misc.cpp:1136-1148                                    */
/* Third-party arithmetic (OpenCV convertTo, pcl::transformPointCloud) is restated   */
/* from the published sources: "parity unpinned".                                    */
/* ========================================================================= */

/* cv::Mat::convertTo(CV_8UC1, alpha, beta) for a float source: saturate_cast<uchar>(cvRound(v*alpha + beta))
 * with the product and sum in float (cvtScale_<float, uchar, float>) and cvRound = round-half-to-even
 * (cvtss2si); NaN and out-of-int-range values convert to INT_MIN, which saturates to 0. */
static uint8_t orc_sat_u8_from_float(float t) {
  if (!(t > -2147483648.0f && t < 2147483648.0f)) return 0; /* cvtss2si "integer indefinite" -> saturates to 0 */
  const int r = (int)lrintf(t); /* current rounding mode: nearest-even */
  return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}
/* depthToCV8UC1, CV_32FC1 branch (misc.cpp:417-418): mono8 = convertTo(CV_8UC1, 100, 0) */
void orc_depth_to_mono8_f32(const float* depth, size_t n, uint8_t* mono8) {
  for (size_t i = 0; i < n; ++i) mono8[i] = orc_sat_u8_from_float(depth[i] * 100.0f + 0.0f);
}
/* CV_16UC1 branch (misc.cpp:420-426): mono8 = convertTo(CV_8UC1, 0.05, -25), depth(float, metres) =
 * convertTo(CV_32FC1, 0.001, 0) */
void orc_depth_u16_to_mono8_f32(const uint16_t* depth_mm, size_t n, uint8_t* mono8, float* depth_m) {
  for (size_t i = 0; i < n; ++i) {
    const float v = (float)depth_mm[i];
    mono8[i] = orc_sat_u8_from_float(v * 0.05f + -25.0f);
    depth_m[i] = v * 0.001f + 0.0f;
  }
}

/* createXYZRGBPointCloud (misc.cpp:467-556), depth and colour image of the same size, skip step s.
 * cloud: ceil(rows/s) x ceil(cols/s) points of 4 floats (x, y, z, rgb bits).  rgb may be NULL (colour
 * bits 0), channels 1 or 3, encoding_bgr swaps red and blue (:488).  Quirk kept: the colour of the very
 * first pixel is never written (`color_idx > 0`, :536): its rgb stays 0. */
void orc_create_point_cloud(const float* depth, int rows, int cols, const uint8_t* rgb, int channels,
                            int encoding_bgr, double fx, double fy, double cx_d, double cy_d,
                            double depth_scaling, double min_depth_d, int s, float* cloud) {
  float fxinv = (float)fx, fyinv = (float)fy; /* getCameraIntrinsics assigns double -> float (:59-62) */
  const float cx = (float)cx_d, cy = (float)cy_d;
  fxinv = (float)(1. / fxinv); /* :67-68 */
  fyinv = (float)(1. / fyinv);
  const int ch = (int)ceil(rows / (float)s), cw = (int)ceil(cols / (float)s); /* :482-483 */
  const float min_depth = (float)min_depth_d;                                   /* :506 */
  const unsigned int pix = (unsigned int)channels;
  const unsigned int color_pix_step = pix * (unsigned int)(cols / cw);                          /* :491 */
  const unsigned int color_row_step = pix * (unsigned int)(rows / ch - 1) * (unsigned int)cols; /* :492 */
  const unsigned int depth_pix_step = (unsigned int)(cols / cw);                                /* :493 */
  const unsigned int depth_row_step = (unsigned int)(rows / ch - 1) * (unsigned int)cols;       /* :494 */
  const int red_idx = (channels == 3 && encoding_bgr) ? 2 : 0, green_idx = 1;
  const int blue_idx = (channels == 3 && encoding_bgr) ? 0 : 2;
  const size_t color_total = (size_t)rows * (size_t)cols * color_pix_step; /* rgb_img.total()*color_pix_step */
  unsigned int color_idx = 0, depth_idx = 0;
  size_t k = 0;
  const size_t n_pts = (size_t)ch * (size_t)cw;
  for (size_t i = 0; i < n_pts; ++i) { cloud[4 * i] = cloud[4 * i + 1] = cloud[4 * i + 2] = 0.f; cloud[4 * i + 3] = 0.f; }
  for (int v = 0; v < rows; v += s, color_idx += color_row_step, depth_idx += depth_row_step) {
    for (int u = 0; u < cols; u += s, color_idx += color_pix_step, depth_idx += depth_pix_step, ++k) {
      if (k == n_pts) break; /* :514 */
      float* pt = cloud + 4 * k;
      const float Z = (float)((double)depth[depth_idx] * depth_scaling); /* :522 */
      if (!(Z >= min_depth)) { /* :525, also NaN */
        pt[0] = (float)((double)((float)u - cx) * 1.0 * (double)fxinv); /* :527 */
        pt[1] = (float)((double)((float)v - cy) * 1.0 * (double)fyinv);
        pt[2] = NAN;
      } else { /* backProject(fxinv, fyinv, cx, cy, u, v, Z, ...), misc2.h:62-64 with u, v as float */
        pt[0] = ((float)u - cx) * Z * fxinv;
        pt[1] = ((float)v - cy) * Z * fyinv;
        pt[2] = Z;
      }
      if (rgb && color_idx > 0 && (size_t)color_idx < color_total) { /* :536 */
        uint32_t r, g, b;
        if (channels == 3) {
          r = rgb[color_idx + red_idx]; g = rgb[color_idx + green_idx]; b = rgb[color_idx + blue_idx];
        } else {
          r = g = b = rgb[color_idx];
        }
        const uint32_t bits = b | (g << 8) | (r << 16); /* RGBValue: Blue, Green, Red, Alpha = 0 */
        memcpy(pt + 3, &bits, 4);
      }
    }
  }
}

/* observationLikelihood (misc.cpp:814-969): the new frame's cloud, transformed by T (new -> old, row-major
 * 4x4 float), is projected into the old frame's raster; every emm__skip_step-th point is classified against
 * the old cloud's depth in a 5x5 neighbourhood sampled with step 2.  Returns inliers / outliers / occluded /
 * all.  fx..cy are the OLD camera's intrinsics (already assigned to float by getCameraIntrinsics) and are
 * divided by cloud_skip (:866-871); depth_covariance() is the frozen value (a18) = depth_cov.
 * pcl::transformPointCloud on a non-dense cloud (PCL 1.7 common/impl/transforms.hpp) leaves points with a
 * non-finite coordinate untouched and computes the others as
 *   x' = T00*x + T01*y + T02*z + T03   (float, left to right). */
void orc_observation_likelihood(const float* new_cloud, const float* old_cloud, int ch, int cw,
                                const float* T, double fx_d, double fy_d, double cx_d, double cy_d,
                                int cloud_skip, int skip_step, double depth_cov, uint32_t counts[4]) {
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  if (skip_step <= 0 || ch <= 1 || cw <= 1) { counts[0] = counts[3] = 1; return; } /* :829-843 */
  float fx = (float)fx_d, fy = (float)fy_d, cx = (float)cx_d, cy = (float)cy_d;
  fx = fx / cloud_skip; fy = fy / cloud_skip; cx = cx / cloud_skip; cy = cy / cloud_skip; /* :868-871 */
  unsigned int good_points = 0, bad_points = 0, occluded_points = 0, all = 0;
  for (int new_ry = 0; new_ry < ch; new_ry += skip_step) {
    for (int new_rx = 0; new_rx < cw; new_rx += skip_step, all++) {
      const float* q = new_cloud + 4 * ((size_t)new_ry * cw + new_rx);
      float px = q[0], py = q[1], pz = q[2];
      if (isfinite(px) && isfinite(py) && isfinite(pz)) {
        const float x = px, y = py, z = pz;
        px = T[0] * x + T[1] * y + T[2] * z + T[3];
        py = T[4] * x + T[5] * y + T[6] * z + T[7];
        pz = T[8] * x + T[9] * y + T[10] * z + T[11];
      }
      if (pz != pz) continue;  /* :886 */
      if (pz < 0) continue;    /* :887 */
      /* round(float d) = (int)floor(d + 0.5) with the sum in double (:804-807); the reference's cast of a
       * non-finite or huge value is undefined: such projections are treated as outside the raster */
      const double dx = floor((double)((px / pz) * fx + cx) + 0.5);
      const double dy = floor((double)((py / pz) * fy + cy) + 0.5);
      if (!(dx >= 0.0 && dx < (double)cw && dy >= 0.0 && dy < (double)ch)) continue; /* :891-896 */
      const int old_rx_center = (int)dx, old_ry_center = (int)dy;
      const int nbhd = 2;
      int good_point = 0, occluded_point = 0, bad_point = 0;
      const int startx = old_rx_center - nbhd > 0 ? old_rx_center - nbhd : 0;
      const int starty = old_ry_center - nbhd > 0 ? old_ry_center - nbhd : 0;
      const int endx = cw < old_rx_center + nbhd + 1 ? cw : old_rx_center + nbhd + 1;
      const int endy = ch < old_ry_center + nbhd + 1 ? ch : old_ry_center + nbhd + 1;
      for (int old_ry = starty; old_ry < endy; old_ry += 2) {
        for (int old_rx = startx; old_rx < endx; old_rx += 2) {
          const float oz = old_cloud[4 * ((size_t)old_ry * cw + old_rx) + 2];
          if (oz != oz) continue; /* :911 */
          const double old_sigma = cloud_skip * depth_cov; /* :914 */
          const double new_sigma = cloud_skip * depth_cov; /* :916 */
          const double joint_sigma = old_sigma + new_sigma;
          /* cdf(old_p.z, p.z, sqrt(joint_sigma)), :809-812 with SQRT_2 = 1.41421 (:801) */
          const double sigma = sqrt(joint_sigma);
          const double p_new_in_front = 0.5 * (1 + erf(((double)oz - (double)pz) / (sigma * 1.41421)));
          if (p_new_in_front < 0.001) occluded_point = 1;
          else if (p_new_in_front < 0.999) good_point = 1;
          else bad_point = 1;
        }
      }
      if (good_point) good_points++;
      else if (occluded_point) occluded_points++;
      else if (bad_point) bad_points++;
    }
  }
  counts[0] = good_points; counts[1] = bad_points; counts[2] = occluded_points; counts[3] = all;
}

/* Boundaries of the two cdf tests as arguments of erf: the smallest doubles q with
 * 0.5*(1+erf(q)) >= 0.001 resp. >= 0.999 under THIS libm (bisection).  For a monotone erf,
 * p < 0.001 <=> q < q_lo and p < 0.999 <=> q < q_hi; the device compares against these constants instead of
 * evaluating erf. */
void orc_emm_erf_boundaries(double* q_lo, double* q_hi) {
  const double target[2] = {0.001, 0.999};
  double out[2];
  for (int k = 0; k < 2; ++k) {
    double lo = -8.0, hi = 8.0; /* f(lo) < target <= f(hi) */
    for (;;) {
      const double mid = lo + (hi - lo) * 0.5;
      if (!(mid > lo && mid < hi)) break;
      if (0.5 * (1 + erf(mid)) >= target[k]) hi = mid; else lo = mid;
    }
    out[k] = hi;
  }
  *q_lo = out[0];
  *q_hi = out[1];
}

/* observation_criterion_met (misc.cpp:1136-1148) */
int orc_observation_criterion_met(unsigned int inliers, unsigned int outliers, unsigned int all,
                                  double obs_thresh, double* quality) {
  if (obs_thresh < 0) return 1;
  *quality = inliers / (double)(inliers + outliers);
  const double certainty = inliers / (double)all;
  return (*quality > obs_thresh) && (certainty > 0.25);
}


/* ========================================================================= */
/* SIFT (128-d float descriptor) matcher: SiftGPUWrapper::match semantics      */
/* src/sift_gpu_wrapper.cpp:169-227 over SiftMatchGPU (CUDA back end):          */
/*   external/SiftGPU/src/SiftGPU/SiftMatchCU.cpp:87-100  (u8 quantisation)     */
/*   ProgramCU.cu:1405-1482 MultiplyDescriptor_Kernel (u8 dot products + per-8- */
/*     row column partials), :1689-1743 RowMatch_Kernel, :1764-1782             */
/*     ColMatch_Kernel, SiftMatchCU.cpp:148-177 GetBestMatch (mutual best).     */
/* ========================================================================= */
#define ORC_SIFT_DIM 128
#define ORC_SIFT_MAX 4096 /* sift_gpu_wrapper.cpp:231 CreateNewSiftMatchGPU(4096) */

static void orc_sift_quantise(const float* d, int n, unsigned char* q) {
  /* SiftMatchCU.cpp:96-99: pub[i] = int(512 * descriptors[i] + 0.5); */
  for (int i = 0; i < n * ORC_SIFT_DIM; ++i) q[i] = (unsigned char)(int)(512 * d[i] + 0.5);
}

static float orc_sift_angle(int dot) {
  /* ProgramCU.cu:1738: acos(min(dot * 0.000003814697265625f, 1.0)) : float product, double
   * min / acos, float result */
  float prod = (float)dot * 0.000003814697265625f;
  double v = (double)prod < 1.0 ? (double)prod : 1.0;
  return (float)acos(v);
}

/* Returns number of matches; mq/mt/dist sized >= n1. */
int orc_sift_match(const float* d1, int n1, const float* d2, int n2, int32_t* mq, int32_t* mt,
                   float* dist_out) {
  if (n1 > ORC_SIFT_MAX) n1 = ORC_SIFT_MAX; /* SiftMatchCU.cpp:93 */
  if (n2 > ORC_SIFT_MAX) n2 = ORC_SIFT_MAX;
  if (n1 <= 0 || n2 <= 0) return 0; /* SiftMatchCU.cpp:141 */
  const float distmax = 0.9f, ratiomax = 0.9f; /* sift_gpu_wrapper.cpp:185 */
  unsigned char* q1 = (unsigned char*)malloc((size_t)n1 * ORC_SIFT_DIM);
  unsigned char* q2 = (unsigned char*)malloc((size_t)n2 * ORC_SIFT_DIM);
  orc_sift_quantise(d1, n1, q1);
  orc_sift_quantise(d2, n2, q2);
  int* dot = (int*)malloc(sizeof(int) * (size_t)n2);
  int* row_match = (int*)malloc(sizeof(int) * (size_t)n1);
  /* column state merged over 8-row blocks in block order (ColMatch_Kernel) */
  int* cmax = (int*)calloc((size_t)n2, sizeof(int));
  int* cidx = (int*)malloc(sizeof(int) * (size_t)n2);
  int* cnxt = (int*)calloc((size_t)n2, sizeof(int));
  int* bmax = (int*)malloc(sizeof(int) * (size_t)n2);
  int* bidx = (int*)malloc(sizeof(int) * (size_t)n2);
  int* bnxt = (int*)malloc(sizeof(int) * (size_t)n2);
  for (int j = 0; j < n2; ++j) cidx[j] = -1;
  int first_block = 1;
  for (int i0 = 0; i0 < n1; i0 += 8) {
    for (int j = 0; j < n2; ++j) { bmax[j] = 0; bidx[j] = -1; bnxt[j] = 0; } /* :1457 */
    for (int i = i0; i < i0 + 8 && i < n1; ++i) {
      const unsigned char* a = q1 + (size_t)i * ORC_SIFT_DIM;
      for (int j = 0; j < n2; ++j) {
        const unsigned char* b = q2 + (size_t)j * ORC_SIFT_DIM;
        int s = 0;
        for (int k = 0; k < ORC_SIFT_DIM; ++k) s += (int)a[k] * (int)b[k];
        dot[j] = s;
        /* :1464-1467 */
        if (s > bmax[j]) { bnxt[j] = bmax[j]; bmax[j] = s; bidx[j] = i; }
        else if (s > bnxt[j]) bnxt[j] = s;
      }
      /* RowMatch_Kernel: 32 threads scan columns t, t+32, ... then a tree reduction */
      int tmax[32], tnxt[32], tidx[32];
      for (int t = 0; t < 32; ++t) {
        int m = 0, nx = 0, id = -1;
        for (int j = t; j < n2; j += 32) {
          int v = dot[j];
          int test = v > m;
          nx = test ? m : (nx > v ? nx : v);
          id = test ? j : id;
          m = test ? v : m;
        }
        tmax[t] = m; tnxt[t] = nx; tidx[t] = id;
      }
      for (int step = 16; step > 0; step /= 2)
        for (int t = 0; t < step; ++t) {
          int v1 = tmax[t], v2 = tmax[t + step];
          int test = v2 > v1;
          int a1 = v1 > tnxt[t + step] ? v1 : tnxt[t + step];
          int a2 = tnxt[t] > v2 ? tnxt[t] : v2;
          tnxt[t] = test ? a1 : a2;
          tidx[t] = test ? tidx[t + step] : tidx[t];
          tmax[t] = test ? v2 : v1;
        }
      float dist = orc_sift_angle(tmax[0]);
      float distn = orc_sift_angle(tnxt[0]);
      row_match[i] = (dist < distmax) && (dist < distn * ratiomax) ? tidx[0] : -1; /* :1742 */
    }
    /* ColMatch_Kernel :1769-1776 */
    for (int j = 0; j < n2; ++j) {
      if (first_block) { cmax[j] = bmax[j]; cidx[j] = bidx[j]; cnxt[j] = bnxt[j]; }
      else if (cmax[j] < bmax[j]) { cnxt[j] = cmax[j] > bnxt[j] ? cmax[j] : bnxt[j]; cmax[j] = bmax[j]; cidx[j] = bidx[j]; }
      else { cnxt[j] = cnxt[j] > bmax[j] ? cnxt[j] : bmax[j]; }
    }
    first_block = 0;
  }
  /* GetBestMatch (SiftMatchCU.cpp:161-171) + the wrapper loop (sift_gpu_wrapper.cpp:194-222) */
  int number = 0;
  for (int i = 0; i < n1 && number < n1; ++i) {
    int j = row_match[i];
    if (j < 0) continue;
    float dist = orc_sift_angle(cmax[j]);
    float distn = orc_sift_angle(cnxt[j]);
    int col_match = (dist < distmax) && (dist < distn * ratiomax) ? cidx[j] : -1;
    if (col_match == i) { mq[number] = i; mt[number] = j; ++number; }
  }
  int n_out = 0, counter = 0;
  for (int m = 0; m < number; ++m) {
    if (mq[m] == 0 || mt[m] == 0) counter++;            /* :199 */
    if ((double)counter > 0.5 * (double)number) { n_out = 0; break; } /* :203 "context error" */
    float sum = 0;
    for (int k = 0; k < ORC_SIFT_DIM; ++k) {
      float a = d1[(size_t)mq[m] * ORC_SIFT_DIM + k] - d2[(size_t)mt[m] * ORC_SIFT_DIM + k];
      float sq = a * a;
      sum += sq;
    }
    dist_out[n_out] = sqrtf(sum); /* :217 */
    mq[n_out] = mq[m];
    mt[n_out] = mt[m];
    ++n_out;
  }
  free(q1); free(q2); free(dot); free(row_match); free(cmax); free(cidx); free(cnxt);
  free(bmax); free(bidx); free(bnxt);
  return n_out;
}

/* matchNodePair with matcher_type == SIFTGPU: SiftGPUWrapper::match, keepStrongestMatches by the
 * L2 distance (node.cpp:553-557, 674), then the same RANSAC. */
/* ------------------------------------------------------------------------- */
/* a11  Node::featureMatching, FLANN branch for float descriptors (node.cpp:610-667) with EXACT neighbours.  */
/* The reference searches 4 randomised kd-trees with 16 checks (:493-505, :634): approximate, not reproducible.  */
/* What it does with the neighbours is restated exactly: ratio of FLANN's squared-L2 distances (:645), accepted   */
/* when nn_distance_ratio > ratio (:648), a train index is used once, first come first served in query order    */
/* (:650-653), DMatch.distance = ratio (:657).  Squared distance in flann::L2<float>::operator()'s order (FLANN   */
/* 1.8 dist.h, not in the tree): four differences per step, result += ((d0*d0 + d1*d1) + d2*d2) + d3*d3.           */
/* desc rows are `dim` floats (dim % 4 == 0).  Returns the number of matches, in query order.                      */
/* ------------------------------------------------------------------------- */
int orc_flann_match(const float* qdesc, int nq, const float* tdesc, int nt, int dim, double nn_distance_ratio,
                    int32_t* mq, int32_t* mt, float* md) {
  if (nq <= 0 || nt < 2) return 0; /* knnSearch with k = 2 */
  char* used = (char*)calloc((size_t)nt, 1);
  int n = 0;
  for (int i = 0; i < nq; ++i) {
    const float* a = qdesc + (size_t)i * dim;
    float b1 = INFINITY, b2 = INFINITY;
    int i1 = -1;
    for (int j = 0; j < nt; ++j) {
      const float* b = tdesc + (size_t)j * dim;
      float result = 0.0f;
      for (int k = 0; k < dim; k += 4) {
        const float d0 = a[k] - b[k], d1 = a[k + 1] - b[k + 1], d2 = a[k + 2] - b[k + 2], d3 = a[k + 3] - b[k + 3];
        result += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
      }
      if (result < b1) { b2 = b1; b1 = result; i1 = j; }
      else if (result < b2) b2 = result;
    }
    const float ratio = b1 / b2;                 /* :645 */
    if (nn_distance_ratio > (double)ratio) {     /* :648 */
      if (i1 < 0 || used[i1]) continue;          /* :650-651 */
      used[i1] = 1;                              /* :653 */
      mq[n] = i; mt[n] = i1; md[n] = ratio;      /* :654-657 */
      ++n;
    }
  }
  free(used);
  return n;
}

static void orc_match_list_node_pair(int32_t* mq, int32_t* mt, float* md, int n, int cap, const float* qxyz1, int32_t qid,
                                     const float* txyz1, int32_t tid, const orc_params* prm, orc_result* out,
                                     float* all_dist);

void orc_match_float_node_pair(const float* qdesc, const float* qxyz1, int nq, int32_t qid, const float* tdesc,
                               const float* txyz1, int nt, int32_t tid, int dim, double nn_distance_ratio,
                               const orc_params* prm, orc_result* out, float* all_dist) {
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  memset(out, 0, sizeof(*out));
  out->id1 = out->id2 = -1;
  memcpy(out->T, I16, sizeof(I16));
  int cap = nq > 0 ? nq : 1;
  int32_t* mq = (int32_t*)malloc(sizeof(int32_t) * (size_t)cap);
  int32_t* mt = (int32_t*)malloc(sizeof(int32_t) * (size_t)cap);
  float* md = (float*)malloc(sizeof(float) * (size_t)cap);
  int n = orc_flann_match(qdesc, nq, tdesc, nt, dim, nn_distance_ratio, mq, mt, md);
  orc_match_list_node_pair(mq, mt, md, n, cap, qxyz1, qid, txyz1, tid, prm, out, all_dist);
}

void orc_match_sift_node_pair(const float* qdesc, const float* qxyz1, int nq, int32_t qid,
                              const float* tdesc, const float* txyz1, int nt, int32_t tid,
                              const orc_params* prm, orc_result* out, float* all_dist) {
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  memset(out, 0, sizeof(*out));
  out->id1 = out->id2 = -1;
  memcpy(out->T, I16, sizeof(I16));
  int cap = nq > 0 ? nq : 1;
  int32_t* mq = (int32_t*)malloc(sizeof(int32_t) * (size_t)cap);
  int32_t* mt = (int32_t*)malloc(sizeof(int32_t) * (size_t)cap);
  float* md = (float*)malloc(sizeof(float) * (size_t)cap);
  int n = orc_sift_match(qdesc, nq, tdesc, nt, mq, mt, md);
  orc_match_list_node_pair(mq, mt, md, n, cap, qxyz1, qid, txyz1, tid, prm, out, all_dist);
}

/* keepStrongestMatches + RANSAC + edge assembly over a (queryIdx, trainIdx, distance) list; frees the lists */
static void orc_match_list_node_pair(int32_t* mq, int32_t* mt, float* md, int n, int cap, const float* qxyz1, int32_t qid,
                                     const float* txyz1, int32_t tid, const orc_params* prm, orc_result* out,
                                     float* all_dist) {
  int maxm = prm->max_matches > ORC_MAX_MATCHES ? ORC_MAX_MATCHES : prm->max_matches;
  /* keep the max_matches smallest by (distance, queryIdx) (D2), ascending */
  char* used = (char*)calloc((size_t)cap, 1);
  int n_all = 0;
  while (n_all < maxm && n_all < n) {
    int best = -1;
    for (int m = 0; m < n; ++m) {
      if (used[m]) continue;
      if (best < 0 || md[m] < md[best] || (md[m] == md[best] && mq[m] < mq[best])) best = m;
    }
    used[best] = 1;
    out->all_q[n_all] = mq[best];
    out->all_t[n_all] = mt[best];
    out->all_hd[n_all] = 0;
    all_dist[n_all] = md[best];
    ++n_all;
  }
  out->n_all = n_all;
  free(mq); free(mt); free(md); free(used);
  int found = 0;
  if (out->n_all >= prm->min_matches)
    found = orc_ransac(qxyz1, txyz1, out->all_q, out->all_t, out->n_all, prm, orc_pair_uid(qid, tid),
                       out->T, &out->rmse, out->inl_idx, &out->n_inl, &out->valid_iterations,
                       &out->real_iterations);
  if (found) {
    out->info_scale = (double)((float)out->n_inl / (out->rmse * out->rmse));
    out->id1 = tid;
    out->id2 = qid;
  } else {
    out->id1 = out->id2 = -1;
    out->info_scale = 0.0;
  }
}
