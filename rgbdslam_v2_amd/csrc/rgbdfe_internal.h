// rgbdfe_internal.h -- shared between the HIP kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rgbdfe.h"

namespace rgbdfe {

// One (newer node, older node) pair as the kernels see it.  Node features live in
// two slabs (descriptor slab: slot x max_kp x 32 B, xyz1 slab: slot x max_kp x 16 B);
// a pair is a couple of slot indices plus the row counts.
struct PairWork {
  uint32_t q_slot, t_slot;  // slab slots of the newer (query) / older (train) node
  uint32_t nq, nt;          // rows
  uint32_t uid;             // RNG stream id of the pair (D1), from (qid, tid)
  int32_t qid, tid;         // node ids (edge.id2 / edge.id1)
  uint32_t pad;
};
static_assert(sizeof(PairWork) == 32, "PairWork layout");

// "no neighbour": hd = 257, idx = 0xFFFF (features.cpp:172-173 -> (257,-1))
constexpr uint32_t kNoMatchKey = (257u << 16) | 0xFFFFu;

struct RansacConst {
  int32_t max_matches, min_matches, ransac_iterations;
  float max_dist_m;
  double sq_max_dist;   // (double)(max_dist_m*max_dist_m)  node.cpp:1152
  double depth_cov;     // D3
  double raster_cov_x;  // misc.cpp:708
  double raster_cov_y;  // misc.cpp:709
  uint32_t seed;
  int32_t g2o_iterations;  // "g2o_transformation_refinement" (parameter_server.cpp:103), 0 = off
};

// launchers (defined in the .hip files)
// returns the number of key planes written per pair (keys[pair][plane][row]); the consumer
// takes the min over planes.  key_planes_capacity = planes the keys buffer can hold in total.
// HammingGeometry = everything of a Hamming launch that depends on the batch's node sizes: query blocks per pair and
// train-row splits (key planes) per pair.  Batches with equal (n_pairs, geometry) are the same launch -- what the
// hipGraph cache of api_batches.hip keys on.  wide = 1: the pipelined MFMA kernel's 512-query blocks (hamming_mfma.hip);
// shape = the MFMA tile of the launch: 16 = 16x16x128 (hamming_mfma_x16_kernel, 512-query blocks only), 32 = 32x32x64,
// 0 = no MFMA (the popcount kernel).
struct HammingGeometry { uint32_t qblocks, tsplit, wide, shape; };
HammingGeometry hamming_nn_geometry(uint32_t n_pairs, uint32_t max_nq, uint32_t max_nt, uint32_t key_planes_capacity);
uint32_t launch_hamming_nn(const uint32_t* desc_pool, const PairWork* work, uint32_t* keys,
                           uint32_t max_kp, uint32_t n_pairs, HammingGeometry geom, hipStream_t stream);
// fp4 MFMA form of the same search (hamming_mfma.hip): descriptors expanded to one fp4 operand nibble per bit, 128 B per
// row in MFMA fragment order, tiles of 32 rows; same keys, bit for bit.  mode 1: row term added by the MFMA (C operand),
// mode 2: by v_add_f32.  Valid for max_kp <= 32768.
uint32_t hamming_mfma_tiles_per_slot(uint32_t max_kp);
size_t hamming_mfma_slab_bytes(uint32_t max_nodes, uint32_t max_kp);
void launch_hamming_expand(const uint32_t* node_rows, uint32_t* slab, uint32_t slot, uint32_t max_kp, uint32_t n,
                           hipStream_t stream);
// pipe_wide (the pipelined kernel, modes 3 / 4): -1 = the library chooses between 256- and 512-query blocks, 0 / 1 = forced;
// wide_shape: the MFMA tile of 512-query blocks, 0 = the library chooses, 16 / 32 = forced (256-query blocks are always 32)
HammingGeometry hamming_mfma_geometry(uint32_t n_pairs, uint32_t max_nq, uint32_t max_nt, uint32_t key_planes_capacity,
                                      int pipe_wide, int wide_shape);
uint32_t launch_hamming_mfma(const uint32_t* slab, const PairWork* work, uint32_t* keys, uint32_t max_kp,
                             uint32_t n_pairs, HammingGeometry geom, int mode, hipStream_t stream);
// place_recognition.hip: every query descriptor votes k - rank for the k candidate nodes holding its nearest matches
// (keys[candidate][plane][row] from the Hamming stage; k <= 8; candidates < 65536)
void launch_place_votes(const uint32_t* keys, uint32_t planes, uint32_t max_kp, const PairWork* work, const uint32_t* seg,
                        uint32_t n_queries, uint32_t max_nq, uint32_t k_neighbours, uint32_t max_hd, uint32_t* votes,
                        hipStream_t stream);
void launch_select_ransac(const float4* xyz_pool, const PairWork* work, const uint32_t* keys,
                          uint32_t key_planes, rgbdfe_match_result* results, uint32_t max_kp,
                          uint32_t n_pairs, const RansacConst& rc, struct PairPrep* prep, double* ec_pool,
                          hipStream_t stream);
// outcome of one RANSAC iteration's refinement loop (node.cpp:1140-1169): refined transform, inlier set, error
struct IterRec {
  float rR[9], rt[3];
  uint64_t rmask[5];
  double rerr;
  int32_t rn;
  int32_t pad;
};
// what the in-order walk needs of an iteration (refined_matches.size(), refined_error): a dense array next to the
// records, so that the walk reads -- and a batch of junk iterations writes, lane = iteration -- whole cache lines instead
// of one 104-byte record per lane (a junk iteration leaves only {1e6, 0} here and no IterRec at all)
struct IterSum {
  double rerr;
  int32_t rn;
  int32_t pad;
};
// what pair_prep_kernel leaves for every select+RANSAC wave of a pair: the selected matches' 3-D points as 7-word
// records (from.xyz, to.xyz, 1/(from.z*to.z)) and the facts about them the waves need
struct alignas(16) PairPrep {
  float M[RGBDFE_MAX_MATCHES * 7];
  uint64_t w_nonzero[RGBDFE_MASK_WORDS];  // matches with a non-zero weight
  int32_t n_all;                          // selected matches
  float pmax;                             // largest finite |coordinate| of their points
  uint32_t fast_alpha;                    // every weight inside the window of the unscaled float division
  uint32_t pad;
};
// per-pair progress of the record / replay schedule: the reference's in-order bookkeeping (node.cpp:1171-1190) as far as
// the refinement kernel (ransac_split.hip) had to run it -- between two windows of a pair of a phased plan; a pair recorded
// in one window, or in shares, keeps the start values the hypothesis kernel wrote.  The result waves
// (select_ransac_kernel<kReplay>) resume the walk at real_iterations and run it to the end of the recorded range.
// walk[n_pairs] holds the batch's counters instead (zeroed by the hypothesis kernel; `it` = the refinement launch's unit
// counter).
struct WalkState {
  int32_t state;             // >= 0: upper bound of the iterations that may still be needed; < 0: the loop has ended
  int32_t it, real_iterations, valid_iterations;
  int32_t best_idx;          // iteration whose record is the best hypothesis so far, -1 = none
  int32_t best_n;
  float rmse;
  int32_t speculate;         // end of the pair's recorded range: the result wave walks [real_iterations, speculate)
};
// what the one-wave kernel and the result waves (select_ransac_kernel<kWhole / kReplay>, select_ransac.hip) are given
struct RecordPlan {
  IterRec* recs = nullptr;   // [pair][iteration] (kReplay)
  IterSum* sums = nullptr;   // [pair][iteration], behind the records in the same allocation (kReplay)
  WalkState* walk = nullptr; // [pair] (kReplay)
  const PairPrep* prep = nullptr;  // [pair]
  double* ec_pool = nullptr;  // select_ransac_ec_region_bytes() per pair (the inlier errors of a refinement round's
                              // scorings, read back lane = slot by the sequential error sums)
  const uint64_t* vmask = nullptr;  // [pair][vmask_words]: SplitPlan::vmask (kReplay)
  int vmask_words = 0;
};
size_t select_ransac_ec_region_bytes();
// ransac_split.hip: the recording stage as a hypothesis kernel (lane = iteration) + ONE refinement launch over the viable
// iterations of the whole batch.
struct SplitPlan {
  IterRec* recs = nullptr;     // [pair][iteration]: the hypothesis kernel leaves a viable iteration's transform in rR / rt,
                               // the refinement kernel the iteration's outcome
  IterSum* sums = nullptr;     // [pair][iteration]
  uint64_t* vmask = nullptr;   // [pair][vmask_words]: bit k of a pair = iteration k passed the pre-screen
  WalkState* walk = nullptr;   // [pair] (+ the batch's counters in walk[n_pairs])
  const PairPrep* prep = nullptr;
  int vmask_words = 0;
  // phased = 0 (small batches, full speculation): a workgroup unit is (pair, share of share_iters iterations); everything is
  //          recorded, the result waves walk.
  // phased = 1: a unit is a pair.  Its range is recorded in WINDOWS inside the kernel -- [0, phase_ends[0]) first, or
  //          [0, I) at once for a pair the pre-screen shows to be junk-heavy -- and between two windows the workgroup's
  //          server runs the reference's in-order bookkeeping over what has been recorded: the loop has ended, or the next
  //          window (the next phase; everything that is left for a junk-heavy pair without a jump of `it`; never beyond
  //          the iterations the pair can still need).  The pair's match records stay in LDS across its windows.
  int phased = 0;
  int n_phases = 1;
  int phase_ends[4] = {0, 0, 0, 0};
  int n_shares = 1;            // phased = 0: units per pair
  int share_iters = 0;
  uint8_t* preclass = nullptr; // [pair]: 2 = at most 9 of the first 14 iterations passed the pre-screen ("junk-heavy" whatever
                               // their refinement gives: such a pair will most likely run all its iterations) -- written by the
                               // hypothesis kernel when preclass_iters > 0
  int preclass_iters = 0;      // the first phase's length (14), 0 = no pre-classification
  uint32_t* unit_counter = nullptr;  // zero at launch: the refinement kernel's workgroups take their units off it
  // phased plans: the pairs that run RANSAC, bucketed by the number of their viable iterations (the hypothesis kernel
  // appends; kOrderBuckets counters, zeroed by pair_prep_kernel, + [bucket][n_pairs] pair indices).  The refinement kernel
  // takes the buckets from the top: a launch is about two generations of resident units per workgroup, and the pairs that
  // keep a workgroup longest should not be the ones it picks up last.
  uint32_t* order_cnt = nullptr;
  uint32_t* order = nullptr;
};
constexpr int kOrderBuckets = 64;
// bucket of a pair with n viable iterations: one per count below 32, then steps of 8
__host__ __device__ inline int order_bucket(int n) { return n < 32 ? n : (32 + (n - 32) / 8 < kOrderBuckets ? 32 + (n - 32) / 8 : kOrderBuckets - 1); }
void launch_ransac_hyp(const PairWork* work, uint32_t n_pairs, const RansacConst& rc, const SplitPlan& plan, hipStream_t stream);
void launch_ransac_refine(uint32_t n_pairs, const RansacConst& rc, const SplitPlan& plan, hipStream_t stream);
int ransac_split_words_per_pair(int ransac_iterations);
int ransac_split_max_share();
int ransac_split_wgs();   // persistent workgroups of a refinement launch on this device
int ransac_split_init();  // once per process before the first batch (not inside a stream capture); returns the CU count
// bytes of the per-pair iteration masks behind the records + summaries of a record buffer of `rec_capacity` records
// (+ 8 bytes per pair: preclass; + the order buckets: kOrderBuckets counters and kOrderBuckets x max_pairs indices)
inline size_t ransac_split_mask_bytes(size_t rec_capacity, size_t max_pairs) { return (rec_capacity / 64 + (5 + 32) * max_pairs + 64 + 64) * 8; }
// where the order buckets of a batch of n_pairs live behind its records (the same for pair_prep_kernel, which zeroes the
// counters, and the plan of the kernels that use them)
inline uint32_t* ransac_split_order_cnt(IterRec* recs, size_t n_pairs, int ransac_iterations) {
  const size_t I = ransac_iterations > 0 ? (size_t)ransac_iterations : 0, n_recs = n_pairs * I;
  uint64_t* vmask = reinterpret_cast<uint64_t*>(reinterpret_cast<IterSum*>(recs + n_recs) + n_recs);
  uint8_t* preclass = reinterpret_cast<uint8_t*>(vmask + n_pairs * (size_t)ransac_split_words_per_pair(ransac_iterations));
  return reinterpret_cast<uint32_t*>(preclass + ((n_pairs + 8 + 7) & ~(size_t)7));
}
// edges.hip: stable compaction of the accepted edges (id1 >= 0) of a shard
void launch_compact_edges(const rgbdfe_match_result* in, uint32_t n, rgbdfe_match_result* out, int32_t* out_index,
                          int32_t index_scale, int32_t index_offset, int32_t* d_dst, int32_t* d_count, hipStream_t stream);
// edges.hip: records -> rgbdfe_compact_result (header + inlier mask, 144 of the 1744 bytes)
void launch_compact_pack(const rgbdfe_match_result* in, uint32_t n, rgbdfe_compact_result* out, hipStream_t stream);
// the inlier stream of a shard (include/rgbdfe.h: rgbdfe_inlier_header): n_headers headers, then the list block; *d_total = its entries
void launch_pack_inliers(const rgbdfe_match_result* in, uint32_t n, uint32_t n_headers, void* stream_out, int32_t* d_total,
                         hipStream_t stream);
// node.cpp:1222-1268 after the RANSAC results exist (rc.g2o_iterations > 0): two-view Gauss-Newton refinement over the
// inliers + re-scoring + the adopt rules.  kp_pool: KeyPoint.pt slab [slot][row] (float2).
void launch_g2o_refine(const PairWork* work, rgbdfe_match_result* results, uint32_t n_pairs, const RansacConst& rc,
                       const struct PairPrep* prep, const float* kp_pool, uint32_t max_kp, double* ec_pool, hipStream_t stream);
void launch_select_ransac_latency(const float4* xyz_pool, const PairWork* work, const uint32_t* keys,
                                  uint32_t key_planes, rgbdfe_match_result* results, uint32_t max_kp,
                                  uint32_t n_pairs, const RansacConst& rc, PairPrep* prep, IterRec* recs, WalkState* walk,
                                  double* ec_pool, int chunk_iters, const int* phase_ends, int n_phases, hipStream_t stream);
void launch_select_ransac_sift_latency(const float4* xyz_pool, const PairWork* work, uint16_t* sm_q,
                                       uint16_t* sm_t, float* sm_d, const int32_t* sm_n, float* all_dist,
                                       rgbdfe_match_result* results, uint32_t max_kp, uint32_t n_pairs,
                                       const RansacConst& rc, PairPrep* prep, IterRec* recs, WalkState* walk,
                                       double* ec_pool, int chunk_iters, const int* phase_ends, int n_phases, hipStream_t stream);
// (the SIFT launchers first sort each pair's match list in place: sift_sort_kernel)
void launch_select_ransac_sift(const float4* xyz_pool, const PairWork* work, uint16_t* sm_q,
                               uint16_t* sm_t, float* sm_d, const int32_t* sm_n,
                               float* all_dist, rgbdfe_match_result* results, uint32_t max_kp,
                               uint32_t n_pairs, const RansacConst& rc, struct PairPrep* prep, double* ec_pool,
                               hipStream_t stream);
// SIFT matcher (sift_match.hip): u8-quantised descriptors as bf16, exact integer dot products
// on the bf16 MFMA, SiftMatchGPU row/column/mutual-best semantics.
void launch_sift_dot(const uint16_t* bf16_pool, const PairWork* work, uint32_t max_kp,
                     uint32_t n_pairs, uint32_t max_nq, uint32_t max_nt, uint32_t key_kinds,
                     uint32_t* row_part, uint32_t* col_part, uint2* col_blocks, hipStream_t stream);
void launch_sift_finish(const float* f32_pool, const PairWork* work, uint32_t max_kp,
                        uint32_t n_pairs, const uint32_t* row_part, uint32_t* col_part, const uint2* col_blocks,
                        uint16_t* sm_q, uint16_t* sm_t, float* sm_d, int32_t* sm_n,
                        hipStream_t stream);
// col_blocks (one-pass float-key path): per pair and 256-row block of the query node, the two largest dot products of every
// train column (float key bits); sift_col_block_bytes_per_pair() bytes per pair.  nullptr = the two-pass form.
size_t sift_col_block_bytes_per_pair();
// FLANN branch with exact neighbours (l2_knn.hip): knn[pair][row] = (d1 bits, d2 bits, nearest train row); then the
// ratio test + train-unique rule -> (queryIdx, trainIdx, ratio) lists in query order
void launch_l2_knn2(const float* f32_pool, const PairWork* work, uint32_t max_kp, uint32_t n_pairs, uint32_t max_nq,
                    uint32_t* knn, hipStream_t stream);
void launch_l2_ratio(const PairWork* work, uint32_t max_kp, uint32_t n_pairs, const uint32_t* knn, uint32_t* claim,
                     double max_ratio, uint16_t* sm_q, uint16_t* sm_t, float* sm_d, int32_t* sm_n, hipStream_t stream);
void launch_sift_quantise(const float* f32, uint16_t* bf16, size_t n_elems, hipStream_t stream);
void launch_project_to_3d(const float* kp_xy, int n_kp, const float* depth, int rows, int cols,
                          float fxinv, float fyinv, float cx, float cy, double depth_scaling,
                          int max_keypoints, int32_t* kept_idx, float4* xyz1, int32_t* n_out,
                          hipStream_t stream, bool truncate = false, const float* z_gathered = nullptr);
constexpr int kProjectFramesMax = 32;   // frames of a super-frame (api_detect.hip)
struct ProjectFrames { int n_frames; int off[kProjectFramesMax]; int n[kProjectFramesMax]; };
void launch_project_to_3d_frames(const ProjectFrames& fr, const float* kpxy, int rows, int cols, float fxinv, float fyinv,
                                 float cx, float cy, double depth_scaling, int max_keypoints, int32_t* kept_idx, float4* xyz1,
                                 int32_t* n_out, hipStream_t stream);
// kp_xys: n_kp x (x, y, KeyPoint::size); z_out[i] = getMinDepthInNeighborhood (misc.cpp:774-793) or NaN
void launch_min_depth(const float* kp_xys, int n_kp, const float* depth, int rows, int cols, float* z_out,
                      hipStream_t stream);
void launch_project_cloud(const float* kp_xy, int n_kp, const float4* pts, bool gathered, int rows, int cols,
                          double maximum_depth, int max_keypoints, int32_t* kept_idx, float4* xyz1, int32_t* n_out,
                          hipStream_t stream);
// one direction of one edge for the environment measurement model (emm.hip)
struct EmmJob {
  const float4* new_samples;  // the sampled points (every skip-th row / column) of the frame that is projected
  const float* old_z;       // ... into this frame's raster: its depth plane (z of every cloud point)
  float T[12];              // rows 0..2 of the 4x4 new -> old transform, row-major
  float fx, fy, cx, cy;     // old camera intrinsics, already divided by cloud_creation_skip_step
};
void launch_depth_to_mono8_f32(const float* depth, size_t n, uint8_t* mono8, hipStream_t stream);
void launch_depth_u16(const uint16_t* depth_mm, size_t n, uint8_t* mono8, float* depth_m, hipStream_t stream);
void launch_create_cloud(const float* depth, int rows, int cols, const uint8_t* rgb, int channels,
                         int encoding_bgr, float fxinv, float fyinv, float cx, float cy, double depth_scaling,
                         float min_depth, int s, int ch, int cw, float4* cloud, float* zplane, hipStream_t stream);
void launch_decimate_cloud(const float4* cloud, int ch, int cw, int skip_step, float4* out, hipStream_t stream);
void launch_emm(const EmmJob* jobs, int n_jobs, int ch, int cw, int skip_step, double d_lo, double d_hi,
                uint32_t* counts, hipStream_t stream);
// map_assembly.hip: transformAndAppendPointCloud (misc.cpp:183-238) over a list of resident clouds.  The (node, point)
// sequence is cut into tiles of kMapTile points that never cross a node; the table has n_nodes + 1 rows (the last one a
// sentinel: first_point = all points, first_tile = all tiles), tile_node[t] = the node of tile t.
constexpr uint32_t kMapTile = 1024;
struct MapNode {
  const float4* cloud;
  int64_t first_point;   // points of the nodes listed before this one (its first row in raster mode)
  uint32_t n_points;
  uint32_t first_tile;
  float R[9], t[3];      // rot (row-major) and trans of the Matrix4f
};
static_assert(sizeof(MapNode) == 72, "MapNode layout");
void launch_map_raster(const MapNode* nodes, const uint32_t* tile_node, uint32_t n_tiles, bool clip, float md2, float4* out,
                       hipStream_t stream);
// compact mode, first half: tile_count[t] = kept points of tile t; tile_first[t] = those in front of tile t
// (tile_first[n_tiles] = the total); node_first[k] = first output row of node k (node_first[n_nodes] = the total)
void launch_map_count_scan(const MapNode* nodes, const uint32_t* tile_node, uint32_t n_nodes, uint32_t n_tiles, bool clip,
                           float md2, uint32_t* tile_count, int64_t* tile_first, int64_t* node_first, hipStream_t stream);
void launch_map_write(const MapNode* nodes, const uint32_t* tile_node, uint32_t n_tiles, const int64_t* tile_first, bool clip,
                      float md2, float4* out, hipStream_t stream);
// voxel_filter.hip: pcl::VoxelGrid's centroids over a cloud of n < 2^31 points (the stages: the head of that file).  The
// host reads VoxHeader twice: behind launch_vox_stats (the box, n_valid) and behind launch_vox_heads (n_cells).
constexpr uint32_t kVoxTile = 1024;      // points (or sorted pairs) of a workgroup in the point and cell passes
constexpr uint32_t kVoxSortTile = 4096;  // pairs of a workgroup in a sort pass
struct VoxHeader {
  float min_p[3], max_p[3];  // the bounding box of the valid points (+inf / -inf when there is none)
  uint32_t n_valid, n_cells;
};
struct VoxGrid {
  float inv;           // 1.0f / leaf
  float min_b[3];      // (float)min_b
  uint32_t mul1, mul2; // div0, div0 * div1 as int32 bits
  uint32_t flip;       // 0x80000000 when the int32 cell index can be negative (the keys then sort as signed), else 0
};
// tile_box: 6 floats per point tile; tile_count: one per point tile; tile_first: one more
void launch_vox_stats(const float4* pts, uint32_t n, float* tile_box, uint32_t* tile_count, uint32_t* tile_first, VoxHeader* hdr,
                      hipStream_t stream);
void launch_vox_keys(const float4* pts, uint32_t n, const VoxGrid& g, const uint32_t* tile_first, uint32_t* keys, uint32_t* idx,
                     hipStream_t stream);
// `passes` stable 8-bit passes from the low byte up over n (key, index) pairs, ping-pong between the two buffers; returns
// the buffer that holds the result.  hist: 256 x (n / kVoxSortTile, rounded up) counters; digit_total: 256
int launch_vox_sort(uint32_t n, int passes, uint32_t* keys[2], uint32_t* idx[2], uint32_t* hist, uint32_t* digit_total,
                    hipStream_t stream);
// cell_start[c] = the first sorted position of cell c, cell_start[n_cells] = n (n + 1 entries suffice); hdr->n_cells
void launch_vox_heads(const uint32_t* keys, uint32_t n, uint32_t* tile_count, uint32_t* tile_first, uint32_t* cell_start,
                      VoxHeader* hdr, hipStream_t stream);
// out[c] = the centroid row of cell c; zplane (may be NULL): its z again, the plane behind a resident cloud
void launch_vox_centroids(const float4* pts, const uint32_t* idx, const uint32_t* cell_start, uint32_t n_cells, float4* out,
                          float* zplane, hipStream_t stream);
// octomap.hip: the occupancy map (include/rgbdfe.h, "occupancy map").  The table is open addressing with linear probing over
// `cap` slots, one array per field: key (x | y << 16 | z << 32; kOctoEmptyKey: free), value (log-odds; bits kOctoNoLeaf: the
// key is claimed, the leaf does not exist yet), colour (r << 16 | g << 8 | b), mark (2 * epoch + occupied of the last cloud
// that touched the slot).  One cloud = launch_octo_cloud with its own epoch (>= 1, ascending).
constexpr uint64_t kOctoEmptyKey = ~0ull;
constexpr uint32_t kOctoNoLeaf = 0xffffffffu;
constexpr uint32_t kOctoMaxSteps = 3u * 65536u;  // no ray between two valid keys takes more steps
struct OctoTable {
  unsigned long long* key;
  float* value;
  uint32_t* colour;
  uint32_t* mark;
  uint32_t cap;
};
struct OctoCtl {
  uint32_t overflow;  // a key found no slot: the cloud that set it and every later cloud of the call change nothing
  uint32_t n_done;    // clouds of the call that were applied
  uint32_t n_leaves;
  uint32_t pad;
};
struct OctoCloud {
  float R[9], t[3];          // as MapNode: row-major rotation, translation = the ray origin
  double inv_res, res;       // 1.0 / resolution, resolution
  double max_range;          // < 0: off
  float hit, miss, clamp_min, clamp_max;
  uint32_t epoch;
};
// scratch of a cloud of n points (all in the context's scratch): as the voxel filter's sort, see api_octomap.hip
struct OctoScratch {
  uint32_t* keys[2];
  uint32_t* idx[2];
  uint32_t *hist, *digits, *tile_count, *tile_first, *cell_start;
  VoxHeader* hdr;
};
void launch_octo_cloud(const OctoTable& tb, OctoCtl* ctl, const float4* pts, uint32_t n, const OctoCloud& c, int sort_passes,
                       const OctoScratch& s, hipStream_t stream);
// every leaf of `from` into the empty table `to` (to.cap >= the leaves of `from`)
void launch_octo_rehash(const OctoTable& from, const OctoTable& to, OctoCtl* ctl, hipStream_t stream);
// every leaf of `src` (n records: key as the table packs it, log-odds, r << 16 | g << 8 | b) into the empty table `to`
// (to.cap >= n); a key that is already there raises *dup
struct OctoLeafIn {
  unsigned long long key;
  float value;
  uint32_t colour;
};
void launch_octo_set_leaves(const OctoLeafIn* src, uint32_t n, const OctoTable& to, OctoCtl* ctl, uint32_t* dup, hipStream_t stream);
// octomap_query.hip: the read side (include/rgbdfe.h, "occupancy map: the read side").  The kernels read the table and write
// their own output rows, nothing else; one launch each.
struct OctoQuery {
  double inv_res, res;      // 1.0 / resolution, resolution
  double max_range2;        // max_range * max_range; < 0: no range limit
  float occupied;           // a leaf is occupied iff its log-odds >= this
  uint32_t ignore_unknown;
};
struct OctoView {
  float R[9], t[3];         // as MapNode: row-major rotation camera -> world, translation = the ray origin
  float fx, fy, cx, cy;
  uint32_t rows, cols;
};
// points: n rows of 3 floats; found[i] = 0 / 1 / 2, leaves[i] = the rgbdfe_octomap_leaf record of point i
void launch_octo_search(const OctoTable& tb, const float* points, uint32_t n, double inv_res, int32_t* found, uint4* leaves,
                        hipStream_t stream);
// rays: n origins (3 floats each), then n directions; hits: n rgbdfe_octomap_ray_hit records
void launch_octo_cast(const OctoTable& tb, const float* origins, const float* directions, uint32_t n, const OctoQuery& q,
                      rgbdfe_octomap_ray_hit* hits, hipStream_t stream);
// cloud: rows * cols rows of the node-cloud format; status: a byte per pixel, may be NULL
void launch_octo_view(const OctoTable& tb, const OctoView& v, const OctoQuery& q, float4* cloud, uint8_t* status, hipStream_t stream);
// octomap_tree.hip: the octree of a map's leaves (include/rgbdfe.h, "the tree of a leaf set"; the stages: the head of that
// file).  Workspace of a map of n leaves in a table of cap slots: see tree_workspace (api_octomap.hip).
constexpr uint32_t kTreeTile = 1024;  // elements of a workgroup in a count / write pass
struct TreeHdr {
  uint32_t cnt[17];  // nodes of depth d (cnt[16] = leaves), as far as the passes went
  uint32_t n_nodes;  // all nodes: the sum the chain scan leaves
  uint32_t n_out;    // records of the depth filter
  uint32_t dup;      // rgbdfe_octomap_set_leaves: a key came twice
  uint32_t pad[4];
};
struct TreeLevel {   // the nodes of one depth in tree order
  float* value;
  uint32_t* colour;  // r << 16 | g << 8 | b | child mask << 24
  uint32_t* first;   // the sorted index of the node's first leaf
};
struct TreeScratch {
  TreeHdr* hdr;
  unsigned long long *code, *scode;  // path codes: of the leaves in slot order, in tree order
  uint32_t* slot;
  uint32_t* keys[2];
  uint32_t* idx[2];
  uint32_t *hist, *digits, *tile_count, *tile_first;
  uint32_t *top, *off;
  TreeLevel level[2];
};
// each returns its number of kernel launches.  leaves: gather, sort, arrange (hdr->cnt[16]; level[0] = depth 16);
// chain: off, hdr->n_nodes; levels: depth 15 down to `down_to`, the records of every node into d_records unless NULL
// (needs chain); filter: the nodes of `depth` (the levels must have gone down to it) with value >= min_log_odds as
// rgbdfe_octomap_leaf records, hdr->n_out
int launch_tree_leaves(const OctoTable& tb, uint32_t n_leaves, const TreeScratch& t, hipStream_t stream);
int launch_tree_chain(uint32_t n_leaves, const TreeScratch& t, hipStream_t stream);
int launch_tree_levels(uint32_t n_leaves, uint32_t down_to, const TreeScratch& t, void* d_records, hipStream_t stream);
int launch_tree_filter(uint32_t n_leaves, uint32_t depth, float min_log_odds, const TreeScratch& t, void* d_out, hipStream_t stream);
void launch_sift_pack(const float* desc_in, const int32_t* kept_idx, const int32_t* n_ptr, int max_rows,
                      bool root_sift, float* raw, float* feat, hipStream_t stream);

// rgbdfe_sift_detect_batch_nodes (sift_nodes.hip): frame f of a chunk -- its kept SIFT features (x, y, KeyPoint::size, -) and
// unnormalised descriptors, its depth image -- becomes the rows [0, n_out[f]) of the destinations: the node's slab rows
// (xyz / feat; NULL for a frame without a node) and the chunk's host-output rows (*_out; NULL when nothing goes back)
constexpr int kSiftNodeFramesMax = 8;   // = SiftExtractor::kMaxBatch
struct SiftNodeFrame {
  const float4* keys; const float2* desc; const float* depth; int n_keys;
  float4* xyz; float2* feat; float4* xyz_out; float2* feat_out; int32_t* kept_out;
};
struct SiftNodeChunk { int n_frames; int32_t* n_out; SiftNodeFrame frame[kSiftNodeFramesMax]; };
// rgbdfe_detect_sift_describe(_batch_nodes) (sift_keys.hip): frame f's aggregate (rgbdfe_keypoint rows) -> projectTo3D's kept
// keypoints in aggregate order, cut at max_keypoints, as SiftGPU keys (x, y, size / 12, angle in radians: the wrapper's double
// arithmetic stored as float), as the keypoints the wrapper rebuilds (rgbdfe_keypoint rows) and as the node launch's
// (x, y, size, 0) rows; n_out[f] = the count (0: the wrapper's empty-list path)
struct SiftKeysFrame {
  const rgbdfe_keypoint* agg; const float* depth; int n_agg;
  float4* keys; rgbdfe_keypoint* rebuilt; float4* node_keys;
};
struct SiftKeysChunk { int n_frames; int32_t* n_out; SiftKeysFrame frame[kSiftNodeFramesMax]; };
void launch_sift_keys_from_detector(const SiftKeysChunk& ch, int rows, int cols, double depth_scaling, int max_keypoints,
                                    bool min_depth, hipStream_t stream);
// descriptor rows into the callers' order: out row (f, r) = src row map[f * stride + r] (a zero row for -1), r < n[f]
struct SiftGather { int n_frames; int n[kSiftNodeFramesMax]; };
void launch_sift_rows_gather(const float* src, const int32_t* map, const SiftGather& g, size_t stride, float* out,
                             hipStream_t stream);
void launch_sift_nodes(const SiftNodeChunk& ch, int rows, int cols, float fxinv, float fyinv, float cx, float cy,
                       double depth_scaling, int max_keypoints, bool min_depth, bool root_sift, hipStream_t stream);

}  // namespace rgbdfe
