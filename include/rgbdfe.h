/*
 * rgbdfe.h -- C ABI of the MI355X-native RGB-D SLAM visual front end.
 *
 * This is the drop-in boundary behind rgbdslam_v2's Node / GraphManager seam
 * (the reference has no FFI of its own; the seams are the C++ signatures cited
 * on each entry point, paths relative to the rgbdslam_v2 tree).  Plain pointers
 * and sizes only; no exceptions cross this boundary; every function returns an
 * rgbdfe_status (0 = ok, <0 = error) unless noted.  INTEGRATION.md shows the
 * reference-side binding.
 *
 * Threading: a context owns its HIP streams and is internally locked; calls on
 * one context from any number of threads serialise (this replaces
 * QtConcurrent::blockingMapped's barrier, graph_manager.cpp:548, one call = one
 * batch of pairs).  rgbdfe_last_error returns a per-thread copy of the message.
 */
#ifndef RGBDFE_H
#define RGBDFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGBDFE_MAX_MATCHES 320   /* capacity for max_matches (reference default 300) */
#define RGBDFE_MASK_WORDS 5      /* RGBDFE_MAX_MATCHES / 64 */
#define RGBDFE_MAX_KEYPOINTS 65535

typedef enum {
  RGBDFE_OK = 0,
  RGBDFE_ERR_INVALID_ARG = -1,
  RGBDFE_ERR_NO_DEVICE = -2,    /* no HIP device / kernels cannot run: never falls back to CPU */
  RGBDFE_ERR_HIP = -3,
  RGBDFE_ERR_UNKNOWN_NODE = -4,
  RGBDFE_ERR_CAPACITY = -5,
  RGBDFE_ERR_OUT_OF_MEMORY = -6,
  RGBDFE_ERR_INTERNAL = -7      /* a C++ exception was caught at the ABI (none ever crosses it) */
} rgbdfe_status;

/* Snapshot of the ParameterServer values the pair path reads at call time
 * (parameter_server.cpp:85,86,100,101,46 ). */
typedef struct {
  int32_t  max_matches;           /* "max_matches"           default 300 (<= RGBDFE_MAX_MATCHES) */
  int32_t  min_matches;           /* "min_matches"           default 20  */
  int32_t  ransac_iterations;     /* "ransac_iterations"     default 200 */
  float    max_dist_for_inliers;  /* "max_dist_for_inliers"  default 3.0 */
  double   depth_cov;             /* value depth_covariance() froze at its first call
                                     (misc2.h:30-35): (sigma_depth * z0^2)^2, default z0 = 1 m -> 1e-4 */
  uint32_t seed;                  /* replaces srand(clock()) (node.cpp:1102) */
  uint32_t g2o_iterations;        /* "g2o_transformation_refinement" default 0 = off (parameter_server.cpp:103): Gauss-
                                     Newton steps of the two-view refinement after RANSAC (node.cpp:1222-1268); needs the
                                     nodes' 2-D keypoints, rgbdfe_upload_node_keypoints */
} rgbdfe_params;

typedef struct {
  int32_t device_id;              /* HIP device ordinal */
  int32_t max_nodes;              /* resident node slots (each max_keypoints rows) */
  int32_t max_keypoints;          /* rows per node slot, <= RGBDFE_MAX_KEYPOINTS */
  int32_t max_pairs_per_batch;    /* pairs per kernel batch (results/keys staging) */
  rgbdfe_params params;
} rgbdfe_config;

/* Per-pair result: the MatchingResult POD (matching_result.h:24-46, edge.h:24-32).
 * This exact layout is what lives in HBM, what is all-gathered between ranks
 * and what rgbdfe_match_* copies to the host. */
typedef struct {
  int32_t  id1, id2;              /* edge.id1 = older node, edge.id2 = newer node; -1,-1 = no edge
                                     (node.cpp:1337-1338, 1419-1422) */
  int32_t  n_all;                 /* |all_matches| after keepStrongestMatches (node.cpp:674) */
  int32_t  n_inl;                 /* |inlier_matches| */
  float    rmse;                  /* MatchingResult::rmse */
  float    trafo[16];             /* ransac_trafo == final_trafo, Eigen::Matrix4f column-major,
                                     maps the newer node's frame into the older node's frame */
  uint32_t pad0;
  double   info_scale;            /* edge.informationMatrix = I6 * info_scale (node.cpp:1335) */
  int32_t  valid_iterations;      /* diagnostics (node.cpp:1216) */
  int32_t  real_iterations;
  uint16_t all_q[RGBDFE_MAX_MATCHES];  /* DMatch.queryIdx, sorted by (hd, queryIdx) */
  uint16_t all_t[RGBDFE_MAX_MATCHES];  /* DMatch.trainIdx */
  uint8_t  all_hd[RGBDFE_MAX_MATCHES]; /* Hamming distance; DMatch.distance = hd/256.0f */
  uint64_t inlier_mask[RGBDFE_MASK_WORDS]; /* bit m set <=> all_*[m] is in inlier_matches */
} rgbdfe_match_result;

/* The same record without its all_matches lists: what GraphManager consumes of a MatchingResult besides GUI drawing
 * (edge ids / transform / information scale, rmse, |inlier_matches|, graph_manager.cpp:554-606; all_matches only feeds
 * graph_mgr_io.cpp:739-1107).  This is the default payload of the multi-GPU gather: 144 B instead of 1744 B per pair.
 * Node features are replicated on every device, and a pair's result does not depend on the batch or the device it ran
 * on, so the full record of a pair whose lists are wanted (updateInlierFeatures, :409-419; drawing) is
 * rgbdfe_match_pair_list(ctx, &q, &t, 1, &full) on ANY device -- byte-identical to the owner's, no fetch needed. */
typedef struct {
  int32_t  id1, id2, n_all, n_inl;
  float    rmse;
  float    trafo[16];
  uint32_t pad0;
  double   info_scale;
  int32_t  valid_iterations, real_iterations;
  uint64_t inlier_mask[RGBDFE_MASK_WORDS];
} rgbdfe_compact_result;

/* The inlier form of a shard's results: what the consumer of the multi-GPU gather reads of a MatchingResult -- the edge
 * (ids, transform, information scale), rmse and counts as above, and the inlier matches' (queryIdx, trainIdx)
 * (GraphManager::updateInlierFeatures, graph_manager.cpp:409-419) -- without the all_matches lists and without a second
 * pair op on the receiving device.  A shard of n pairs is ONE byte stream:
 *   n_headers x rgbdfe_inlier_header   (the leading 104 bytes of rgbdfe_match_result; `first_inlier` = position of the pair's
 *                                       first inlier in the list block; headers n .. n_headers-1 are padding: ids -1, no inliers)
 *   total x uint32                     (the list block: query row | train row << 16 of every inlier, pair after pair, inliers
 *                                       in match order = ascending bit of inlier_mask)
 * total = sum of n_inl: 104 + 4 * n_inl bytes per pair instead of 1744 (configs[1]: ~260).  The default payload of
 * bench.py --gpus N. */
typedef struct {
  int32_t  id1, id2, n_all, n_inl;
  float    rmse;
  float    trafo[16];
  uint32_t first_inlier;
  double   info_scale;
  int32_t  valid_iterations, real_iterations;
} rgbdfe_inlier_header;

typedef struct rgbdfe_ctx rgbdfe_ctx;

/* ---- lifetime ---------------------------------------------------------- */
void rgbdfe_default_config(rgbdfe_config* cfg);
int  rgbdfe_create(const rgbdfe_config* cfg, rgbdfe_ctx** out);
void rgbdfe_destroy(rgbdfe_ctx* ctx);
/* ---- several GPUs behind ONE handle --------------------------------------------------
 * The reference's caller is one process (GraphManager::nodeComparisons, graph_manager.cpp:541-548), so the
 * drop-in form of "shard the candidate pairs over the 8 GPUs of a node" is a context that owns one device
 * context + one host thread per listed device (cfg->device_id is ignored).  With such a handle
 *   - rgbdfe_upload_node / _sift_node / _node_cloud / release / set_* act on every device (node features are
 *     replicated: 48 B per keypoint, trivial in 288 GB);
 *   - rgbdfe_match_node_pairs / _pair_list / _sift_pair_list shard the list pair k -> device k mod G; each device
 *     writes its results to the caller's out[k] directly and the call returns when all are done (the same
 *     barrier semantics as the single-device call; results do not depend on G);
 *   - rgbdfe_observation_likelihood shards its jobs the same way; frame-level calls (detect / describe /
 *     project_to_3d ...) run on the first device;
 *   - entry points that take device pointers are refused: use rgbdfe_device_context(ctx, i) for those.
 * rgbdfe_match_pair_list_allgather is the device-resident form: d_out[i] is a buffer on device i holding
 * G * per records, per = ceil(n_pairs / G) (returned in *records_per_device); afterwards EVERY buffer holds ALL
 * results -- pair k at record (k mod G) * per + k / G, unused tail records filled with 0xFF bytes (ids -1) --
 * exchanged with ONE ncclAllGather of the fixed-size PODs (RCCL over xGMI, loaded at run time), or with peer
 * copies when RCCL cannot be used (a device listed twice, RGBDFE_GATHER=p2p); rgbdfe_gather_transport tells which.
 * A device may be listed more than once (two shards on one GPU: how a 1-GPU box tests the sharding). */
int  rgbdfe_create_multi(const rgbdfe_config* cfg, const int32_t* device_ids, int32_t n_devices, rgbdfe_ctx** out);
int  rgbdfe_device_count(rgbdfe_ctx* ctx);                       /* 1 for rgbdfe_create handles */
rgbdfe_ctx* rgbdfe_device_context(rgbdfe_ctx* ctx, int32_t i);   /* the i-th device's own context (owned by ctx) */
int  rgbdfe_match_pair_list_allgather(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                      int32_t n_pairs, void* const* d_out, int32_t* records_per_device);
/* The same with only the ACCEPTED edges travelling (an all-pairs loop-closure sweep rejects most pairs: id1 == -1,
 * node.cpp:1419): every device compacts its shard in shard order, `*stride` = the largest count of a device; on return
 * d_out[j] holds device i's edges_per_device[i] records at [i * stride, ...), d_index[j] (optional, may be NULL) their
 * positions in the caller's pair list.  Buffers as above (n_devices * ceil(n_pairs / n_devices) records / int32). */
int  rgbdfe_match_pair_list_allgather_edges(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                            int32_t n_pairs, void* const* d_out, int32_t* const* d_index,
                                            int32_t* edges_per_device, int32_t* stride);
const char* rgbdfe_gather_transport(rgbdfe_ctx* ctx);            /* "rccl", "p2p" or "none" (last allgather) */
/* Exchanges the latest rgbdfe_match_pair_list_allgather_inliers call issued: 1 = the one collective sized before the
 * devices had counted their lists, 2 = a list had outgrown that size (and the group's first call: 1, after reading the
 * counts); 0 for other handles / before the first call. */
int  rgbdfe_gather_exchanges(rgbdfe_ctx* ctx);
/* Host time (microseconds) the calling thread spent enqueueing the latest sharded batch on all devices of a multi handle:
 * the shards are submitted by ONE thread, device after device.  With graph capture on (rgbdfe_set_graph_capture; OFF by
 * default) a batch's launch chain is a cached hipGraph per device -- one hipGraphLaunch (+ a read-back or pack enqueue) per
 * device; with the default it is the chain's ~10 kernel launches per device.  0 for single-device contexts. */
int  rgbdfe_group_submit_us(rgbdfe_ctx* ctx, double* us);
/* The compact form of rgbdfe_match_pair_list_allgather: d_out[i] holds G * per rgbdfe_compact_result, same placement
 * (pair k at (k mod G) * per + k / G, unused tail records 0xFF); 12x fewer bytes cross xGMI. */
int  rgbdfe_match_pair_list_allgather_compact(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                              int32_t n_pairs, void* const* d_out, int32_t* records_per_device);
/* The inlier form of the all-gather (rgbdfe_inlier_header below the result structs): every device packs its shard into an
 * inlier stream -- per = ceil(n_pairs / G) headers of 104 bytes, then (queryIdx | trainIdx << 16) of every inlier match --
 * and on return d_out[j] holds device i's stream at byte offset i * (*stride_bytes); list_entries[i] = entries of device
 * i's list block (*stride_bytes = per * 104 + 4 * C with C >= the largest of them: the exchange is sized from the lists of
 * the group's earlier calls, so that packing and the ONE collective are enqueued without a host read between them; C is the
 * largest list itself on a group's first call and whenever a list has outgrown the earlier ones by more than a quarter --
 * rgbdfe_gather_exchanges).  Pair k of the caller's list = header k / G of device k mod G.  What GraphManager reads of a MatchingResult (edge, rmse, counts, inlier_matches for
 * updateInlierFeatures, graph_manager.cpp:409-419) at ~260 bytes per pair instead of 1744.  Buffers: G * per *
 * (104 + 4 * RGBDFE_MAX_MATCHES) bytes each (the worst case). */
int  rgbdfe_match_pair_list_allgather_inliers(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                              int32_t n_pairs, void* const* d_out, int32_t* records_per_device,
                                              int32_t* list_entries, int64_t* stride_bytes);
/* d_records (n rgbdfe_match_result in HBM) -> d_compact (n rgbdfe_compact_result in HBM), enqueued on `stream`
 * (hipStream_t; NULL = the context's stream): what a one-process-per-GPU caller runs between rgbdfe_wait_ticket and its
 * own ncclAllGather (bench.py --gpus N).  Single-device contexts only. */
int  rgbdfe_pack_compact(rgbdfe_ctx* ctx, const void* d_records, int32_t n, void* d_compact, void* stream);
int  rgbdfe_sizeof_compact_result(void);
/* d_records (n rgbdfe_match_result in HBM) -> the inlier stream of the shard at d_stream (see rgbdfe_inlier_header; capacity
 * n_headers * 104 + 4 * sum of n_inl bytes, at most n_headers * 104 + n * 4 * RGBDFE_MAX_MATCHES), *d_total (device int32) =
 * entries of the list block; enqueued on `stream` (hipStream_t; NULL = the context's stream).  n_headers >= n: the
 * header count every rank of a gather pads its shard to.  Single-device contexts only. */
int  rgbdfe_pack_inliers(rgbdfe_ctx* ctx, const void* d_records, int32_t n, int32_t n_headers, void* d_stream,
                         int32_t* d_total, void* stream);
int  rgbdfe_sizeof_inlier_header(void);
int  rgbdfe_set_params(rgbdfe_ctx* ctx, const rgbdfe_params* p);
const char* rgbdfe_status_string(int status);
const char* rgbdfe_last_error(rgbdfe_ctx* ctx);

/* ---- node residency (replaces Node::feature_descriptors_ / feature_locations_3d_,
 *      node.h:167-178; lifetime follows GraphManager::addNode / clearFeatureInformation,
 *      graph_manager.h:156-161, node.cpp:1431-1443) ---------------------------- */
/* desc: n x 32 bytes, row-major, continuous (cv::Mat CV_8U, node.cpp:567-568);
 * xyz1: n x 4 float, (x,y,z,1) as Node::projectTo3D writes them (node.cpp:955). */
int rgbdfe_upload_node(rgbdfe_ctx* ctx, int32_t node_id, const uint8_t* desc,
                       const float* xyz1, int32_t n);
/* Many nodes in one call (offline runs: the nodes of a stretch of frames): the same residency as n_nodes calls of
 * rgbdfe_upload_node, with one pinned staging pass, back-to-back copies and expansion launches and ONE wait -- ~10 us per
 * node instead of ~65.  desc[i]: counts[i] x 32 bytes, xyz1[i]: counts[i] x 4 floats.  Nothing is uploaded when an argument
 * is bad, a node has more than max_keypoints rows, an id appears twice or the free slots do not suffice. */
int rgbdfe_upload_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const uint8_t* const* desc,
                        const float* const* xyz1, const int32_t* counts);
/* same, sources already in device memory (device-to-device copy on `stream`, a hipStream_t).
 * Ordering: stream == NULL copies on the context's stream and returns when the node is resident.  With a caller
 * stream the copies are enqueued there and the call returns at once; every batch submitted to this context
 * afterwards (any entry point) waits for them on the device, and the sources must stay valid until `stream` has
 * passed the copies.  Overwriting a resident node first waits for the batches in flight. */
int rgbdfe_upload_node_device(rgbdfe_ctx* ctx, int32_t node_id, const void* d_desc,
                              const void* d_xyz1, int32_t n, void* stream);
/* Node::feature_locations_2d_ (KeyPoint.pt, n x 2 float) of a resident node: only the g2o refinement reads them
 * (edgeToFeature, transformation_estimation.cpp:95-125).  n must equal the node's row count. */
int rgbdfe_upload_node_keypoints(rgbdfe_ctx* ctx, int32_t node_id, const float* kp_xy, int32_t n);
int rgbdfe_release_node(rgbdfe_ctx* ctx, int32_t node_id);
int rgbdfe_node_count(rgbdfe_ctx* ctx, int32_t node_id); /* rows of a resident node or <0 */

/* ---- node read-back: the way out of the slabs (nodes that a batch detector wrote straight into their slots with NULL host
 *      outputs exist nowhere else) ------------------------------------------------------------------------------------
 * rgbdfe_download_nodes: the listed resident nodes in the order given (an id may appear twice).  Row counts are prefix-
 *   summed into row_offsets[n_nodes + 1]; every array is packed without gaps in that order, node i's rows at
 *   row_offsets[i] .. row_offsets[i + 1]:
 *     desc   32 bytes per row for ORB nodes (kind 0); 128 floats per row for SIFT (1) and float / FLANN (2) nodes, rows of a
 *            narrower float node zero-padded as they are resident -- the raw form the node was uploaded or detected with,
 *            not the fp4 / bf16 operands derived from it.  One call takes nodes of ONE kind: a mixed list is
 *            RGBDFE_ERR_INVALID_ARG.
 *     xyz1   4 floats per row.
 *     kp_xy  2 floats per row (rgbdfe_upload_node_keypoints); zeros for a node that holds no keypoints.
 *     stats  1 byte per row: feature_matching_stats_ (rgbdfe_node_feature_stats).  Zeros while no call has ever counted on
 *            this context; the read-back does not allocate the counters.
 *     kinds  [n_nodes]: the kind, with RGBDFE_NODE_HAS_KEYPOINTS or-ed in for a node that holds keypoints.
 *   Any output pointer may be NULL.  capacity_rows (of every array given) below the total is RGBDFE_ERR_CAPACITY with the
 *   total in row_offsets[n_nodes] and nothing else written.  With every array NULL and a capacity that suffices the call
 *   only fills row_offsets and kinds, without device work: the sizing call in front of the real one.  An id that is not
 *   resident is RGBDFE_ERR_UNKNOWN_NODE before any device work.  The call waits for the batches in flight on the context,
 *   as overwriting a node does.  Cost: one small table upload, ONE kernel launch, one device-to-host copy per array given
 *   and one wait, whatever n_nodes -- rgbdfe_upload_nodes' mirror image.  Single-device contexts (a multi-device handle
 *   answers from its first device, where every node is resident too).
 * rgbdfe_download_node: one node; returns its row count (>= 0) or a status; *kind and *has_keypoints may be NULL.
 * rgbdfe_download_nodes_stats: out[0..n_out) = { kernel launches of the latest read-back, its device-to-host copies, bytes
 *   of the read-back staging buffer, 1 if the context's feature counters have been allocated else 0 }.
 * rgbdfe_set_node_feature_stats: writes a resident node's counters back (n must equal its rows): what a restore needs
 *   behind the upload, which zeroes them. */
#define RGBDFE_NODE_HAS_KEYPOINTS 0x100
#define RGBDFE_DOWNLOAD_STATS 4
int rgbdfe_download_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc,
                          float* xyz1, float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds);
int rgbdfe_download_node(rgbdfe_ctx* ctx, int32_t node_id, int32_t capacity_rows, void* desc, float* xyz1, float* kp_xy,
                         uint8_t* stats, int32_t* kind, int32_t* has_keypoints);
int rgbdfe_download_nodes_stats(rgbdfe_ctx* ctx, int64_t* out, int32_t n_out);
/* diagnostics (tools/bench_session.py): rgbdfe_download_nodes' result through the obvious way -- per node one device-to-host
 * copy per array straight out of the slabs, one wait at the end; rgbdfe_download_nodes_stats then counts no launch and the copies */
int rgbdfe_debug_download_nodes_copy_loop(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc,
                                          float* xyz1, float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds);
int rgbdfe_set_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, const uint8_t* stats, int32_t n);

/* ---- the pair op -------------------------------------------------------- */
/* Batched Node::matchNodePair (node.h:85, node.cpp:1305-1429): for one new node and
 * n candidates.  1:1 replacement of
 *   QtConcurrent::blockingMapped(nodes_to_comp, bind(&Node::matchNodePair,new_node,_1))
 * (graph_manager.cpp:548): synchronous, out[i] belongs to candidate_ids[i]. */
int rgbdfe_match_node_pairs(rgbdfe_ctx* ctx, int32_t new_node_id, const int32_t* candidate_ids,
                            int32_t n_pairs, rgbdfe_match_result* out);
/* general pair list (query = newer node, train = older node) */
int rgbdfe_match_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                           int32_t n_pairs, rgbdfe_match_result* out);
/* asynchronous, results stay in device memory (d_out: n_pairs rgbdfe_match_result in HBM);
 * enqueued on `stream` (hipStream_t; NULL = the context's stream).  n_pairs must be
 * <= max_pairs_per_batch. */
int rgbdfe_match_pair_list_device(rgbdfe_ctx* ctx, const int32_t* query_ids,
                                  const int32_t* train_ids, int32_t n_pairs, void* d_out,
                                  void* stream);
/* Fully asynchronous form for pipelined callers: the batch is enqueued on one of the
 * context's internal streams (consecutive batches alternate streams, so batch k+1 overlaps the
 * tail of batch k) and identified by *ticket.  rgbdfe_wait_ticket makes `stream` (a
 * hipStream_t) wait for that batch, or blocks the host when stream == NULL.  d_out must stay
 * valid and untouched until the ticket has been waited for. */
int rgbdfe_submit_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                            int32_t n_pairs, void* d_out, int64_t* ticket);
int rgbdfe_wait_ticket(rgbdfe_ctx* ctx, int64_t ticket, void* stream);
/* The asynchronous form with results in HOST memory -- what GraphManager consumes (graph_manager.cpp:409-419, 554-560) at
 * the rate the device produces it: batch k's results travel device -> host behind batch k on its internal stream while
 * batch k+1 (submitted before the wait) computes on the other one.  payload RGBDFE_HOST_RECORDS: n_pairs
 * rgbdfe_match_result; RGBDFE_HOST_INLIERS: the inlier stream of the batch (rgbdfe_inlier_header above: n_pairs headers,
 * then the list block -- ~260 instead of 1744 bytes per pair on configs[1]); out_bytes = capacity of `out` (the worst case
 * of the inlier stream is n_pairs * (104 + 4 * RGBDFE_MAX_MATCHES)).  `out` stays the library's until rgbdfe_wait_host
 * (ticket) returns; *bytes_written (may be NULL) = the payload's size.  When `out` is pinned (hipHostMalloc /
 * rgbdfe_host_register) the download goes straight into it, otherwise through a pinned stage and one memcpy inside
 * rgbdfe_wait_host.  At most two jobs in flight per context (one per internal stream): a third submit before a wait is
 * refused with RGBDFE_ERR_CAPACITY.  Same results as rgbdfe_match_pair_list.  Single-device contexts only.
 * One waiter per ticket (a second concurrent rgbdfe_wait_host of the same ticket is refused).  When the payload does not
 * fit `out` (the inlier stream's list block is sized by the results), rgbdfe_wait_host returns RGBDFE_ERR_CAPACITY with
 * *bytes_written = the size the payload needs and the job STAYS pending: rgbdfe_wait_host_into(ticket, out2, bytes2)
 * collects it into a larger buffer (pageable or pinned; through the library's pinned stage), out2 == NULL drops it. */
#define RGBDFE_HOST_RECORDS 0
#define RGBDFE_HOST_INLIERS 1
int rgbdfe_submit_pair_list_host(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                                 void* out, size_t out_bytes, int payload, int64_t* ticket);
int rgbdfe_wait_host(rgbdfe_ctx* ctx, int64_t ticket, int64_t* bytes_written);
int rgbdfe_wait_host_into(rgbdfe_ctx* ctx, int64_t ticket, void* out, size_t out_bytes, int64_t* bytes_written);
int rgbdfe_synchronize(rgbdfe_ctx* ctx);

/* ---- SIFT (128-d float descriptor) nodes: matcher_type == "SIFTGPU" ------------------------
 * Replaces SiftGPUWrapper::match (sift_gpu_wrapper.h:61, sift_gpu_wrapper.cpp:169-227) inside
 * Node::featureMatching (node.cpp:553-557): u8-quantised dot products (exact on the bf16 MFMA),
 * acos distance / ratio tests, mutual best, DMatch.distance = float L2 of the raw descriptors.
 * desc128: n x 128 float, as Node::siftgpu_descriptors holds them (node.h:172). */
int rgbdfe_upload_sift_node(rgbdfe_ctx* ctx, int32_t node_id, const float* desc128,
                            const float* xyz1, int32_t n);
/* Batched matchNodePair for SIFT nodes.  out_dist (may be NULL): n_pairs x RGBDFE_MAX_MATCHES
 * floats, the DMatch.distance of out[i].all_q/all_t (all_hd is 0 on this path). */
int rgbdfe_match_sift_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                int32_t n_pairs, rgbdfe_match_result* out, float* out_dist);
/* same, asynchronous with results in HBM (see rgbdfe_submit_pair_list); d_out_dist may be NULL */
int rgbdfe_submit_sift_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids,
                                 int32_t n_pairs, void* d_out, void* d_out_dist, int64_t* ticket);
/* Twin of SiftGPUWrapper::match for two resident SIFT nodes: the mutual-best matches in ascending
 * query order (before keepStrongestMatches).  Arrays sized >= rows of the query node. */
int rgbdfe_sift_match_nodes(rgbdfe_ctx* ctx, int32_t query_id, int32_t train_id, int32_t* match_q,
                            int32_t* match_t, float* match_dist, int32_t* n_matches);

/* ---- float-descriptor nodes on Node::featureMatching's FLANN branch (node.cpp:610-667; a11) -------------------------
 * matcher_type == "FLANN" with a float extractor (SURF / SIFT / GFTT ...): knn-2 of every descriptor of the newer node
 * in the older node, ratio = dists[2i] / dists[2i+1] over FLANN's squared-L2 distances (:645), accepted when
 * nn_distance_ratio > ratio (:648), each train index once, first come first served in query order (:650-653),
 * DMatch.distance = the ratio (:657); then keepStrongestMatches and RANSAC as for every matcher.  The reference's
 * neighbours come from 4 randomised kd-trees searched with 16 checks (:493-505, :634) -- approximate and not
 * reproducible; here they are the EXACT two nearest (squared distance accumulated in flann::L2<float>'s order,
 * lowest row wins ties): the superset-quality replacement SURVEY.md 8(a) a11 names.
 * desc: n x dim float (Node::feature_descriptors_), dim a multiple of 4, <= 128.  out_dist (may be NULL) receives
 * the ratios of out[i].all_q/all_t (all_hd is 0 on this path). */
int rgbdfe_upload_float_node(rgbdfe_ctx* ctx, int32_t node_id, const float* desc, int32_t dim, const float* xyz1,
                             int32_t n);
int rgbdfe_match_flann_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs,
                                 double nn_distance_ratio, rgbdfe_match_result* out, float* out_dist);

/* ---- pieces of the pair op, exposed for A/B and parity ------------------- */
/* Batched bruteForceSearchORB (features.h:14, features.cpp:168-182) of every row of
 * query node against train node: out_hd[i] in [0,257], out_idx[i] (or -1), including
 * the reference's "last train row is never searched" behaviour. */
int rgbdfe_hamming_nn_nodes(rgbdfe_ctx* ctx, int32_t query_id, int32_t train_id,
                            int32_t* out_hd, int32_t* out_idx);
/* Drop-in twin of bruteForceSearchORB for host buffers (uploads, runs the kernel,
 * downloads; for A/B only -- the batched entry points are the product path). */
int rgbdfe_hamming_nn_host(rgbdfe_ctx* ctx, const uint8_t* qdesc, int32_t nq,
                           const uint8_t* tdesc, int32_t nt, int32_t* out_hd, int32_t* out_idx);

/* ---- per-frame depth filter + back-projection (removeDepthless node.cpp:67-97,
 *      projectTo3D node.cpp:900-965, backProject misc2.h:49-65) ---------------- */
/* kp_xy: n_kp x 2 float (KeyPoint.pt), depth: rows x cols float32 metres (NaN = invalid),
 * host buffers.  Writes kept_idx (indices into kp_xy, ascending) and xyz1 (n x 4) for the
 * first max_keypoints survivors; *n_out = survivors. */
int rgbdfe_project_to_3d(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* depth,
                         int32_t rows, int32_t cols, double fx, double fy, double cx, double cy,
                         double depth_scaling, int32_t max_keypoints, int32_t* kept_idx,
                         float* xyz1, int32_t* n_out);

/* a22 (i), the Node constructor that receives the sensor's organised point cloud (node.cpp:252-369):
 * rgbdfe_project_to_3d_cloud is Node::projectTo3D's point-cloud overload (node.cpp:855-898): lookup
 * point_cloud->at((int)x, (int)y) -- truncation --, drop when z > maximum_depth ("maximum_depth") or a coordinate is NaN,
 * the cloud's own (x, y, z, 1) is stored, cut at max_keypoints.  cloud: rows x cols x 4 float (x, y, z, rgb), host.
 * rgbdfe_detect_describe_cloud is that constructor's feature path: detect (:293) -> projectTo3D(cloud) (:308) ->
 * compute (:311), with the detector state / max_keypoints of rgbdfe_detector_configure; no removeDepthless, no
 * retainBest.  The 3-D points stay with their keypoints through compute()'s border filter and regrouping (the
 * reference leaves feature_locations_3d_ out of step there, its assert at :318). */
int rgbdfe_project_to_3d_cloud(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* cloud, int32_t rows,
                               int32_t cols, double maximum_depth, int32_t max_keypoints, int32_t* kept_idx, float* xyz1,
                               int32_t* n_out);

/* a20, SIFTGPU feature path: Node::projectTo3DSiftGPU (node.cpp:695-769) -- depth lookup with the
 * keypoint coordinates TRUNCATED to int (:733), no inside-the-image test (indices are clamped here
 * where the reference would read out of bounds), NaN depth drops the keypoint, stop at max_keypoints
 * (:748); the used descriptors are re-packed densely (:752-766) into
 *   siftgpu_descriptors  [n_out x 128] raw copy  = Node::siftgpu_descriptors, what rgbdfe_upload_sift_node takes
 *   feature_descriptors  [n_out x 128] (may be NULL) = Node::feature_descriptors_, RootSIFT-normalised by
 *                        squareroot_descriptor_space (node.cpp:1557-1571) when use_root_sift != 0
 *                        (parameter "use_root_sift", node.cpp:233-239).
 * kp_xy: n_kp x 2 f32, desc_in: n_kp x 128 f32, depth: rows x cols f32; outputs sized for
 * min(n_kp, max_keypoints) rows. */
int rgbdfe_sift_node_features(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* desc_in,
                              const float* depth, int32_t rows, int32_t cols, double fx, double fy,
                              double cx, double cy, double depth_scaling, int32_t max_keypoints,
                              int32_t use_root_sift, int32_t* kept_idx, float* xyz1,
                              float* siftgpu_descriptors, float* feature_descriptors, int32_t* n_out);
/* The same with "use_feature_min_depth" on (parameter_server.cpp:90, node.cpp:727-731): a keypoint's depth is
 * getMinDepthInNeighborhood(depth, pt, size) (misc.cpp:774-793); kp_size = cv::KeyPoint::size per keypoint (for SiftGPU
 * keypoints 12 * scale, what rgbdfe_sift_detect returns). */
int rgbdfe_sift_node_features_min_depth(rgbdfe_ctx* ctx, const float* kp_xy, const float* kp_size, int32_t n_kp,
                                        const float* desc_in, const float* depth, int32_t rows, int32_t cols, double fx,
                                        double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                        int32_t use_root_sift, int32_t* kept_idx, float* xyz1, float* siftgpu_descriptors,
                                        float* feature_descriptors, int32_t* n_out);

/* Two schedules of a batch's RANSAC work give byte-identical results:
 *   record / replay       (default) the refinement loops of a pair's iterations are spread over many waves, which write
 *                         each iteration's outcome; one wave per pair then replays the records in iteration order with
 *                         the reference's bookkeeping (node.cpp:1171-1190).  Three launches: every iteration's hypothesis
 *                         and a lane-parallel pre-screen of the junk ones, ONE refinement launch over the viable
 *                         iterations of the whole batch, the result waves.  Up to 256 pairs all iterations are recorded
 *                         (full speculation, a pair's range cut into shares: one node against 20 candidates returns in
 *                         0.2-0.4 ms instead of 5.7 ms); in larger batches a pair is recorded in up to four windows
 *                         ([0,14), [14,70), [70,140), [140,200) for 200 iterations) with the bookkeeping run between
 *                         them, so recording stops where the reference stops iterating -- except that a pair whose
 *                         loop has not jumped ahead (it += 10 / 20) and whose hypotheses are mostly junk is recorded to
 *                         the end at once.  Batches beyond 2^24 / ransac_iterations (or 65535) pairs run as pieces of
 *                         that size;
 *   one wave per pair     a wave runs a pair's whole loop (windows of 7 iterations, replayed in order): exactly the
 *                         iterations the reference runs, but a pair takes ~4.6 ms however idle the chip is and a
 *                         launch lasts as long as its slowest pair.  Kept as the byte reference of record / replay; the
 *                         library takes it by itself only when the record buffer cannot be allocated.
 * Batches of at most max_pairs pairs (ORB, SIFT, FLANN) take record / replay.  Defaults: max_pairs = INT32_MAX (every
 * batch), chunk_iterations = 0 (automatic: 4 up to 64 pairs, 7 up to 640, 14 up to 1280, 28 above; the shares of a
 * fully speculated batch are derived from it); max_pairs = 0 forces one wave per pair.
 * A negative chunk_iterations selects the windowed plan for every batch size, with |chunk_iterations| in the place of
 * the automatic value (a testing aid: small batches are faster with full speculation). */
int rgbdfe_set_latency_mode(rgbdfe_ctx* ctx, int32_t max_pairs, int32_t chunk_iterations);

/* Which kernel computes the Hamming nearest neighbours of an ORB batch (identical keys, bit for bit):
 *   1            the descriptor bits as fp4 (+-1) operands of v_mfma_f32_32x32x64_f8f6f4: hd = (256 + dot) / 2, exact
 *                in the f32 accumulator, the row index folded into the accumulator's initial value (hamming_mfma.hip);
 *   3            the same contraction as a software pipeline inside every wave (the reduction of one accumulator and the
 *                LDS reads of the next train tile sit between the MFMAs of the other accumulator; train tiles arrive by
 *                global_load_lds through three LDS buffers);
 *   2            as 1, the row index added by the VALU instead of the matrix core's C operand;
 *   0            xor + popcount on the VALU (hamming_nn.hip) -- also what nodes with max_keypoints > 32768 get;
 *   4            mode 3's kernel with 512 instead of 256 queries per block (four query tiles per wave), whatever the batch.
 * RGBDFE_HAMMING_MODE_DEFAULT is the mode of a new context; environment variable RGBDFE_HAMMING_MODE overrides it.
 * A context left at mode 3 picks the block width per batch: 512 queries where the batch fills the chip many times over
 * without splitting the train rows, 256 otherwise (every live-SLAM batch); environment variable RGBDFE_HAMMING_WIDE = 0 / 1
 * (read by rgbdfe_create) fixes it, and rgbdfe_set_hamming_mode(ctx, 3) asks for 256-query blocks by name.
 * rgbdfe_hamming_wide_last: 1 = the latest Hamming launch of the context ran 512-query blocks, 0 = it did not, -1 = there
 * was none yet.
 * Mode 3's 512-query blocks exist on both shapes of the fp4 MFMA: 32x32x64 tiles (mode 4's kernel) and 16x16x128 tiles
 * (same blocks, same slab, same keys).  rgbdfe_set_hamming_shape(ctx, 0 | 16 | 32): 0 = the library's choice, 16 / 32 =
 * that tile wherever mode 3 runs 512-query blocks; environment variable RGBDFE_HAMMING_SHAPE (read by rgbdfe_create) sets
 * the same.  256-query blocks, modes 1, 2 and mode 4 by name are 32x32x64 whatever the shape.
 * rgbdfe_hamming_shape_last: 16 / 32 = the MFMA tile of the latest Hamming launch of the context, 0 = it ran the popcount
 * kernel, -1 = there was none yet. */
#define RGBDFE_HAMMING_MODE_DEFAULT 3
int rgbdfe_set_hamming_mode(rgbdfe_ctx* ctx, int32_t mode);
int rgbdfe_hamming_wide_last(rgbdfe_ctx* ctx);
int rgbdfe_set_hamming_shape(rgbdfe_ctx* ctx, int32_t shape);
int rgbdfe_hamming_shape_last(rgbdfe_ctx* ctx);

/* ---- frame-level data either side of the pair path ----------------
 * rgbdfe_depth_to_mono8: depthToCV8UC1 (misc.cpp:414-430), the detection mask the listener derives from
 *   the depth image.  depth_is_u16 == 0: depth is rows x cols f32 (metres), mono8 = convertTo(CV_8UC1, 100)
 *   (:418), depth_m is ignored.  depth_is_u16 != 0: depth is u16 millimetres, mono8 = convertTo(CV_8UC1,
 *   0.05, -25) (:423) and depth_m (required) = the float image in metres (:424-425).
 * rgbdfe_upload_node_cloud: createXYZRGBPointCloud (misc.cpp:467-556) on the device.  Builds the node's
 *   structured cloud -- (rows/cloud_skip) x (cols/cloud_skip) points of 4 floats (x, y, z, rgb bits
 *   0x00RRGGBB) -- from its depth image (f32, metres x depth_scaling; Z < min_depth or NaN -> z = NaN with
 *   x, y at 1 m, :525-530) and keeps it resident under node_id (Node::pc_col) for the environment measurement
 *   model; rgb (rows x cols x rgb_channels u8, channels 1 or 3, may be NULL) only colours the points.
 *   cloud_skip = cloud_creation_skip_step must divide rows and cols (the reference crashes otherwise, :479).
 *   cloud_out (may be NULL) receives a copy.  rgbdfe_release_node also drops the node's cloud.
 * rgbdfe_observation_likelihood: observationLikelihood (misc.cpp:814-969) for a batch of directed edges:
 *   job i projects the cloud of new_ids[i], transformed by transforms[i] (16 floats, column-major, new ->
 *   old), into the raster of old_ids[i] and classifies every emm_skip_step-th point (parameter
 *   "emm__skip_step", 8) against the old depth.  pairwiseObservationLikelihood (node.cpp:1520-1554) is two
 *   jobs per edge, (newer, older, final_trafo) and (older, newer, final_trafo.inverse()), with the counts
 *   summed; matchNodePair then keeps the edge iff rgbdfe_observation_criterion_met(inliers, outliers,
 *   occluded + inliers + outliers, observability_threshold) (node.cpp:1341-1342, misc.cpp:1136-1148).
 *   depth_covariance() is params.depth_cov (the reference's frozen static, misc2.h:30-35).
 *   One batch, one cloud size: every structured cloud named by a call, new or old, must have the dimensions of job 0's
 *   old cloud, and every old cloud its cloud_skip; otherwise the call returns RGBDFE_ERR_INVALID_ARG and writes nothing to out.
 *   (The reference returns all-zero counts for one pair of "differing width", misc.cpp:844-847: that result is not
 *   reproduced; send such pairs in calls of their own size.)  If job 0's old cloud is unstructured (rows or cols
 *   <= 1, rgbdfe_reduce_node_cloud), every old cloud of the call must be, and every job answers inliers = all = 1
 *   (misc.cpp:835-843).  emm_skip_step <= 0 answers the same for every job (:831). */
typedef struct rgbdfe_emm_counts {
  uint32_t inliers, outliers, occluded, all;
} rgbdfe_emm_counts;
int rgbdfe_depth_to_mono8(rgbdfe_ctx* ctx, const void* depth, int32_t depth_is_u16, int32_t rows, int32_t cols,
                          uint8_t* mono8, float* depth_m);
int rgbdfe_upload_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, const float* depth, int32_t rows, int32_t cols,
                             const uint8_t* rgb, int32_t rgb_channels, int32_t encoding_bgr, double fx,
                             double fy, double cx, double cy, double depth_scaling, double min_depth,
                             int32_t cloud_skip, float* cloud_out);
int rgbdfe_release_node_cloud(rgbdfe_ctx* ctx, int32_t node_id);
int rgbdfe_observation_likelihood(rgbdfe_ctx* ctx, int32_t n, const int32_t* new_ids, const int32_t* old_ids,
                                  const float* transforms, int32_t emm_skip_step, rgbdfe_emm_counts* out);
int rgbdfe_observation_criterion_met(uint32_t inliers, uint32_t outliers, uint32_t all,
                                     double observability_threshold, double* quality);

/* ---- map assembly: the resident node clouds as one world-frame cloud --------------------------------------
 * rgbdfe_assemble_map is transformAndAppendPointCloud (misc.cpp:183-238, the non-HEMACLOUDS form) over a list of
 *   resident node clouds: the loop of GraphManager::saveAllCloudsToFile (graph_mgr_io.cpp:529-552), on the device.
 *   node_ids are processed in the order given (pass graph_ order, without the nodes that have no valid estimate); an
 *   id may appear more than once; clouds of different sizes may be mixed.  transforms: n_nodes x 16 floats, each a
 *   column-major Matrix4f = pcl_ros::transformAsMatrix(world2cam); the composition world2cam = cam2rgb *
 *   eigenTransf2TF(v->estimate()) stays with the caller.  maximum_depth is the parameter of that name, taken as
 *   float: negative or NaN disables the range clip, +inf (the reference default) never clips.
 *   preserve_raster == 0 ("preserve_raster_on_save" off): points beyond the range (squared distance in float >
 *   maximum_depth squared) and points with a NaN coordinate are dropped, the others are transformed; the output is
 *   the kept points in (node, point) order.  preserve_raster != 0: every point keeps its row; a point beyond the
 *   range gets quiet-NaN coordinates (0x7fc00000) and keeps its rgb word, a point with a NaN coordinate is copied
 *   untransformed (the finite x, y "at 1 m" beside a NaN z of createXYZRGBPointCloud included).
 *   out: capacity rows of 4 floats (x, y, z, rgb bits).  *n_out = rows of the assembled cloud; node_offsets (may be
 *   NULL; n_nodes + 1 entries) = the first output row of every node, node_offsets[n_nodes] = *n_out, in both modes.
 *   capacity < *n_out: RGBDFE_ERR_CAPACITY with *n_out = the needed size (out's contents are then unspecified); the
 *   sum of the listed clouds' sizes always suffices.  An id without a cloud: RGBDFE_ERR_UNKNOWN_NODE, before any
 *   device work.  n_nodes == 0: RGBDFE_OK, *n_out = 0.
 * rgbdfe_assemble_map_device: the same with `d_out` a device pointer of the context's device (the first device of a
 *   multi-device handle); no point crosses to the host.  The kernels run on `stream` (NULL: the context's own); the
 *   call returns when they have finished.  n_out and node_offsets are host pointers.
 * rgbdfe_download_node_cloud: the resident cloud of a node -- rows x cols x 4 floats exactly as cloud_out of
 *   rgbdfe_upload_node_cloud would have received them, also for the clouds the sensor batch path keeps.  rows / cols
 *   (may be NULL) are set whenever the node has a cloud; capacity_points < rows x cols: RGBDFE_ERR_CAPACITY. */
int rgbdfe_assemble_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                        double maximum_depth, int32_t preserve_raster, float* out, int64_t capacity, int64_t* n_out,
                        int64_t* node_offsets);
int rgbdfe_assemble_map_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                               double maximum_depth, int32_t preserve_raster, void* d_out, int64_t capacity,
                               int64_t* n_out, int64_t* node_offsets, void* stream);
int rgbdfe_download_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, float* cloud_out, int64_t capacity_points,
                               int32_t* rows, int32_t* cols);

/* ---- voxel filter: a cloud reduced to the centroids of its occupied grid cells ----------------------------
 * rgbdfe_voxel_filter is the pcl::VoxelGrid<point_type> of Node::reducePointCloud (node.cpp:1448-1460; parameter
 *   "voxelfilter_size", parameter_server.cpp:159) with the filter's defaults: cubic leaf, all fields downsampled, no
 *   filter field, min_points_per_voxel 0, an input that is not dense.  PCL is not part of the reference tree: the
 *   statements below are this library's contract (restated, not pinned).  Points are rows of 4 floats
 *   (x, y, z, rgb bits); all arithmetic is float32 with one rounding per operation.
 *   L = (float)voxelfilter_size, inv = 1.0f / L; unless L > 0 and inv is finite and non-zero: RGBDFE_ERR_INVALID_ARG.
 *   A point is valid iff x, y and z are finite; invalid points take part in nothing.  No valid point, or n_in == 0:
 *   *n_out = 0, RGBDFE_OK.  min_p / max_p = the exact componentwise bounds of the valid points.
 *   Leaf too small: d[a] = (int64)((max_p[a] - min_p[a]) * inv) + 1; if a float product is >= 2^31 or d0 * d1 * d2 >
 *   INT32_MAX, the filter hands back its input: *n_out = n_in, out = every input row in order, byte for byte (the
 *   invalid ones too), *flags has RGBDFE_VOXEL_LEAF_TOO_SMALL, the status is RGBDFE_OK.
 *   Grid: min_b[a] = (int)floorf(min_p[a] * inv), max_b likewise, div[a] = max_b[a] - min_b[a] + 1, mul = (1, div0,
 *   div0 * div1) as int32.  Cell of a point: ijk[a] = (int)(floorf(p[a] * inv) - (float)min_b[a]), idx = ijk0 + ijk1 *
 *   mul1 + ijk2 * mul2 (int32).  One output row per occupied cell, in ascending idx.  With n the cell's member count,
 *   each of x, y, z is the float sum of the members in ascending input index, starting from the first member's value,
 *   divided by (float)n (IEEE division); r, g, b (bits 23-16, 15-8, 7-0 of the rgb word) are converted to float,
 *   summed and divided likewise, truncated with (int), and packed as r << 16 | g << 8 | b (top byte 0).
 *   PCL's own order inside a cell is what an unstable std::sort leaves; against any order the cells, their order,
 *   their counts and (while 255 n < 2^24) the rgb words are the same, and x, y, z differ by at most
 *   2 n 2^-24 max|coordinate|.
 *   out: capacity rows.  capacity < *n_out: RGBDFE_ERR_CAPACITY with *n_out = the needed size, before the output
 *   pass; n_in rows always suffice.  n_in >= 2^31: RGBDFE_ERR_CAPACITY.  flags may be NULL.
 * rgbdfe_voxel_filter_device: the same over device buffers of the context's device (the first device of a
 *   multi-device handle); no point crosses to the host.  The kernels run on `stream` (NULL: the context's own); the
 *   call returns when they have finished.  d_out must not overlap d_points (refused where the ranges show it).  n_out
 *   and flags are host pointers.
 * rgbdfe_reduce_node_cloud is Node::reducePointCloud: the node's resident cloud is replaced by its filtered cloud,
 *   unstructured (rgbdfe_download_node_cloud then reports rows 1, cols *n_out; 0 points are a cloud too).  The cached
 *   samples of the measurement model are dropped, the intrinsics kept; rgbdfe_observation_likelihood answers for such
 *   a cloud as the reference does for an unstructured one (misc.cpp:835-843: inliers = all = 1; parameter_server.cpp:233
 *   calls the combination an error), rgbdfe_assemble_map takes it like any other cloud.  With
 *   RGBDFE_VOXEL_LEAF_TOO_SMALL the cloud stays as it is.  A node without a cloud: RGBDFE_ERR_UNKNOWN_NODE. */
#define RGBDFE_VOXEL_LEAF_TOO_SMALL 1
int rgbdfe_voxel_filter(rgbdfe_ctx* ctx, const float* points, int64_t n_in, double voxelfilter_size, float* out,
                        int64_t capacity, int64_t* n_out, int32_t* flags);
int rgbdfe_voxel_filter_device(rgbdfe_ctx* ctx, const void* d_points, int64_t n_in, double voxelfilter_size,
                               void* d_out, int64_t capacity, int64_t* n_out, int32_t* flags, void* stream);
int rgbdfe_reduce_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, double voxelfilter_size, int64_t* n_out,
                             int32_t* flags);

/* ---- occupancy map: node clouds ray-cast into a colour OctoMap on the device ------------------------------
 * An rgbdfe_octomap is the octree of ColorOctomapServer (ColorOctomapServer.cpp:61-129), fed as
 *   GraphManager::renderToOctomap / saveOctomapImpl feed it (graph_mgr_io.cpp:253-329): insertPointCloud(cloud, origin,
 *   max_range, lazy_eval = true) and then averageNodeColor per point, one cloud after another.  Its state is the set of
 *   leaves, all at depth 16 (lazy insertion, nothing prunes): key, log-odds, colour.  The octomap library is not part
 *   of the reference tree: the statements below are this library's contract, a restatement of the published 1.6-1.9
 *   line (restated, not pinned).  One rounding per operation; "float" is binary32, "double" binary64.
 *   Parameters (rgbdfe_octomap_default_params: parameter_server.cpp:56-64): resolution > 0 and finite with a finite
 *   inverse, prob_hit / prob_miss / clamping_min / clamping_max inside (0, 1), clamping_min <= clamping_max, else
 *   RGBDFE_ERR_INVALID_ARG.  logodds(p) = (float)log(p / (1 - p)) (double, then one conversion); occupancy_threshold
 *   is used by the read side only (the third block) and is checked there.
 *   A cloud = rows of 4 floats (x, y, z, rgb bits) and a column-major Matrix4f (as rgbdfe_assemble_map takes it);
 *   origin = its translation column (T[12], T[13], T[14]).
 *   Transform: a row whose x, y and z are finite becomes p[a] = ((R[a][0] * x + R[a][1] * y) + R[a][2] * z) + t[a] in
 *   float.  A row with a non-finite coordinate before or after the transform contributes nothing, neither to the
 *   occupancy nor to the colours.
 *   Key of a coordinate c (float): k = floor((1.0 / resolution) * (double)c) + 32768, valid iff 0 <= k < 65536; a
 *   point's key is valid iff its three are.  Centre of key k = ((double)(k - 32768) + 0.5) * resolution.
 *   Range (computeUpdate without a bounding box): d = p - origin in float, norm = sqrt((double)((dx * dx + dy * dy) +
 *   dz * dz)) with the sum in float.  max_range < 0 or norm <= max_range: the ray origin -> p yields free cells, and
 *   p's cell, if its key is valid, is occupied.  Otherwise the ray is origin -> origin + (d / (float)norm) *
 *   (float)max_range, free cells only.  max_range NaN: RGBDFE_ERR_INVALID_ARG; +inf never clips.
 *   Ray origin -> e (computeRayKeys, Amanatides & Woo): nothing if a key of origin or e is invalid or the two keys are
 *   equal; otherwise the origin's cell is free.  d = e - origin, length = (float)norm(d) as above, dir = d / length in
 *   float; step[a] = sign of dir[a].  For step[a] != 0: tMax[a] = ((centre(key[a]) + (double)(float)(step[a] *
 *   resolution * 0.5)) - (double)origin[a]) / (double)dir[a], tDelta[a] = resolution / fabs((double)dir[a]); DBL_MAX
 *   both where step[a] == 0.  Each iteration takes a = tMax0 < tMax1 ? (tMax0 < tMax2 ? 0 : 2) : (tMax1 < tMax2 ? 1 : 2)
 *   (a tie falls to the later axis), then key[a] += step[a] (16-bit, wrapping) and tMax[a] += tDelta[a]; it ends when
 *   the key equals e's key, or when min(tMax) > (double)length (the library's guard against a missed end cell), in
 *   both cases without a cell; otherwise the cell is free.  A ray ends after 196608 iterations (no ray between two valid
 *   keys needs more; the library has no such bound).
 *   Per cloud: the free and the occupied set are formed over the whole cloud, a cell in both is occupied only, and
 *   every cell of either set takes exactly one update: a new leaf starts at 0 with colour (255, 255, 255); value =
 *   value + logodds(prob_hit or prob_miss) in float, then value < logodds(clamping_min) -> that bound, value >
 *   logodds(clamping_max) -> that bound.
 *   Colour (averageNodeColor), after the cloud's occupancy update: over the contributing rows in ascending index,
 *   those beyond max_range included: if the row's key is valid and a leaf (free or occupied) exists there, then with
 *   r, g, b = bits 23-16, 15-8, 7-0 of the row's rgb word: a leaf whose colour is not (255, 255, 255) takes (prev +
 *   new) / 2 per channel in integer arithmetic, a leaf whose colour is (255, 255, 255) takes the new colour.  (An
 *   average that lands on white therefore starts again, as in the library.)
 *   Clouds are applied strictly one after another in list order: clamping and the colour rule do not commute.
 *   Pruning, the bounding-box branch, occupancyFilter and .bt files are out of scope; inner nodes
 *   (updateInnerOccupancy), depth queries and .ot files: the next block.
 * rgbdfe_octomap_create: a map of capacity_cells cells (1 <= capacity_cells < 2^31; 20 bytes each) on the context's
 *   device (the first device of a multi-device handle); params NULL = the defaults.  Destroy the map before the
 *   context.  rgbdfe_octomap_reset is ColorOctomapServer::reset (no leaves, same parameters, same capacity).
 *   rgbdfe_octomap_reserve re-houses the leaves in a table of capacity_cells cells on the device (fewer than the map
 *   has leaves: RGBDFE_ERR_CAPACITY, nothing changes).
 * Capacity: the map holds at most capacity_cells leaves and never drops a cell silently.  A cloud fits iff the
 *   leaves before it plus the new cells of its free and occupied sets are at most capacity_cells.  If a cloud does
 *   not fit, the call returns RGBDFE_ERR_CAPACITY with *n_done = the number of clouds applied in full, and the map
 *   equals, leaf for leaf, the map after those clouds; reserve more and go on with the rest of the list.
 *   The table is open addressing with linear probing: exact up to the last cell, but fast only while the load stays
 *   well below 1 (the wrappers double the capacity when a cloud does not fit).
 * rgbdfe_octomap_insert_nodes: node_ids / transforms exactly as rgbdfe_assemble_map takes them (ids may repeat, sizes
 *   may be mixed, a cloud reduced by rgbdfe_reduce_node_cloud is an ordinary input); max_range is the reference's
 *   maximum_depth.  An id without a cloud: RGBDFE_ERR_UNKNOWN_NODE before any state changes.  n_done may be NULL.
 * rgbdfe_octomap_insert_cloud: the same for one host array of n rows (n >= 2^31: RGBDFE_ERR_CAPACITY).
 * rgbdfe_octomap_leaves: the leaves as 16-byte records in ascending key[0] | key[1] << 16 | key[2] << 32; capacity <
 *   the number of leaves: RGBDFE_ERR_CAPACITY with *n_out = the needed size, before anything is written.
 * rgbdfe_octomap_stats: out[0] = capacity_cells, out[1] = leaves, out[2] = kernel launches of the last insert call,
 *   out[3] = kernel launches of the last tree / tree_device / nodes_at_depth / write call, out[4] = kernel launches
 *   of the last search / cast_rays / view_cloud / view_cloud_device call; further entries 0. */
typedef struct rgbdfe_octomap rgbdfe_octomap;
typedef struct rgbdfe_octomap_params {
  double resolution;           /* octomap_resolution, 0.05 */
  double prob_hit;             /* octomap_prob_hit, 0.9 */
  double prob_miss;            /* octomap_prob_miss, 0.4 */
  double clamping_min;         /* octomap_clamping_min, 0.001 */
  double clamping_max;         /* octomap_clamping_max, 0.999 */
  double occupancy_threshold;  /* octomap_occupancy_threshold, 0.5: the read side's default */
} rgbdfe_octomap_params;
typedef struct rgbdfe_octomap_leaf {
  uint16_t key[3];
  uint16_t zero0;
  float log_odds;
  uint8_t rgb[3];
  uint8_t zero1;
} rgbdfe_octomap_leaf;
void rgbdfe_octomap_default_params(rgbdfe_octomap_params* params);
int rgbdfe_octomap_create(rgbdfe_ctx* ctx, const rgbdfe_octomap_params* params, int64_t capacity_cells,
                          rgbdfe_octomap** map);
void rgbdfe_octomap_destroy(rgbdfe_octomap* map);
int rgbdfe_octomap_reset(rgbdfe_octomap* map);
int rgbdfe_octomap_reserve(rgbdfe_octomap* map, int64_t capacity_cells);
int rgbdfe_octomap_insert_nodes(rgbdfe_octomap* map, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                                double max_range, int32_t* n_done);
int rgbdfe_octomap_insert_cloud(rgbdfe_octomap* map, const float* points, int64_t n, const float* transform,
                                double max_range);
int rgbdfe_octomap_size(rgbdfe_octomap* map, int64_t* n_leaves);
int rgbdfe_octomap_leaves(rgbdfe_octomap* map, rgbdfe_octomap_leaf* out, int64_t capacity, int64_t* n_out);
int rgbdfe_octomap_stats(rgbdfe_octomap* map, int64_t* out, int32_t n_out);

/* ---- occupancy map: the tree of a leaf set -- inner nodes, one depth, .ot files ---------------------------------
 * What ColorOctomapServer::save (ColorOctomapServer.cpp:38-58: updateInnerOccupancy is :128, then AbstractOcTree::write)
 *   and ColorOctomapServer::render (:187-268, the nodes of octomap_display_level) need beyond the leaves, built on the
 *   device from the leaves of an rgbdfe_octomap.  As above, the contract is this library's restatement of the published
 *   octomap 1.6-1.9 line (restated, not pinned).
 *   Shape and order: all leaves are at depth 16, the root at depth 0.  On the way down the child index at depth d
 *   (1 .. 16) is taken from bit b = 16 - d of the key (computeChildIdx): ((k0 >> b) & 1) | ((k1 >> b) & 1) << 1 |
 *   ((k2 >> b) & 1) << 2.  A leaf's path code is the 48-bit number of its 16 child indices, the depth-1 index most
 *   significant.  Depth-first pre-order with the children in ascending index = the nodes ordered by (path code of their
 *   first leaf, depth); every file and query order below is that order.
 *   The tree is a pure function of the leaf set (lazy insertion creates inner nodes and never reads them, nothing
 *   prunes, updateInnerOccupancy overwrites every inner value).  An empty map has no nodes, not even a root; otherwise
 *   the root exists.
 *   Inner node values, bottom-up from the final children (updateOccupancyChildren, updateColorChildren /
 *   getAverageChildColor): log_odds = the float maximum over the existing children, starting from -FLT_MAX (a subtree
 *   of free cells has a negative value).  Colour: over the existing children whose colour is not (255, 255, 255), c
 *   their number, each channel = the integer sum divided by c, truncated; c = 0: (255, 255, 255).  The average is
 *   hierarchical (a parent averages its children's already truncated colours, not the leaves below), and an inner node
 *   that comes out white counts as unset one level up (the library's rule: reproduced, not mended).
 *   Node record (rgbdfe_octomap_node, 8 bytes, the bytes ColorOcTreeNode writes): float log_odds (little endian),
 *   uint8_t rgb[3], uint8_t children (bit i set iff child i exists; 0 for a leaf).
 *   .ot file (AbstractOcTree::write): the lines "# Octomap OcTree file", "# (feel free to add / change comments, but
 *   leave the first line as it is!)", "#", "id ColorOcTree", "size <number of nodes>", "res <resolution as printf %g>",
 *   "data", each ended by '\n', then the node records in pre-order.  An empty map: "size 0" and no data.
 * rgbdfe_octomap_tree: the records in pre-order to host memory.  capacity < the number of nodes: RGBDFE_ERR_CAPACITY
 *   with *n_nodes = the needed size, before anything is written.  rgbdfe_octomap_tree_device: the same into device
 *   memory of the map's device (`stream` NULL: the context's stream; the call returns when the records are in place).
 *   A map with more than (2^32 - 1) / 17 leaves is refused by every call of this block (RGBDFE_ERR_CAPACITY): node
 *   positions are 32-bit on the device.
 * rgbdfe_octomap_nodes_at_depth: the nodes of one depth (0 .. 16) whose log_odds >= min_log_odds by float comparison,
 *   in tree order, as rgbdfe_octomap_leaf records whose key is the first cell's key with the low 16 - depth bits
 *   cleared (the key keyToCoord(key, depth) takes); -INFINITY returns every node of the depth.  NaN or a depth outside
 *   0 .. 16: RGBDFE_ERR_INVALID_ARG; capacity as above with *n_out.  This is the set render() walks at
 *   octomap_display_level.  With s = 16 - depth, a node's edge is resolution * 2^s (getNodeSize(depth)) and its centre
 *   on axis a is keyToCoord(key[a], depth) = (floor(((double)key[a] - 32768) / 2^s) + 0.5) * (resolution * 2^s); the
 *   division is exact for the keys returned here.  "occupancy >= thr" corresponds to log_odds >= log(thr / (1 - thr));
 *   that conversion and render()'s alpha byte stay with the caller (exp in double is not bit-reproducible between the
 *   device and a host libm, and this interface does not need it).
 * rgbdfe_octomap_write: ColorOctomapServer::save: the header on the host, the payload built on the device.  A file
 *   that cannot be opened: RGBDFE_ERR_INVALID_ARG; a write that fails: RGBDFE_ERR_INTERNAL and the file is removed,
 *   so that nothing partial stays behind under the name.
 * rgbdfe_octomap_set_leaves: the map's contents replaced by these n leaves (any order), parameters and capacity
 *   unchanged.  n above the capacity: RGBDFE_ERR_CAPACITY, nothing changes.  A repeated key, a non-zero padding field
 *   or a non-finite log-odds: RGBDFE_ERR_INVALID_ARG, the map is left empty.
 * rgbdfe_octomap_read: an .ot file parsed on the host, then rgbdfe_octomap_set_leaves.  Inner values in the file are
 *   ignored (they are a function of the leaves).  Refused with RGBDFE_ERR_INVALID_ARG and a message that says which
 *   (the map is unchanged): a first line other than the format's, an id other than ColorOcTree, a res whose %g text
 *   differs from the map's, a truncated file, a size that does not match the records (or bytes behind them), a node
 *   above depth 16 without children (a pruned file from elsewhere) or one of depth 16 with children.
 * None of these calls changes the leaves except the last two; a tree call between two inserts does not alter what the
 *   later insert produces.  Nothing is cached: every call works from the leaves as they are.  The calls' workspace
 *   (about 76 bytes per leaf) belongs to the map and goes with rgbdfe_octomap_destroy. */
typedef struct rgbdfe_octomap_node {
  float log_odds;
  uint8_t rgb[3];
  uint8_t children;
} rgbdfe_octomap_node;
int rgbdfe_octomap_tree(rgbdfe_octomap* map, rgbdfe_octomap_node* out, int64_t capacity, int64_t* n_nodes);
int rgbdfe_octomap_tree_device(rgbdfe_octomap* map, void* d_out, int64_t capacity, int64_t* n_nodes, void* stream);
int rgbdfe_octomap_nodes_at_depth(rgbdfe_octomap* map, int32_t depth, float min_log_odds, rgbdfe_octomap_leaf* out,
                                  int64_t capacity, int64_t* n_out);
int rgbdfe_octomap_write(rgbdfe_octomap* map, const char* path);
int rgbdfe_octomap_set_leaves(rgbdfe_octomap* map, const rgbdfe_octomap_leaf* leaves, int64_t n);
int rgbdfe_octomap_read(rgbdfe_octomap* map, const char* path);

/* ---- occupancy map: the read side -- point lookups, ray casts, the map seen from a pose ------------------------
 * What a consumer of the map asks it: OcTreeBaseImpl::search, OccupancyOcTreeBase::isNodeOccupied / castRay -- the
 *   primitives under ColorOctomapServer::occupancyFilter (ColorOctomapServer.cpp:132-185: coordToKey, search,
 *   keyToCoord; the filter itself stays out of scope for the reasons of the first block).  As above, the contract is this
 *   library's restatement of the published octomap 1.6-1.9 line (restated, not pinned), one rounding per
 *   operation.  Keys, centres and the norm are those of the first block; a centre as a float is (float)centre(k).
 *   Leaf at a key: a leaf exists iff the table holds the key and its value word is a leaf's (a key that an unfinished
 *   cloud claimed and that never became a leaf is not one).  All leaves are at depth 16, so search(key) is this lookup.
 *   Occupied: a leaf is occupied iff log_odds >= occupied_log_odds by float comparison.  occupied_log_odds is a float
 *   of the call; NaN stands for the map's own, logodds(params.occupancy_threshold), which rgbdfe_octomap_occupied_log_odds
 *   returns.  occupancy_threshold is checked where it is used: that getter, and a call that passes NaN, return
 *   RGBDFE_ERR_INVALID_ARG unless it lies inside (0, 1); rgbdfe_octomap_create accepts any value.
 *   Search of a point (three floats, world frame): found = 2 if a coordinate is non-finite or the key invalid (the record
 *   is zero); otherwise the record carries the key, and found = 1 with the leaf's log-odds and colour, or found = 0
 *   with both zero.
 *   Ray cast (castRay) of origin o and direction d, three floats each; the checks in this order:
 *   1. o non-finite or its key invalid: BAD_ORIGIN (steps 0, key and centre zero).  Otherwise end = o's cell.
 *   2. The origin's cell: an occupied leaf there: HIT with 0 steps.  No leaf and ignore_unknown == 0: UNKNOWN with 0
 *      steps.  (A leaf that is not occupied, or no leaf with ignore_unknown != 0: go on.)
 *   3. n = sqrt((double)((dx * dx + dy * dy) + dz * dz)) with the sum in float, dir = d / (float)n in float, step[a] =
 *      sign of dir[a].  n not > 0 (NaN too), a non-finite dir[a], or step == (0, 0, 0) (an infinite n divides every
 *      component to zero): BAD_DIRECTION with 0 steps, end = o's cell.
 *   4. For step[a] != 0: tMax[a] = ((centre(key[a]) + ((double)step[a] * resolution) * 0.5) - (double)o[a]) /
 *      (double)dir[a], tDelta[a] = resolution / fabs((double)dir[a]); DBL_MAX both where step[a] == 0.  This is
 *      computeRayKeys of the first block with one difference: the half-cell offset is taken in double and not rounded
 *      through float -- castRay's own wording, restated from memory like the rest.
 *   5. Each iteration takes a = tMax0 < tMax1 ? (tMax0 < tMax2 ? 0 : 2) : (tMax1 < tMax2 ? 1 : 2) (a tie falls to the
 *      later axis).  key[a] == 0 with step[a] < 0, or key[a] == 65535 with step[a] > 0: OUT_OF_BOUNDS, end = the
 *      current cell (nothing wraps here, unlike insertion).  Otherwise key[a] += step[a], tMax[a] += tDelta[a], steps
 *      += 1, end = the new cell.  Then, if max_range > 0: q = (float)centre(end) - o per axis in float, s =
 *      ((double)(q0 * q0) + (double)(q1 * q1)) + (double)(q2 * q2) with the squares in float; s > max_range *
 *      max_range (double): OUT_OF_RANGE (equality goes on).  Then the cell: an occupied leaf: HIT; a leaf that is not
 *      occupied: the walk goes on; no leaf: UNKNOWN unless ignore_unknown != 0.
 *   6. After 196608 iterations: STEP_LIMIT.  Every iteration moves one key one cell in a fixed direction or ends the
 *      walk, so no walk gets there; the status exists so that the loop is finite without that argument.
 *   max_range NaN: RGBDFE_ERR_INVALID_ARG; max_range <= 0: no range limit.
 *   Hit record (rgbdfe_octomap_ray_hit, 36 bytes, rgbdfe_sizeof_octomap_ray_hit): status, steps (the cells moved), the
 *   end cell's key and float centre, and -- zero unless the status is HIT -- the leaf's log-odds and colour.
 *   View cloud: a column-major Matrix4f camera -> world (R and t as the first block reads them; R is taken as given),
 *   fx, fy, cx, cy (doubles, converted to float once; any value: a pixel whose direction comes out unusable is
 *   BAD_DIRECTION), rows x cols.  Pixel (row v, column u): o = t; x = ((float)u - (float)cx) / (float)fx, y = ((float)v -
 *   (float)cy) / (float)fy; d[a] = (R[a][0] * x + R[a][1] * y) + R[a][2] in float; then the ray cast above.  Output row
 *   v * cols + u, 4 floats as a node cloud's: for a HIT, with q = (float)centre(end) - o per axis in float, p[c] =
 *   (R[0][c] * q0 + R[1][c] * q1) + R[2][c] * q2 (the camera frame again) and the word r << 16 | g << 8 | b as float
 *   bits; otherwise x = y = z = the quiet NaN 0x7fc00000 and the word 0.  status (may be NULL): the ray's status, one
 *   byte per pixel.  The cloud is organised (rows x cols) and is an ordinary input of rgbdfe_display_geometry, the voxel
 *   filter, ICP and rgbdfe_upload_node_cloud.
 *   Work bound: a key that is not in the table costs a probe run to the next free slot -- 1/2 (1 + 1 / (1 - load)^2)
 *   probes expected: 2.5 at load 0.5, 8.5 at 0.75, most of the table when it is nearly full, once per step of every ray.
 *   Every call of this block with work to do therefore returns RGBDFE_ERR_CAPACITY, nothing run ("reserve" in the
 *   message), when 4 * leaves > 3 * capacity_cells; rgbdfe_octomap_reserve first (the wrappers reserve to a load of at
 *   most 0.5 and repeat the call).
 * rgbdfe_octomap_search: n points (3 floats each) from host memory; found[i] and leaves[i] as above.
 * rgbdfe_octomap_cast_rays: n origins and n directions (3 floats each) from host memory, one ignore_unknown / max_range
 *   / occupied_log_odds for all; hits[i] as above.
 * rgbdfe_octomap_view_cloud: the view to host memory (out: rows * cols * 4 floats; status: rows * cols bytes or NULL).
 *   rgbdfe_octomap_view_cloud_device: the same into device memory of the map's device (`stream` NULL: the context's
 *   stream; the call returns when the rows are in place); nothing is read back.
 * Arguments: n < 0, rows < 0, cols < 0, or a NULL array with work to do: RGBDFE_ERR_INVALID_ARG.  n or rows * cols >=
 *   2^31: RGBDFE_ERR_CAPACITY.  n == 0 or rows * cols == 0 succeeds and launches nothing (before the work bound is
 *   looked at).  One kernel launch per call: rgbdfe_octomap_stats has it as out[4] (0 after an empty call).
 * None of these calls changes a leaf; a query between two inserts does not alter what the later insert produces. */
#define RGBDFE_OCTOMAP_RAY_HIT 1
#define RGBDFE_OCTOMAP_RAY_UNKNOWN 2
#define RGBDFE_OCTOMAP_RAY_OUT_OF_RANGE 3
#define RGBDFE_OCTOMAP_RAY_OUT_OF_BOUNDS 4
#define RGBDFE_OCTOMAP_RAY_BAD_ORIGIN 5
#define RGBDFE_OCTOMAP_RAY_BAD_DIRECTION 6
#define RGBDFE_OCTOMAP_RAY_STEP_LIMIT 7
typedef struct rgbdfe_octomap_ray_hit {
  int32_t status;    /* RGBDFE_OCTOMAP_RAY_* */
  uint32_t steps;
  uint16_t key[3];
  uint16_t zero0;
  float centre[3];
  float log_odds;
  uint8_t rgb[3];
  uint8_t zero1;
} rgbdfe_octomap_ray_hit;
int rgbdfe_sizeof_octomap_ray_hit(void);
int rgbdfe_octomap_occupied_log_odds(rgbdfe_octomap* map, float* out);
int rgbdfe_octomap_search(rgbdfe_octomap* map, const float* points, int64_t n, int32_t* found,
                          rgbdfe_octomap_leaf* leaves);
int rgbdfe_octomap_cast_rays(rgbdfe_octomap* map, const float* origins, const float* directions, int64_t n,
                             int32_t ignore_unknown, double max_range, float occupied_log_odds,
                             rgbdfe_octomap_ray_hit* hits);
int rgbdfe_octomap_view_cloud(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy,
                              int32_t rows, int32_t cols, int32_t ignore_unknown, double max_range,
                              float occupied_log_odds, float* out, uint8_t* status);
int rgbdfe_octomap_view_cloud_device(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx,
                                     double cy, int32_t rows, int32_t cols, int32_t ignore_unknown, double max_range,
                                     float occupied_log_odds, void* d_out, void* d_status, void* stream);

/* ---- candidate selection for loop closure ----------------------------------
 * rgbdfe_potential_edge_targets is GraphManager::getPotentialEdgeTargetsWithDijkstra (graph_manager.cpp:204-324): the
 * ids of the earlier nodes a new node is to be compared with -- `sequential_targets` direct predecessors, then
 * `geodesic_targets` drawn (weighted by their distance in time, :266) from the graph neighbourhood of the predecessor
 * within `geodesic_depth` edges (g2o::HyperDijkstra with UniformCostFunction, :230-233), then `sampled_targets` drawn
 * uniformly from the remaining matchable keyframes (:297-317).  Order as in the reference's QList: sampled ids first
 * (latest draw first), sequential ones after, the predecessor last when include_predecessor != 0.  The list feeds
 * rgbdfe_match_node_pairs.  Host code, no device work.
 * The pose-graph object holds what the reference reads from graph_, camera_vertices, keyframe_ids_ and the optimizer's
 * edges: rgbdfe_pose_graph_add_node per Node added to the graph (id_, vertex_id_, matchable_, and whether it became a
 * keyframe, graph_manager.cpp:655), rgbdfe_pose_graph_add_edge per edge added to the optimizer (:811).
 * rand_fn(rand_state) replaces rand() (pass a wrapper of rand() for the reference's stream); NULL selects a
 * counter-based generator seeded with `seed`, which makes the selection reproducible.
 * Returns RGBDFE_ERR_CAPACITY (with *n_out = the needed size) when ids_out is too small. */
typedef struct rgbdfe_pose_graph rgbdfe_pose_graph;
typedef int (*rgbdfe_rand_fn)(void* state);
rgbdfe_pose_graph* rgbdfe_pose_graph_create(void);
void rgbdfe_pose_graph_destroy(rgbdfe_pose_graph* g);
int rgbdfe_pose_graph_add_node(rgbdfe_pose_graph* g, int32_t node_id, int32_t vertex_id, int32_t matchable,
                               int32_t keyframe);
int rgbdfe_pose_graph_add_edge(rgbdfe_pose_graph* g, int32_t node_id1, int32_t node_id2);
int rgbdfe_pose_graph_set_matchable(rgbdfe_pose_graph* g, int32_t node_id, int32_t matchable);
int rgbdfe_potential_edge_targets(const rgbdfe_pose_graph* g, int32_t sequential_targets, int32_t geodesic_targets,
                                  int32_t sampled_targets, int32_t geodesic_depth, int32_t predecessor_id,
                                  int32_t include_predecessor, rgbdfe_rand_fn rand_fn, void* rand_state, uint32_t seed,
                                  int32_t* ids_out, int32_t capacity, int32_t* n_out);

/* ---- pose-graph optimisation (GraphManager::optimizeGraphImpl, graph_manager.cpp:938-1066) ----------
 * The stage between the edges of rgbdfe_match_node_pairs and the `transforms` of rgbdfe_assemble_map /
 * rgbdfe_octomap_insert_nodes: Levenberg-Marquardt over g2o::EdgeSE3 with a Huber kernel, solved by block-Jacobi
 * preconditioned conjugate gradients (backend_solver "pcg"), on the device.  g2o is not part of the reference tree: the
 * contract is this library's restatement (restated, not pinned), tests/pose_graph_oracle.py states it
 * literally and the device gives its bytes.  Everything is double; the only operations are + - * / sqrt and comparisons.
 *
 *   Vertices: the nodes of the graph object in ascending node id, each an SE(3) estimate (identity until set) and a
 *     `fixed` flag (rgbdfe_pose_graph_set_fixed, or a pose_relative_to strategy kept by the graph: the block
 *     "fixation strategies, pruning and the evaluation rounds" below; fixationOfVertices :911-937).
 *     Free vertices are numbered in that order.  No fixed vertex at all is legal.
 *   Edges: those added with rgbdfe_pose_graph_add_edge_se3, in insertion order: measurement Z and a 6x6 information
 *     matrix O (row-major; any symmetric matrix).  Edges of rgbdfe_pose_graph_add_edge carry no measurement: ignored.
 *   Sums of three products are (a0 b0 + a1 b1) + a2 b2; longer ones run left to right.
 *   Error  e = toVectorMQT(Z^-1 Xi^-1 Xj): A = Xi^-1 Xj (Ra = Ri' Rj, ta = Ri'(tj - ti)), D = Z^-1 A (RD = Rz' Ra,
 *     tD = Rz'(ta - tz)); e = (tD, x, y, z of the quaternion of RD).  Matrix -> quaternion: trace > 0: s = sqrt(trace + 1),
 *     w = s / 2, (x, y, z) = (R21 - R12, R02 - R20, R10 - R01) * (0.5 / s); otherwise i = the largest diagonal entry (i = 0;
 *     R11 > R00: 1; R22 > Rii: 2), j, k cyclic, s = sqrt(Rii - Rjj - Rkk + 1), q_i = s / 2, w = (Rkj - Rjk) * (0.5 / s),
 *     q_j = (Rji + Rij) * (0.5 / s), q_k = (Rki + Rik) * (0.5 / s); then divided by its norm, all four signs flipped when w < 0.
 *   Update  X <- X * fromVectorMQT(d): translation d[0..2]; rotation from v = d[3..5]: w = 1 - |v|^2, w < 0: identity,
 *     else the matrix of the quaternion (v, sqrt(w)).  The rotation block is never re-orthogonalised (g2o does so every
 *     1000 updates); the error's quaternion is normalised instead.
 *   Jacobians at a zero update, with Q = w I + [u]x of the error quaternion (u, w):
 *     de/dXj = [RD 0; 0 Q],  de/dXi = [-Rz'  2 Rz'[ta]x; 0  -Q Ra'].
 *   Huber, delta 1: chi2 = e'Oe; chi2 <= 1: rho = chi2, w = 1; else rho = 2 sqrt(chi2) - 1, w = 1 / sqrt(chi2).  An edge
 *     contributes w J'OJ and -w J'Oe (OJ first, then J'(OJ), then times w); the graph's chi2 is the sum of rho.
 *   H and b: a vertex's diagonal block and part of b add its edges' contributions in insertion order; the off-diagonal
 *     blocks are the distinct pairs of free vertices in the order the edges first join them, stored with row < column (an
 *     edge whose first vertex has the larger free index contributes transposed), adding their edges in insertion order.
 *   Sums over edges (chi2) and vertices (dot products) go through one tree: leaves of 64 consecutive values (zero
 *     padded) halved 32, 16 .. 1; leaf k is added into accumulator k % 64 in ascending k; the 64 accumulators are halved
 *     the same way.  A dot product's value per vertex is its six products left to right.
 *   PCG on (H + lambda I) x = b: M = the diagonal blocks of H + lambda I, applied through their Cholesky factors;
 *     x = 0, r = b, z = M^-1 r, p = z; while not r'z <= 1e-6 (absolute) and fewer than 6 * (free vertices) iterations:
 *     q = A p (per row: the diagonal block's terms, then the vertex's off-diagonal blocks in block order),
 *     alpha = r'z / p'q, x += alpha p, r -= alpha q, z = M^-1 r, beta = r'z_new / r'z, p = z + beta p.
 *   Levenberg-Marquardt as g2o's OptimizationAlgorithmLevenberg: per rgbdfe_pose_graph_optimize call lambda = 1e-5 *
 *     max |diag H| of the first linearisation, ni = 2.  An iteration linearises, then tries up to 10 times: solve, apply to
 *     a copy of the estimates, gain = (chi2 - chi2_trial) / (dx'(lambda dx + b) + 1e-3); gain > 0 and chi2_trial finite:
 *     keep, lambda *= clamp(1 - (2 gain - 1)^3, 1/3, 2/3), ni = 2; otherwise drop the copy, lambda *= ni, ni *= 2.  Trials
 *     go on while gain < 0.  After 10 trials, or at gain == 0 (g2o's released code: neither accepted nor retried), the call
 *     ends; that iteration counts as done, as in SparseOptimizer::optimize.
 *
 * rgbdfe_pose_graph_set_estimate / get_estimate: 16 doubles, a column-major 4x4 (rotation and translation are kept).
 * rgbdfe_pose_graph_add_edge_se3: also registers the topology as rgbdfe_pose_graph_add_edge does; set_estimate != 0:
 *   X2 = X1 * Z (addEdgeToG2O :858,864).  node_id1 == node_id2: RGBDFE_ERR_INVALID_ARG.
 * rgbdfe_pose_graph_chi2: the sum of rho at the current estimates (0 without a measured edge).
 * rgbdfe_pose_graph_linearize: one linearisation to host arrays: errors (6 per edge) and weights (w per edge) in
 *   insertion order; free_ids (node ids), h_diag (36 per free vertex, row-major), b (6 per free vertex); off_rows /
 *   off_cols (free indices) and h_off (36 per block); *chi2.  Any array may be NULL.  A capacity below the count:
 *   RGBDFE_ERR_CAPACITY with the three counts set.
 * rgbdfe_pose_graph_optimize: SparseOptimizer::optimize(iterations).  rgbdfe_pose_graph_optimize_graph: the loop of
 *   optimizeGraphImpl (:996-1014): break_criterion >= 1: optimize(ceil(c / 10)) until c iterations are done or a call
 *   does none; otherwise optimize(5) while chi2 / chi2_prev < 1 - c (first chi2_prev: DBL_MAX).  Every measured edge
 *   takes part.  A graph with no measured edge or no free vertex: 0 iterations, estimates untouched.
 *   report (may be NULL): iterations done and the final chi2; for the first RGBDFE_POSE_GRAPH_REPORT_ITERATIONS
 *   iterations (of all calls of the loop) the trials, each trial's PCG iterations, chi2 before and after, lambda after;
 *   kernel launches, read-backs, seconds spent building and uploading the plan, seconds in all.
 * rgbdfe_pose_graph_transforms: the estimates of node_ids as column-major Matrix4f rows (float), what rgbdfe_assemble_map
 *   and rgbdfe_octomap_insert_nodes take; composing with cam2rgb stays with the caller.
 * Errors: an unknown node id: RGBDFE_ERR_UNKNOWN_NODE before any state changes; a non-finite input: RGBDFE_ERR_INVALID_ARG.
 * The device buffers belong to the graph object and go with rgbdfe_pose_graph_destroy. */
#define RGBDFE_POSE_GRAPH_REPORT_ITERATIONS 64
#define RGBDFE_POSE_GRAPH_MAX_TRIALS 10
typedef struct rgbdfe_pose_graph_iteration {
  int32_t trials;
  int32_t pcg_iterations[RGBDFE_POSE_GRAPH_MAX_TRIALS];
  int32_t pad;
  double chi2_before, chi2_after, lambda;
} rgbdfe_pose_graph_iteration;
typedef struct rgbdfe_pose_graph_report {
  int32_t iterations;   /* Levenberg-Marquardt iterations done */
  int32_t recorded;     /* entries of it[] */
  double chi2;
  int64_t launches, readbacks;
  double upload_seconds, total_seconds;
  rgbdfe_pose_graph_iteration it[RGBDFE_POSE_GRAPH_REPORT_ITERATIONS];
} rgbdfe_pose_graph_report;
int rgbdfe_pose_graph_set_estimate(rgbdfe_pose_graph* g, int32_t node_id, const double* transform);
int rgbdfe_pose_graph_get_estimate(const rgbdfe_pose_graph* g, int32_t node_id, double* transform);
int rgbdfe_pose_graph_set_fixed(rgbdfe_pose_graph* g, int32_t node_id, int32_t fixed);
int rgbdfe_pose_graph_add_edge_se3(rgbdfe_pose_graph* g, int32_t node_id1, int32_t node_id2, const double* transform,
                                   const double* information, int32_t set_estimate);
int rgbdfe_pose_graph_chi2(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2);
int rgbdfe_pose_graph_linearize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* errors, double* weights, int32_t edge_capacity,
                                int32_t* n_edges, int32_t* free_ids, double* h_diag, double* b, int32_t vertex_capacity,
                                int32_t* n_free, int32_t* off_rows, int32_t* off_cols, double* h_off, int32_t block_capacity,
                                int32_t* n_blocks, double* chi2);
int rgbdfe_pose_graph_optimize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, int32_t iterations, rgbdfe_pose_graph_report* report);
int rgbdfe_pose_graph_optimize_graph(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double break_criterion,
                                     rgbdfe_pose_graph_report* report);
int rgbdfe_pose_graph_transforms(const rgbdfe_pose_graph* g, int32_t n, const int32_t* node_ids, float* out);

/* ---- fixation strategies, pruning and the evaluation rounds (OpenNIListener::evaluation, openni_listener.cpp:431-518) ----
 * What the reference runs at the end of every benchmark sequence, on the graph object of the block above and under its
 * contract (restated, not pinned; tests/pose_graph_eval_oracle.py states it literally, the device gives
 * its bytes).  A graph that calls none of these behaves as before.
 *
 * Strategies (pose_relative_to).  rgbdfe_pose_graph_set_strategy keeps one of RGBDFE_POSE_RELATIVE_TO_* in the graph.
 *   NONE (the default): the flags of rgbdfe_pose_graph_set_fixed are used as they stand, nothing below applies.  Otherwise:
 *   rgbdfe_pose_graph_add_node sets earliest_loop_closure_node to the new node's id (graph_manager.cpp:444).
 *   rgbdfe_pose_graph_add_edge_se3: INAFFECTED clears the flags of both vertices (:889-892); LARGEST_LOOP sets
 *     earliest = min(earliest, id1, id2) (:893-896).
 *   rgbdfe_pose_graph_optimize_graph starts with fixationOfVertices (:911-937): FIRST: all flags cleared, the node of
 *     lowest id fixed (the reference indexes graph_[0], its first node); PREVIOUS: with more than two nodes, all flags
 *     cleared and the node of second-highest id fixed (graph_[size - 2]), otherwise the flags stay; LARGEST_LOOP:
 *     fixed = (id < earliest) for every node; INAFFECTED: nothing.  It ends (:1031-1036) with every flag set under
 *     INAFFECTED and every flag cleared under the others, on every return path.
 *   The reference's quirk is kept: the Dijkstra vertex set of its `inaffected` branch (:969-977) is overridden by
 *     initializeOptimization(cam_cam_edges_) at :991, so every active measured edge takes part under every strategy and an
 *     edge between two fixed vertices counts in chi2.
 *   rgbdfe_pose_graph_optimize, _linearize and _chi2 apply no strategy.
 *
 * rgbdfe_pose_graph_edge_errors: per measured edge in insertion order, at the current estimates: chi2 = e'Oe before Huber
 *   (g2o's Edge::chi2()), err_sq = e.e summed left to right (printEdgeErrors :1321-1334), the active flag.  Any array may be
 *   NULL.  A pruned edge reports 0, 0, 0.  capacity below the count: RGBDFE_ERR_CAPACITY with *n_edges set.
 * rgbdfe_pose_graph_prune_edges: pruneEdgesWithErrorAbove (:1106-1246) as it behaves, on the device, a lane per edge.
 *   Every ACTIVE edge with chi2 > (double)thresh (a NaN chi2 compares false: kept) is counted, its measurement becomes the
 *   identity, and:  |id1 - id2| != 1 and both vertices have degree > 1: the edge becomes inactive (RGBDFE_PRUNE_REMOVED; its
 *   information stays);  |id1 - id2| != 1 otherwise: information = 1e-100 I (RGBDFE_PRUNE_DISCOUNTED);  |id1 - id2| == 1:
 *   information = I, the zero-motion assumption (RGBDFE_PRUNE_ZERO_MOTION).  Every other edge: RGBDFE_PRUNE_KEPT.
 *   Degree = the measured edges ever added that touch the node, inactive ones included (the reference erases an edge from
 *   cam_cam_edges_ only, never from the optimiser: v->edges().size() never shrinks).  Hence: verdicts do not depend on the
 *   order of the edges within a call; and both edges of a degree-2 vertex can be removed in one call, which disconnects
 *   the vertex in spite of the reference's comment.  verdicts (may be NULL): a byte per edge; *n_pruned: the count.
 *   capacity below the edge count: RGBDFE_ERR_CAPACITY with *n_pruned = the edge count, nothing changed.
 *   An inactive edge keeps its slot and contributes nothing from then on: rho 0 in its place of the chi2 tree (whose shape
 *   still depends on the number of edges ever added alone), no entry in the lists of H and b, no part in later prune
 *   calls; rgbdfe_pose_graph_linearize reports error 0 and weight 0 for it.  An optimisation with no active edge does
 *   0 iterations.
 * rgbdfe_pose_graph_get_edge: an edge by insertion index: ids, measurement (16 doubles, column-major), information (36,
 *   row-major), active; any output may be NULL.  index out of range: RGBDFE_ERR_INVALID_ARG.
 * rgbdfe_pose_graph_get_fixed: a node's flag.
 * rgbdfe_pose_graph_sanity_check: sanityCheck (:1347-1360), host code: thresh *= thresh in FLOAT; an active edge whose
 *   measurement has (tx tx + ty ty) + tz tz > (double)thresh takes information 0.000001 I.  Returns the number of edges
 *   changed (a negative status on a NULL graph or a NaN threshold).
 * rgbdfe_pose_graph_evaluate: evaluation()'s five rounds.  Round 0: optimize_graph(optimizer_iterations) under the current
 *   strategy; the strategy then becomes FIRST and stays; round 1: optimize_graph(optimizer_iterations); rounds 2, 3, 4:
 *   prune_edges(5.0f / 1.0f / 0.25f) > 0 ? optimize_graph(optimizer_iterations) : optimize_graph(1.0).  The rounds are
 *   issued as those single calls (each uploads its own plan), so the bytes are theirs.  out (may be NULL): per round chi2,
 *   iterations, edges pruned, launches, read-backs, upload seconds (prune and optimisation together), seconds in all.
 *   estimates (may be NULL): after every round the estimates of all nodes in ascending id, 16 column-major doubles each:
 *   5 * n * 16 values, what saveTrajectory(.. iteration_k) logs.  capacity_nodes below n: RGBDFE_ERR_CAPACITY, nothing done.
 * rgbdfe_pose_graph_write_trajectory: the estimate file of saveTrajectory (graph_mgr_io.cpp:615-677, logTransform
 *   misc.cpp:90-93), host code.  Per listed node world2base = ((init_base_pose * base2points) * X) * base2points^-1 in
 *   double (16 column-major doubles each, NULL = identity; one base2points for all nodes; products by the sum rule above;
 *   the rigid inverse is R', -R't), written as "%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n" = stamp, tx ty tz, then x y z w
 *   of the matrix -> quaternion conversion above (QTextStream's fixed notation has precision 6).  That conversion returns
 *   w >= 0 where tf's getRotation does not flip: the same rotation, which ATE tools do not see.  With frame_id != NULL
 *   the first line is "# TF Coordinate Frame ID: <frame_id>(data: <child_frame_id>)".  The ground-truth file is the
 *   caller's.  An unknown node: RGBDFE_ERR_UNKNOWN_NODE, a path that cannot be opened: RGBDFE_ERR_INVALID_ARG (as
 *   rgbdfe_octomap_write), nothing written.
 * An unknown strategy, a NULL graph: RGBDFE_ERR_INVALID_ARG; in every error case the graph is unchanged. */
#define RGBDFE_POSE_RELATIVE_TO_NONE 0
#define RGBDFE_POSE_RELATIVE_TO_FIRST 1
#define RGBDFE_POSE_RELATIVE_TO_PREVIOUS 2
#define RGBDFE_POSE_RELATIVE_TO_LARGEST_LOOP 3
#define RGBDFE_POSE_RELATIVE_TO_INAFFECTED 4
#define RGBDFE_PRUNE_KEPT 0
#define RGBDFE_PRUNE_REMOVED 1
#define RGBDFE_PRUNE_DISCOUNTED 2
#define RGBDFE_PRUNE_ZERO_MOTION 3
#define RGBDFE_POSE_GRAPH_EVALUATION_ROUNDS 5
typedef struct rgbdfe_pose_graph_round {
  double chi2;
  int32_t iterations;   /* Levenberg-Marquardt iterations of the round's optimize_graph */
  int32_t pruned;       /* edges counted by the round's prune call (rounds 2 .. 4) */
  int64_t launches, readbacks;
  double upload_seconds, seconds;
} rgbdfe_pose_graph_round;
typedef struct rgbdfe_pose_graph_evaluation {
  rgbdfe_pose_graph_round round[RGBDFE_POSE_GRAPH_EVALUATION_ROUNDS];
} rgbdfe_pose_graph_evaluation;
int rgbdfe_pose_graph_set_strategy(rgbdfe_pose_graph* g, int32_t strategy);
int rgbdfe_pose_graph_get_fixed(const rgbdfe_pose_graph* g, int32_t node_id, int32_t* fixed);
int rgbdfe_pose_graph_get_edge(const rgbdfe_pose_graph* g, int32_t index, int32_t* node_id1, int32_t* node_id2, double* transform,
                               double* information, int32_t* active);
int rgbdfe_pose_graph_sanity_check(rgbdfe_pose_graph* g, float thresh);
int rgbdfe_pose_graph_edge_errors(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2, double* err_sq, int32_t* active,
                                  int32_t capacity, int32_t* n_edges);
int rgbdfe_pose_graph_prune_edges(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, float thresh, uint8_t* verdicts, int32_t capacity,
                                  int32_t* n_pruned);
int rgbdfe_pose_graph_evaluate(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double optimizer_iterations,
                               rgbdfe_pose_graph_evaluation* out, double* estimates, int32_t capacity_nodes);
int rgbdfe_pose_graph_write_trajectory(const rgbdfe_pose_graph* g, const char* path, int32_t n, const int32_t* node_ids,
                                       const double* timestamps, const double* base2points, const double* init_base_pose,
                                       const char* frame_id, const char* child_frame_id);

/* ---- ICP fallback (Node::matchNodePair node.cpp:1349-1378, filterCloud and icpAlignment icp.cpp:20-89) ----------
 * What the reference does when RANSAC finds no transformation between two adjacent frames: both dense clouds are
 * subsampled and aligned by icp_method "icp", PCL's point-to-point IterativeClosestPoint.  icp_nl and GICP are not
 * served.  PCL is not part of the reference tree: the contract is this library's restatement (restated, not pinned;
 * DESIGN.md 4.22), tests/icp_oracle.py states it literally and the device gives its bytes.  The nearest neighbour is an
 * exact brute-force search (no kd-tree).  Clouds are rows of 4 floats (x, y, z, rgb bits).  Every float and double
 * operation is rounded once (-ffp-contract=off); sums of three products are (a0 b0 + a1 b1) + a2 b2.
 *
 *   Subsampling = filterCloud, literally.  V = the indices of the rows whose z is not NaN, ascending.
 *     step = (float)|V| / (float)desired_size, and step < 1 becomes 1.  The samples are the rows V[(unsigned)i] for
 *     `float i = 0; i < (float)|V|; i += step`.  The float recurrence is part of the contract: |V| = 3072 and
 *     desired_size = 100 give 101 samples, (2999, 7) gives 8.  desired_size <= 0: RGBDFE_ERR_INVALID_ARG.  A cloud of more
 *     than 2^24 rows: RGBDFE_ERR_CAPACITY (beyond it the recurrence need not advance).
 *     Named deviation: within the alignment a sampled row with a non-finite x or y takes part in nothing, neither as source
 *     nor as target (createXYZRGBPointCloud never makes such a row).  rgbdfe_filter_cloud returns the rows as they are.
 *   Alignment = icpAlignment.  Source S and target T are the two sampled clouds, the guess G a column-major Matrix4f of
 *     which the upper three rows are used.  Working copy P = G S: ((R0 x + R1 y) + R2 z) + t per row, as rgbdfe_assemble_map
 *     transforms.  F = G, mse_0 = DBL_MAX.  Iteration k = 1, 2, ...:
 *     1. Correspondences.  For every source row i the running minimum starts at +inf without an index and takes target row
 *        j, in ascending j, when d2 = (dx dx + dy dy) + dz dz (float, dx = P.x - T.x) is < the minimum: equal distances
 *        answer with the lowest index, a row whose every d2 is +inf or NaN has no neighbour (j = -1).  The pair is kept iff
 *        j >= 0 and !((double)d2 > maxdist * maxdist) (the product in double).  c = the number kept.  c < 3: the job stops,
 *        state RGBDFE_ICP_NO_CORRESPONDENCES, converged = 0 (mse is then the sum of d2 / c, 0 for c = 0).
 *     2. Seventeen sums in double over the source rows in ascending i, a row without a kept pair contributing zero: c, d2,
 *        P (3), T_j (3), T_j P' (9; the products of the two floats in double).  Each goes through the tree of the pose-graph
 *        block: leaves of 64 consecutive values (zero padded) halved 32, 16 .. 1; leaf k is added into accumulator k % 64 in
 *        ascending k; the 64 accumulators are halved the same way.  No floating-point atomics.
 *     3. Increment.  H = (sum T P' - (sum T)(sum P)' / c) / c in double, each entry rounded once to float; m_P = sum P / c
 *        and m_T = sum T / c likewise.  U, V = the JacobiSVD<Matrix3f> restatement of the RANSAC stage on H;
 *        R = U diag(1, 1, s) V' with s = -1 iff det(U) det(V) < 0 (Eigen's umeyama rule for rank >= 2; its det(Sigma) test
 *        for lower rank is not mirrored: named deviation); t = m_T - R m_P.  P <- R P + t per row as above;
 *        F <- [R t] F: its rotation R R_F, its translation (R t_F) + t, its last row (0, 0, 0, 1).
 *     4. Stop rules, in this order: k >= max_iterations -> RGBDFE_ICP_ITERATIONS;
 *        0.5 ((R00 + R11) + R22 - 1) >= 1 - transformation_epsilon and (tx tx + ty ty) + tz tz <= transformation_epsilon,
 *        both in double -> RGBDFE_ICP_TRANSFORM; with mse_k = sum d2 / c: |mse_k - mse_(k-1)| < 1e-12 -> RGBDFE_ICP_ABS_MSE;
 *        |mse_k - mse_(k-1)| / mse_(k-1) < euclidean_fitness_epsilon -> RGBDFE_ICP_REL_MSE; otherwise the next iteration.
 *        All four count as converged.
 *     The result is F if converged, else G's sixteen floats as given (icp.cpp:81-87).
 *   A reproduced quirk: with the reference's setEuclideanFitnessEpsilon(1) the relative test passes at k = 2 for almost any
 *     input, so the reference's fallback is a two-step ICP.  rgbdfe_icp_default_params reproduces it; a caller who passes
 *     1e-6 gets the full loop.
 *
 * rgbdfe_icp_default_params: the values icpAlignment sets and gicp_max_cloud_size: 0.05, 50, 1e-8, 1.0, 10000.
 *   max_iterations outside 1 .. 1000, a NaN parameter or a negative distance: RGBDFE_ERR_INVALID_ARG.
 * rgbdfe_icp_align_nodes: n_jobs alignments over resident node clouds (rgbdfe_upload_node_cloud, the sensor batch path) as
 *   one batch, jobs of different sizes mixed; an id may repeat.  guesses: n_jobs x 16 floats, NULL = identity.
 *   transforms_out: n_jobs x 16 floats, column-major.  reports_out may be NULL.  An id without a cloud:
 *   RGBDFE_ERR_UNKNOWN_NODE before any device work.  n_jobs == 0: RGBDFE_OK.  More than 65535 jobs: RGBDFE_ERR_CAPACITY.
 *   In the reference's use the source is the OLDER node's cloud and the target the newer one's (node.cpp:1362-1364).
 * rgbdfe_icp_align_clouds: the same for two host clouds.  nn_index_out / nn_d2_out (each may be NULL): j(i) and d2 of the
 *   last iteration for every sampled source row, dropped pairs included; debug_capacity rows, fewer than the sampled source
 *   count is RGBDFE_ERR_CAPACITY.
 * rgbdfe_filter_cloud: filterCloud alone: the sampled rows' indices and the rows (each may be NULL); capacity < *n_out:
 *   RGBDFE_ERR_CAPACITY with *n_out = the needed size.
 * report: launches and readbacks are those of the whole call (the same in every job's report).  The loop: two launches
 *   per iteration for the whole batch, enqueued in chunks of 2, 4, 8, 16, 16 ... iterations with one read of the jobs'
 *   records per chunk; an iteration enqueued after a job has stopped returns at once for that job.
 * Device memory: a call keeps, in buffers that grow to the largest call and stay with the context, 8 bytes per 256 rows of
 *   every distinct cloud it names (the rows too for host clouds) and about 50 bytes per sample and job.
 * Multi-device handles use their first device. */
#define RGBDFE_ICP_RUNNING 0   /* never reported */
#define RGBDFE_ICP_NO_CORRESPONDENCES 1
#define RGBDFE_ICP_ITERATIONS 2
#define RGBDFE_ICP_TRANSFORM 3
#define RGBDFE_ICP_ABS_MSE 4
#define RGBDFE_ICP_REL_MSE 5
typedef struct rgbdfe_icp_params {
  double max_correspondence_distance;
  double transformation_epsilon;
  double euclidean_fitness_epsilon;
  int32_t max_iterations;
  int32_t desired_size;
} rgbdfe_icp_params;
typedef struct rgbdfe_icp_report {
  int32_t converged, state, iterations;
  int32_t correspondences;      /* c of the last iteration */
  double mse;                   /* of the last iteration */
  int32_t n_source, n_target;   /* the sample counts */
  int64_t launches, readbacks;
} rgbdfe_icp_report;
void rgbdfe_icp_default_params(rgbdfe_icp_params* p);
int rgbdfe_icp_align_nodes(rgbdfe_ctx* ctx, int32_t n_jobs, const int32_t* source_ids, const int32_t* target_ids,
                           const float* guesses, const rgbdfe_icp_params* params, float* transforms_out,
                           rgbdfe_icp_report* reports_out);
int rgbdfe_icp_align_clouds(rgbdfe_ctx* ctx, const float* source, int64_t n_source, const float* target, int64_t n_target,
                            const float* guess, const rgbdfe_icp_params* params, float* transform_out,
                            rgbdfe_icp_report* report_out, int32_t* nn_index_out, float* nn_d2_out, int64_t debug_capacity);
int rgbdfe_filter_cloud(rgbdfe_ctx* ctx, const float* cloud, int64_t n, int32_t desired_size, int32_t* indices_out,
                        float* rows_out, int64_t capacity, int64_t* n_out);

/* ---- display geometry: resident node clouds as GL points, triangles and triangle strips -------------------
 * rgbdfe_display_geometry is GLViewer::addPointCloud's choice (glviewer.cpp:693-711) among pointCloud2GLPoints
 *   (:955-987), pointCloud2GLTriangleList (:989-1042) and pointCloud2GLStrip (:776-906) for every listed node, with
 *   setGLColor in its plain form (:91-93; not HEMACLOUDS, not RGB_IS_4TH_DIM), on the device.  The contract is that
 *   code, statement by statement; its quirks are reproduced (DESIGN.md 4.24 lists them).
 *   node_ids / transforms as rgbdfe_assemble_map takes them (ids may repeat, cloud sizes may be mixed); transforms may be
 *   NULL: the vertices stay in the node frame.
 *   A vertex is a row of 4 floats: x, y, z of a glVertex3f call and the rgb word, bit for bit, of the point the
 *   preceding setGLColor call was given (bytes 0, 1, 2 = b, g, r: a GL_BGRA colour as it stands).  A node's vertex
 *   stream is the sequence of glVertex3f calls of the reference function for its cloud.
 *   Validity (validXYZ, :44-47): a point is invalid iff max_depth < z or any of z, y, x is not finite, with max_depth =
 *   (float)maximum_depth.  The test is on z, not on the range; the finite x, y "at 1 m" beside a NaN z is invalid.
 *   Distances (squaredEuclideanDistance, :768-773): (dx*dx + dy*dy) + dz*dz in float, one rounding per operation.  Every
 *   test is `d / depth <= t` or `d / depth > t` with an IEEE float division, t = (float)squared_meshing_threshold, depth
 *   the squared distance of the named point from the origin.  A point in the origin gives depth 0: the inf and NaN
 *   ratios decide as the comparison operators decide them.
 *   Form of node k (node_types[k]; may be NULL): RGBDFE_DISPLAY_POINTS when its cloud has rows <= 1 (the state
 *   rgbdfe_reduce_node_cloud leaves) or squared_meshing_threshold < 0, else display_type.
 *   POINTS: x outer over [0, cols), y inner over [0, rows); every valid point, in that order.
 *   TRIANGLES: x outer over [0, cols - 1), y inner over [0, rows - 1); per cell with pi = (x, y), pj = (x + 1, y), pk =
 *   (x, y + 1), pl = (x + 1, y + 1) the triangles (pi, pl, pj) and then (pi, pk, pl) under the conditions of :1016-1036.
 *   visualization_skip_step is not read.
 *   TRIANGLE_STRIP: the state machine of :798-898 with step = visualization_skip_step: rows y = 0, step, ... < rows -
 *   step; columns x = 0; x < cols - step; x += step, with the extra x++ of :829 (afterwards x need not be a multiple of
 *   step).  Both start forms (upper point first; lower first, `flip`), the doubled test of :810-811; `*(ul - step)` is
 *   the point step columns to the left in the same row.  The second vertex of a running step has the lower (flip: the
 *   upper) point's x, y, z and the rgb word of the step's first vertex (:886).  A strip ends at every glEnd, the one at
 *   the end of a row included; strips of one or two vertices are strips.
 *   With transforms every vertex is ((R0 x + R1 y) + R2 z) + t per row of its point, the arithmetic of
 *   rgbdfe_assemble_map in the same order: a vertex equals the assembled map's row of that point bit for bit.  All
 *   validity and threshold tests use the untransformed point (the viewer applies cloud_matrices in GL).
 *   Output.  vertices: vertex_capacity rows; the nodes' streams in the order of node_ids.  *n_vertices = the rows;
 *   node_offsets (may be NULL; n_nodes + 1 entries) = the first vertex of every node, then *n_vertices.  strips:
 *   strip_capacity records of two int64 (first vertex as an index into the whole stream, vertex count), one per
 *   glBegin(GL_TRIANGLE_STRIP), in stream order.  *n_strips = the records; node_strip_offsets (may be NULL; n_nodes + 1
 *   entries) = the first record of every node, then *n_strips.  POINTS and TRIANGLES nodes own no records.
 *   Errors.  display_type not one of the three, visualization_skip_step < 1: RGBDFE_ERR_INVALID_ARG, nothing is
 *   written.  An id without a cloud: RGBDFE_ERR_UNKNOWN_NODE, before any device work.  vertex_capacity < *n_vertices or
 *   strip_capacity < *n_strips: RGBDFE_ERR_CAPACITY with both needed sizes, the offsets and node_types set (the
 *   buffers' contents are then untouched).  n_nodes == 0: RGBDFE_OK, both sizes 0.
 *   Sizes that always suffice for a cloud of rows x cols points: POINTS rows * cols vertices; TRIANGLES 6 * (rows - 1) *
 *   (cols - 1) vertices (two triangles per cell); TRIANGLE_STRIP with Y = ceil((rows - step) / step) visited rows and X
 *   = ceil((cols - step) / step) visited columns at most (none unless rows > step and cols > step): 2 * X * Y vertices
 *   (a column sends at most two; an all-valid flat row reaches 2 * X) and ceil(X / 2) * Y records (the column whose test
 *   ends a strip starts none).
 * rgbdfe_display_geometry_device: the same with d_vertices / d_strips device pointers of the context's device (the
 *   first device of a multi-device handle); no vertex crosses to the host.  The kernels run on `stream` (NULL: the
 *   context's own); the call returns when they have finished.  Sizes, offsets and node_types are host pointers.
 * rgbdfe_display_default_params: POINTS, 1, 0.0009, +inf (parameter_server.cpp:151, :139, :148, :38). */
#define RGBDFE_DISPLAY_POINTS 0
#define RGBDFE_DISPLAY_TRIANGLES 1
#define RGBDFE_DISPLAY_TRIANGLE_STRIP 2
typedef struct rgbdfe_display_params {
  int32_t display_type;             /* cloud_display_type (default "POINTS") */
  int32_t visualization_skip_step;  /* default 1; read by the strip form only, as in the reference */
  double squared_meshing_threshold; /* default 0.0009; < 0: every node is drawn as points (glviewer.cpp:697) */
  double maximum_depth;             /* default +inf */
} rgbdfe_display_params;
void rgbdfe_display_default_params(rgbdfe_display_params* p);
int rgbdfe_display_geometry(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                            const rgbdfe_display_params* params, float* vertices, int64_t vertex_capacity,
                            int64_t* n_vertices, int64_t* node_offsets, int64_t* strips, int64_t strip_capacity,
                            int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types);
int rgbdfe_display_geometry_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                                   const rgbdfe_display_params* params, void* d_vertices, int64_t vertex_capacity,
                                   int64_t* n_vertices, int64_t* node_offsets, void* d_strips, int64_t strip_capacity,
                                   int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types, void* stream);

/* ---- rendering: the display-geometry stream rasterised into images on the device -----------------------------
 * rgbdfe_render_nodes is what GL does with the vertex rows in GLViewer::paintGL / drawClouds / drawOneCloud
 *   (glviewer.cpp:291-425) under the state of initializeGL (:195-211): a software rasteriser, since an Instinct card
 *   has no graphics pipeline.  GL leaves rasterisation details to the implementation; this block fixes one admissible
 *   choice (restated, not pinned; DESIGN.md 4.28 names each choice).  tests/render_oracle.py restates it in Python.
 *   Input.  node_ids / transforms / display_params exactly as rgbdfe_display_geometry takes them.  The primitives are
 *   that call's vertex stream; node k is drawn in the form that call reports in node_types[k]; a vertex is the stream's
 *   row, bit for bit.  A primitive's id is the index in the whole stream of its first vertex: a point's id is its own
 *   vertex; list triangle j of a node whose stream starts at o has id o + 3 j and vertices (o + 3 j, + 1, + 2) (one or
 *   two rows left over at the end of a node draw nothing); triangle i of a strip record (s, count), 0 <= i < count - 2,
 *   has id s + i and vertices (s + i, s + i + 1, s + i + 2) for even i, (s + i + 1, s + i, s + i + 2) for odd i.
 *   Strips of fewer than three vertices draw nothing.  A stream of more than 2^32 - 2 vertices: RGBDFE_ERR_CAPACITY.
 *   Camera.  view (GL's modelview without the per-cloud matrix) and projection, 4 x 4 doubles, column-major as the
 *   Matrix4f of `transforms` (element (row, column) at [4 * column + row]).  Per vertex, in double, one rounding per
 *   operation, a sum of products as ((a0 b0 + a1 b1) + a2 b2) + a3 b3:
 *     world = the row's x, y, z (already ((R0 x + R1 y) + R2 z) + t in float), w = 1 (so a3 b3 is view's fourth column);
 *     eye = view . world;  clip = projection . eye;  ndc = clip.xyz / clip.w (three divisions);
 *     x_w = ((ndc.x + 1) * W) / 2,  y_w = ((ndc.y + 1) * H) / 2,  z_w = (ndc.z / 2) + 1/2.
 *   y_w points up: image row = H - 1 - window row.  No transcendental function runs on the device.
 *   Depth test.  GL_LESS with the primitives drawn in stream order: a pixel shows the fragment with the smallest
 *   float32 depth, among equal depths the one of the smallest primitive id.  The images do not depend on the order in
 *   which the device meets the primitives, nor on max_vertices_in_flight.
 *   Points (glPointSize(gl_point_size), not smoothed).  n = floor(gl_point_size + 1/2) clamped to [1, 64].  A point whose
 *   clip coordinates fail -w <= x, y, z <= w, or whose w is not positive and finite, is not drawn.  Otherwise it covers
 *   the n x n pixels from floor(x_w) - (n - 1) / 2 (odd n) or floor(x_w + 1/2) - n / 2 (even n) on, the same in y, cut
 *   at the viewport.  Every covered pixel takes (float)z_w and the vertex's colour word (bytes 0, 1, 2 of the row's
 *   fourth float = b, g, r; alpha 255).
 *   Triangles (GL_FILL, GL_SMOOTH, GL_CULL_FACE with counter-clockwise front faces, no blending, :355).
 *     Deviation from GL, stated: nothing is clipped against near / far or a guard band.  A triangle with a vertex whose w
 *     is not positive and finite, that fails -w <= z <= w, or whose |x_w| or |y_w| is not <= 16384 is not drawn at all
 *     (so every edge function stays below 2^53 and converts to double exactly).
 *     Snapping: X = floor(x_w * 256 + 1/2), Y likewise (1/256 pixel; ties go up), as 64-bit integers.
 *     area = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0).  Zero draws nothing.  Negative (seen from behind): not drawn when
 *     cull is 1; when cull is 0 vertices 1 and 2 change places and the triangle is drawn.
 *     Coverage: the sample of pixel (px, py) is (256 px + 128, 256 py + 128).  e_i for i = 0, 1, 2 is the edge function of
 *     the edge from vertex a = (i + 1) % 3 to b = (i + 2) % 3: e_i = (Xb - Xa)(sy - Ya) - (Yb - Ya)(sx - Xa).  The sample is
 *     covered iff every e_i > 0, or e_i = 0 on an edge that owns its samples: Yb - Ya < 0, or Yb - Ya = 0 and Xb - Xa < 0
 *     (the left and the top edges of the triangle in the image: a top-left rule).  A sample on an edge two triangles
 *     share belongs to exactly one of them.
 *     Depth = (float)(((e0 z0 + e1 z1) + e2 z2) / ((e0 + e1) + e2)) with the vertices' double z_w and the e_i converted to
 *     double: GL's screen-space interpolation.
 *     Colour per channel: q_i = e_i / w_i (w = clip.w), c = ((q0 c0 + q1 c1) + q2 c2) / ((q0 + q1) + q2), then
 *     floor(c + 1/2) clamped to [0, 255] (perspective-correct, GL_SMOOTH); alpha 255.
 *   Output.  H x W images, row 0 at the top.  rgba: 4 bytes per pixel, r, g, b, a; clear_rgba where nothing was drawn.
 *   depth: float32, 1.0 where nothing was drawn (what glReadPixels(GL_DEPTH_COMPONENT) gives).  ids (may be NULL): int64
 *   primitive id, -1 where nothing was drawn.  node_index (may be NULL): int32 position in node_ids of the primitive's
 *   node, -1 where nothing was drawn.
 *   max_vertices_in_flight: 0 = the library's default (2^23); above 0 the node list is processed in groups of consecutive
 *   nodes whose vertices together stay within it (at most 2^30); a single node with more: RGBDFE_ERR_CAPACITY.  The
 *   scratch is 20 bytes per vertex in flight and 8 per pixel.
 *   Errors.  NULL ctx / params / rgba / depth, width or height outside [1, 4096], a view / projection entry or
 *   gl_point_size that is not finite, gl_point_size <= 0, cull not 0 or 1, max_vertices_in_flight < 0, and whatever
 *   rgbdfe_display_geometry refuses: RGBDFE_ERR_INVALID_ARG, nothing is written.  An id without a cloud:
 *   RGBDFE_ERR_UNKNOWN_NODE before any device work, nothing is written.  n_nodes == 0: RGBDFE_OK, cleared images.
 * rgbdfe_render_nodes_device: the same with device pointers of the context's device for the four images; the kernels
 *   run on `stream` (NULL: the context's own); the call returns when they have finished.
 * rgbdfe_render_default_params: 640 x 480, the view of rgbdfe_render_viewer_view's defaults, the projection of
 *   rgbdfe_render_perspective's defaults at aspect 640 / 480, gl_point_size 1 (parameter_server.cpp:143), cull 1,
 *   clear_rgba 3, 3, 3, 3 (the viewer's 0.01 grey, :128), max_vertices_in_flight 0.
 * Host helpers, plain double arithmetic, sums of products left to right (csrc/render_camera.h):
 *   rgbdfe_render_perspective(fovy, aspect, z_near, z_far, out): gluPerspective; fovy in DEGREES.  The reference passes
 *   fov_ = 100 / 180 * pi -- radians -- as that argument (:118, :444), so its field of view is 1.745 degrees; the
 *   reference's values are fovy = 100.0 / 180.0 * 3.14159265358979323846, z_near 0.1, z_far 1e4 and
 *   aspect = (float)W / (float)H.
 *   rgbdfe_render_viewer_view(x_tra, y_tra, z_tra, x_rot, y_rot, z_rot, rotation_stepping, viewpoint, out): the
 *   modelview of drawClouds (:356-377): glTranslatef, glRotatef about x, y, z by (int)((rot / 16) / rotation_stepping) *
 *   rotation_stepping degrees, glMultMatrix(viewpoint).  The translations and angles are rounded to float as GL takes
 *   them.  viewpoint (NULL: identity) is the INVERSE of a camera pose, as setViewPoint makes it (:1122-1125).
 *   initialPosition's values (:137-144): 0, 0, -50, 180 * 16, 0, 0, stepping 1.
 *   rgbdfe_render_sensor_camera(fx, fy, cx, cy, W, H, z_near, z_far, pose, view_out, projection_out): the camera
 *   under which a point (x, y, z) of the sensor frame at the rigid `pose` (NULL: identity; z forward, y down) lands at
 *   x_w = fx x / z + cx + 1/2 and at image row fy y / z + cy + 1/2 from the top (y_w = H - that): a cloud rendered
 *   through its own intrinsics puts point (u, v) on pixel (u, v).
 *   rgbdfe_render_unproject(x, y, depth, view, projection, W, H, out3): gluUnProject over the viewport (0, 0, W, H), as
 *   setClickedPosition uses it (:1127-1153; x, y in window coordinates, y up).  Returns RGBDFE_OK, or
 *   RGBDFE_ERR_INVALID_ARG when projection . view is singular.
 * rgbdfe_render_fragment_stats(ctx, enable, out2): diagnostics (tools/bench_render.py).  out2 (may be NULL) receives what
 *   the latest render call counted: the fragments offered to the depth test, and those that lowered a pixel's word when
 *   they arrived (this one depends on the order of arrival; at least the pixels drawn).  Both are 0 unless counting was
 *   on.  Then enable = 1 / 0 turns the counting kernels on / off for the calls that follow (-1: as it is).  The images
 *   are the same bytes either way; the counting kernels take a returning atomic per won fragment and two adds per lane. */
typedef struct rgbdfe_render_params {
  int32_t width, height;
  double view[16];
  double projection[16];
  double gl_point_size;
  int32_t cull;
  uint8_t clear_rgba[4];
  int64_t max_vertices_in_flight;
} rgbdfe_render_params;
void rgbdfe_render_default_params(rgbdfe_render_params* p);
int rgbdfe_render_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                        const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params,
                        uint8_t* rgba, float* depth, int64_t* ids, int32_t* node_index);
int rgbdfe_render_nodes_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                               const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params,
                               void* d_rgba, void* d_depth, void* d_ids, void* d_node_index, void* stream);
void rgbdfe_render_perspective(double fovy, double aspect, double z_near, double z_far, double* out16);
void rgbdfe_render_viewer_view(double x_tra, double y_tra, double z_tra, double x_rot, double y_rot, double z_rot,
                               double rotation_stepping, const double* viewpoint, double* out16);
void rgbdfe_render_sensor_camera(double fx, double fy, double cx, double cy, int32_t width, int32_t height, double z_near,
                                 double z_far, const double* pose, double* view_out16, double* projection_out16);
int rgbdfe_render_unproject(double x, double y, double depth, const double* view, const double* projection, int32_t width,
                            int32_t height, double* out3);
int rgbdfe_render_fragment_stats(rgbdfe_ctx* ctx, int32_t enable, int64_t* out2);

/* GPU prefilter in front of the pair path (second half): what loop_closing.cpp's
 * GraphManager::getNeighbours (:190-277, behind DO_LOOP_CLOSING, never wired into nodeComparisons) sketched -- every
 * descriptor of the new node votes `k_neighbours - rank` (:241) for the nodes holding its k nearest descriptors, a
 * node's votes are divided by its descriptor count (:263), the nodes are ranked by that score (:269) -- with EXACT
 * binary neighbours instead of an approximate kd-tree: a descriptor's k nearest nodes are the k candidates whose best
 * match (the Hamming stage's keys) has the smallest distance, ties to the candidate listed first; matches with
 * hd >= max_hd do not vote (128 = featureMatching's gate, node.cpp:572; 257 = every match votes).
 * out_ids / out_scores: the at most max_out best candidates in descending score order (ties: listed first); candidates
 * without a vote are not returned.  k_neighbours in [1, 8].  Feed out_ids to rgbdfe_match_node_pairs. */
int rgbdfe_place_recognition(rgbdfe_ctx* ctx, int32_t query_id, const int32_t* candidate_ids, int32_t n_candidates,
                             int32_t k_neighbours, int32_t max_hd, int32_t max_out, int32_t* out_ids, float* out_scores,
                             int32_t* n_out);
/* Many query nodes at once (an offline loop-closure sweep: ONE Hamming launch + ONE vote launch for all of them).
 * Query s has the candidates candidate_ids[candidate_offsets[s] .. candidate_offsets[s+1]-1] (offsets[0] = 0, at most
 * 65535 per query, offsets[n_queries] <= max_pairs_per_batch); its ranked list goes to out_ids / out_scores
 * [s * max_out ...], its length to out_counts[s]. */
int rgbdfe_place_recognition_batch(rgbdfe_ctx* ctx, const int32_t* query_ids, int32_t n_queries,
                                   const int32_t* candidate_offsets, const int32_t* candidate_ids, int32_t k_neighbours,
                                   int32_t max_hd, int32_t max_out, int32_t* out_ids, float* out_scores,
                                   int32_t* out_counts);

/* ---- per-frame feature path: detect + describe (Node::Node, node.cpp:139-210) -----------------
 * rgbdfe_detect_describe replaces, for one frame,
 *   detector->detect(gray, kps, mask)   the 3x3 grid of threshold-adaptive ORB detectors built by
 *                                       createDetector("ORB") (features.h:9, features.cpp:63-113,
 *                                       feature_adjuster.cpp:85-317); its per-cell FAST thresholds
 *                                       persist across frames inside the context, like the reference's
 *                                       detector_ object (openni_listener.h:195)
 *   removeDepthless + KeyPointsFilter::retainBest(max_keypoints)          (node.cpp:186-191)
 *   extractor->compute(gray, kps, desc) cv::ORB::create() defaults        (features.cpp:117-119)
 *   projectTo3D                                                           (node.cpp:900-965)
 * gray: rows x cols u8; mask: rows x cols u8 (depth_mono8, non-zero = usable) or NULL;
 * depth: rows x cols float32 metres (NaN = no measurement).  Outputs are sized by the caller for
 * max_keypoints entries: keypoints, descriptors (32 bytes each), xyz1 (4 floats each). */
typedef struct {
  float x, y;       /* cv::KeyPoint::pt (level-0 pixel coordinates) */
  float size;       /* 31 * scale of the octave; FAST: 7 */
  float angle;      /* degrees (cv::fastAtan2 of the intensity centroid); FAST: -1 */
  float response;   /* Harris response; FAST: the FAST score (cornerScore) */
  int32_t octave;   /* pyramid level; FAST: 0 */
} rgbdfe_keypoint;
/* parameter_server.cpp:83,87,89; resets the per-cell thresholds */
int rgbdfe_detector_configure(rgbdfe_ctx* ctx, int32_t max_keypoints, int32_t grid_resolution,
                              int32_t adjuster_max_iterations);
/* the current per-cell FAST thresholds (grid_resolution^2 doubles) */
int rgbdfe_detector_thresholds(rgbdfe_ctx* ctx, double* thresholds, int32_t* n_cells);
/* The inverse: n_cells must equal grid_resolution^2 of the configured grid, every threshold must be finite.  The thresholds
 * are all a grid detector (either type) carries from one frame to the next, so a context that is configured like another
 * and given its thresholds detects the following frames as that one would. */
int rgbdfe_detector_set_thresholds(rgbdfe_ctx* ctx, const double* thresholds, int32_t n_cells);
/* Parameter "feature_detector_type" (parameter_server.cpp, createDetector in features.cpp:63-113) with the default ORB
 * extractor.  RGBDFE_DETECTOR_ORB (the default): the grid of adaptive cv::ORB detectors.  RGBDFE_DETECTOR_FAST: the same grid
 * and threshold adaptation around cv::FastFeatureDetector (DetectorAdjuster("FAST", 20), feature_adjuster.cpp:88-91):
 * keypoints of size 7, angle -1, response = FAST score, octave 0, then Node::Node's ORB-extractor steps (removeDepthless,
 * retainBest(max_keypoints), cv::ORB::compute, projectTo3D; node.cpp:183-210).  rgbdfe_detect_describe, _batch, _batch_nodes,
 * _cloud and rgbdfe_detector_thresholds follow the type; the detector configuration (rgbdfe_detector_configure) is shared.
 * Setting a type resets the per-cell thresholds to 20, as a fresh createDetector does; an unknown type is
 * RGBDFE_ERR_INVALID_ARG.  Under FAST, rgbdfe_detect_describe_batch_nodes accepts NULL keypoints / descriptors / xyz1 (any
 * of them): those host outputs are not written, the nodes are. */
#define RGBDFE_DETECTOR_ORB 0
#define RGBDFE_DETECTOR_FAST 1
int rgbdfe_set_detector_type(rgbdfe_ctx* ctx, int32_t type);
/* "use_feature_min_depth" (parameter_server.cpp:90, default off): a keypoint's depth is the nearest valid depth in its
 * neighbourhood (getMinDepthInNeighborhood, misc.cpp:774-793) instead of the pixel under it -- in removeDepthless
 * (node.cpp:82) and projectTo3D (:940).  rgbdfe_set_feature_min_depth switches rgbdfe_detect_describe(_batch) over;
 * rgbdfe_project_to_3d_min_depth is rgbdfe_project_to_3d in that mode (kp_size = cv::KeyPoint::size per keypoint).
 * The SIFTGPU call site (node.cpp:730) is rgbdfe_sift_node_features_min_depth. */
int rgbdfe_set_feature_min_depth(rgbdfe_ctx* ctx, int32_t on);
int rgbdfe_project_to_3d_min_depth(rgbdfe_ctx* ctx, const float* kp_xy, const float* kp_size, int32_t n_kp,
                                   const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx,
                                   double cy, double depth_scaling, int32_t max_keypoints, int32_t* kept_idx,
                                   float* xyz1, int32_t* n_out);
int rgbdfe_detect_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth,
                           int32_t rows, int32_t cols, double fx, double fy, double cx, double cy,
                           double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors,
                           float* xyz1, int32_t* n_out);
/* Page-locks a range of the caller's host memory (hipHostRegister) / releases it.  rgbdfe_detect_describe copies image
 * buffers that are page-locked straight to the device; pageable ones (cv::Mat data as cv_bridge hands it over,
 * openni_listener.cpp) first go through the library's own pinned staging buffer, ~60 us per 640x480 frame.  An
 * integration that owns its image buffers registers them once.  ptr / bytes: as malloc'ed or page-aligned; registering
 * a range twice is an error. */
int rgbdfe_host_register(rgbdfe_ctx* ctx, void* ptr, size_t bytes);
int rgbdfe_host_unregister(rgbdfe_ctx* ctx, void* ptr);
/* A run of frames through the same detector state, in order: the same keypoints, descriptors and points as n_frames
 * calls of rgbdfe_detect_describe (the per-cell thresholds carry over from frame to frame, feature_adjuster.cpp:185-224),
 * with up to 7 frames sharing every kernel launch (64 / grid_resolution^2 frames per launch chain: the device pass runs at
 * floor thresholds and the adjuster is replayed over the scored corners on the host) and three launch chains
 * in flight.  For offline runs (bag files, OpenNIListener in "batch_processing" mode): 10-14 k frames/s at 640 x 480 for runs
 * of >= 56 frames.  Threads: the first call creates 11 worker threads inside the context (7 for the CPU halves of the
 * descriptions and the replay, 4 for staging copies; pure CPU work, they never enter the HIP runtime) that live until
 * rgbdfe_destroy, plus one helper thread per call.  mask may be NULL (no masks) or hold NULL entries; out_stride >= the configured
 * max_keypoints: frame f's outputs start at row f * out_stride of keypoints / descriptors (32 B rows) / xyz1 (4 floats),
 * n_out[f] of them. */
int rgbdfe_detect_describe_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                 const uint8_t* const* mask, const float* const* depth, int32_t rows, int32_t cols,
                                 double fx, double fy, double cx, double cy, double depth_scaling, int32_t out_stride,
                                 rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out);
/* The same, and frame f's features also become the resident node node_ids[f] (>= 0; negative: no node for that frame) --
 * what Node::Node + GraphManager::addNode + rgbdfe_upload_node do, without the features' trip to the host and back: the
 * descriptors and points are copied into the node slabs from the description's device buffers (the host outputs are filled
 * as before).  A frame WITHOUT features becomes an EMPTY node (n = 0), exactly what rgbdfe_upload_node(id, ..., 0)
 * leaves: a fresh id takes a slot and is resident (a pair against it is matched and comes back without an edge), an id that
 * exists is rewritten to n = 0 -- its old features are gone.  An id that exists and gets features is rewritten in place.
 * Capacity is checked for the whole batch before the first frame is detected, counting every fresh id as one slot (empty
 * frames consume theirs, so the count is exact). */
int rgbdfe_detect_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                       const uint8_t* const* mask, const float* const* depth, int32_t rows, int32_t cols,
                                       double fx, double fy, double cx, double cy, double depth_scaling, int32_t out_stride,
                                       rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out,
                                       const int32_t* node_ids);
/* the point-cloud constructor's feature path (see rgbdfe_project_to_3d_cloud above) */
int rgbdfe_detect_describe_cloud(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* cloud,
                                 int32_t rows, int32_t cols, double maximum_depth, rgbdfe_keypoint* keypoints,
                                 uint8_t* descriptors, float* xyz1, int32_t* n_out);
/* pieces, for A/B against cv::ORB: detect() of one image with a fixed FAST threshold (no grid,
 * feature_adjuster.cpp:94) and compute() for given keypoints (may drop border keypoints and
 * regroups them by octave, like cv::ORB::compute).  rgbdfe_orb_detect returns RGBDFE_ERR_CAPACITY with *n_out = the number
 * of keypoints (none written) when `capacity` rows are too few. */
int rgbdfe_orb_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                      int32_t fast_threshold, rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out);
int rgbdfe_orb_compute(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols,
                       rgbdfe_keypoint* keypoints, int32_t n, uint8_t* descriptors, int32_t* n_out);
/* A/B piece of the FAST detector: cv::FastFeatureDetector::create(threshold)->detect(gray, keypoints, mask) on one whole
 * image (no grid): FAST-9/16 with non-maximum suppression, then KeyPointsFilter::runByPixelsMask; keypoints in raster order,
 * size 7, angle -1, response = score, octave 0.  threshold is clamped to [0, 255] as cv::FAST does.  Returns
 * RGBDFE_ERR_CAPACITY with *n_out = the number of keypoints (none written) when `capacity` rows are too few. */
int rgbdfe_fast_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                       int32_t threshold, rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out);

/* ---- SIFT extraction (feature_detector_type / feature_extractor_type == "SIFTGPU") ---------------------------------
 * rgbdfe_sift_detect replaces SiftGPUWrapper::detect (sift_gpu_wrapper.h:49, sift_gpu_wrapper.cpp:113-167; called from
 * Node::Node, node.cpp:149-152, 282-286) with an empty keypoint list: SiftGPU's scale-space extrema detection, orientation
 * assignment and 4x4x8 descriptors with the options the wrapper's constructor sets (:29-88) -- first octave -1 (the image
 * is up-sampled x2), 5 DoG levels per octave, edge threshold 10, sub-pixel localisation, two orientations per keypoint,
 * UNNORMALISED descriptors ("-unn"), at most ~max_keypoints features chosen from the coarse octaves down ("-tc2",
 * parameter "max_keypoints") -- on the pipeline of SiftGPU's CUDA back end (external/SiftGPU/src/SiftGPU/ProgramCU.cu,
 * PyramidCU.cpp).  gray: rows x cols u8; mask is ignored, as the reference ignores it.  keypoints[i]: pt = SiftGPU's
 * (x, y), size = 12 * scale, angle in degrees (the wrapper's conversion, :156-160), response = octave = 0; desc128: n x 128
 * floats = what the wrapper returns as `descriptors` and Node::projectTo3DSiftGPU / rgbdfe_sift_node_features take.
 * Returns RGBDFE_ERR_CAPACITY with *n_out = the number of features when `capacity` rows are too few.
 * The wrapper's second mode (a caller-provided keypoint list, :132-142) is rgbdfe_sift_describe below. */
int rgbdfe_sift_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                       int32_t max_keypoints, rgbdfe_keypoint* keypoints, float* desc128, int32_t capacity, int32_t* n_out);
/* SiftGPUWrapper::detect with a non-empty keypoint list (sift_gpu_wrapper.cpp:132-142): feature_extractor_type == "SIFTGPU"
 * behind another detector (node.cpp:166-171) -- SiftGPU::SetKeypointList with its default "keys have orientation"
 * (SiftGPU.h:150), i.e. descriptors at the given positions, scales (size / 12) and orientations (angle, degrees), no
 * detection, no orientation assignment.  keypoints[n] are rewritten as the wrapper rebuilds them (size and angle through its
 * float conversions, response = octave = 0); desc128: n x 128 floats, unnormalised, row i for keypoint i. */
int rgbdfe_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols, rgbdfe_keypoint* keypoints, int32_t n,
                         float* desc128);
/* A run of frames of one size (offline processing of a recorded sequence): the results of n_frames single calls -- the
 * pipeline keeps no state between images -- with up to 8 frames sharing every launch (a frame alone is ~70 dependent
 * launches over planes of a few thousand pixels to 1.2 Mpixel and cannot fill the chip).  Frame f's keypoints / descriptors
 * go to row f * out_stride of keypoints / desc128 (128 floats per row), its count to n_out[f]; RGBDFE_ERR_CAPACITY when a
 * frame has more than out_stride features (n_out is complete, the rows of the other frames are valid). */
int rgbdfe_sift_detect_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, int32_t rows, int32_t cols,
                             int32_t max_keypoints, int32_t out_stride, rgbdfe_keypoint* keypoints, float* desc128,
                             int32_t* n_out);
/* Node::Node's SIFTGPU branch for a run of frames (node.cpp:147-176, 695-769, 1557-1571), straight into resident nodes: the
 * SIFTGPU counterpart of rgbdfe_detect_describe_batch_nodes.  Frame f's node equals what rgbdfe_sift_detect (or the batch),
 * then rgbdfe_sift_node_features(..., max_keypoints, use_root_sift) -- rgbdfe_sift_node_features_min_depth with kp_size =
 * the keypoints' size under rgbdfe_set_feature_min_depth(ctx, 1) -- then rgbdfe_upload_float_node(node_ids[f],
 * feature_descriptors, 128, xyz1, n) give: kind 2 (the FLANN branch, rgbdfe_match_flann_pair_list), same rows, same bits.
 * The descriptors and points stay on the device from the extraction to the slabs; depth[f] is a rows x cols float image.
 * max_keypoints serves both as SiftGPU's "-tc2" limit and as projectTo3DSiftGPU's cut (the first max_keypoints survivors in
 * list order, :748), as in the reference; it must lie in [1, the context's max_keypoints] (RGBDFE_ERR_INVALID_ARG).
 * node_ids is required: a negative id means no node for that frame, an id may appear once.  The node table follows
 * rgbdfe_detect_describe_batch_nodes: free slots are checked for the whole batch before any work (each fresh id counts once),
 * a frame without features that have depth becomes an empty node (n = 0), an existing id -- of any kind -- is rewritten in
 * place after the pair lanes that may read it have finished.
 * Host outputs, each optional (NULL: not written; all three NULL: no descriptor crosses to the host): keypoints = the kept
 * keypoints (feature_locations_2d_ after the erase and the cut, fields as rgbdfe_sift_detect reports them), xyz1 = 4 floats
 * per point, feature_descriptors = 128 floats per row; frame f's rows start at row f * out_stride.  n_out[f] is always
 * written; RGBDFE_ERR_CAPACITY when a frame keeps more than out_stride rows and a host output was asked for (n_out is
 * complete, the nodes and the other frames' rows are valid). */
int rgbdfe_sift_detect_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                   const float* const* depth, int32_t rows, int32_t cols,
                                   double fx, double fy, double cx, double cy, double depth_scaling,
                                   int32_t max_keypoints, int32_t use_root_sift, const int32_t* node_ids,
                                   int32_t out_stride, rgbdfe_keypoint* keypoints, float* xyz1,
                                   float* feature_descriptors, int32_t* n_out);

/* ---- SIFTGPU descriptors behind the grid detector (feature_detector_type ORB / FAST, feature_extractor_type SIFTGPU) ----
 * rgbdfe_detect is detector->detect alone (node.cpp:160) for the context's detector type and grid state: the grid-adapted
 * detector's aggregate (feature_adjuster.cpp:185-317) in aggregate order -- no removeDepthless, no retainBest -- with the
 * detector's own fields (ORB: size 31 * 1.2^octave, angle, Harris response, octave; FAST: size 7, angle -1, score, octave 0).
 * The per-cell thresholds advance exactly as rgbdfe_detect_describe advances them on the same frame.  The aggregate never
 * holds more than max_total = floor(1.5 * max_keypoints) keypoints (keepStrongest(max_total / cells) per cell): a smaller
 * capacity is RGBDFE_ERR_INVALID_ARG, refused before any state changes. */
int rgbdfe_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                  rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out);
/* Node::Node's steps for that setting, one frame (node.cpp:160, 165-176): rgbdfe_detect -> projectTo3D (node.cpp:900-965:
 * the first max_keypoints keypoints with depth, in aggregate order) -> SiftGPUWrapper::detect with that list
 * (rgbdfe_sift_describe) -> projectTo3DSiftGPU + RootSIFT under use_root_sift (rgbdfe_sift_node_features).  The same bits as
 * those calls composed; rgbdfe_set_feature_min_depth switches both depth lookups to the _min_depth forms.  When projectTo3D
 * keeps no keypoint the wrapper gets an EMPTY list and SiftGPU detects on its own (sift_gpu_wrapper.cpp:133,
 * SiftPyramid.cpp:154-156): the frame then gets rgbdfe_sift_detect(..., max_keypoints) -> rgbdfe_sift_node_features.
 * max_keypoints is the detector's (rgbdfe_detector_configure); outputs hold that many rows: keypoints (as the wrapper rebuilds
 * them: size 12 * scale, angle in degrees, response = octave = 0), xyz1 (4 floats), siftgpu_descriptors and
 * feature_descriptors (128 floats; feature_descriptors may be NULL). */
int rgbdfe_detect_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth, int32_t rows,
                                int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling,
                                int32_t use_root_sift, rgbdfe_keypoint* keypoints, float* xyz1, float* siftgpu_descriptors,
                                float* feature_descriptors, int32_t* n_out);
/* A run of frames through the same detector state: n_frames calls of rgbdfe_detect_sift_describe, each followed by
 * rgbdfe_upload_float_node(node_ids[f], feature_descriptors, 128, xyz1, n) -- kind 2 nodes, what
 * rgbdfe_match_flann_pair_list reads.  node_ids is required (negative: no node; an id may appear once); the node table follows
 * rgbdfe_detect_describe_batch_nodes (free slots checked for the whole batch first, a frame without features becomes an empty
 * node, an existing id is rewritten in place).  mask may be NULL or hold NULL entries; out_stride >= max_keypoints
 * (RGBDFE_ERR_INVALID_ARG); each host output may be NULL; frame f's rows start at row f * out_stride, n_out[f] of them.
 * Up to 8 frames share every launch after the detection; with all host outputs NULL no descriptor crosses
 * PCIe.  Multi-device handles process the frames on the first device and hand the nodes to the others. */
int rgbdfe_detect_sift_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                            const uint8_t* const* mask, const float* const* depth, int32_t rows, int32_t cols,
                                            double fx, double fy, double cx, double cy, double depth_scaling,
                                            int32_t use_root_sift, const int32_t* node_ids, int32_t out_stride,
                                            rgbdfe_keypoint* keypoints, float* xyz1, float* feature_descriptors, int32_t* n_out);

/* ---- ORB descriptors behind SiftGPU's detection (feature_detector_type SIFTGPU, feature_extractor_type ORB) --------------
 * Node::Node's steps for that setting, one frame (node.cpp:149-152, 183-210): SiftGPUWrapper::detect's own detection with
 * "-tc2 max_keypoints" (its descriptors are never computed), the keypoints as the wrapper rebuilds them (size 12 * scale, angle
 * in degrees, response = octave = 0), removeDepthless, retainBest(max_keypoints) + resize (every response is 0: the first
 * max_keypoints survivors in SiftGPU's list order), cv::ORB::compute (the 31-pixel border filter, rBRIEF at each keypoint's own
 * angle on level 0), projectTo3D.  The cut comes before the border filter, so a frame can keep fewer than max_keypoints rows
 * although SiftGPU found more.  The same bits as rgbdfe_sift_detect(..., max_keypoints) -> removeDepthless and the cut ->
 * rgbdfe_orb_compute -> rgbdfe_project_to_3d; rgbdfe_set_feature_min_depth switches both depth lookups to the neighbourhood
 * of size 12 * scale (rgbdfe_project_to_3d_min_depth).  max_keypoints must lie in [1, the context's max_keypoints]
 * (RGBDFE_ERR_INVALID_ARG).  Outputs hold max_keypoints rows: keypoints, descriptors (32 bytes), xyz1 (4 floats); the node is
 * matched by the ORB branch (rgbdfe_upload_node, rgbdfe_match_pair_list). */
int rgbdfe_sift_detect_orb_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const float* depth, int32_t rows, int32_t cols,
                                    double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                    rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out);
/* A run of frames of one size: n_frames calls of rgbdfe_sift_detect_orb_describe, each followed by rgbdfe_upload_node(node_ids[f],
 * descriptors, xyz1, n) -- kind 0 (ORB) nodes, what rgbdfe_match_pair_list reads; the keypoints never cross PCIe between the
 * SIFT detection and the nodes.  node_ids is required (negative: no node; an id may appear once); the node table follows
 * rgbdfe_detect_describe_batch_nodes (free slots checked for the whole batch first, a frame without features becomes an empty
 * node, an existing id of any kind is rewritten in place after the pair lanes that may read it have finished).  Each host
 * output may be NULL (all NULL: nothing but n_out comes back); frame f's rows start at row f * out_stride, n_out[f] of them;
 * out_stride < max_keypoints while an output is asked for is RGBDFE_ERR_CAPACITY, refused before any work.  Up to 8 frames
 * share every launch.  Multi-device handles process the frames on the first device and hand the nodes to
 * the others. */
int rgbdfe_sift_detect_orb_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray,
                                                const float* const* depth, int32_t rows, int32_t cols, double fx, double fy,
                                                double cx, double cy, double depth_scaling, int32_t max_keypoints,
                                                const int32_t* node_ids, int32_t out_stride, rgbdfe_keypoint* keypoints,
                                                uint8_t* descriptors, float* xyz1, int32_t* n_out);
/* stage access for parity tests: the pyramid geometry of the latest frame, one Gaussian plane (octave index from 0, level
 * 0 .. levels-1; padded width x height floats), the keypoint candidates of one (octave, DoG level) as rows of
 * (x, y, extremum sign, dx, dy, ds) in list order, before the feature-count limit */
int rgbdfe_sift_geometry(rgbdfe_ctx* ctx, int32_t* octave_min, int32_t* octave_num, int32_t* levels, int32_t* dog_levels);
int rgbdfe_sift_debug_plane(rgbdfe_ctx* ctx, int32_t octave, int32_t level, float* out, int32_t capacity_floats, int32_t* w,
                            int32_t* h);
int rgbdfe_sift_debug_candidates(rgbdfe_ctx* ctx, int32_t octave, int32_t dog_level, float* out, int32_t capacity_rows,
                                 int32_t* n);

/* ---- sensor frames -------------------------------------------------------- */
/* The frames as the sensor messages carry them: a colour (or mono) image and a raw depth image, possibly of another size.
 * The library does the listener's and Node::Node's image preparation on the device (csrc/ingest.hip), in front of the
 * detect / describe / project chain of the entry points above.  In the reference's order:
 *  1. Depth size.  If the depth image's size differs from the visual image's, every later step sees the depth image
 *     resampled to the visual size by nearest neighbour on the raw samples (openni_listener.cpp:651-655): source column
 *     min(floor(x * (1.0 / ((double)dst_cols / src_cols))), src_cols - 1), rows alike, in double (OpenCV 3.3 resizeNN).
 *  2. depthToCV8UC1 (misc.cpp:414-430).  32FC1: mono8 = convertTo(CV_8UC1, 100).  16UC1: mono8 = convertTo(CV_8UC1, 0.05,
 *     -25) and depth_m = convertTo(CV_32FC1, 0.001): the bytes and bits of rgbdfe_depth_to_mono8.  A 16UC1 hole therefore
 *     is 0.0f, not NaN: removeDepthless keeps keypoints on it, and the mask is zero below about 0.5 m.
 *  3. Gray (node.cpp:139-144).  MONO8: the bytes themselves.  RGB8 and BGR8 are both CV_8UC3, and the reference applies
 *     CV_RGB2GRAY to the channels AS STORED whatever the encoding: gray = (c0*4899 + c1*9617 + c2*1868 + 8192) >> 14
 *     (OpenCV 3.3 RGB2Gray<uchar>).  A bgr8 frame gets the red weight on its blue channel; that is reproduced, not mended.
 *  4. Node::Node's steps as the existing entry points perform them, with the context's detector type
 *     (RGBDFE_DETECTOR_ORB / _FAST), grid state, thresholds and rgbdfe_set_feature_min_depth mode.
 *  5. Cloud (node.cpp:126-132): createXYZRGBPointCloud on the float depth of step 2 and the visual image as stored, with
 *     the caller's encoding_bgr (a parameter in the reference, not derived from the message).
 * Contract: a sensor call gives, bit for bit, what the corresponding existing call gives when it is fed the three planes of
 * rgbdfe_ingest_frame for the same frame.  The SIFTGPU detector / extractor combinations are served by
 * rgbdfe_ingest_frame followed by the existing calls.  Not covered: Bayer and 4-channel images. */
#define RGBDFE_VISUAL_MONO8 0   /* CV_8UC1: used as it is (node.cpp:142-143) */
#define RGBDFE_VISUAL_RGB8  1   /* CV_8UC3 */
#define RGBDFE_VISUAL_BGR8  2   /* CV_8UC3; differs from RGB8 only for the cloud's colour */
#define RGBDFE_DEPTH_32FC1  0   /* metres, NaN = no measurement */
#define RGBDFE_DEPTH_16UC1  1   /* millimetres, 0 = no measurement */
typedef struct rgbdfe_sensor_frame {
  const uint8_t* visual; int32_t visual_rows, visual_cols, visual_step /* bytes per row */, visual_encoding;
  const void*    depth;  int32_t depth_rows,  depth_cols,  depth_step  /* bytes per row */, depth_encoding;
} rgbdfe_sensor_frame;
int rgbdfe_sizeof_sensor_frame(void);
/* Steps 1-3: what the listener and Node::Node hand to detector->detect / removeDepthless / projectTo3D.  Outputs are
 * visual_rows x visual_cols, each may be NULL. */
int rgbdfe_ingest_frame(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, uint8_t* gray, uint8_t* mono8, float* depth_m);
/* rgbdfe_detect_describe on a sensor frame (the context's detector type, ORB extractor). */
int rgbdfe_sensor_detect_describe(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, double fx, double fy, double cx, double cy,
                                  double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1,
                                  int32_t* n_out);
typedef struct rgbdfe_sensor_cloud {   /* NULL pointer = no clouds */
  int32_t cloud_skip; int32_t encoding_bgr; double min_depth;
} rgbdfe_sensor_cloud;
/* rgbdfe_detect_describe_batch_nodes on a run of sensor frames of one geometry (visual size, depth size, both encodings);
 * node_ids may be NULL (= rgbdfe_detect_describe_batch).  With `cloud` (which needs node_ids), frame f's structured cloud
 * is also kept under node_ids[f] as rgbdfe_upload_node_cloud would keep it.  Everything that can be refused
 * (RGBDFE_ERR_INVALID_ARG: NULL frame / image pointers, unknown encodings, a step smaller than a row, non-positive sizes,
 * frames that differ in geometry, a cloud_skip that does not divide the visual size, cloud without node_ids) is refused
 * before any detector state changes.  Node-table rules and the multi-device behaviour are those of
 * rgbdfe_detect_describe_batch_nodes. */
int rgbdfe_sensor_detect_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames,
                                              double fx, double fy, double cx, double cy, double depth_scaling,
                                              int32_t out_stride, rgbdfe_keypoint* keypoints, uint8_t* descriptors,
                                              float* xyz1, int32_t* n_out, const int32_t* node_ids,
                                              const rgbdfe_sensor_cloud* cloud);

/* ---- the SLAM step (GraphManager::addNode, graph_manager.cpp:360-898; isBigTrafo / isSmallTrafo misc.cpp:272-315) --------
 * One call per frame over the stages above: the frame is uploaded or detected into a node of the context first (the
 * caller names it: `slot` below is that node id), rgbdfe_slam_add_node then selects candidates, compares, decides, updates
 * the pose graph and optimises, and reports what it did.  The contract is the reference's code with its quirks
 * (restated; DESIGN.md 4.27 names every choice and deviation).
 *
 * An rgbdfe_slam borrows a context (may be NULL: the decision machine alone, see rgbdfe_slam_begin) and a pose graph the
 *   caller made; the strategy is whatever the caller set on that graph.  It keeps graph_ as a table graph id -> slot,
 *   keyframe_ids_, next_seq_id, curr_best_result_, valid_tf_estimate_ and the stamp of every node, and the counters of
 *   sequential and loop-closure edges.  Graph ids are the reference's: id = graph_.size() when the frame passes the feature
 *   gate, vertex_id = id.  Every output speaks in graph ids.  A dropped frame consumes no id and its slot stays the caller's.
 * The step, for a node of n_rows rows stamped (stamp_sec, stamp_nsec):
 *   1. n_rows < min_matches: RGBDFE_SLAM_TOO_FEW_FEATURES, nothing changes (also with keep_all_nodes, addNode :687).
 *   2. Empty graph: firstNode (:360-402): id 0, estimate init_base_pose, fixed, keyframe 0: RGBDFE_SLAM_FIRST.
 *   3. nodeComparisons (:421-658).  earliest_loop_closure_node = the new id, under every strategy, RGBDFE_POSE_RELATIVE_TO_NONE
 *      included (:444; the keyframe rule below reads it, the optimiser only under LARGEST_LOOP).  prev_best is read from a
 *      fresh result and is always -1 (:452-453): the "reuse best" append of :524-526 never happens.
 *      Initial comparison, only when min_translation_meter > 0 or min_rotation_degree > 0: against graph_[size - 1].  An
 *        edge with !isBigTrafo || !isSmallTrafo: RGBDFE_SLAM_MOTION_OUT_OF_BOUNDS, the frame is dropped, curr_best_result_
 *        keeps the result and broadcast_pose = X(previous) * Z.  Otherwise addEdgeToG2O(edge, largeEdge = 1, set_estimate =
 *        1) and predecessor_matched = 1.
 *      Candidates: rgbdfe_potential_edge_targets(predecessor_candidates - 1, neighbor_candidates, min_sampled_candidates,
 *        geodesic_depth, ...): after a matched predecessor with predecessor_id = curr_best.id1 and include_predecessor = 0,
 *        otherwise with the sequentially previous id and include_predecessor = 1.  Draws: the generator of
 *        rgbdfe_slam_set_rand, else the counter-based one seeded with seed + (add_node / begin calls before this one).
 *      Comparisons in list order as one batch (the concurrent_edge_construction branch, :531-583).  Per result with an edge:
 *        dt = stamp(new) - stamp(older) as ros::Duration (integer seconds and nanoseconds, normalised, sec + 1e-9 nsec);
 *        accepted iff isSmallTrafo(T, dt) and addEdgeToG2O(edge, largeEdge = isBigTrafo(T), set_estimate = n_inl > best.n_inl);
 *        then predecessor_matched |= (id1 == id2 - 1), updateInlierFeatures, valid_tf_estimate[id1] = 1, best = this result if
 *        n_inl > best.n_inl, edge_to_keyframe |= (id1 is a keyframe).
 *      addEdgeToG2O (:811-898): the new node has no vertex yet and !largeEdge: refused.  Otherwise the vertex is created
 *        (rgbdfe_pose_graph_add_node) with X2 = X1 * Z, or X2 = X1 * Z is written when set_estimate; the edge is
 *        rgbdfe_pose_graph_add_edge_se3 with information I * info_scale (1e-2 I for an ICP edge, node.cpp:1407 -- the only value
 *        the reference defines for one); |id1 - id2| > predecessor_candidates counts as a loop closure, else as sequential.
 *      isBigTrafo / isSmallTrafo on the double cast of the float transform, host libm, no contraction: angle = acos((trace -
 *        1) / 2) * 180 / pi without a clamp (a NaN fails both comparisons), dist = sqrt((tx tx + ty ty) + tz tz); big: dist >
 *        min_translation_meter || angle > min_rotation_degree; small: seconds <= 0, or dist / seconds < max_translation_meter
 *        && angle / seconds < max_rotation_degree.
 *      Constant-position edge (:624-655) iff (!found && have_odometry_frame) || (!found && keep_anyway) ||
 *        (!predecessor_matched && |dt_prev| < 0.1), keep_anyway = keep_all_nodes || (n_rows > min_matches && keep_good_nodes),
 *        |dt_prev| as float: edge (previous id -> new id, identity, I / |dt_prev|) with largeEdge = set_estimate = 1,
 *        valid_tf_estimate[new] = 0, curr_best_result_ = an empty result carrying this edge.  Deviation: |dt_prev| == 0 would
 *        hand the optimiser an infinite matrix; the edge is then not added (constant_position = RGBDFE_SLAM_CONSTANT_SKIPPED).
 *      found = an edge was added, the constant-position edge included.
 *   4. found (:704-751): id % create_cloud_every_nth_node != 0: the node's cloud is released.  !edge_to_keyframe &&
 *      earliest_loop_closure_node > keyframe_ids_.back(): addKeyframe(id - 1) (earliest is lowered only under LARGEST_LOOP).
 *      optimizer_skip_step > 0 && vertices % optimizer_skip_step == 0: rgbdfe_pose_graph_optimize_graph(optimizer_iterations),
 *      synchronously.  RGBDFE_SLAM_ADDED.
 *      not found, one node in the graph and n_rows > rows of node 0 (:762-769): the graph is reset and the new node becomes
 *      firstNode: RGBDFE_SLAM_REPLACED_FIRST (node 0's slot is released); otherwise RGBDFE_SLAM_NO_MATCH, the frame is dropped.
 *   5. addKeyframe (:784-809): with clear_non_keyframes and >= 2 keyframes every node strictly between the two most recent
 *      keyframes loses its features and its cloud (its slot is released, slot_of becomes -1, matchable 0), before the new
 *      id is appended.  A later comparison with such a node gives no edge.
 * Not built: localization_only_, landmarks, odometry edges from tf, GUI signals and rviz markers,
 *   octomap_online_creation (chain rgbdfe_octomap_insert_nodes), concurrent optimisation, the non-concurrent comparison order,
 *   max_connections.
 * matchNodePair's chain behind the pair op (node.cpp:1340-1377), inside rgbdfe_slam_add_node, each stage one batch per list:
 *   use_icp != 0: the ICP fallback (rgbdfe_icp_align_nodes with its default parameters, the older node's cloud onto the new
 *   node's, identity guess) serves the results WITHOUT a RANSAC transformation whose node is adjacent (new id - its id <= 1);
 *   a converged alignment is an edge with final_trafo = icp_trafo (the literal assignment), information 1e-2 I, no inliers
 *   (RGBDFE_SLAM_RESULT_ICP).  observability_threshold > 0: the pairwise observation likelihood (two
 *   rgbdfe_observation_likelihood jobs per edge with emm__skip_step, rgbdfe_observation_criterion_met) on the RANSAC edges
 *   only; an edge it withdraws (RGBDFE_SLAM_RESULT_WITHDRAWN) is not offered to ICP.  The nodes named need resident clouds
 *   (RGBDFE_ERR_UNKNOWN_NODE otherwise).
 *
 * rgbdfe_slam_begin / rgbdfe_slam_feed: the decision machine without the device, for callers that run the comparisons
 *   themselves.  begin either finishes the step (*n_ids = 0, *step filled) or hands out graph ids to compare the new node
 *   with (*n_ids > 0); feed takes their results -- results[k] belongs to ids[k]: an edge iff results[k].id1 >= 0, its ids are
 *   taken from the list, not from the record (whose ids name the context's nodes) -- and again finishes or hands out the
 *   next list.  flags (may be NULL) per result: RGBDFE_SLAM_RESULT_ICP: an ICP edge; RGBDFE_SLAM_RESULT_WITHDRAWN: the
 *   measurement model withdrew the edge.  A node whose slot was released (slot_of -1) has no features: feed a record
 *   with id1 = -1 for it.  With a context, the finished step releases slots and clouds and optimises as add_node does;
 *   without one the step only says what is due (optimize_due, cloud_released, cleared_first / _last, released_slot).
 * rgbdfe_slam_add_node = begin, rgbdfe_match_pair_list_device per list, feed, and ONE launch of the inlier-statistics
 *   kernel over the batch's records where they lie in device memory.  Single-device contexts.  rgbdfe_slam_create refuses
 *   (RGBDFE_ERR_CAPACITY) parameters whose longest candidate list -- predecessor + neighbor + sampled candidates -- exceeds
 *   max_pairs_per_batch or RGBDFE_SLAM_MAX_CANDIDATES, so no step can fail for its size half way.  A device error in the
 *   middle of a step (a failed launch or copy) abandons the step: the call returns the error, and what the step had added to
 *   the graph by then stays -- rgbdfe_slam_reset before the object is used again.
 * feature_matching_stats_ (node.h, updateInlierFeatures graph_manager.cpp:409-419): every node slot of a context has
 *   max_keypoints saturating 8-bit counters, zero when a node is uploaded or detected into the slot.
 *   rgbdfe_update_inlier_features: for every pair k with accept[k] != 0 and every set bit m of its record's inlier_mask,
 *   stats[query_ids[k]][all_q[m]] and stats[train_ids[k]][all_t[m]] are incremented, stopping at 255 -- the sequential loop's
 *   result whatever the order (32-bit compare-and-swap on the containing word; integers only).  d_records: n
 *   rgbdfe_match_result in device memory (what rgbdfe_match_pair_list_device left); the lists make no second trip to the
 *   host.  No launch when no accept byte is set.  *launched (may be NULL) = kernel launches.
 *   rgbdfe_node_feature_stats: the counters of a node's rows (capacity < rows: RGBDFE_ERR_CAPACITY); returns the row count.
 * rgbdfe_pose_graph_add_keyframe: appends to keyframe_ids_ (the reference promotes id - 1 after the fact).
 * rgbdfe_pose_graph_clear: resetGraph: nodes, edges, keyframes gone; the strategy stays. */
#define RGBDFE_SLAM_MAX_CANDIDATES 64
#define RGBDFE_SLAM_TOO_FEW_FEATURES 1
#define RGBDFE_SLAM_FIRST 2
#define RGBDFE_SLAM_MOTION_OUT_OF_BOUNDS 3
#define RGBDFE_SLAM_ADDED 4
#define RGBDFE_SLAM_NO_MATCH 5
#define RGBDFE_SLAM_REPLACED_FIRST 6
#define RGBDFE_SLAM_VERDICT_NO_EDGE 0
#define RGBDFE_SLAM_VERDICT_ACCEPTED 1
#define RGBDFE_SLAM_VERDICT_NOT_SMALL 2
#define RGBDFE_SLAM_VERDICT_TOO_SHORT 3      /* addEdgeToG2O refused: no vertex yet and not a big transformation */
#define RGBDFE_SLAM_VERDICT_WITHDRAWN 4      /* by the measurement model */
#define RGBDFE_SLAM_VERDICT_OUT_OF_BOUNDS 5  /* the initial comparison's edge */
#define RGBDFE_SLAM_VERDICT_ICP 16           /* or-ed in: the edge came from the ICP fallback */
#define RGBDFE_SLAM_RESULT_ICP 1
#define RGBDFE_SLAM_RESULT_WITHDRAWN 2
#define RGBDFE_SLAM_CONSTANT_NONE 0
#define RGBDFE_SLAM_CONSTANT_ADDED 1
#define RGBDFE_SLAM_CONSTANT_SKIPPED 2
typedef struct rgbdfe_slam_params {
  int32_t min_matches;              /* 20    (parameter_server.cpp:85) */
  int32_t predecessor_candidates;   /* 4 */
  int32_t neighbor_candidates;      /* 4 */
  int32_t min_sampled_candidates;   /* 4 */
  int32_t geodesic_depth;           /* 3 */
  int32_t keep_all_nodes;           /* 0 */
  int32_t keep_good_nodes;          /* 0 */
  int32_t clear_non_keyframes;      /* 0 */
  int32_t create_cloud_every_nth_node;  /* 1 */
  int32_t optimizer_skip_step;      /* 1 */
  int32_t use_icp;                  /* 0 */
  int32_t emm__skip_step;           /* 8 */
  int32_t have_odometry_frame;      /* 0: "odom_frame_name" is empty */
  uint32_t seed;                    /* 0 */
  double min_translation_meter;     /* 0.0 */
  double min_rotation_degree;       /* 0.0 */
  double max_translation_meter;     /* 1e10 */
  double max_rotation_degree;       /* 360 */
  double optimizer_iterations;      /* 0.01 */
  double observability_threshold;   /* -0.6 */
  double init_base_pose[16];        /* identity; column-major */
} rgbdfe_slam_params;
typedef struct rgbdfe_slam_step {
  int32_t status;                   /* RGBDFE_SLAM_* */
  int32_t id;                       /* the graph id assigned, or -1 */
  int32_t found;                    /* nodeComparisons' return value */
  int32_t initial_id;               /* the node of the initial comparison, or -1 */
  int32_t initial_verdict;
  int32_t n_candidates;
  int32_t candidates[RGBDFE_SLAM_MAX_CANDIDATES];
  uint8_t verdicts[RGBDFE_SLAM_MAX_CANDIDATES];
  int32_t best_id1, best_id2, best_n_inl;   /* curr_best_result_ after the step (-1, -1, 0: an empty result) */
  int32_t predecessor_matched;
  int32_t edge_to_keyframe;
  int32_t keyframe_added;           /* or -1 */
  int32_t cleared_first, cleared_last;  /* the ids addKeyframe cleared (inclusive), or -1, -1 */
  int32_t released_slot;            /* REPLACED_FIRST: the slot of the node that was replaced, else -1 */
  int32_t constant_position;        /* RGBDFE_SLAM_CONSTANT_* */
  int32_t cloud_released;           /* id % create_cloud_every_nth_node != 0 */
  int32_t has_broadcast_pose;
  int32_t optimize_due, optimized, lm_iterations;
  int32_t sequential_edges, loop_closure_edges;   /* the counters after the step */
  int32_t stats_launches;           /* launches of the inlier-statistics kernel (0 or 1) */
  double motion_estimate[16];       /* curr_motion_estimate: the new vertex's estimate when it was last written */
  double broadcast_pose[16];        /* MOTION_OUT_OF_BOUNDS: previous * incremental */
  double chi2;                      /* after the optimisation */
  double seconds[4];                /* candidates, comparisons, decisions, optimisation */
} rgbdfe_slam_step;
typedef struct rgbdfe_slam rgbdfe_slam;
void rgbdfe_slam_default_params(rgbdfe_slam_params* p);
int rgbdfe_slam_create(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, const rgbdfe_slam_params* p, rgbdfe_slam** out);
void rgbdfe_slam_destroy(rgbdfe_slam* s);
int rgbdfe_slam_reset(rgbdfe_slam* s);
int rgbdfe_slam_set_rand(rgbdfe_slam* s, rgbdfe_rand_fn rand_fn, void* rand_state);
int rgbdfe_slam_add_node(rgbdfe_slam* s, int32_t slot, int64_t stamp_sec, int32_t stamp_nsec, rgbdfe_slam_step* out);
int rgbdfe_slam_begin(rgbdfe_slam* s, int32_t slot, int32_t n_rows, int64_t stamp_sec, int32_t stamp_nsec, int32_t* ids,
                      int32_t capacity, int32_t* n_ids, rgbdfe_slam_step* step);
int rgbdfe_slam_feed(rgbdfe_slam* s, const rgbdfe_compact_result* results, const uint8_t* flags, int32_t n, int32_t* ids,
                     int32_t capacity, int32_t* n_ids, rgbdfe_slam_step* step);
int rgbdfe_slam_node_count(const rgbdfe_slam* s);                 /* graph_.size() */
int rgbdfe_slam_slot_of(const rgbdfe_slam* s, int32_t id);        /* the slot, -1: released, < -1: an error status */
int rgbdfe_slam_valid_tf(const rgbdfe_slam* s, int32_t id);       /* 0 / 1, or an error status */
int rgbdfe_slam_keyframes(const rgbdfe_slam* s, int32_t* ids, int32_t capacity, int32_t* n_out);
int rgbdfe_sizeof_slam_step(void);
int rgbdfe_update_inlier_features(rgbdfe_ctx* ctx, const void* d_records, const int32_t* query_ids, const int32_t* train_ids,
                                  const uint8_t* accept, int32_t n, int32_t* launched);
int rgbdfe_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, uint8_t* out, int32_t capacity);
int rgbdfe_pose_graph_add_keyframe(rgbdfe_pose_graph* g, int32_t node_id);
int rgbdfe_pose_graph_clear(rgbdfe_pose_graph* g);

/* ---- session files: save and resume nodes, pose graph and SLAM state --------------------------------------------------
 * A run that is saved, torn down, loaded into fresh objects and continued produces, byte for byte, what the uninterrupted
 * run produces.  Everything below is little-endian; doubles and floats travel as their bytes (NaN payloads, -0.0 and
 * denormals survive); "zeros to 8" pads with zero bytes up to the next multiple of 8 counted from the start of the string,
 * payload or file.  CRC-32 is zlib's (zlib.crc32).  Nothing depends on time, pointers, slot numbers or hash-map order:
 * the same state gives the same bytes.
 *
 * The two byte strings (no device, no context: both work on objects created with ctx == NULL).  Envelope: 8 bytes magic,
 * u32 version 1, u32 CRC-32 of the bytes [16, length), u64 length of the whole string (a multiple of 8), then the body.
 *   Two-call pattern: *bytes is the length; capacity below it is RGBDFE_ERR_CAPACITY with nothing written.  A failed call
 *   leaves its cause with rgbdfe_last_error(NULL) (per calling thread), and with the context's where the object has one.
 * rgbdfe_pose_graph_serialize / _deserialize, magic "RGBDFEPG".  Body:
 *     i32 strategy, i32 earliest_loop_closure_node, u32 n_nodes, u32 n_edges, u32 n_keyframes, u32 n_links,
 *     u32 n_extra_vertices, u32 0
 *     nodes in ascending id, 112 bytes each: i32 node id, i32 vertex id, u8 matchable, u8 fixed, 6 x u8 0, 12 x f64 estimate
 *       (rotation row-major, then translation: rgbdfe_pose_graph_get_estimate's matrix is column-major)
 *     edges in insertion order, 400 bytes each: i32 id1, i32 id2, u8 active, 7 x u8 0, 12 x f64 measurement (as an estimate),
 *       36 x f64 information row-major
 *     keyframes: n x i32;  links: n x (i32 u, i32 v), u < v, ascending: edges without a measurement
 *       (rgbdfe_pose_graph_add_edge), as vertex ids;  extra vertices: n x i32 ascending: camera vertices that are no node's
 *       vertex id;  zeros to 8.
 *   camera_vertices and the adjacency are rebuilt from those.  The target of a deserialise must be empty (a new graph, or
 *   rgbdfe_pose_graph_clear), else RGBDFE_ERR_INVALID_ARG; it takes the stored strategy, and the optimiser's device buffers
 *   are dropped, so that no plan of an earlier graph survives.  A string that is truncated, extended or changed in any byte
 *   is refused (RGBDFE_ERR_INVALID_ARG) and the graph stays empty.
 * rgbdfe_slam_serialize / _deserialize, magic "RGBDFESM".  Body:
 *     the parameters in the order of rgbdfe_slam_params: 13 x i32 (min_matches .. have_odometry_frame), u32 seed, 6 x f64
 *     (min_translation_meter .. observability_threshold), 16 x f64 init_base_pose
 *     u32 n_nodes, u32 n_keyframes, i32 next_seq_id, u32 calls (steps begun: the library's own generator draws from seed +
 *     calls), i32 sequential_edges, i32 loop_closure_edges, i32 best_id1, i32 best_id2, i32 best_n_inl (curr_best_result_), u32 0
 *     per graph id: n x i32 slot (-1: released), n x i32 rows, n x i64 stamp seconds, n x i32 stamp nanoseconds, n x u8
 *     valid_tf, zeros to 4, keyframes n x i32, zeros to 8.
 *   Serialising while a step is in flight (between rgbdfe_slam_begin and the rgbdfe_slam_feed that finishes it) is refused
 *   with RGBDFE_ERR_INVALID_ARG.  The target of a deserialise must be fresh or reset (rgbdfe_slam_reset) and must have been
 *   created with the stored parameters: otherwise RGBDFE_ERR_INVALID_ARG, the message naming the first field that differs.
 *   Its graph is not touched: deserialise that one too.  A generator given with rgbdfe_slam_set_rand and its state stay the
 *   caller's: neither is stored, and a resumed run draws what the uninterrupted one draws only if the caller restores them.
 * rgbdfe_pose_graph_node_ids: the graph's node ids in ascending order (capacity below *n_out: RGBDFE_ERR_CAPACITY).
 *
 * rgbdfe_session_save(ctx, slam, graph, flags, path) / rgbdfe_session_load(ctx, slam, graph, path); slam / graph may be NULL.
 * The file: a 32-byte header -- the 8 bytes "RGBDFESS", u32 version 1, u32 flags, u64 file length, u64 0 -- then chunks of
 * (4-byte tag, u32 CRC-32 of the payload, u64 payload length, payload, zeros to 8) in the fixed order
 *   "CONF"  i32 max_keypoints of the context, i32 rgbdfe_abi_version(), u32 node kinds present (bit k: kind k), u32 0
 *   "DETE"  i32 detector type (RGBDFE_DETECTOR_*), i32 detector max_keypoints, i32 grid_resolution, i32 adjuster_max_iterations,
 *           i32 feature_min_depth (0 / 1), i32 n_cells, n_cells x f64 thresholds
 *   "NODE"  u32 n_nodes, u32 0, then n x i32 each: ids (ascending), kinds, rows, has_keypoints (0 / 1); then for every kind
 *           present, in the order 0 (ORB), 1 (SIFT), 2 (float), that kind's nodes in ascending id packed as
 *           rgbdfe_download_nodes packs them: desc (32 bytes per row for kind 0, else 128 x f32), zeros to 8, xyz1 (4 x f32
 *           per row), zeros to 8, kp_xy (2 x f32 per row; zeros for a node without keypoints), zeros to 8, stats (1 byte per
 *           row), zeros to 8
 *   "CLOU"  only with RGBDFE_SESSION_CLOUDS in flags: u32 n_clouds, u32 0, then per cloud in ascending node id: i32 id,
 *           i32 rows, i32 cols, i32 cloud_skip, f32 fx, fy, cx, cy, rows x cols x 4 x f32 points (rgbdfe_download_node_cloud's)
 *   "GRPH"  the graph's byte string, when a graph was passed;  "SLAM"  the machine's, when a slam was passed
 *   "END "  empty.
 * Saving: written to path + ".tmp", then renamed; if anything fails nothing stays under either name.  Refused
 *   (RGBDFE_ERR_INVALID_ARG, "busy") while a host job (rgbdfe_submit_pair_list_host) or a step is pending.  Single-device
 *   contexts.  The OctoMap keeps its own .ot files and is not part of a session.
 * Loading: the whole file is validated before anything changes -- magic, version, length, every CRC, every count against its
 *   chunk's length, then capacity (rows above the context's max_keypoints, or more nodes than free slots:
 *   RGBDFE_ERR_CAPACITY), then the id rule (an id of the file that is already resident, with or without a cloud, a graph
 *   or slam target that is not empty, a slam whose parameters differ: RGBDFE_ERR_INVALID_ARG; a GRPH / SLAM chunk without an
 *   object to take it is validated and skipped -- a viewer loads the nodes and the graph alone); every other defect is RGBDFE_ERR_INVALID_ARG with the cause in rgbdfe_last_error.  Then the nodes
 *   go in through the upload paths (every derived form -- fp4 operands, bf16, flags -- is rebuilt by the code that builds it
 *   for an upload), keypoints, counters, clouds, the detector's type, configuration and thresholds, feature_min_depth, the
 *   graph and the machine.  RANSAC and matcher parameters (rgbdfe_set_params) are the caller's to set again.
 * rgbdfe_restore_node_cloud: a resident cloud from the points rgbdfe_download_node_cloud returns and the fields
 *   rgbdfe_node_cloud_info reports: indistinguishable from the cloud that rgbdfe_upload_node_cloud or the sensor path built
 *   (the depth plane behind the points is their z; the measurement model's samples are rebuilt on first use). */
#define RGBDFE_SESSION_CLOUDS 1
int rgbdfe_pose_graph_serialize(const rgbdfe_pose_graph* g, uint8_t* out, int64_t capacity, int64_t* bytes);
int rgbdfe_pose_graph_deserialize(rgbdfe_pose_graph* g, const uint8_t* in, int64_t bytes);
int rgbdfe_pose_graph_node_ids(const rgbdfe_pose_graph* g, int32_t* ids, int32_t capacity, int32_t* n_out);
int rgbdfe_slam_serialize(rgbdfe_slam* s, uint8_t* out, int64_t capacity, int64_t* bytes);
int rgbdfe_slam_deserialize(rgbdfe_slam* s, const uint8_t* in, int64_t bytes);
int rgbdfe_session_save(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, uint32_t flags, const char* path);
int rgbdfe_session_load(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, const char* path);
int rgbdfe_restore_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, const float* points, int32_t rows, int32_t cols, double fx,
                              double fy, double cx, double cy, int32_t cloud_skip);
/* out8 = { rows, cols, cloud_skip, fx, fy, cx, cy, 0 } of a node's resident cloud (the intrinsics as the floats they are
 * kept as) */
int rgbdfe_node_cloud_info(rgbdfe_ctx* ctx, int32_t node_id, double* out8);

/* ---- map files: PCD and PLY of the assembled map and of node clouds ------------------------------------------------------
 * GraphManager::saveAllCloudsToFile (graph_mgr_io.cpp:502-582) and saveIndividualCloudsToFile (:330-433): what a batch run
 * ends with.  The two file formats are restated from PCL 1.7's writers, NOT pinned on PCL's compiled code (PCL is on no
 * machine this library is built on): the statements below are the contract.  Everything is little-endian.
 *
 * PCD -- pcl::io::savePCDFile(name, cloud, true) of a PointXYZRGB cloud.  The header is exactly these lines, each ended by
 *   '\n', followed by the data with no padding:
 *       # .PCD v0.7 - Point Cloud Data file format
 *       VERSION 0.7
 *       FIELDS x y z rgb
 *       SIZE 4 4 4 4
 *       TYPE F F F F
 *       COUNT 1 1 1 1
 *       WIDTH <w>
 *       HEIGHT <h>
 *       VIEWPOINT <ox> <oy> <oz> <qw> <qx> <qy> <qz>
 *       POINTS <w*h>
 *       DATA binary
 *   The data is w*h rows of 16 bytes: this library's cloud row (x, y, z, rgb word) bit for bit, NaN payloads included.  Each
 *   viewpoint number is the float as a C++ stream prints it by default: printf("%g") of the value.  The aggregate map has
 *   WIDTH n, HEIGHT 1, VIEWPOINT 0 0 0 1 0 0 0.
 * PLY -- pcl::io::savePLYFileBinary.  The header is "ply", "format binary_little_endian 1.0", "comment PCL generated",
 *   "element vertex <n>", "property float x" / y / z, "property uchar red" / green / blue, "element camera 1", then one
 *   "property float" line each for view_px view_py view_pz x_axisx x_axisy x_axisz y_axisx y_axisy y_axisz z_axisx z_axisy
 *   z_axisz focal scalex scaley centerx centery, "property int viewportx", "property int viewporty", "property float k1",
 *   "property float k2", "end_header", each line ended by '\n'.  Then n vertex records of 15 bytes: x, y, z as float bits, then
 *   r, g, b = bits 23-16, 15-8 and 7-0 of the rgb word.  Every row of the cloud is a vertex, raster mode's NaN rows included.
 *   The camera record (84 bytes) follows: origin 0 0 0, the identity rotation row by row, five zero floats, viewportx = width
 *   and viewporty = height as int32, two zero floats.
 * Name rule (the reference's): a path ending in ".ply" in any letter case gives PLY; any other path gives PCD, and ".pcd" is
 *   appended unless the path already ends in it in any case (rgbdfe_cloud_file_path applies the rule without writing).
 * Deviations from the reference: an aggregate of zero points creates no file and returns RGBDFE_OK with a count of 0 (PCL
 *   throws); 2^31 points or more is RGBDFE_ERR_CAPACITY; a path that cannot be opened is RGBDFE_ERR_INVALID_ARG; a failed write
 *   is RGBDFE_ERR_INTERNAL and the file is removed (as rgbdfe_octomap_write); rgbdfe_save_node_clouds leaves the resident
 *   cloud as it is (the reference transforms it in place, so a second save there moves it twice).
 *
 * rgbdfe_save_map is saveAllCloudsToFile: node_ids / transforms / maximum_depth / preserve_raster mean exactly what they
 *   mean for rgbdfe_assemble_map, and the file's data section is, byte for byte, the rows that call returns (their 15-byte
 *   repacking for PLY).  The map is never whole anywhere: a count and a scan over the list give the total and every node's
 *   first row (the header is written from them), then the list is cut into groups of consecutive nodes whose clouds sum to
 *   at most chunk_points points (0: 2^20; values below 64 count as 64; a larger cloud is a group of its own), each group is
 *   assembled into one of two device buffers, its file bytes land in one of two page-locked slots (PLY: packed by
 *   cloud_pack_ply_kernel straight into the slot; PCD: an asynchronous copy), and a writer thread writes slot g while group
 *   g + 1 runs.  The file's bytes do not depend on chunk_points.  path_written (may be NULL) receives the path after the
 *   name rule, NUL-terminated (path_capacity too small: RGBDFE_ERR_CAPACITY before anything happens).  stats (may be NULL):
 *   device_scratch_bytes = pinned_bytes = 2 x 16 x the largest group's points <= 2 x 16 x max(chunk_points, largest listed
 *   cloud); table_bytes = the node and tile tables beside them in the context's scratch.
 * rgbdfe_save_node_clouds is saveIndividualCloudsToFile without its ground-truth branch: every listed node with a non-empty
 *   cloud gets <basename>_%04d.pcd and <basename>_%04d.txt, numbered by graph_ids[k] (NULL: node_ids[k]).  poses: n
 *   column-major 4x4 doubles (the vertex estimates; tf is the caller's).  transform_individual_clouds == 0: the resident
 *   cloud untouched, organised (WIDTH cols, HEIGHT rows); its viewpoint is the pose: the translation cast to float, the
 *   rotation through the matrix -> quaternion conversion of rgbdfe_pose_graph_write_trajectory, cast to float.  != 0:
 *   pcl::transformPointCloud with the pose cast to float (== raster-mode assembly of the node alone with the clip off), and
 *   the reference's quirk: Quaternionf(0,0,0,1) is (w, x, y, z), so the viewpoint is "0 0 0 0 0 0 1" and the exported
 *   rotation is diag(-1, -1, 1).  The .txt holds three rows "r0 r1 r2 t " of Eigen's Quaternionf::toRotationMatrix() of the
 *   float quaternion (restated) and the float origin, then "0 0 0 1" and a newline, every number as printf("%g").
 *   An unknown node is RGBDFE_ERR_UNKNOWN_NODE before anything is written; *n_written counts the nodes written.
 * Host-only calls (no device, no context; the cause of a failure: rgbdfe_last_error(NULL)):
 *   rgbdfe_save_cloud_file writes width x height rows held in host memory (viewpoint: 7 floats or NULL for the aggregate's;
 *     PLY ignores it and stores width / height as the viewport).
 *   rgbdfe_cloud_file_info reads a file's header; rgbdfe_load_cloud_file also returns its rows as 4-float rows (a PLY
 *     vertex's rgb word has a zero top byte); capacity below the file's points is RGBDFE_ERR_CAPACITY with *info filled.
 *     Both read exactly the two layouts above with a data section of exactly the promised length: other field lists, ascii
 *     or compressed data, big-endian, counts that are not decimal numbers below 2^31, a shorter or longer file are
 *     RGBDFE_ERR_INVALID_ARG.  Nothing is read past the file. */
#define RGBDFE_CLOUD_FILE_PCD 0
#define RGBDFE_CLOUD_FILE_PLY 1
typedef struct rgbdfe_map_file_stats {
  int64_t points;                /* rows of the file */
  int64_t bytes_written;         /* the whole file */
  int32_t format;                /* RGBDFE_CLOUD_FILE_* */
  int32_t groups;
  int64_t device_scratch_bytes;  /* the two group buffers */
  int64_t pinned_bytes;          /* the two page-locked slots */
  int64_t table_bytes;           /* node table, tile tables, counts */
} rgbdfe_map_file_stats;
typedef struct rgbdfe_cloud_file_header {
  int32_t format;                /* RGBDFE_CLOUD_FILE_* */
  int32_t width, height;         /* PLY: the camera record's viewport */
  int32_t reserved;
  int64_t points, header_bytes, data_bytes;
  float viewpoint[7];            /* ox oy oz qw qx qy qz (PLY: 0 0 0 1 0 0 0) */
  float reserved2;
} rgbdfe_cloud_file_header;
int rgbdfe_save_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth,
                    int32_t preserve_raster, const char* path, int64_t chunk_points, char* path_written, int64_t path_capacity,
                    rgbdfe_map_file_stats* stats);
int rgbdfe_save_node_clouds(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const int32_t* graph_ids,
                            const double* poses, int32_t transform_individual_clouds, const char* basename, int32_t* n_written);
int rgbdfe_save_cloud_file(const float* points, int32_t width, int32_t height, const float* viewpoint, int32_t format,
                           const char* path);
int rgbdfe_cloud_file_info(const char* path, rgbdfe_cloud_file_header* info);
int rgbdfe_load_cloud_file(const char* path, float* out, int64_t capacity, rgbdfe_cloud_file_header* info);
int rgbdfe_cloud_file_path(const char* path, char* path_out, int64_t capacity, int32_t* format);

/* ---- measurement --------------------------------------------------------- */
/* When enabled, every launch of the dominant kernels is bracketed by HIP events on the
 * stream it runs on; totals are read back with rgbdfe_get_kernel_time. */
enum { RGBDFE_KERNEL_HAMMING = 0, RGBDFE_KERNEL_RANSAC = 1, RGBDFE_KERNEL_SIFT_DOT = 2,
       RGBDFE_KERNEL_SIFT_FINISH = 3, RGBDFE_KERNEL_EMM = 4, RGBDFE_KERNEL_ICP_NN = 5 /* `pairs` counts job-iterations */,
       RGBDFE_KERNEL_COUNT = 6 };
int rgbdfe_set_profiling(rgbdfe_ctx* ctx, int enable);
int rgbdfe_get_kernel_time(rgbdfe_ctx* ctx, int which, double* total_ms, int64_t* launches,
                           int64_t* pairs);
int rgbdfe_reset_kernel_time(rgbdfe_ctx* ctx);
/* The hipGraph cache of the ORB pair path (one executable graph per distinct batch shape: pair count, Hamming launch
 * geometry, output buffer): out[0..n_out) = { captures, graph launches, misses (graphable batches whose shape was not
 * cached), batches issued as plain launches because the shapes kept missing, captures another thread invalidated,
 * cached graphs that failed to launch, graphs cached now, graphs enabled (RGBDFE_GRAPHS) }; summed over the devices
 * of a multi handle. */
#define RGBDFE_GRAPH_STATS 8
int rgbdfe_graph_stats(rgbdfe_ctx* ctx, int64_t* out, int32_t n_out);
/* Cached hipGraphs for the launch chain of ORB pair batches (one hipGraphLaunch instead of ~12 enqueues per batch: 2-3 %
 * on the 4000-pair headline, 20 % of the submission cost of a multi-device handle).  OFF by default: while a capture is
 * open, hipDeviceSynchronize() (torch.cuda.synchronize(), a synchronous hipMemcpy on the NULL stream ...) on any OTHER
 * thread of the process fails with hipErrorStreamCaptureUnsupported, and the library cannot know what the host
 * application's threads do.  Turn it on when every thread that calls HIP is yours (bench.py does).  RGBDFE_GRAPHS=1 / 0 in
 * the environment sets the initial value of new contexts. */
int rgbdfe_set_graph_capture(rgbdfe_ctx* ctx, int enable);

/* ABI self-description (lets bindings verify struct layout) */
int rgbdfe_sizeof_match_result(void);
int rgbdfe_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RGBDFE_H */
