// rgbdfe_host.h -- what the host-side translation units of librgbdfe.so share: the context (node store, lanes, graph cache,
// staging), the batch machinery's entry points (api_batches.hip), the single-device implementation of every entry point
// (namespace impl: api_context / api_pairs / api_detect / api_frame / api_map / api_voxel / api_octomap.hip) and the multi-device group (api_group.hip).
// rgbdfe_api.hip holds the extern "C" layer only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "device_layout.h"
#include "fast_host.h"
#include "orb_host.h"
#include "sift_extract.h"
#include "rgbdfe_internal.h"
#include "sensor_host.h"

using namespace rgbdfe;

namespace rgbdfe_host {

// a frame's structured point cloud, resident for the environment measurement model
struct CloudEntry {
  float4* d = nullptr;  // ch x cw points, followed by the ch x cw depth plane (z only) the EMM gathers from
  int ch = 0, cw = 0;   // 1 x n (n >= 0) behind rgbdfe_reduce_node_cloud: unstructured
  float fx = 0, fy = 0, cx = 0, cy = 0;  // as getCameraIntrinsics assigns them (double -> float)
  int cloud_skip = 1;                    // cloud_creation_skip_step the cloud was built with
  float4* d_samples = nullptr;           // the points the EMM visits for emm skip step `samples_skip`, dense
  int samples_skip = 0;                  // 0: not built (invalidated by a re-upload)
};

// smallest double q with 0.5 * (1 + erf(q)) >= target under the host's libm (bisection)
inline double erf_boundary(double target) {
  double lo = -8.0, hi = 8.0;
  for (;;) {
    const double mid = lo + (hi - lo) * 0.5;
    if (!(mid > lo && mid < hi)) break;
    if (0.5 * (1 + std::erf(mid)) >= target) hi = mid; else lo = mid;
  }
  return hi;
}

// smallest double d with d / denom >= q (denom > 0): the exact pre-image of the test `d / denom < q`
inline double division_boundary(double q, double denom) {
  double c = q * denom;
  while (c / denom >= q) c = std::nextafter(c, -INFINITY);
  while (c / denom < q) c = std::nextafter(c, INFINITY);
  return c;
}

struct NodeEntry {
  uint32_t slot;
  uint32_t n;
  uint32_t kind;  // 0 = ORB (32-byte binary descriptors), 1 = SIFT (128 floats), 2 = float descriptors (FLANN branch)
  uint32_t flags = 0;  // bit 0 (SIFT): every row's quantised squared norm is < 2^19 (sift_match.hip's fast keys)
                       // bit 1: the slot holds THIS node's KeyPoint.pt (rgbdfe_upload_node_keypoints after the latest upload)
};
constexpr uint32_t kNodeHasKeypoints = 2u;

inline uint32_t mix32_host(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// RNG stream id of a pair: depends on the two node ids only, so a pair yields the same
// result in any batch, on any rank.
inline uint32_t pair_uid(int32_t qid, int32_t tid) {
  return mix32_host((uint32_t)qid * 0x9E3779B1u ^ ((uint32_t)tid + 0x7F4A7C15u));
}

}  // namespace rgbdfe_host
using namespace rgbdfe_host;

namespace rgbdfe_host {

class TaskPool {  // a few persistent worker threads for pure-CPU jobs
 public:
  explicit TaskPool(int n) {
    for (int i = 0; i < n; ++i) th_.emplace_back([this] { run(); });
  }
  ~TaskPool() {
    { std::lock_guard<std::mutex> l(m_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : th_) if (t.joinable()) t.join();
  }
  void submit(std::function<void()> f) {
    { std::lock_guard<std::mutex> l(m_); q_.push_back(std::move(f)); ++pending_; }
    cv_.notify_one();
  }
  void wait_all() {
    std::unique_lock<std::mutex> l(m_);
    done_.wait(l, [&] { return pending_ == 0; });
  }
  int size() const { return (int)th_.size(); }
 private:
  void run() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || !q_.empty(); });
        if (stop_ && q_.empty()) return;
        f = std::move(q_.front());
        q_.erase(q_.begin());
      }
      try { f(); } catch (...) { failed_ = true; }
      { std::lock_guard<std::mutex> l(m_); --pending_; }
      done_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::vector<std::function<void()>> q_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  int pending_ = 0;
  bool stop_ = false;
 public:
  bool failed_ = false;
};

}  // namespace rgbdfe_host
using namespace rgbdfe_host;

// A stream that must run BESIDE the context's main stream gets another priority class: the runtime maps the streams of one
// priority onto a small pool of hardware queues (4 by default), and two streams that land on the same queue execute one
// after the other -- which two do depends on every stream the process created before (measured: the SIFT batch's second chunk
// stream shared the main stream's queue in a process that had run the ORB batch before, 0.24 instead of 0.18 ms per frame).
// Priority classes have their own queues.  which: -1 = the lowest, +1 = the highest priority the device offers.
inline hipError_t create_side_stream(hipStream_t* s, int which) {
  int lo = 0, hi = 0;   // hipDeviceGetStreamPriorityRange: numerically lower = higher priority
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || lo == hi) { (void)hipGetLastError(); return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, which > 0 ? hi : lo);
}

struct rgbdfe_ctx;
struct rgbdfe_slam;
struct rgbdfe_pose_graph;
namespace rgbdfe_host {
int fail(rgbdfe_ctx* ctx, int code, const std::string& msg);

// device memory that lives for one call (or, as a member, with its owner)
struct DeviceBuffer {
  void* p = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { if (p) (void)hipFree(p); }
  int alloc(rgbdfe_ctx* ctx, size_t bytes, const char* msg) {
    if (hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, msg);
    }
    return RGBDFE_OK;
  }
};

// a buffer that only grows: ensure() frees and allocates larger when `bytes` exceeds what it holds.  The owner frees p.
struct GrowBuffer {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(rgbdfe_ctx* ctx, size_t want, const char* msg) {
    if (want <= bytes) return RGBDFE_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, msg);
    }
    bytes = want;
    return RGBDFE_OK;
  }
};
}  // namespace rgbdfe_host

struct rgbdfe_ctx {
  rgbdfe_config cfg{};
  std::mutex mu;
  std::mutex err_mu;        // guards last_error only (fail() may run before `mu` is taken)
  std::string last_error;
  // multi-device group handle (rgbdfe_create_multi): the per-device contexts and one host thread per device
  struct Group* group = nullptr;
  hipStream_t stream = nullptr;
  // slabs
  uint32_t* d_desc = nullptr;  // max_nodes x max_kp x 8 dwords (+ pad rows)
  float4* d_xyz = nullptr;     // max_nodes x max_kp
  uint32_t* d_desc4 = nullptr; // max_nodes x max_kp x 32 dwords: every descriptor bit as an fp4 (+-1) operand nibble, in
                               // MFMA fragment order per tile of 32 rows (hamming_mfma.hip)
  float* d_kp2d = nullptr;     // max_nodes x max_kp x 2: KeyPoint.pt (allocated with the first rgbdfe_upload_node_keypoints)
  uint8_t* d_feat_stats = nullptr;  // max_nodes x feat_stats_stride(): feature_matching_stats_ (api_slam.hip), allocated zeroed
                                    // with the first call that reads or writes it; until then every counter is 0 by definition
  size_t feat_stats_stride() const { return ((size_t)cfg.max_keypoints + 3u) & ~(size_t)3u; }
  hipStream_t orb_upload_stream = nullptr;  // rgbdfe_detect_describe_batch: uploads of frame k+1 beside frame k
  hipStream_t orb_compute_stream = nullptr; // ... and frame k's description beside frame k+1's detection
  hipEvent_t orb_upload_done[OrbWorkspace::kSets] = {};
  hipEvent_t orb_describe_done[OrbWorkspace::kSets] = {};  // frame f's description has left its image set
  bool feature_min_depth = false;  // "use_feature_min_depth" (parameter_server.cpp:90): rgbdfe_set_feature_min_depth
  bool sift_fast = true;       // sift_match.hip's float keys where a pair qualifies (RGBDFE_SIFT_FAST_KEYS=0: never)
  int hamming_mode = RGBDFE_HAMMING_MODE_DEFAULT;   // rgbdfe.h: 0 = popcount kernel (hamming_nn.hip), 1 / 2 / 3 / 4 = fp4 MFMA kernels (hamming_mfma.hip)
  int hamming_wide = -1;       // mode 3: -1 = 256- or 512-query blocks per batch (hamming_mfma_geometry), 0 / 1 = always that one
                               // (RGBDFE_HAMMING_WIDE at rgbdfe_create; rgbdfe_set_hamming_mode(3) sets 0, mode 4 is always wide)
  int hamming_wide_last = -1;  // the latest Hamming launch: 1 = 512-query blocks, 0 = any other kernel, -1 = none yet
  int hamming_shape = 0;       // MFMA tile of mode 3's 512-query blocks: 0 = the library's choice, 16 = 16x16x128, 32 = 32x32x64
                               // (RGBDFE_HAMMING_SHAPE at rgbdfe_create, rgbdfe_set_hamming_shape; mode 4 is always 32)
  int hamming_shape_last = -1; // the latest Hamming launch: 16 / 32 = its MFMA tile, 0 = the popcount kernel, -1 = none yet
  // Batches run on kLanes internal HIP streams ("lanes"), each with its own keys / results
  // staging, so that batch k+1's Hamming kernel fills the SIMDs that batch k's RANSAC tail
  // leaves idle.  The pair lists go through a ring of pinned buffers so the host can prepare
  // batch k+1 while batch k runs.
#ifndef RGBDFE_LANES
#define RGBDFE_LANES 2  // measured on the bench: 2 lanes 1.50 ms per step, 3 lanes 1.71, 4 lanes 1.50
#endif
  static constexpr int kLanes = RGBDFE_LANES;
  static constexpr int kRing = 2 * RGBDFE_LANES;
  struct Lane {
    hipStream_t stream = nullptr;
    IterRec* d_recs = nullptr;              // record / replay: per pair x RANSAC iteration outcome records
    size_t recs_capacity = 0;               // in records
    WalkState* d_walk = nullptr;            // record / replay: per pair progress (max_pairs)
    PairPrep* d_prep = nullptr;             // selected matches of every pair of the batch (max_pairs)
    double* d_ec = nullptr;                 // error pool of select+RANSAC: one region per pair of a piece
    size_t ec_regions = 0;
    uint32_t* d_keys = nullptr;             // max_pairs x max_kp
    rgbdfe_match_result* d_results = nullptr;  // staging for the host-output entry points
    // SIFT scratch (allocated with the first SIFT node)
    uint32_t* d_row_part = nullptr;   // max_pairs x max_kp x 3
    uint32_t* d_col_part = nullptr;   // max_pairs x max_kp x 3 (per train row)
    uint2* d_col_blocks = nullptr;    // max_pairs x sift_col_block_bytes_per_pair() (one-pass matcher: per-row-block column partials)
    uint16_t* d_sm_q = nullptr;       // max_pairs x max_kp
    uint16_t* d_sm_t = nullptr;
    float* d_sm_d = nullptr;
    int32_t* d_sm_n = nullptr;        // max_pairs
    float* d_all_dist = nullptr;      // max_pairs x RGBDFE_MAX_MATCHES
  };
  uint16_t* d_sift_bf16 = nullptr;  // max_nodes x max_kp x 128 (u8-quantised values as bf16)
  float* d_sift_f32 = nullptr;      // max_nodes x max_kp x 128 (raw descriptors)
  bool sift_ready = false;
  struct Slot {
    PairWork* h_work = nullptr;  // pinned
    PairWork* d_work = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false;
    bool failed = false;         // the batch with `ticket` did not launch completely
    int64_t ticket = 0;
  };
  Lane lanes[kLanes];
  Slot ring[kRing];
  // Batches of at most latency_pairs ORB pairs take the record / replay path (select_ransac.hip): the refinement
  // work of one pair is spread over ceil(ransac_iterations / latency_chunk_iters) waves.  0 disables it.
  // Measured (tools/bench_batch_sweep.py, bench.py --ransac-path): record / replay wins up to ~2000 pairs per batch
  // (uniform short waves fill the chip and have no straggler tail), the one-wave kernel above (it skips the
  // iterations the reference's early exits skip, and overlapped batches hide its tail).
  int32_t latency_pairs = INT32_MAX;  // record / replay for every batch size (rgbdfe_set_latency_mode)
  int32_t latency_chunk_iters = 0;  // 0 = automatic: 4 iterations per wave up to 64 pairs, 7 up to 640, 14 up to 1280, 28 above
  int64_t next_ticket = 1;
  // The launch chain of an ORB batch (pair-list upload, Hamming, pair_prep, recording / walk launches, result launch:
  // ~12 enqueues) as a hipGraph: captured once per distinct batch shape, then ONE hipGraphLaunch per batch -- what keeps
  // a single submitting thread ahead of several devices (rgbdfe_create_multi) and shortens the live-SLAM call.
  // Everything a kernel argument or a grid depends on is part of the key -- and nothing else: node sizes count only
  // through the Hamming stage's launch geometry (HammingGeometry), so frames with different keypoint counts share graphs.
  struct GraphKey {
    int32_t n; uint32_t qblocks, tsplit; int32_t slot, latency, chunk, hamming_mode, n_phases; int32_t ends[4];
    RansacConst rc;
    void* d_out; void* d_recs; void* d_ec; void* d_walk; void* d_keys;
  };
  struct GraphEntry { GraphKey key; hipGraph_t graph; hipGraphExec_t exec; uint64_t used; };
  std::vector<GraphEntry> graphs;
  uint64_t graph_clock = 0;
  int64_t graph_launches = 0, graph_captures = 0;
  int64_t graph_misses = 0;          // graphable batches whose shape was not cached
  int64_t graph_plain_batches = 0;   // of those: issued as plain launches without a capture attempt
  int64_t graph_launch_failures = 0; // cached executable graphs that failed to launch (dropped)
  int32_t graph_miss_run = 0;        // misses since the last hit
  static constexpr int32_t kGraphMissRun = 8, kGraphRetry = 16;
  // Off by default (round 4): while a capture is open, a device-wide synchronisation on ANY thread of the process fails with
  // hipErrorStreamCaptureUnsupported -- relaxed mode spares other threads' allocations and copies, not that -- and a
  // drop-in library may not make its host application's unrelated HIP calls fail (rgbdslam is a multi-threaded Qt / ROS
  // process).  A caller that owns every thread touching HIP turns it on: rgbdfe_set_graph_capture / RGBDFE_GRAPHS=1.
  bool use_graphs = false;
  hipStream_t capture_stream = nullptr;  // graphs are captured here, never on a stream other threads may wait on
  long graph_capture_failures = 0;       // captures another thread's HIP call invalidated (the batch then ran as plain launches)
  uint8_t* upload_stage = nullptr; size_t upload_stage_bytes = 0;  // pinned staging of rgbdfe_upload_nodes
  hipEvent_t ev_in = nullptr;  // orders a caller's stream before a lane
  hipEvent_t nodes_ready = nullptr;  // recorded behind the latest rgbdfe_upload_node_device copies; every batch waits for it
  hipEvent_t nodes_ready_ev = nullptr;  // (storage; nodes_ready points here once the first such upload happened)
  rgbdfe_match_result* h_results = nullptr;  // pinned staging of the synchronous host-output entry points
  // rgbdfe_submit_pair_list_host / rgbdfe_wait_host: one job per lane -- the results of the batch on lane li go device ->
  // pinned stage li (or straight into the caller's buffer when that is pinned) behind the batch, on the lane's stream, while
  // the other lane computes the next batch; the copy-out to pageable caller memory happens in rgbdfe_wait_host
  struct HostJob {
    bool pending = false;
    bool waiting = false;         // a thread is inside rgbdfe_wait_host for this job (one waiter per job)
    bool direct = false;          // the download went straight into the caller's (pinned / registered) buffer
    int payload = 0;              // RGBDFE_HOST_RECORDS / RGBDFE_HOST_INLIERS
    int64_t ticket = 0;
    int32_t n = 0;
    void* out = nullptr;
    size_t out_bytes = 0;
    hipEvent_t copied = nullptr;  // the download has ended (inlier payload: headers + the list block's length)
  };
  HostJob host_jobs[kLanes];
  uint8_t* h_stage[kLanes] = {};    // pinned: max_pairs records, or the largest inlier stream of max_pairs pairs
  uint8_t* d_inl_stream[kLanes] = {};  // inlier payload: the packed stream in HBM
  int32_t* d_inl_total[kLanes] = {};
  int32_t* h_inl_total[kLanes] = {};   // pinned
  // scratch for single-pair helpers / project_to_3d
  void* d_scratch = nullptr;
  size_t scratch_bytes = 0;
  GrowBuffer render;         // api_render.hip: a call's visibility words, staged images, vertex group and queue
  bool render_count_fragments = false;   // rgbdfe_render_fragment_stats: the counting kernels (diagnostics)
  int64_t render_fragments[2] = {0, 0};  // the latest render call's fragments offered / that lowered a word on arrival
  GrowBuffer node_pack;      // api_session.hip: a read-back's node table and packed rows (rgbdfe_download_nodes)
  int64_t node_pack_launches = 0, node_pack_copies = 0;   // the latest read-back's kernel launches / device-to-host copies
  GrowBuffer icp;            // api_icp.hip: the samples, working copies and records of a call (d_scratch holds its tile counts and offsets)
  OrbWorkspace orb;
  OrbWorkspace orb_super;  // rgbdfe_detect_describe_batch: up to 7 frames per launch chain (its own image sets)
  std::unique_ptr<TaskPool> detect_pool, stage_pool;  // its worker threads (created by the first batch call, kept)
  SiftExtractor sift2, sift3;   // rgbdfe_sift_detect_batch rotates over three extractors (three chunks in flight)
  hipStream_t sift_stream1 = nullptr, sift_stream2 = nullptr, sift_stream3 = nullptr;
  SiftExtractor sift;  // rgbdfe_sift_detect (sift_extract.hip)
  // rgbdfe_sift_detect_batch_nodes: per chunk set (3 of them, 8 frames each) the pinned staging and the device copy of the
  // depth images, the node counts and the host-output rows (8 x max_keypoints); the depth copies go on a stream of their own
  struct SiftNodeBufs {
    size_t plane = 0;                                   // floats per depth image
    float* h_depth = nullptr; float* d_depth = nullptr;
    int32_t* d_n = nullptr; int32_t* h_n = nullptr;
    float4* d_xyz_out = nullptr; float* d_feat_out = nullptr; int32_t* d_kept_out = nullptr;
    float4* h_xyz_out = nullptr; float* h_feat_out = nullptr; int32_t* h_kept_out = nullptr;
    hipStream_t depth_stream = nullptr;
    hipEvent_t depth_done[3] = {};
  } sn;
  // rgbdfe_detect_sift_describe(_batch_nodes) (api_sift_behind.hip): one chunk of up to 8 frames, `rows_per_frame` rows each --
  // the detector's aggregates and depth images going up, the kept keys / rebuilt keypoints / counts coming back, the
  // descriptors in the callers' order and the output rows on the device; one allocation each side, laid out by api_sift_behind
  struct SiftBehindBufs {
    size_t plane = 0; int rows_per_frame = 0, agg_per_frame = 0;
    void* dev = nullptr; void* pin = nullptr;
    float* d_qdesc = nullptr; float4* d_qkeys = nullptr; size_t q_cap = 0;   // SiftGPU's own features of empty-list frames
  } sb;
  // rgbdfe_sift_detect_orb_describe(_batch_nodes) (api_sift_orb.hip): per chunk set (3 of them, 8 frames each) the blurred
  // frames, the described keypoints, the output rows (max_keypoints per frame) and the counts on the device and their
  // page-locked copies, laid out by api_sift_orb; the depth images travel through `sn`'s staging
  struct SiftOrbBufs {
    int rows = 0, cols = 0;
    void* dev = nullptr; void* pin = nullptr;
    int8_t* d_pattern = nullptr;   // rBRIEF's bit pattern
  } so;
  // the sensor entry points (api_sensor.hip): page-locked and device buffers for the frames' raw bytes (one per staging
  // buffer / image set / chunk slot of the pipeline that uses them), the float depth planes of the single-frame paths and
  // the resampling tables of the latest geometry
  struct SensorBufs {
    static constexpr int kPinned = 6, kDevice = 3;
    uint8_t* h_raw[kPinned] = {}; size_t h_cap[kPinned] = {};
    uint8_t* d_raw[kDevice] = {}; size_t d_cap[kDevice] = {};
    float* d_depth[2] = {}; size_t depth_cap[2] = {};
    uint8_t* d_planes = nullptr; size_t planes_cap = 0;   // rgbdfe_ingest_frame: gray | mono8
    int32_t* d_maps = nullptr; size_t maps_cap = 0;
    int maps_key[4] = {0, 0, 0, 0};                       // W, H, dW, dH of the tables in d_maps
  } sensor;
  int orb_max_keypoints = 0;  // 0 = detector not configured yet
  // feature_detector_type (rgbdfe_set_detector_type): RGBDFE_DETECTOR_ORB or RGBDFE_DETECTOR_FAST.  Both use the detector
  // configuration and the per-cell thresholds of `orb` (the reference's one detector_ object); FAST runs in `fast`.
  int32_t detector_type = RGBDFE_DETECTOR_ORB;
  FastWorkspace fast;
  std::unordered_map<int32_t, NodeEntry> nodes;
  std::unordered_map<int32_t, CloudEntry> clouds;
  double emm_q_lo = 0.0, emm_q_hi = 0.0;  // cdf boundaries 0.001 / 0.999 as arguments of erf
  std::vector<uint32_t> free_slots;
  RansacConst rc{};
  // profiling
  bool profiling = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  double k_ms[RGBDFE_KERNEL_COUNT] = {};
  int64_t k_launches[RGBDFE_KERNEL_COUNT] = {};
  int64_t k_pairs[RGBDFE_KERNEL_COUNT] = {};
  // ORB batch: a -[hamming]- b -[ransac]- c ; SIFT batch: a -[dot]- b -[finish]- c -[ransac]- d
  struct Pending { hipEvent_t a, b, c, d; int32_t pairs; bool sift; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;
};

namespace rgbdfe_host {
// the copy threads behind the batch pipelines' staging helpers (StagingRing): RGBDFE_STAGE_THREADS of them, 4 by default
inline TaskPool& stage_pool(rgbdfe_ctx* ctx) {
  static const int n = getenv("RGBDFE_STAGE_THREADS") ? std::max(1, atoi(getenv("RGBDFE_STAGE_THREADS"))) : 4;
  if (!ctx->stage_pool) ctx->stage_pool.reset(new TaskPool(n));
  return *ctx->stage_pool;
}
// PairWork::pad bit 0 for a SIFT pair: dot products < 2^19 (Cauchy-Schwarz over the two nodes' squared norms) and at
// most 32 column tiles of 32 on either side -- see sift_row_top2_kernel
inline uint32_t sift_fast_keys(const rgbdfe_ctx* ctx, const NodeEntry& q, const NodeEntry& t) {
  return (ctx->sift_fast && (q.flags & t.flags & 1u) && q.n <= 1024u && t.n <= 1024u) ? 1u : 0u;
}
}  // namespace rgbdfe_host


using namespace rgbdfe_host;

// ---- batch machinery (api_batches.hip)
namespace rgbdfe_host {
struct PhasePlan { int ends[4]; int n_phases; };
constexpr size_t kMaxEcRegions = (size_t)1 << 16;  // pairs of a record / replay piece at most (1.2 GB of error pool)
int fail(rgbdfe_ctx* ctx, int code, const std::string& msg);
void fill_ransac_const(rgbdfe_ctx* ctx);
int validate_params(rgbdfe_ctx* ctx, const rgbdfe_params& p);
int ensure_scratch(rgbdfe_ctx* ctx, size_t bytes);
hipEvent_t get_event(rgbdfe_ctx* ctx);
void drain_pending(rgbdfe_ctx* ctx);
int ensure_ec_pool(rgbdfe_ctx* ctx, rgbdfe_ctx::Lane& lane, size_t regions, hipStream_t stream);
int want_latency_path(rgbdfe_ctx* ctx, rgbdfe_ctx::Lane& lane, int32_t n, hipStream_t stream, bool* use, int* chunk_out, PhasePlan* plan);
bool hamming_on_mfma(const rgbdfe_ctx* ctx);
HammingGeometry hamming_geometry(const rgbdfe_ctx* ctx, uint32_t n, uint32_t max_nq, uint32_t max_nt);
uint32_t launch_hamming(rgbdfe_ctx* ctx, const PairWork* d_work, uint32_t* d_keys, uint32_t n, HammingGeometry geom, hipStream_t stream);
uint32_t launch_hamming(rgbdfe_ctx* ctx, const PairWork* d_work, uint32_t* d_keys, uint32_t n, uint32_t max_nq, uint32_t max_nt, hipStream_t stream);
bool capture_stream_ready(rgbdfe_ctx* ctx);
int enqueue_pairs(rgbdfe_ctx* ctx, const int32_t* qids, const int32_t* tids, int32_t n, rgbdfe_match_result* d_out, hipEvent_t wait_for, int64_t* ticket_out, int* lane_out, int matcher = 0, float* d_out_dist = nullptr, double flann_ratio = 0.95);
int wait_ticket(rgbdfe_ctx* ctx, int64_t ticket, hipStream_t stream);
}  // namespace rgbdfe_host
#define HIP_TRY(ctx, expr)                                                          \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess)                                                           \
      return fail(ctx, RGBDFE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// ---- the node table (api_context.hip): ctx->nodes and ctx->free_slots change here and in rgbdfe_release_node only.
// ctx->mu is held.  A slot leaves free_slots together with the entry that names it, so no failure can lose one.
namespace rgbdfe_host {
// the pair lanes have finished every batch that may still read a node slot
int wait_for_pair_lanes(rgbdfe_ctx* ctx);
// The slot of node_id.  Resident: its own, its entry untouched, after wait_for_pair_lanes (lanes_idle: the caller has waited
// already).  Fresh: a free slot, registered at once as an empty node of `kind` -- or RGBDFE_ERR_CAPACITY.  The caller writes
// the final entry (count, kind, flags) once the rows are in place.
int acquire_node_slot(rgbdfe_ctx* ctx, int32_t node_id, uint32_t kind, uint32_t* slot, bool lanes_idle = false);
// A batch of ids (negative: no node, where negative_is_none), all or nothing: RGBDFE_ERR_INVALID_ARG with `twice` when an id appears twice,
// RGBDFE_ERR_CAPACITY when the fresh ids outnumber the free slots; waits for the pair lanes only if some id is resident.
// slot_of == NULL: a check only, the caller takes the slots one by one (acquire_node_slot with lanes_idle).  Otherwise the
// fresh ids are registered at once as empty nodes of `kind`, resident entries stay as they are, and slot_of[i] is the slot
// of node_ids[i] (-1: no node).
int reserve_node_slots(rgbdfe_ctx* ctx, int32_t n, const int32_t* node_ids, uint32_t kind, std::vector<int64_t>* slot_of,
                       const char* twice = "a node id appears twice", bool negative_is_none = true);
bool node_id_twice(int32_t n, const int32_t* node_ids, bool negative_is_none = true);

// frame f of a batch call: every image pointer given
template <class A, class B = A>
bool frames_non_null(int32_t n, const A* const* a, const B* const* b = nullptr) {
  for (int32_t f = 0; f < n; ++f)
    if (!a[f] || (b && !b[f])) return false;
  return true;
}

// SiftGPUWrapper::detect's keypoints (sift_gpu_wrapper.cpp:156-160: size = 12 * scale, angle = orientation in degrees,
// response = octave = 0) and the way back (:135-138).  Double products, one cast to float: part of parity.
inline rgbdfe_keypoint sift_key_to_keypoint(const SiftKey& k) {
  return rgbdfe_keypoint{k.x, k.y, (float)(12.0 * k.s), (float)(k.o * 180.0 / 3.1415927), 0.f, 0};
}
inline SiftKey keypoint_to_sift_key(const rgbdfe_keypoint& p) {
  SiftKey k{};
  k.x = p.x; k.y = p.y;
  k.s = (float)(p.size / 12.0);
  k.o = (float)(p.angle / 180.0 * 3.1415927);
  return k;
}

// one allocation carved into 256-byte aligned pieces: carve() hands out offsets, at<T>() turns one into a pointer
struct Arena {
  size_t size = 0;
  size_t carve(size_t bytes) { const size_t off = size; size += round256(bytes); return off; }
};
template <class T> T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// ---- device memory of the mapping and geometry entry points (api_frame / api_map / api_display / api_voxel / api_octomap /
// api_icp / api_pose_graph.hip): the layouts come from device_layout.h, the pieces below need HIP or the context
static_assert(kSortTilePairs == kVoxSortTile, "sort_workspace() sizes launch_vox_sort's histogram");

// the node's resident cloud, or NULL (the caller fails with RGBDFE_ERR_UNKNOWN_NODE in its own words)
inline CloudEntry* resident_cloud(rgbdfe_ctx* ctx, int32_t node_id) {
  auto it = ctx->clouds.find(node_id);
  return (it == ctx->clouds.end() || !it->second.d) ? nullptr : &it->second;
}

// a column-major Matrix4f as the row-major rotation and the translation the kernels take
inline void rigid_of_matrix4f(const float* T, float R[9], float t[3]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = T[c * 4 + r];
    t[r] = T[12 + r];
  }
}

// The node table of a call and its tile -> node map as the first two uploaded blocks of a layout: `table` holds the n nodes
// and the sentinel row behind them, whose first_tile is the number of tiles.
struct NodeTableBlocks { Block table, tile_node; };
template <class Node>
NodeTableBlocks put_node_table(DeviceLayout& lay, const std::vector<Node>& table) {
  NodeTableBlocks b;
  b.table = lay.put(table.data(), sizeof(Node) * table.size());
  b.tile_node = lay.put(nullptr, 4 * (size_t)table.back().first_tile);
  uint32_t* tile_node = lay.staged<uint32_t>(b.tile_node);
  for (size_t k = 0; k + 1 < table.size(); ++k)   // (the bounds by value: the stores may alias the table as far as the compiler knows)
    std::fill(tile_node + table[k].first_tile, tile_node + table[k + 1].first_tile, (uint32_t)k);
  return b;
}

// where a call's output goes: the caller's device pointer, or (NULL) a staging buffer of the call's own that finish() copies
// to the host
struct OutputSink {
  void* d;   // where the kernels write (staged: valid after ready())
  explicit OutputSink(void* d_caller) : d(d_caller), staged_(d_caller == nullptr) {}
  int ready(rgbdfe_ctx* ctx, size_t bytes, const char* msg) {
    if (!staged_) return RGBDFE_OK;
    bytes_ = bytes;
    const int rc = stage_.alloc(ctx, bytes, msg);
    d = stage_.p;
    return rc;
  }
  hipError_t finish(void* h_out, hipStream_t st) {   // enqueues the copy back; the caller synchronises before the sink goes
    return staged_ ? hipMemcpyAsync(h_out, d, bytes_, hipMemcpyDeviceToHost, st) : hipSuccess;
  }
 private:
  bool staged_;
  size_t bytes_ = 0;
  DeviceBuffer stage_;
};

// ---- the SIFT chunk pipeline (api_detect.hip): three extractors (ctx->sift, sift2, sift3), three chunk streams, chunks of
// SiftExtractor::kMaxBatch frames in the order begin(c + 2) / finish_orientations(c + 1) / finish_descriptors(c) /
// finish_outputs(c) -- see sift_chunk_pipeline
struct SiftChunk {
  int32_t c;          // chunk index: frames c * kMaxBatch .. + nf
  int set, nf;        // c % 3: the chunk's extractor, stream and buffer set; its frames
  hipStream_t stream;
  const SiftExtractor* ex;
  const std::vector<SiftKey>* keys;   // [nf], filled by finish_outputs (valid in `after`)
  const float* const* desc;           // [nf]
  const float* d_depth;               // depth staging: the chunk's nf planes on the device (ordered before `behind`'s launches)
};
// the stream of buffer set `set`: the context's main stream until a call with more than one chunk has created the three
inline hipStream_t sift_chunk_stream(const rgbdfe_ctx* ctx, int set) {
  const hipStream_t s[3] = {ctx->sift_stream1, ctx->sift_stream2, ctx->sift_stream3};
  return s[set] ? s[set] : ctx->stream;
}
struct SiftChunkSteps {
  // on the chunk's stream behind its finish_descriptors (may be empty); an error's text goes to `err`
  std::function<int(const SiftChunk&, std::string& err)> behind;
  // where rgbdfe_sift_detect_batch copies chunk c - 1 out: behind chunk c's finish_descriptors and chunk c + 2's begin
  std::function<int(const SiftChunk&, std::string& err)> after;
};
// depth != NULL: a helper thread stages each chunk's depth images through ctx->sn (sift_nodes_prepare has run) beside its
// extraction.  timing: RGBDFE_SIFT_TIMING's line on stderr.  A failure is reported through fail() after the streams drained.
int sift_chunk_pipeline(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const float* const* depth, int32_t rows,
                        int32_t cols, int32_t max_keypoints, const SiftChunkSteps& steps, bool timing = false);
}  // namespace rgbdfe_host

// ---- the single-device implementation of the entry points (api_context / api_pairs / api_detect / api_frame / api_map.hip)
namespace impl {
// helpers shared between the implementation files
int upload_nodes_locked(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const uint8_t* const* desc,
                        const float* const* xyz1, const int32_t* counts);
// rgbdfe_display_geometry(_device) with ctx->mu held (api_display.hip); api_render.hip draws what it writes
int display_locked(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                   const rgbdfe_display_params* params, float* h_vertices, void* d_vertices, int64_t vertex_capacity,
                   int64_t* n_vertices, int64_t* node_offsets, int64_t* h_strips, void* d_strips, int64_t strip_capacity,
                   int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types, bool to_device, void* stream,
                   bool sizes_only);
void ensure_detector(rgbdfe_ctx* ctx);
int ensure_sift(rgbdfe_ctx* ctx);                 // the float / bf16 node slabs (api_pairs.hip)
void sift_nodes_release(rgbdfe_ctx* ctx);        // rgbdfe_ctx::sn (api_detect.hip)
void sift_behind_release(rgbdfe_ctx* ctx);       // rgbdfe_ctx::sb (api_sift_behind.hip)
void sift_orb_release(rgbdfe_ctx* ctx);          // rgbdfe_ctx::so (api_sift_orb.hip)
void sensor_release(rgbdfe_ctx* ctx);            // rgbdfe_ctx::sensor (api_sensor.hip)
// rgbdfe_ctx::sensor: n_pinned page-locked and n_device device buffers of `bytes` each for raw frames, and (depth_planes of
// them, at most 2) float planes of `plane` pixels
int sensor_ensure(rgbdfe_ctx* ctx, int n_pinned, int n_device, size_t bytes, int depth_planes, size_t plane);
// rgbdfe_ctx::sn for frames of `plane` pixels: the depth staging and the counts, the host-output rows when host_out (api_detect.hip)
int sift_nodes_prepare(rgbdfe_ctx* ctx, size_t plane, bool host_out);
int detector_max_keypoints(rgbdfe_ctx* ctx);     // the detector's max_keypoints (rgbdfe_detector_configure; 600 by default)
// the grid detector's aggregate of one frame (detector->detect, node.cpp:160) for the context's type; ctx->mu held
int detect_aggregate(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                     std::vector<KpOut>& kps);
// feature_detector_type "FAST" (api_fast.hip): Node::Node's feature path for n_frames frames (the host outputs may be NULL
// when node_ids is given), and the grid detector's keypoints of one frame alone (the point-cloud path)
int fast_detect_describe(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask,
                         const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy,
                         double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints, uint8_t* descriptors,
                         float* xyz1, int32_t* n_out, const int32_t* node_ids, const SensorRun* sensor = nullptr);
int fast_grid_keypoints(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols,
                        std::vector<KpOut>& kps);
void kp_to_abi(const std::vector<KpOut>& v, rgbdfe_keypoint* out);
// ---- sensor frames (api_sensor.hip; the ORB single-frame form in api_detect.hip)
int sensor_run_build(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, SensorRun& run);   // validation + index tables
int sensor_run_device(rgbdfe_ctx* ctx, SensorRun& run);                                                     // the tables on the device
int sensor_batch_validate(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, const int32_t* node_ids,
                          const rgbdfe_sensor_cloud* cloud, SensorRun& run);
// nf raw frames staged in ctx->sensor.h_raw[hbuf] -> d_raw[dbuf] on `s`, then the ingest launch into the outputs named in `outs`
int sensor_upload_ingest(rgbdfe_ctx* ctx, const SensorRun& run, int hbuf, int dbuf, int nf, IngestParams outs, hipStream_t s);
int detect_describe_sensor_frame(rgbdfe_ctx* ctx, const SensorRun& run, double fx, double fy, double cx, double cy,
                                 double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1,
                                 int32_t* n_out);
int rgbdfe_ingest_frame(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, uint8_t* gray, uint8_t* mono8, float* depth_m);
int rgbdfe_sensor_detect_describe(rgbdfe_ctx* ctx, const rgbdfe_sensor_frame* frame, double fx, double fy, double cx, double cy,
                                  double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1,
                                  int32_t* n_out);
int rgbdfe_sensor_detect_describe_batch(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, double fx, double fy,
                                        double cx, double cy, double depth_scaling, int32_t out_stride,
                                        rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out,
                                        const int32_t* node_ids);
int rgbdfe_sensor_clouds(rgbdfe_ctx* ctx, int32_t n_frames, const rgbdfe_sensor_frame* frames, double fx, double fy, double cx,
                         double cy, double depth_scaling, const int32_t* node_ids, const rgbdfe_sensor_cloud* cloud);
void rgbdfe_default_config(rgbdfe_config* cfg);
int rgbdfe_create(const rgbdfe_config* cfg, rgbdfe_ctx** out);
void rgbdfe_destroy(rgbdfe_ctx* ctx);
int rgbdfe_set_params(rgbdfe_ctx* ctx, const rgbdfe_params* p);
const char* rgbdfe_status_string(int status);
const char* rgbdfe_last_error(rgbdfe_ctx* ctx);
int rgbdfe_upload_node(rgbdfe_ctx* ctx, int32_t node_id, const uint8_t* desc, const float* xyz1, int32_t n);
int rgbdfe_upload_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const uint8_t* const* desc, const float* const* xyz1, const int32_t* counts);
int rgbdfe_upload_node_device(rgbdfe_ctx* ctx, int32_t node_id, const void* d_desc, const void* d_xyz1, int32_t n, void* stream);
int rgbdfe_upload_node_keypoints(rgbdfe_ctx* ctx, int32_t node_id, const float* kp_xy, int32_t n);
int rgbdfe_release_node(rgbdfe_ctx* ctx, int32_t node_id);
int rgbdfe_node_count(rgbdfe_ctx* ctx, int32_t node_id);
int rgbdfe_match_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs, rgbdfe_match_result* out, int64_t out_stride = 1);
int rgbdfe_match_node_pairs(rgbdfe_ctx* ctx, int32_t new_node_id, const int32_t* candidate_ids, int32_t n_pairs, rgbdfe_match_result* out);
int rgbdfe_match_pair_list_device(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs, void* d_out, void* stream);
int rgbdfe_submit_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs, void* d_out, int64_t* ticket);
int rgbdfe_wait_ticket(rgbdfe_ctx* ctx, int64_t ticket, void* stream);
int rgbdfe_submit_pair_list_host(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs, void* out, size_t out_bytes, int payload, int64_t* ticket);
int rgbdfe_wait_host(rgbdfe_ctx* ctx, int64_t ticket, int64_t* bytes_written);
int rgbdfe_wait_host_into(rgbdfe_ctx* ctx, int64_t ticket, void* out, size_t out_bytes, int64_t* bytes_written);
int rgbdfe_synchronize(rgbdfe_ctx* ctx);
int rgbdfe_upload_sift_node(rgbdfe_ctx* ctx, int32_t node_id, const float* desc128, const float* xyz1, int32_t n);
int rgbdfe_upload_float_node(rgbdfe_ctx* ctx, int32_t node_id, const float* desc, int32_t dim, const float* xyz1, int32_t n);
int rgbdfe_match_sift_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs, rgbdfe_match_result* out, float* out_dist, int64_t out_stride = 1, int matcher = 1, double flann_ratio = 0.95);
int rgbdfe_submit_sift_pair_list(rgbdfe_ctx* ctx, const int32_t* query_ids, const int32_t* train_ids, int32_t n_pairs, void* d_out, void* d_out_dist, int64_t* ticket);
int rgbdfe_sift_match_nodes(rgbdfe_ctx* ctx, int32_t query_id, int32_t train_id, int32_t* match_q, int32_t* match_t, float* match_dist, int32_t* n_matches);
int rgbdfe_detector_configure(rgbdfe_ctx* ctx, int32_t max_keypoints, int32_t grid_resolution, int32_t adjuster_max_iterations);
int rgbdfe_set_detector_type(rgbdfe_ctx* ctx, int32_t type);
int rgbdfe_fast_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols, int32_t threshold, rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out);
int rgbdfe_detector_thresholds(rgbdfe_ctx* ctx, double* thresholds, int32_t* n_cells);
int rgbdfe_orb_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols, int32_t fast_threshold, rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out);
int rgbdfe_orb_compute(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols, rgbdfe_keypoint* keypoints, int32_t n, uint8_t* descriptors, int32_t* n_out);
int rgbdfe_sift_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* /*mask*/, int32_t rows, int32_t cols, int32_t max_keypoints, rgbdfe_keypoint* keypoints, float* desc128, int32_t capacity, int32_t* n_out);
int rgbdfe_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, int32_t rows, int32_t cols, rgbdfe_keypoint* keypoints, int32_t n, float* desc128);
int rgbdfe_sift_detect_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, int32_t rows, int32_t cols, int32_t max_keypoints, int32_t out_stride, rgbdfe_keypoint* keypoints, float* desc128, int32_t* n_out);
int rgbdfe_sift_detect_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints, int32_t use_root_sift, const int32_t* node_ids, int32_t out_stride, rgbdfe_keypoint* keypoints, float* xyz1, float* feature_descriptors, int32_t* n_out);
int rgbdfe_sift_debug_plane(rgbdfe_ctx* ctx, int32_t octave, int32_t level, float* out, int32_t capacity_floats, int32_t* w, int32_t* h);
int rgbdfe_sift_debug_candidates(rgbdfe_ctx* ctx, int32_t octave, int32_t dog_level, float* out, int32_t capacity_rows, int32_t* n);
int rgbdfe_sift_geometry(rgbdfe_ctx* ctx, int32_t* octave_min, int32_t* octave_num, int32_t* levels, int32_t* dog_levels);
int rgbdfe_detect_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out);
int rgbdfe_detect_describe_batch(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask, const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t out_stride, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out, const int32_t* node_ids = nullptr, const SensorRun* sensor = nullptr);
int rgbdfe_hamming_nn_nodes(rgbdfe_ctx* ctx, int32_t query_id, int32_t train_id, int32_t* out_hd, int32_t* out_idx);
int rgbdfe_place_recognition_batch(rgbdfe_ctx* ctx, const int32_t* query_ids, int32_t n_queries, const int32_t* candidate_offsets, const int32_t* candidate_ids, int32_t k_neighbours, int32_t max_hd, int32_t max_out, int32_t* out_ids, float* out_scores, int32_t* out_counts);
int rgbdfe_place_recognition(rgbdfe_ctx* ctx, int32_t query_id, const int32_t* candidate_ids, int32_t n_candidates, int32_t k_neighbours, int32_t max_hd, int32_t max_out, int32_t* out_ids, float* out_scores, int32_t* n_out);
int rgbdfe_hamming_nn_host(rgbdfe_ctx* ctx, const uint8_t* qdesc, int32_t nq, const uint8_t* tdesc, int32_t nt, int32_t* out_hd, int32_t* out_idx);
int rgbdfe_project_to_3d(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints, int32_t* kept_idx, float* xyz1, int32_t* n_out);
int rgbdfe_set_feature_min_depth(rgbdfe_ctx* ctx, int32_t on);
int rgbdfe_project_to_3d_min_depth(rgbdfe_ctx* ctx, const float* kp_xy, const float* kp_size, int32_t n_kp, const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints, int32_t* kept_idx, float* xyz1, int32_t* n_out);
int rgbdfe_project_to_3d_cloud(rgbdfe_ctx* ctx, const float* kp_xy, int32_t n_kp, const float* cloud, int32_t rows, int32_t cols, double maximum_depth, int32_t max_keypoints, int32_t* kept_idx, float* xyz1, int32_t* n_out);
int rgbdfe_detect_describe_cloud(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* cloud, int32_t rows, int32_t cols, double maximum_depth, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out);
int rgbdfe_detect(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, int32_t rows, int32_t cols, rgbdfe_keypoint* keypoints, int32_t capacity, int32_t* n_out);
int rgbdfe_detect_sift_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const uint8_t* mask, const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t use_root_sift, rgbdfe_keypoint* keypoints, float* xyz1, float* siftgpu_descriptors, float* feature_descriptors, int32_t* n_out);
int rgbdfe_detect_sift_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const uint8_t* const* mask, const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t use_root_sift, const int32_t* node_ids, int32_t out_stride, rgbdfe_keypoint* keypoints, float* xyz1, float* feature_descriptors, int32_t* n_out);
int rgbdfe_sift_detect_orb_describe(rgbdfe_ctx* ctx, const uint8_t* gray, const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out);
int rgbdfe_sift_detect_orb_describe_batch_nodes(rgbdfe_ctx* ctx, int32_t n_frames, const uint8_t* const* gray, const float* const* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints, const int32_t* node_ids, int32_t out_stride, rgbdfe_keypoint* keypoints, uint8_t* descriptors, float* xyz1, int32_t* n_out);
int rgbdfe_sift_node_features(rgbdfe_ctx* ctx, const float* kp_xy, const float* kp_size, int32_t n_kp, const float* desc_in, const float* depth, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double depth_scaling, int32_t max_keypoints, int32_t use_root_sift, int32_t* kept_idx, float* xyz1, float* siftgpu_descriptors, float* feature_descriptors, int32_t* n_out);
int rgbdfe_depth_to_mono8(rgbdfe_ctx* ctx, const void* depth, int32_t depth_is_u16, int32_t rows, int32_t cols, uint8_t* mono8, float* depth_m);
int rgbdfe_upload_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, const float* depth, int32_t rows, int32_t cols, const uint8_t* rgb, int32_t rgb_channels, int32_t encoding_bgr, double fx, double fy, double cx, double cy, double depth_scaling, double min_depth, int32_t cloud_skip, float* cloud_out);
int rgbdfe_release_node_cloud(rgbdfe_ctx* ctx, int32_t node_id);
int rgbdfe_assemble_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth, int32_t preserve_raster, float* out, int64_t capacity, int64_t* n_out, int64_t* node_offsets);
int rgbdfe_assemble_map_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth, int32_t preserve_raster, void* d_out, int64_t capacity, int64_t* n_out, int64_t* node_offsets, void* stream);
int rgbdfe_download_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, float* cloud_out, int64_t capacity_points, int32_t* rows, int32_t* cols);
int rgbdfe_voxel_filter(rgbdfe_ctx* ctx, const float* points, int64_t n_in, double voxelfilter_size, float* out, int64_t capacity, int64_t* n_out, int32_t* flags);
int rgbdfe_voxel_filter_device(rgbdfe_ctx* ctx, const void* d_points, int64_t n_in, double voxelfilter_size, void* d_out, int64_t capacity, int64_t* n_out, int32_t* flags, void* stream);
int rgbdfe_reduce_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, double voxelfilter_size, int64_t* n_out, int32_t* flags);
// api_display.hip
void rgbdfe_display_default_params(rgbdfe_display_params* p);
int rgbdfe_display_geometry(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, const rgbdfe_display_params* params, float* vertices, int64_t vertex_capacity, int64_t* n_vertices, int64_t* node_offsets, int64_t* strips, int64_t strip_capacity, int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types);
int rgbdfe_display_geometry_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, const rgbdfe_display_params* params, void* d_vertices, int64_t vertex_capacity, int64_t* n_vertices, int64_t* node_offsets, void* d_strips, int64_t strip_capacity, int64_t* n_strips, int64_t* node_strip_offsets, int32_t* node_types, void* stream);
// api_render.hip
void rgbdfe_render_default_params(rgbdfe_render_params* p);
int rgbdfe_render_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params, uint8_t* rgba, float* depth, int64_t* ids, int32_t* node_index);
int rgbdfe_render_nodes_device(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, const rgbdfe_display_params* display_params, const rgbdfe_render_params* render_params, void* d_rgba, void* d_depth, void* d_ids, void* d_node_index, void* stream);
void rgbdfe_render_perspective(double fovy, double aspect, double z_near, double z_far, double* out16);
void rgbdfe_render_viewer_view(double x_tra, double y_tra, double z_tra, double x_rot, double y_rot, double z_rot, double rotation_stepping, const double* viewpoint, double* out16);
void rgbdfe_render_sensor_camera(double fx, double fy, double cx, double cy, int32_t width, int32_t height, double z_near, double z_far, const double* pose, double* view_out16, double* projection_out16);
int rgbdfe_render_unproject(double x, double y, double depth, const double* view, const double* projection, int32_t width, int32_t height, double* out3);
int rgbdfe_render_fragment_stats(rgbdfe_ctx* ctx, int32_t enable, int64_t* out2);
// api_pose_graph.hip
int rgbdfe_pose_graph_chi2(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2);
int rgbdfe_pose_graph_linearize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* errors, double* weights, int32_t edge_capacity, int32_t* n_edges, int32_t* free_ids, double* h_diag, double* b, int32_t vertex_capacity, int32_t* n_free, int32_t* off_rows, int32_t* off_cols, double* h_off, int32_t block_capacity, int32_t* n_blocks, double* chi2);
int rgbdfe_pose_graph_optimize(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, int32_t iterations, rgbdfe_pose_graph_report* report);
int rgbdfe_pose_graph_optimize_graph(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double break_criterion, rgbdfe_pose_graph_report* report);
int rgbdfe_pose_graph_edge_errors(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double* chi2, double* err_sq, int32_t* active, int32_t capacity, int32_t* n_edges);
int rgbdfe_pose_graph_prune_edges(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, float thresh, uint8_t* verdicts, int32_t capacity, int32_t* n_pruned);
int rgbdfe_pose_graph_evaluate(rgbdfe_ctx* ctx, rgbdfe_pose_graph* g, double optimizer_iterations, rgbdfe_pose_graph_evaluation* out, double* estimates, int32_t capacity_nodes);
// api_icp.hip
void rgbdfe_icp_default_params(rgbdfe_icp_params* p);
int rgbdfe_icp_align_nodes(rgbdfe_ctx* ctx, int32_t n_jobs, const int32_t* source_ids, const int32_t* target_ids, const float* guesses, const rgbdfe_icp_params* params, float* transforms_out, rgbdfe_icp_report* reports_out);
int rgbdfe_icp_align_clouds(rgbdfe_ctx* ctx, const float* source, int64_t n_source, const float* target, int64_t n_target, const float* guess, const rgbdfe_icp_params* params, float* transform_out, rgbdfe_icp_report* report_out, int32_t* nn_index_out, float* nn_d2_out, int64_t debug_capacity);
int rgbdfe_filter_cloud(rgbdfe_ctx* ctx, const float* cloud, int64_t n, int32_t desired_size, int32_t* indices_out, float* rows_out, int64_t capacity, int64_t* n_out);
// api_octomap.hip (the map keeps the context it lives on; `owner` is the handle it was created through)
void rgbdfe_octomap_default_params(rgbdfe_octomap_params* p);
rgbdfe_ctx* octomap_owner(rgbdfe_octomap* map);
int rgbdfe_octomap_create(rgbdfe_ctx* ctx, rgbdfe_ctx* owner, const rgbdfe_octomap_params* params, int64_t capacity_cells, rgbdfe_octomap** out);
void rgbdfe_octomap_destroy(rgbdfe_octomap* map);
int rgbdfe_octomap_reset(rgbdfe_octomap* map);
int rgbdfe_octomap_reserve(rgbdfe_octomap* map, int64_t capacity_cells);
int rgbdfe_octomap_insert_nodes(rgbdfe_octomap* map, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double max_range, int32_t* n_done);
int rgbdfe_octomap_insert_cloud(rgbdfe_octomap* map, const float* points, int64_t n, const float* transform, double max_range);
int rgbdfe_octomap_size(rgbdfe_octomap* map, int64_t* n_leaves);
int rgbdfe_octomap_leaves(rgbdfe_octomap* map, rgbdfe_octomap_leaf* out, int64_t capacity, int64_t* n_out);
int rgbdfe_octomap_stats(rgbdfe_octomap* map, int64_t* out, int32_t n_out);
int rgbdfe_octomap_tree(rgbdfe_octomap* map, rgbdfe_octomap_node* out, int64_t capacity, int64_t* n_nodes);
int rgbdfe_octomap_tree_device(rgbdfe_octomap* map, void* d_out, int64_t capacity, int64_t* n_nodes, void* stream);
int rgbdfe_octomap_nodes_at_depth(rgbdfe_octomap* map, int32_t depth, float min_log_odds, rgbdfe_octomap_leaf* out, int64_t capacity, int64_t* n_out);
int rgbdfe_octomap_write(rgbdfe_octomap* map, const char* path);
int rgbdfe_octomap_set_leaves(rgbdfe_octomap* map, const rgbdfe_octomap_leaf* leaves, int64_t n);
int rgbdfe_octomap_read(rgbdfe_octomap* map, const char* path);
int rgbdfe_octomap_occupied_log_odds(rgbdfe_octomap* map, float* out);
int rgbdfe_octomap_search(rgbdfe_octomap* map, const float* points, int64_t n, int32_t* found, rgbdfe_octomap_leaf* leaves);
int rgbdfe_octomap_cast_rays(rgbdfe_octomap* map, const float* origins, const float* directions, int64_t n, int32_t ignore_unknown, double max_range, float occupied_log_odds, rgbdfe_octomap_ray_hit* hits);
int rgbdfe_octomap_view_cloud(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int32_t ignore_unknown, double max_range, float occupied_log_odds, float* out, uint8_t* status);
int rgbdfe_octomap_view_cloud_device(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int32_t ignore_unknown, double max_range, float occupied_log_odds, void* d_out, void* d_status, void* stream);
int rgbdfe_observation_likelihood(rgbdfe_ctx* ctx, int32_t n, const int32_t* new_ids, const int32_t* old_ids, const float* transforms, int32_t emm_skip_step, rgbdfe_emm_counts* out);
int rgbdfe_observation_criterion_met(uint32_t inliers, uint32_t outliers, uint32_t all, double observability_threshold, double* quality);
int rgbdfe_set_latency_mode(rgbdfe_ctx* ctx, int32_t max_pairs, int32_t chunk_iterations);
int rgbdfe_set_hamming_mode(rgbdfe_ctx* ctx, int32_t mode);
int rgbdfe_hamming_wide_last(rgbdfe_ctx* ctx);
int rgbdfe_set_hamming_shape(rgbdfe_ctx* ctx, int32_t shape);
int rgbdfe_hamming_shape_last(rgbdfe_ctx* ctx);
int rgbdfe_set_profiling(rgbdfe_ctx* ctx, int enable);
int rgbdfe_get_kernel_time(rgbdfe_ctx* ctx, int which, double* total_ms, int64_t* launches, int64_t* pairs);
int rgbdfe_reset_kernel_time(rgbdfe_ctx* ctx);
int rgbdfe_sizeof_match_result(void);
int rgbdfe_sizeof_compact_result(void);
int rgbdfe_pack_compact(rgbdfe_ctx* ctx, const void* d_records, int32_t n, void* d_compact, void* stream);
int rgbdfe_set_graph_capture(rgbdfe_ctx* ctx, int enable);
int rgbdfe_pack_inliers(rgbdfe_ctx* ctx, const void* d_records, int32_t n, int32_t n_headers, void* d_stream, int32_t* d_total, void* stream);
int rgbdfe_sizeof_inlier_header(void);
int rgbdfe_graph_stats(rgbdfe_ctx* ctx, int64_t* out, int32_t n_out);
int rgbdfe_abi_version(void);
int rgbdfe_update_inlier_features(rgbdfe_ctx* ctx, const void* d_records, const int32_t* query_ids, const int32_t* train_ids,
                                  const uint8_t* accept, int32_t n, int32_t* launched);
int rgbdfe_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, uint8_t* out, int32_t capacity);
int ensure_feature_stats(rgbdfe_ctx* ctx);       // the counters of every slot, allocated zeroed on first use (api_slam.hip)
// api_session.hip
int rgbdfe_download_nodes(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc, float* xyz1,
                          float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds);
int rgbdfe_debug_download_nodes_copy_loop(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, int64_t capacity_rows, void* desc,
                                          float* xyz1, float* kp_xy, uint8_t* stats, int64_t* row_offsets, int32_t* kinds);
int rgbdfe_download_node(rgbdfe_ctx* ctx, int32_t node_id, int32_t capacity_rows, void* desc, float* xyz1, float* kp_xy,
                         uint8_t* stats, int32_t* kind, int32_t* has_keypoints);
int rgbdfe_download_nodes_stats(rgbdfe_ctx* ctx, int64_t* out, int32_t n_out);
int rgbdfe_set_node_feature_stats(rgbdfe_ctx* ctx, int32_t node_id, const uint8_t* stats, int32_t n);
int rgbdfe_detector_set_thresholds(rgbdfe_ctx* ctx, const double* thresholds, int32_t n_cells);
int rgbdfe_node_cloud_info(rgbdfe_ctx* ctx, int32_t node_id, double* out8);
int rgbdfe_restore_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, const float* points, int32_t rows, int32_t cols, double fx, double fy,
                              double cx, double cy, int32_t cloud_skip);
int rgbdfe_session_save(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, uint32_t flags, const char* path);
int rgbdfe_session_load(rgbdfe_ctx* ctx, rgbdfe_slam* slam, rgbdfe_pose_graph* graph, const char* path);
// api_map_files.hip
int rgbdfe_save_map(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const float* transforms, double maximum_depth,
                    int32_t preserve_raster, const char* path, int64_t chunk_points, char* path_written, int64_t path_capacity,
                    rgbdfe_map_file_stats* stats);
int rgbdfe_save_node_clouds(rgbdfe_ctx* ctx, int32_t n_nodes, const int32_t* node_ids, const int32_t* graph_ids, const double* poses,
                            int32_t transform_individual_clouds, const char* basename, int32_t* n_written);
}  // namespace impl

// ---- the rgbdfe_slam object as api_session.hip needs it (api_slam.hip)
namespace rgbdfe_host {
// rgbdfe_slam_deserialize's checks (the string, a fresh target, equal parameters); the object changes only with `commit`
int slam_deserialize(rgbdfe_slam* s, const uint8_t* in, int64_t bytes, bool commit);
rgbdfe_ctx* slam_context(rgbdfe_slam* s);
rgbdfe_pose_graph* slam_graph(rgbdfe_slam* s);
}  // namespace rgbdfe_host

// ---- several devices behind one handle (api_group.hip)
#include <dlfcn.h>
namespace rgbdfe_host {

// the handful of RCCL entry points the gather needs, resolved at run time (no link-time dependency for 1-GPU users)
struct Rccl {
  void* handle = nullptr;
  int (*CommInitAll)(void**, int, const int*) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool load() {
    if (handle) return true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (handle) break;
    }
    if (!handle) return false;
    CommInitAll = (decltype(CommInitAll))dlsym(handle, "ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))dlsym(handle, "ncclCommDestroy");
    AllGather = (decltype(AllGather))dlsym(handle, "ncclAllGather");
    GroupStart = (decltype(GroupStart))dlsym(handle, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(handle, "ncclGroupEnd");
    GetErrorString = (decltype(GetErrorString))dlsym(handle, "ncclGetErrorString");
    return CommInitAll && CommDestroy && AllGather && GroupStart && GroupEnd;
  }
};
constexpr int kNcclChar = 0;  // ncclInt8 / ncclChar (rccl.h: ncclDataType_t)

struct Worker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::function<int()> job;
  bool has_job = false, quit = false;
  int rc = RGBDFE_OK;
};

}  // namespace rgbdfe_host

struct Group {
  std::vector<rgbdfe_ctx*> children;
  std::vector<int> device_ids;
  std::vector<std::unique_ptr<Worker>> workers;
  Rccl rccl;
  std::vector<void*> comms;      // one communicator per device once the RCCL path has been set up
  bool rccl_tried = false, rccl_ok = false;
  std::vector<hipStream_t> gather_streams;  // one per device
  std::vector<hipEvent_t> gather_events;
  std::string transport = "none";
  // edges-only gather: per device a compacted copy of its shard, the survivors' global pair indices, scan scratch
  std::vector<rgbdfe_match_result*> edge_recs;
  std::vector<int32_t*> edge_idx, edge_dst, edge_cnt;
  std::vector<int32_t*> edge_cnt_host;  // pinned
  std::vector<char*> inl_stream;        // inlier gather: per device the shard's inlier stream (rgbdfe_inlier_header), worst case
  int32_t edge_cap = 0;                 // records per device the scratch holds
  // inlier gather: entries of a device's list block the exchange is sized for BEFORE the devices have counted their lists
  // (the longest list of the earlier calls + a quarter; 0: nothing seen yet), and how many exchanges the latest call issued
  size_t inl_cap_entries = 0;
  int inl_exchanges = 0;
  double last_submit_us = 0.0;          // host time the calling thread spent enqueueing the latest sharded batch on all devices
  // One call at a time on a group handle (rgbdfe.h: calls on one context serialise): covers the workers' job slots and
  // transport / rccl_* / edge_* above.  Recursive: the gather entry points hold it around their group_run.
  std::recursive_mutex mu;
};
namespace rgbdfe_host {
void worker_main(Worker* w);
int group_run(rgbdfe_ctx* gctx, const std::function<int(int)>& fn);
void group_destroy(rgbdfe_ctx* gctx);
int group_create(const rgbdfe_config* cfg, const int32_t* device_ids, int32_t n, rgbdfe_ctx** out);
int group_match(rgbdfe_ctx* gctx, const int32_t* q, const int32_t* t, int32_t n, rgbdfe_match_result* out, bool sift, float* out_dist);
int group_each(rgbdfe_ctx* gctx, const std::function<int(int)>& fn);
int group_submit(rgbdfe_ctx* gctx, const std::function<int(int)>& fn);
bool group_setup_rccl(rgbdfe_ctx* gctx);
int group_ensure_edge_scratch(rgbdfe_ctx* gctx, int32_t per);
int group_match_allgather(rgbdfe_ctx* gctx, const int32_t* q, const int32_t* t, int32_t n, void* const* d_out, int32_t* records_per_device, bool compact = false);
int group_match_allgather_edges(rgbdfe_ctx* gctx, const int32_t* q, const int32_t* t, int32_t n, void* const* d_out, int32_t* const* d_index, int32_t* counts, int32_t* stride_out);
int group_match_allgather_inliers(rgbdfe_ctx* gctx, const int32_t* q, const int32_t* t, int32_t n, void* const* d_out, int32_t* records_per_device, int32_t* totals, int64_t* stride_bytes);
int group_only_single(rgbdfe_ctx* ctx, const char* what);
// ---- the exception barrier: nothing thrown inside the library crosses the C ABI (node.cpp:1424 "never throws") ------
template <class F>
int guarded(rgbdfe_ctx* ctx, F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    try { return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "host allocation failed"); } catch (...) { return RGBDFE_ERR_OUT_OF_MEMORY; }
  } catch (const std::exception& e) {
    try { return fail(ctx, RGBDFE_ERR_INTERNAL, std::string("internal error: ") + e.what()); } catch (...) { return RGBDFE_ERR_INTERNAL; }
  } catch (...) {
    return RGBDFE_ERR_INTERNAL;
  }
}
}  // namespace rgbdfe_host
using namespace rgbdfe_host;
#define RGBDFE_IS_GROUP(ctx) ((ctx) && (ctx)->group)
// broadcast to every device of a group, or the plain call
#define RGBDFE_ALL(ctx, call_on_c)                                                          \
  guarded(ctx, [&]() -> int {                                                               \
    if (RGBDFE_IS_GROUP(ctx))                                                               \
      return group_run(ctx, [&](int i_) -> int { rgbdfe_ctx* c = ctx->group->children[(size_t)i_]; return call_on_c; }); \
    rgbdfe_ctx* c = ctx;                                                                    \
    return call_on_c;                                                                       \
  })
// frame-level work of a group runs on its first device
#define RGBDFE_FIRST(ctx, call_on_c)                                                        \
  guarded(ctx, [&]() -> int {                                                               \
    rgbdfe_ctx* c = RGBDFE_IS_GROUP(ctx) ? ctx->group->children[0] : ctx;                   \
    const int rc_ = call_on_c;                                                              \
    if (rc_ != RGBDFE_OK && RGBDFE_IS_GROUP(ctx)) {                                         \
      std::string m_; { std::lock_guard<std::mutex> e_(c->err_mu); m_ = c->last_error; }    \
      fail(ctx, rc_, m_);                                                                   \
    }                                                                                       \
    return rc_;                                                                             \
  })
