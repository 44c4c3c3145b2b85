// rgbdfe.hpp -- header-only C++ host side above the C ABI (include/rgbdfe.h), mirroring the slice of
// rgbdslam_v2's interface that the pair path exposes: same names, argument meaning and error behaviour
// as src/node.h, src/matching_result.h, src/edge.h and GraphManager::nodeComparisons' fan-out
// (src/graph_manager.cpp:541-548), without the OpenCV / Eigen / Qt / ROS types.
//
//   reference                                   here
//   cv::DMatch                                  rgbdslam::DMatch {queryIdx, trainIdx, distance}
//   Eigen::Matrix4f (column-major)              std::array<float,16> (column-major)
//   LoadedEdge3D / MatchingResult               rgbdslam::LoadedEdge3D / rgbdslam::MatchingResult
//   Node::matchNodePair(const Node*)            rgbdslam::Node::matchNodePair(const Node*)
//   QtConcurrent::blockingMapped(nodes, ...)    rgbdslam::GraphManager::nodeComparisons(new_node, nodes)
//   GraphManager::getPotentialEdgeTargetsWithDijkstra   rgbdslam::GraphManager::getPotentialEdgeTargetsWithDijkstra
// No exceptions are thrown on the pair path: like Node::matchNodePair (node.cpp:1424-1426) failures end
// in a MatchingResult whose edge ids are -1.
#ifndef RGBDFE_HPP
#define RGBDFE_HPP

#include <array>
#include <cmath>
#include <utility>
#include <cstdint>
#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rgbdfe.h"

namespace rgbdslam {

struct DMatch {  // cv::DMatch
  int queryIdx = -1, trainIdx = -1, imgIdx = -1;
  float distance = 0.f;
};

struct LoadedEdge3D {  // src/edge.h:24-32
  int id1 = -1, id2 = -1;
  std::array<double, 16> transform{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};  // Isometry3d, column-major
  double informationScale = 0.0;  // informationMatrix = Identity(6,6) * informationScale (node.cpp:1335)
};

struct MatchingResult {  // src/matching_result.h:24-46
  std::vector<DMatch> inlier_matches, all_matches;
  LoadedEdge3D edge;
  float rmse = 0.0f;
  std::array<float, 16> ransac_trafo{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
  std::array<float, 16> final_trafo{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
  std::array<float, 16> icp_trafo{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};   // set by GraphManager::icpFallback
  unsigned int inlier_points = 0, outlier_points = 0, occluded_points = 0, all_points = 0;  // environment measurement model
};

// float_dist: the DMatch.distance values of a SIFT / FLANN pair (float L2, rgbdfe_match_sift_pair_list's out_dist), or null
inline MatchingResult toMatchingResult(const rgbdfe_match_result& r, const float* float_dist = nullptr) {
  MatchingResult mr;
  mr.all_matches.resize((size_t)r.n_all);
  for (int m = 0; m < r.n_all; ++m) {
    mr.all_matches[m].queryIdx = r.all_q[m];
    mr.all_matches[m].trainIdx = r.all_t[m];
    mr.all_matches[m].distance = float_dist ? float_dist[m] : r.all_hd[m] / 256.0f;  // node.cpp:573 without the random jitter
  }
  for (int m = 0; m < r.n_all; ++m)
    if ((r.inlier_mask[m >> 6] >> (m & 63)) & 1ull) mr.inlier_matches.push_back(mr.all_matches[m]);
  mr.rmse = r.rmse;
  for (int i = 0; i < 16; ++i) mr.ransac_trafo[i] = mr.final_trafo[i] = r.trafo[i];  // node.cpp:1334
  mr.edge.id1 = r.id1;
  mr.edge.id2 = r.id2;
  if (r.id1 >= 0) {
    for (int i = 0; i < 16; ++i) mr.edge.transform[i] = (double)r.trafo[i];  // node.cpp:1339
    mr.edge.informationScale = r.info_scale;
  }
  return mr;
}

// Owns the rgbdfe context (one GPU).  Construction throws (like the reference's fatal start-up errors);
// the per-pair calls never do.
class FrontEnd {
 public:
  explicit FrontEnd(const rgbdfe_config& cfg) {
    rgbdfe_ctx* c = nullptr;
    const int st = rgbdfe_create(&cfg, &c);
    if (st != RGBDFE_OK) throw std::runtime_error(std::string("rgbdfe_create: ") + rgbdfe_status_string(st));
    ctx_.reset(c, rgbdfe_destroy);
  }
  // Several GPUs behind one handle (rgbdfe_create_multi): nodes are replicated, nodeComparisons shards its candidates
  // (candidate k -> device k mod G) -- nothing else in this header changes.
  FrontEnd(const rgbdfe_config& cfg, const std::vector<int32_t>& device_ids) {
    rgbdfe_ctx* c = nullptr;
    const int st = rgbdfe_create_multi(&cfg, device_ids.data(), (int32_t)device_ids.size(), &c);
    if (st != RGBDFE_OK)
      throw std::runtime_error(std::string("rgbdfe_create_multi: ") + rgbdfe_status_string(st) + ": " + rgbdfe_last_error(nullptr));
    ctx_.reset(c, rgbdfe_destroy);
  }
  int deviceCount() const { return rgbdfe_device_count(ctx_.get()); }
  static rgbdfe_config defaultConfig() {
    rgbdfe_config c;
    rgbdfe_default_config(&c);
    return c;
  }
  rgbdfe_ctx* get() const { return ctx_.get(); }

  // Parameter "feature_detector_type" with the default ORB extractor (createDetector, features.cpp:63-113): "ORB" or "FAST";
  // the per-cell thresholds restart at 20.  Throws on any other type.
  void setDetectorType(const std::string& type) {
    const int t = type == "FAST" ? RGBDFE_DETECTOR_FAST : type == "ORB" ? RGBDFE_DETECTOR_ORB : -1;
    const int st = rgbdfe_set_detector_type(ctx_.get(), t);
    if (st != RGBDFE_OK) throw std::runtime_error("feature_detector_type " + type + ": " + rgbdfe_status_string(st));
  }
  // cv::FastFeatureDetector::create(threshold)->detect(image, keypoints, mask) on the whole image (the A/B piece of the FAST
  // detector); mask may be nullptr.  Throws on failure.
  std::vector<rgbdfe_keypoint> fastDetect(const uint8_t* gray, const uint8_t* mask, int rows, int cols, int threshold) const {
    std::vector<rgbdfe_keypoint> kp(4096);
    int32_t n = 0;
    int st = rgbdfe_fast_detect(ctx_.get(), gray, mask, rows, cols, threshold, kp.data(), (int32_t)kp.size(), &n);
    if (st == RGBDFE_ERR_CAPACITY) {  // n = the number found: once more with room for all of them
      kp.resize((size_t)n);
      st = rgbdfe_fast_detect(ctx_.get(), gray, mask, rows, cols, threshold, kp.data(), (int32_t)kp.size(), &n);
    }
    if (st != RGBDFE_OK) throw std::runtime_error(std::string("rgbdfe_fast_detect: ") + rgbdfe_last_error(ctx_.get()));
    kp.resize((size_t)n);
    return kp;
  }

  // Resident nodes back on the host (rgbdfe_download_nodes): the listed nodes, all of one kind, in the order given and
  // packed without gaps -- node i's rows are row_offsets[i] .. row_offsets[i + 1] of every array.  desc holds 32 bytes per
  // row for ORB nodes and 128 floats per row for SIFT / float nodes; kp_xy is zero for a node without keypoints.
  struct NodeRows {
    std::vector<int64_t> row_offsets;
    std::vector<int32_t> kinds;           // 0 ORB, 1 SIFT, 2 float
    std::vector<uint8_t> has_keypoints;
    std::vector<uint8_t> desc;            // bytes
    std::vector<float> xyz1, kp_xy;
    std::vector<uint8_t> stats;           // feature_matching_stats_
  };
  // Throws on failure (an id that is not resident, nodes of different kinds).
  NodeRows downloadNodes(const std::vector<int32_t>& node_ids) const {
    NodeRows r;
    const int32_t n = (int32_t)node_ids.size();
    r.row_offsets.assign((size_t)n + 1, 0);
    r.kinds.assign((size_t)n, 0);
    int st = rgbdfe_download_nodes(ctx_.get(), n, node_ids.data(), INT64_MAX, nullptr, nullptr, nullptr, nullptr,
                                   r.row_offsets.data(), r.kinds.data());   // the sizing call: no array, no device work
    const size_t rows = (size_t)r.row_offsets[(size_t)n];
    if (st == RGBDFE_OK && rows > 0) {
      r.desc.resize(rows * ((n > 0 && (r.kinds[0] & 0xff) != 0) ? 512 : 32));
      r.xyz1.resize(rows * 4);
      r.kp_xy.resize(rows * 2);
      r.stats.resize(rows);
      st = rgbdfe_download_nodes(ctx_.get(), n, node_ids.data(), (int64_t)rows, r.desc.data(), r.xyz1.data(), r.kp_xy.data(),
                                 r.stats.data(), r.row_offsets.data(), r.kinds.data());
    }
    if (st != RGBDFE_OK) throw std::runtime_error(std::string("rgbdfe_download_nodes: ") + rgbdfe_last_error(ctx_.get()));
    r.has_keypoints.resize((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
      r.has_keypoints[(size_t)i] = (r.kinds[(size_t)i] & RGBDFE_NODE_HAS_KEYPOINTS) ? 1 : 0;
      r.kinds[(size_t)i] &= 0xff;
    }
    return r;
  }
  // a node's feature_matching_stats_ written back behind its upload (a restore); false: not resident, or a wrong count
  bool setNodeFeatureStats(int32_t node_id, const std::vector<uint8_t>& stats) const {
    return rgbdfe_set_node_feature_stats(ctx_.get(), node_id, stats.data(), (int32_t)stats.size()) == RGBDFE_OK;
  }
  // The grid detector's per-cell thresholds: all it carries from frame to frame.
  std::vector<double> detectorThresholds() const {
    std::vector<double> t(64);
    int32_t n = 0;
    if (rgbdfe_detector_thresholds(ctx_.get(), t.data(), &n) != RGBDFE_OK) n = 0;
    t.resize((size_t)n);
    return t;
  }
  bool setDetectorThresholds(const std::vector<double>& t) const {
    return rgbdfe_detector_set_thresholds(ctx_.get(), t.data(), (int32_t)t.size()) == RGBDFE_OK;
  }

 private:
  std::shared_ptr<rgbdfe_ctx> ctx_;
};

// src/sift_gpu_wrapper.h:49 -- SiftGPUWrapper::detect(image, keypoints, descriptors, mask): SiftGPU's extraction with the
// options the reference's constructor sets (sift_gpu_wrapper.cpp:29-88).  keypoints: pt, size = 12 * scale, angle in
// degrees; descriptors: n x 128 floats, unnormalised.  `mask` does not exist here: the reference ignores it.
class SiftGPUWrapper {
 public:
  explicit SiftGPUWrapper(const FrontEnd& fe, int max_keypoints) : fe_(fe), max_keypoints_(max_keypoints) {}
  void detect(const uint8_t* image, int rows, int cols, std::vector<rgbdfe_keypoint>& keypoints,
              std::vector<float>& descriptors) const {
    if (!keypoints.empty()) {   // "Use Keypoints if provided" (:132-142): descriptors for the caller's keypoints
      descriptors.assign(keypoints.size() * 128, 0.f);
      if (rgbdfe_sift_describe(fe_.get(), image, rows, cols, keypoints.data(), (int32_t)keypoints.size(), descriptors.data()) !=
          RGBDFE_OK) {
        keypoints.clear();
        descriptors.clear();
      }
      return;
    }
    int32_t cap = 2 * max_keypoints_ + 1024, n = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      keypoints.resize((size_t)cap);
      descriptors.resize((size_t)cap * 128);
      const int rc = rgbdfe_sift_detect(fe_.get(), image, nullptr, rows, cols, max_keypoints_, keypoints.data(),
                                        descriptors.data(), cap, &n);
      if (rc == RGBDFE_OK) break;
      if (rc != RGBDFE_ERR_CAPACITY) { n = 0; break; }   // "SIFTGPU->RunSIFT() failed!" (:158): no features
      cap = n;                                            // n = the number of features: once more with room for them
    }
    keypoints.resize((size_t)n);
    descriptors.resize((size_t)n * 128);
  }
 private:
  FrontEnd fe_;
  int max_keypoints_;
};

// A colour (or mono) image and a raw depth image as the sensor messages carry them (rgbdfe_sensor_frame): what
// OpenNIListener::noCloudCallback receives.  visual_encoding: RGBDFE_VISUAL_MONO8 / _RGB8 / _BGR8 (sensor_msgs "mono8" / "rgb8" /
// "bgr8"); depth_encoding: RGBDFE_DEPTH_32FC1 (metres) / _16UC1 (millimetres).  Steps are bytes per row (cv::Mat::step).
struct SensorFrame : rgbdfe_sensor_frame {
  SensorFrame(const uint8_t* visual_data, int visual_rows_, int visual_cols_, size_t visual_step_, int visual_encoding_,
              const void* depth_data, int depth_rows_, int depth_cols_, size_t depth_step_, int depth_encoding_) {
    visual = visual_data; visual_rows = visual_rows_; visual_cols = visual_cols_; visual_step = (int32_t)visual_step_;
    visual_encoding = visual_encoding_;
    depth = depth_data; depth_rows = depth_rows_; depth_cols = depth_cols_; depth_step = (int32_t)depth_step_;
    depth_encoding = depth_encoding_;
  }
};

class Node {  // the slice of src/node.h the pair path touches
 public:
  // feature_descriptors: n x 32 bytes (cv::Mat CV_8U, continuous); feature_locations_3d: n x (x,y,z,1)
  Node(const FrontEnd& fe, int id, const uint8_t* feature_descriptors, const float* feature_locations_3d, int n)
      : id_(id), fe_(fe), n_(n) {
    matchable_ = rgbdfe_upload_node(fe_.get(), id_, feature_descriptors, feature_locations_3d, n) == RGBDFE_OK;
  }
  // The depth-image constructor (src/node.cpp:139-210): detect (grid of threshold-adaptive ORB detectors) ->
  // removeDepthless -> retainBest(max_keypoints) -> cv::ORB::compute -> projectTo3D, then the node's features go to the
  // device.  gray / mask: rows x cols uint8 (mask may be null), depth: rows x cols float metres.  The 2-D keypoints,
  // descriptors and points stay available as in the reference (feature_locations_2d_, feature_descriptors_,
  // feature_locations_3d_).  The detector's per-cell thresholds live in the FrontEnd and carry over from node to node.
  Node(const FrontEnd& fe, int id, const uint8_t* gray, const uint8_t* mask, const float* depth, int rows, int cols,
       double fx, double fy, double cx, double cy, double depth_scaling, int max_keypoints)
      : id_(id), fe_(fe), n_(0) {
    std::vector<rgbdfe_keypoint> kp((size_t)max_keypoints);
    feature_descriptors_.resize((size_t)max_keypoints * 32);
    feature_locations_3d_.resize((size_t)max_keypoints * 4);
    int32_t n = 0;
    if (rgbdfe_detect_describe(fe_.get(), gray, mask, depth, rows, cols, fx, fy, cx, cy, depth_scaling, kp.data(),
                               feature_descriptors_.data(), feature_locations_3d_.data(), &n) != RGBDFE_OK)
      n = 0;
    n_ = n;
    feature_descriptors_.resize((size_t)n * 32);
    feature_locations_3d_.resize((size_t)n * 4);
    feature_locations_2d_.assign(kp.begin(), kp.begin() + n);
    matchable_ = n > 0 && rgbdfe_upload_node(fe_.get(), id_, feature_descriptors_.data(), feature_locations_3d_.data(), n) == RGBDFE_OK;
  }
  // The same constructor on the images as the listener receives them (openni_listener.cpp:651-659 + node.cpp:139-210): the
  // depth image is resampled to the visual size where it differs, depthToCV8UC1 makes the detection mask (and metres of a
  // 16UC1 image), a CV_8UC3 image goes through CV_RGB2GRAY -- all on the device, in front of the steps above
  // (rgbdfe_sensor_detect_describe).
  Node(const FrontEnd& fe, int id, const SensorFrame& frame, double fx, double fy, double cx, double cy, double depth_scaling,
       int max_keypoints)
      : id_(id), fe_(fe), n_(0) {
    std::vector<rgbdfe_keypoint> kp((size_t)max_keypoints);
    feature_descriptors_.resize((size_t)max_keypoints * 32);
    feature_locations_3d_.resize((size_t)max_keypoints * 4);
    int32_t n = 0;
    if (rgbdfe_sensor_detect_describe(fe_.get(), &frame, fx, fy, cx, cy, depth_scaling, kp.data(), feature_descriptors_.data(),
                                      feature_locations_3d_.data(), &n) != RGBDFE_OK)
      n = 0;
    n_ = n;
    feature_descriptors_.resize((size_t)n * 32);
    feature_locations_3d_.resize((size_t)n * 4);
    feature_locations_2d_.assign(kp.begin(), kp.begin() + n);
    matchable_ = n > 0 && rgbdfe_upload_node(fe_.get(), id_, feature_descriptors_.data(), feature_locations_3d_.data(), n) == RGBDFE_OK;
  }
  // A node of 128-d float descriptors for matcher_type == "SIFTGPU" (Node::siftgpu_descriptors, node.h:172;
  // Node::featureMatching's SIFTGPU branch, node.cpp:553-557): desc128 = n x 128 floats
  struct SiftDescriptors {};
  Node(const FrontEnd& fe, int id, const float* desc128, const float* feature_locations_3d, int n, SiftDescriptors)
      : id_(id), fe_(fe), n_(n), sift_(true) {
    matchable_ = rgbdfe_upload_sift_node(fe_.get(), id_, desc128, feature_locations_3d, n) == RGBDFE_OK;
  }
  // The depth-image constructor with feature_detector_type == "SIFTGPU" (node.cpp:147-152, 195-200): SiftGPUWrapper::detect ->
  // projectTo3DSiftGPU (:695-769: truncating depth lookup, NaN depth drops the keypoint, max_keypoints cut, descriptors
  // re-packed) -> the node's siftgpu_descriptors go to the device for the SIFTGPU matcher branch.
  struct SiftGPU {};
  Node(const FrontEnd& fe, int id, const uint8_t* gray, const float* depth, int rows, int cols, double fx, double fy, double cx,
       double cy, double depth_scaling, int max_keypoints, SiftGPU)
      : id_(id), fe_(fe), n_(0), sift_(true) {
    std::vector<rgbdfe_keypoint> kp;
    std::vector<float> desc;
    SiftGPUWrapper(fe, max_keypoints).detect(gray, rows, cols, kp, desc);
    const int m = (int)kp.size();
    std::vector<float> xy((size_t)m * 2);
    for (int i = 0; i < m; ++i) { xy[(size_t)2 * i] = kp[(size_t)i].x; xy[(size_t)2 * i + 1] = kp[(size_t)i].y; }
    std::vector<int32_t> kept((size_t)(m > 0 ? m : 1));
    feature_locations_3d_.resize((size_t)(m > 0 ? m : 1) * 4);
    siftgpu_descriptors_.resize((size_t)(m > 0 ? m : 1) * 128);
    int32_t n = 0;
    if (m > 0 && rgbdfe_sift_node_features(fe_.get(), xy.data(), m, desc.data(), depth, rows, cols, fx, fy, cx, cy, depth_scaling,
                                           max_keypoints, 0, kept.data(), feature_locations_3d_.data(),
                                           siftgpu_descriptors_.data(), nullptr, &n) != RGBDFE_OK)
      n = 0;
    n_ = n;
    feature_locations_3d_.resize((size_t)n * 4);
    siftgpu_descriptors_.resize((size_t)n * 128);
    for (int i = 0; i < n; ++i) feature_locations_2d_.push_back(kp[(size_t)kept[(size_t)i]]);
    matchable_ = n > 0 && rgbdfe_upload_sift_node(fe_.get(), id_, siftgpu_descriptors_.data(), feature_locations_3d_.data(), n) == RGBDFE_OK;
  }
  // The point-cloud constructor (src/node.cpp:218-369): detect -> projectTo3D(cloud) (maximum_depth, truncating lookup,
  // the max_keypoints cut, :855-898) -> cv::ORB::compute.  cloud: rows x cols x (x, y, z, rgb) floats, organised.
  struct FromPointCloud {};
  Node(const FrontEnd& fe, int id, const uint8_t* gray, const uint8_t* mask, const float* cloud, int rows, int cols,
       double maximum_depth, int max_keypoints, FromPointCloud)
      : id_(id), fe_(fe), n_(0) {
    std::vector<rgbdfe_keypoint> kp((size_t)max_keypoints);
    feature_descriptors_.resize((size_t)max_keypoints * 32);
    feature_locations_3d_.resize((size_t)max_keypoints * 4);
    int32_t n = 0;
    if (rgbdfe_detect_describe_cloud(fe_.get(), gray, mask, cloud, rows, cols, maximum_depth, kp.data(),
                                     feature_descriptors_.data(), feature_locations_3d_.data(), &n) != RGBDFE_OK)
      n = 0;
    n_ = n;
    feature_descriptors_.resize((size_t)n * 32);
    feature_locations_3d_.resize((size_t)n * 4);
    feature_locations_2d_.assign(kp.begin(), kp.begin() + n);
    matchable_ = n > 0 && rgbdfe_upload_node(fe_.get(), id_, feature_descriptors_.data(), feature_locations_3d_.data(), n) == RGBDFE_OK;
  }
  ~Node() { clearFeatureInformation(); }
  Node(const Node&) = delete;
  Node& operator=(const Node&) = delete;

  // src/node.cpp:1305-1429.  Never throws; no edge <=> mr.edge.id1 == -1 && mr.edge.id2 == -1.
  MatchingResult matchNodePair(const Node* older_node) const {
    rgbdfe_match_result pod;
    if (!matchable_ || !older_node || !older_node->matchable_) return MatchingResult();
    if (sift_) {  // SiftGPUWrapper::match semantics; the distances are the float L2 of the raw descriptors
      std::vector<float> dist((size_t)RGBDFE_MAX_MATCHES);
      if (rgbdfe_match_sift_pair_list(fe_.get(), &id_, &older_node->id_, 1, &pod, dist.data()) != RGBDFE_OK)
        return MatchingResult();
      return toMatchingResult(pod, dist.data());
    }
    if (rgbdfe_match_node_pairs(fe_.get(), id_, &older_node->id_, 1, &pod) != RGBDFE_OK) return MatchingResult();
    return toMatchingResult(pod);
  }
  // src/node.cpp:535-690 (ORB branch): matches sorted by (hd, queryIdx), at most max_matches
  unsigned int featureMatching(const Node* other, std::vector<DMatch>* matches) const {
    *matches = matchNodePair(other).all_matches;
    return (unsigned int)matches->size();
  }
  // Node::pc_col (createXYZRGBPointCloud, src/misc.cpp:467-556): built on the device from the depth image and kept
  // resident for the environment measurement model; rgb may be null
  bool setPointCloud(const float* depth, int rows, int cols, const uint8_t* rgb, int rgb_channels, bool encoding_bgr,
                     double fx, double fy, double cx, double cy, double depth_scaling, double minimum_depth,
                     int cloud_creation_skip_step) {
    return rgbdfe_upload_node_cloud(fe_.get(), id_, depth, rows, cols, rgb, rgb_channels, encoding_bgr ? 1 : 0, fx, fy,
                                    cx, cy, depth_scaling, minimum_depth, cloud_creation_skip_step, nullptr) == RGBDFE_OK;
  }
  // ... and a copy of it for the host: rows x cols x (x, y, z, rgb bits), also for a cloud the sensor batch path has kept.
  // A cloud of no points (a reduced cloud without a valid point: 1 row, 0 columns) is a cloud too: true and empty.
  bool pointCloud(std::vector<float>* cloud, int* rows = nullptr, int* cols = nullptr) const {
    int32_t r = 0, c = 0;
    // the size first (RGBDFE_ERR_CAPACITY reports it; a cloud of no points is RGBDFE_OK), then the points
    const int rc = rgbdfe_download_node_cloud(fe_.get(), id_, nullptr, 0, &r, &c);
    if (rc != RGBDFE_OK && rc != RGBDFE_ERR_CAPACITY) return false;
    cloud->resize((size_t)r * (size_t)c * 4);
    if (rows) *rows = r;
    if (cols) *cols = c;
    return rc == RGBDFE_OK || rgbdfe_download_node_cloud(fe_.get(), id_, cloud->data(), (int64_t)r * c, &r, &c) == RGBDFE_OK;
  }
  // Node::reducePointCloud (src/node.cpp:1448-1460): pc_col becomes its voxel-filtered cloud, unstructured (pointCloud()
  // then reports 1 row).  Like the reference, vfs <= 0 changes nothing (the reference warns: "Point Clouds can't be reduced
  // because of invalid voxelfilter_size").  points / flags (optional): the rows of the cloud afterwards, rgbdfe_voxel_filter's flags.
  bool reducePointCloud(double vfs, int64_t* points = nullptr, int32_t* flags = nullptr) {
    if (!(vfs > 0.0)) return false;
    int64_t n = 0;
    int32_t f = 0;
    if (rgbdfe_reduce_node_cloud(fe_.get(), id_, vfs, &n, &f) != RGBDFE_OK) return false;
    if (points) *points = n;
    if (flags) *flags = f;
    return true;
  }
  // feature_locations_2d_ (node.h:160): only the g2o pair refinement reads them (params.g2o_iterations > 0,
  // node.cpp:1222-1268); kp_xy = n x (u, v)
  bool setKeypoints(const float* kp_xy) { return rgbdfe_upload_node_keypoints(fe_.get(), id_, kp_xy, n_) == RGBDFE_OK; }
  void clearFeatureInformation() {  // src/node.cpp:1431-1443
    if (matchable_) rgbdfe_release_node(fe_.get(), id_);
    matchable_ = false;
  }
  int id_;
  bool matchable_ = false;
  // filled by the depth-image constructor only (node.h:160-170)
  std::vector<rgbdfe_keypoint> feature_locations_2d_;
  std::vector<uint8_t> feature_descriptors_;   // n x 32
  std::vector<float> feature_locations_3d_;    // n x (x, y, z, 1)
  std::vector<float> siftgpu_descriptors_;     // n x 128 (node.h:172; SiftGPU nodes built from an image)
  int featureCount() const { return n_; }

 private:
  const FrontEnd& fe_;
  int n_;
  bool sift_ = false;
  friend class GraphManager;
};

class GraphManager {  // candidate selection (graph_manager.cpp:204-324) + the fan-out of nodeComparisons (:531-583)
 public:
  explicit GraphManager(const FrontEnd& fe)
      : fe_(fe), topology_(rgbdfe_pose_graph_create(), &rgbdfe_pose_graph_destroy) {
    if (!topology_) throw std::runtime_error("rgbdfe_pose_graph_create failed");
  }
  // what addNode / addEdgeToG2O tell the pose graph (graph_manager.cpp:681, :811); candidate selection reads it
  void nodeAdded(const Node* n, int vertex_id, bool keyframe) {
    rgbdfe_pose_graph_add_node(topology_.get(), n->id_, vertex_id, n->matchable_ ? 1 : 0, keyframe ? 1 : 0);
  }
  void edgeAdded(int id1, int id2) { rgbdfe_pose_graph_add_edge(topology_.get(), id1, id2); }
  // GraphManager::addEdgeToG2O (graph_manager.cpp:811-909): the edge with its measurement enters the optimizer (and the
  // topology candidate selection reads); set_estimate: the second node's estimate becomes X1 * transform (:858,864)
  bool addEdgeToG2O(const LoadedEdge3D& edge, bool set_estimate = false) {
    double info[36] = {0};
    for (int k = 0; k < 6; ++k) info[7 * k] = edge.informationScale;
    return rgbdfe_pose_graph_add_edge_se3(topology_.get(), edge.id1, edge.id2, edge.transform.data(), info,
                                          set_estimate ? 1 : 0) == RGBDFE_OK;
  }
  // pose_relative_to (fixationOfVertices, :911-937): the caller fixes the vertices of its choice, or the graph keeps a strategy
  // (RGBDFE_POSE_RELATIVE_TO_FIRST / _PREVIOUS / _LARGEST_LOOP / _INAFFECTED; _NONE: the flags of setFixed as they stand)
  bool setPoseRelativeTo(int strategy) { return rgbdfe_pose_graph_set_strategy(topology_.get(), strategy) == RGBDFE_OK; }
  bool setFixed(int node_id, bool fixed = true) {
    return rgbdfe_pose_graph_set_fixed(topology_.get(), node_id, fixed ? 1 : 0) == RGBDFE_OK;
  }
  // double GraphManager::optimizeGraph(double break_criterion) (:938-1066; optimizer_iterations, default 0.01): Levenberg-
  // Marquardt + PCG on the device; returns chi2, negative on failure.  report (optional): iterations, trials, PCG counts.
  double optimizeGraph(double break_criterion = 0.01, rgbdfe_pose_graph_report* report = nullptr) {
    rgbdfe_pose_graph_report local;
    rgbdfe_pose_graph_report* rep = report ? report : &local;
    if (rgbdfe_pose_graph_optimize_graph(fe_.get(), topology_.get(), break_criterion, rep) != RGBDFE_OK) return -1.0;
    return rep->chi2;
  }
  // unsigned int GraphManager::pruneEdgesWithErrorAbove(float thresh) (:1106-1246) on the device; -1 on failure.
  // verdicts (optional): RGBDFE_PRUNE_* per measured edge in insertion order
  int pruneEdgesWithErrorAbove(float thresh, std::vector<uint8_t>* verdicts = nullptr) {
    int32_t n = 0;
    // the edge count: RGBDFE_ERR_CAPACITY reports it, a graph without measured edges is RGBDFE_OK
    const int rc = rgbdfe_pose_graph_edge_errors(fe_.get(), topology_.get(), nullptr, nullptr, nullptr, 0, &n);
    if (rc != RGBDFE_OK && rc != RGBDFE_ERR_CAPACITY) return -1;
    std::vector<uint8_t> local((size_t)n);
    int32_t pruned = 0;
    if (rgbdfe_pose_graph_prune_edges(fe_.get(), topology_.get(), thresh, local.data(), n, &pruned) != RGBDFE_OK) return -1;
    if (verdicts) verdicts->swap(local);
    return pruned;
  }
  // void GraphManager::sanityCheck(float thresh) (:1347-1360); returns the number of edges changed
  int sanityCheck(float thresh) { return rgbdfe_pose_graph_sanity_check(topology_.get(), thresh); }
  // the five optimisation rounds of OpenNIListener::evaluation (openni_listener.cpp:431-518); estimates (optional): after
  // every round all nodes in ascending id, 16 column-major doubles each
  bool evaluation(double optimizer_iterations, rgbdfe_pose_graph_evaluation* out = nullptr, std::vector<double>* estimates = nullptr,
                  int n_nodes = 0) {
    if (estimates) estimates->assign((size_t)RGBDFE_POSE_GRAPH_EVALUATION_ROUNDS * 16 * (size_t)n_nodes, 0.0);
    return rgbdfe_pose_graph_evaluate(fe_.get(), topology_.get(), optimizer_iterations, out, estimates ? estimates->data() : nullptr,
                                      n_nodes) == RGBDFE_OK;
  }
  // GraphManager::saveTrajectory's estimate file (graph_mgr_io.cpp:615-677), TUM format
  bool saveTrajectory(const std::string& path, const std::vector<int32_t>& node_ids, const std::vector<double>& stamps,
                      const double* base2points = nullptr, const double* init_base_pose = nullptr, const char* frame_id = nullptr,
                      const char* child_frame_id = nullptr) const {
    if (node_ids.size() != stamps.size()) return false;
    return rgbdfe_pose_graph_write_trajectory(topology_.get(), path.c_str(), (int32_t)node_ids.size(), node_ids.data(), stamps.data(),
                                              base2points, init_base_pose, frame_id, child_frame_id) == RGBDFE_OK;
  }
  // the estimates of node_ids as n x 16 floats (column-major Matrix4f): the world2cam of assembleMap / the OctoMap calls
  std::vector<float> transforms(const std::vector<int32_t>& node_ids) const {
    std::vector<float> out(16 * node_ids.size());
    if (rgbdfe_pose_graph_transforms(topology_.get(), (int32_t)node_ids.size(), node_ids.data(), out.data()) != RGBDFE_OK) return {};
    return out;
  }
  // QList<int> GraphManager::getPotentialEdgeTargetsWithDijkstra(new_node, sequential_targets, geodesic_targets,
  // sampled_targets, predecessor_id, include_predecessor); geodesic_depth is the parameter server's "geodesic_depth".
  // rand_fn == nullptr: reproducible draws from `seed` instead of rand().
  std::vector<int> getPotentialEdgeTargetsWithDijkstra(const Node* /*new_node*/, int sequential_targets,
                                                       int geodesic_targets, int sampled_targets,
                                                       int predecessor_id = -1, bool include_predecessor = false,
                                                       int geodesic_depth = 3, rgbdfe_rand_fn rand_fn = nullptr,
                                                       void* rand_state = nullptr, uint32_t seed = 0) const {
    std::vector<int32_t> ids((size_t)(sequential_targets + geodesic_targets + sampled_targets + 1));
    int32_t n = 0;
    if (rgbdfe_potential_edge_targets(topology_.get(), sequential_targets, geodesic_targets, sampled_targets,
                                      geodesic_depth, predecessor_id, include_predecessor ? 1 : 0, rand_fn, rand_state,
                                      seed, ids.data(), (int32_t)ids.size(), &n) != RGBDFE_OK)
      return {};
    return std::vector<int>(ids.begin(), ids.begin() + n);
  }
  // GraphManager::getNeighbours (loop_closing.cpp:190-277): candidates ranked by the votes of the new node's
  // descriptors (exact Hamming neighbours); returns at most max_out node ids, best first
  std::vector<int> getNeighbours(const Node* new_node, const std::vector<const Node*>& candidates, int neighbour_cnt,
                                 int max_out, int max_hd = 256) const {
    std::vector<int32_t> ids, out((size_t)std::max(max_out, 0));
    std::vector<float> score(out.size());
    for (const Node* n : candidates) ids.push_back(n->id_);
    int32_t n_out = 0;
    if (ids.empty() || out.empty() ||
        rgbdfe_place_recognition(fe_.get(), new_node->id_, ids.data(), (int32_t)ids.size(), neighbour_cnt, max_hd,
                                 (int32_t)out.size(), out.data(), score.data(), &n_out) != RGBDFE_OK)
      return {};
    return std::vector<int>(out.begin(), out.begin() + n_out);
  }
  // Node::matchNodePair's ICP branch (node.cpp:1356-1377) for the results of nodeComparisons(new_node, nodes_to_comp): every
  // result WITHOUT an edge whose node is adjacent (new id - its id <= 1) is aligned by rgbdfe_icp_align_nodes in one batch,
  // source = the older node's resident cloud, target = the new node's, guess = identity.  When converged: icp_trafo,
  // final_trafo = icp_trafo (the literal assignment, whatever direction the RANSAC transforms have), edge.id1 / id2 and
  // edge.transform are set (:1370-1373) and nothing else.  Returns the number of results that got an edge, -1 on an error.
  int icpFallback(const Node* new_node, const std::vector<const Node*>& nodes_to_comp, std::vector<MatchingResult>& results,
                  const rgbdfe_icp_params* params = nullptr, std::vector<rgbdfe_icp_report>* reports = nullptr) const {
    rgbdfe_icp_params prm;
    if (params) prm = *params; else rgbdfe_icp_default_params(&prm);
    std::vector<size_t> served;
    std::vector<int32_t> source, target;
    for (size_t i = 0; i < results.size() && i < nodes_to_comp.size(); ++i)
      if (results[i].edge.id1 < 0 && new_node->id_ - nodes_to_comp[i]->id_ <= 1) {
        served.push_back(i);
        source.push_back(nodes_to_comp[i]->id_);
        target.push_back(new_node->id_);
      }
    if (served.empty()) return 0;
    std::vector<float> T(16 * served.size());
    std::vector<rgbdfe_icp_report> rep(served.size());
    if (rgbdfe_icp_align_nodes(fe_.get(), (int32_t)served.size(), source.data(), target.data(), nullptr, &prm, T.data(),
                               rep.data()) != RGBDFE_OK)
      return -1;
    int edges = 0;
    for (size_t k = 0; k < served.size(); ++k) {
      if (!rep[k].converged) continue;
      MatchingResult& mr = results[served[k]];
      for (int i = 0; i < 16; ++i) {
        mr.icp_trafo[i] = mr.final_trafo[i] = T[16 * k + i];
        mr.edge.transform[i] = (double)T[16 * k + i];
      }
      mr.edge.id1 = source[k];
      mr.edge.id2 = target[k];
      ++edges;
    }
    if (reports) *reports = rep;
    return edges;
  }
  // 1:1 replacement of QtConcurrent::blockingMapped(nodes_to_comp, bind(&Node::matchNodePair, new_node, _1))
  std::vector<MatchingResult> nodeComparisons(const Node* new_node, const std::vector<const Node*>& nodes_to_comp) const {
    std::vector<int32_t> ids;
    ids.reserve(nodes_to_comp.size());
    for (const Node* n : nodes_to_comp) ids.push_back(n->id_);
    std::vector<rgbdfe_match_result> pods(ids.size());
    std::vector<MatchingResult> out(ids.size());
    if (ids.empty()) return out;
    if (new_node->sift_) {  // matcher_type == "SIFTGPU": the same fan-out over the SIFT pair op
      std::vector<int32_t> q(ids.size(), new_node->id_);
      std::vector<float> dist(ids.size() * (size_t)RGBDFE_MAX_MATCHES);
      if (rgbdfe_match_sift_pair_list(fe_.get(), q.data(), ids.data(), (int32_t)ids.size(), pods.data(), dist.data()) != RGBDFE_OK)
        return out;
      for (size_t i = 0; i < pods.size(); ++i) out[i] = toMatchingResult(pods[i], dist.data() + i * (size_t)RGBDFE_MAX_MATCHES);
      return out;
    }
    if (rgbdfe_match_node_pairs(fe_.get(), new_node->id_, ids.data(), (int32_t)ids.size(), pods.data()) != RGBDFE_OK)
      return out;
    for (size_t i = 0; i < pods.size(); ++i) out[i] = toMatchingResult(pods[i]);
    return out;
  }

  // bool GraphManager::addNode(Node* new_node) (graph_manager.cpp:681-782) as one call over the stages above: the node is
  // resident under new_node->id_ (its slot), the stamp is its header's.  Candidate selection, the pair batch, the
  // decisions, the pose graph, updateInlierFeatures and the optimiser run inside; `step` (optional) says what happened, in
  // graph ids (step->id: the id the node got, -1 when the frame was dropped; slotOf(id) leads back to the slot).  The
  // parameters are fixed by the first call (slamParams() before it changes them).  Returns what the reference returns:
  // the node was added.  false is a dropped frame OR a failed call: lastAddNodeStatus() tells them apart (RGBDFE_OK after a
  // step that ran, whatever it decided; the rgbdfe_status of the failing call otherwise, rgbdfe_last_error has its words).
  // Do not mix with nodeAdded / addEdgeToG2O on the same object: the step keeps the graph itself.
  rgbdfe_slam_params& slamParams() {
    if (!slam_params_set_) { rgbdfe_slam_default_params(&slam_params_); slam_params_set_ = true; }
    return slam_params_;
  }
  bool addNode(const Node* new_node, int64_t stamp_sec, int32_t stamp_nsec, rgbdfe_slam_step* step = nullptr) {
    if (!slam_) {
      rgbdfe_slam* s = nullptr;
      add_node_status_ = rgbdfe_slam_create(fe_.get(), topology_.get(), &slamParams(), &s);
      if (add_node_status_ != RGBDFE_OK) return false;
      slam_.reset(s);
    }
    rgbdfe_slam_step local;
    rgbdfe_slam_step* st = step ? step : &local;
    add_node_status_ = rgbdfe_slam_add_node(slam_.get(), new_node->id_, stamp_sec, stamp_nsec, st);
    if (add_node_status_ != RGBDFE_OK) return false;
    return st->status == RGBDFE_SLAM_FIRST || st->status == RGBDFE_SLAM_ADDED || st->status == RGBDFE_SLAM_REPLACED_FIRST;
  }
  int lastAddNodeStatus() const { return add_node_status_; }
  // Session files (rgbdfe_session_save / _load): the front end's resident nodes -- features, keypoints, counters, with
  // `clouds` their clouds --, the detector's state, this object's graph and, once addNode has run, its decision machine.
  // loadSession wants a fresh GraphManager on a FrontEnd that holds none of the file's nodes, with slamParams() as they were
  // when the file was written; the run then continues, byte for byte, as the saved one would have.  The loaded nodes are
  // resident under their ids without a Node object: release them with rgbdfe_release_node.  false: lastAddNodeStatus() has
  // the status, rgbdfe_last_error the cause.
  bool saveSession(const std::string& path, bool clouds = false) {
    add_node_status_ = rgbdfe_session_save(fe_.get(), slam_.get(), topology_.get(), clouds ? RGBDFE_SESSION_CLOUDS : 0u, path.c_str());
    return add_node_status_ == RGBDFE_OK;
  }
  bool loadSession(const std::string& path) {
    if (!slam_) {
      rgbdfe_slam* s = nullptr;
      add_node_status_ = rgbdfe_slam_create(fe_.get(), topology_.get(), &slamParams(), &s);
      if (add_node_status_ != RGBDFE_OK) return false;
      slam_.reset(s);
    }
    add_node_status_ = rgbdfe_session_load(fe_.get(), slam_.get(), topology_.get(), path.c_str());
    return add_node_status_ == RGBDFE_OK;
  }
  int slotOf(int graph_id) const { return slam_ ? rgbdfe_slam_slot_of(slam_.get(), graph_id) : RGBDFE_ERR_UNKNOWN_NODE; }
  bool validTfEstimate(int graph_id) const { return slam_ && rgbdfe_slam_valid_tf(slam_.get(), graph_id) == 1; }
  std::vector<int32_t> keyframeIds() const {
    std::vector<int32_t> ids;
    if (!slam_) return ids;
    int32_t n = 0;
    ids.resize((size_t)rgbdfe_slam_node_count(slam_.get()) + 1);
    if (rgbdfe_slam_keyframes(slam_.get(), ids.data(), (int32_t)ids.size(), &n) != RGBDFE_OK) n = 0;
    ids.resize((size_t)n);
    return ids;
  }

 private:
  const FrontEnd& fe_;
  std::unique_ptr<rgbdfe_pose_graph, void (*)(rgbdfe_pose_graph*)> topology_;
  std::unique_ptr<rgbdfe_slam, void (*)(rgbdfe_slam*)> slam_{nullptr, &rgbdfe_slam_destroy};   // (goes before topology_)
  rgbdfe_slam_params slam_params_;
  bool slam_params_set_ = false;
  int add_node_status_ = RGBDFE_OK;
};

// The loop of GraphManager::saveAllCloudsToFile (src/graph_mgr_io.cpp:529-552): transformAndAppendPointCloud
// (src/misc.cpp:183-238) for the pc_col of every listed node, on the device.  node_ids in graph_ order without the nodes
// that have no valid estimate; world2cam = n x 16 floats, the column-major Matrix4f of pcl_ros::transformAsMatrix(cam2rgb *
// eigenTransf2TF(v->estimate())) per node; maximum_depth and preserve_raster_on_save are the parameters of those names.
// aggregate_cloud = rows of (x, y, z, rgb bits); node_offsets (optional) = the first row of every node, then the row count.
// voxelfilter_size > 0 (parameter "voxelfilter_size"): the aggregate cloud is voxel-filtered on the device before it is
// returned (GraphManager::reducePointCloud's filter, applied to the whole map); node_offsets then still describe the
// unfiltered cloud.  This header knows no device allocator, so the assembled points pass through the host between the two
// device steps; a caller with device buffers of its own chains rgbdfe_assemble_map_device and voxelFilter instead.
inline bool assembleAllClouds(const FrontEnd& fe, const std::vector<int32_t>& node_ids, const std::vector<float>& world2cam,
                              double maximum_depth, bool preserve_raster_on_save, std::vector<float>* aggregate_cloud,
                              std::vector<int64_t>* node_offsets = nullptr, double voxelfilter_size = 0.0) {
  if (world2cam.size() != node_ids.size() * 16) return false;
  std::vector<int64_t> off(node_ids.size() + 1, 0);
  int64_t n = 0;
  const int32_t raster = preserve_raster_on_save ? 1 : 0;
  // the size first (RGBDFE_ERR_CAPACITY reports it; an empty result is RGBDFE_OK), then the points
  int rc = rgbdfe_assemble_map(fe.get(), (int32_t)node_ids.size(), node_ids.data(), world2cam.data(), maximum_depth, raster,
                               nullptr, 0, &n, off.data());
  if (rc != RGBDFE_OK && rc != RGBDFE_ERR_CAPACITY) return false;
  aggregate_cloud->resize((size_t)n * 4);
  if (rc == RGBDFE_ERR_CAPACITY &&
      rgbdfe_assemble_map(fe.get(), (int32_t)node_ids.size(), node_ids.data(), world2cam.data(), maximum_depth, raster,
                          aggregate_cloud->data(), n, &n, off.data()) != RGBDFE_OK)
    return false;
  if (node_offsets) *node_offsets = off;
  if (voxelfilter_size > 0.0 && n > 0) {
    std::vector<float> filtered((size_t)n * 4);  // n rows always suffice
    int64_t kept = 0;
    if (rgbdfe_voxel_filter(fe.get(), aggregate_cloud->data(), n, voxelfilter_size, filtered.data(), n, &kept, nullptr) != RGBDFE_OK)
      return false;
    filtered.resize((size_t)kept * 4);
    aggregate_cloud->swap(filtered);
  }
  return true;
}

// GraphManager::saveAllCloudsToFile (src/graph_mgr_io.cpp:502-582) as a whole: the loop above AND the file, streamed group
// by group so that the map is never whole in memory (rgbdfe_save_map).  filename follows the reference's name rule (*.ply in
// any case: binary PLY; otherwise binary PCD, ".pcd" appended unless it is there); path_written (optional) receives the
// name after the rule, stats (optional) the call's report.  No point: no file, true, stats->points == 0.
inline bool rgbdfe_save_map(const FrontEnd& fe, const std::vector<int32_t>& node_ids, const std::vector<float>& world2cam,
                            double maximum_depth, bool preserve_raster_on_save, const std::string& filename,
                            std::string* path_written = nullptr, rgbdfe_map_file_stats* stats = nullptr, int64_t chunk_points = 0) {
  if (world2cam.size() != node_ids.size() * 16) return false;
  std::vector<char> written(filename.size() + 8, 0);
  if (::rgbdfe_save_map(fe.get(), (int32_t)node_ids.size(), node_ids.data(), world2cam.data(), maximum_depth,
                        preserve_raster_on_save ? 1 : 0, filename.c_str(), chunk_points, written.data(), (int64_t)written.size(),
                        stats) != RGBDFE_OK)
    return false;
  if (path_written) *path_written = written.data();
  return true;
}

// GraphManager::saveIndividualCloudsToFile (src/graph_mgr_io.cpp:330-433) without its ground-truth branch:
// <file_basename>_%04d.pcd and .txt per listed node with a non-empty cloud, numbered by graph_ids (empty: node_ids).  poses =
// n x 16 doubles, the column-major v->estimate().matrix() per node (world2points where tf is involved: the caller's);
// transform_individual_clouds is the parameter of that name.  The resident clouds stay as they are.
inline bool rgbdfe_save_node_clouds(const FrontEnd& fe, const std::vector<int32_t>& node_ids, const std::vector<int32_t>& graph_ids,
                                    const std::vector<double>& poses, bool transform_individual_clouds,
                                    const std::string& file_basename, int32_t* n_written = nullptr) {
  if (poses.size() != node_ids.size() * 16 || (!graph_ids.empty() && graph_ids.size() != node_ids.size())) return false;
  return ::rgbdfe_save_node_clouds(fe.get(), (int32_t)node_ids.size(), node_ids.data(), graph_ids.empty() ? nullptr : graph_ids.data(),
                                   poses.data(), transform_individual_clouds ? 1 : 0, file_basename.c_str(), n_written) == RGBDFE_OK;
}

// The host-only calls: a cloud in host memory (rows of x, y, z, rgb bits) to a file of `format` (RGBDFE_CLOUD_FILE_*), a
// file's header, and a file's rows.  No device, no context: rgbdfe_last_error(NULL) has the cause of a failure.
inline bool rgbdfe_save_cloud_file(const std::vector<float>& points, int32_t width, int32_t height, int32_t format,
                                   const std::string& path, const float* viewpoint7 = nullptr) {
  if (width < 0 || height < 0 || points.size() != (size_t)width * (size_t)height * 4) return false;
  return ::rgbdfe_save_cloud_file(points.data(), width, height, viewpoint7, format, path.c_str()) == RGBDFE_OK;
}
inline bool rgbdfe_cloud_file_info(const std::string& path, rgbdfe_cloud_file_header* info) {
  return ::rgbdfe_cloud_file_info(path.c_str(), info) == RGBDFE_OK;
}
inline bool rgbdfe_load_cloud_file(const std::string& path, std::vector<float>* points, rgbdfe_cloud_file_header* info = nullptr) {
  rgbdfe_cloud_file_header h;
  if (::rgbdfe_cloud_file_info(path.c_str(), &h) != RGBDFE_OK) return false;
  points->resize((size_t)h.points * 4);
  if (::rgbdfe_load_cloud_file(path.c_str(), points->data(), h.points, &h) != RGBDFE_OK) return false;
  if (info) *info = h;
  return true;
}

// GLViewer::addPointCloud (src/glviewer.cpp:693-735) for every listed node, on the device: what pointCloud2GLPoints,
// pointCloud2GLTriangleList or pointCloud2GLStrip would have sent to the node's display list (rgbdfe_display_geometry).
// display_type is the parameter "cloud_display_type" ("POINTS", "TRIANGLES", anything else but "ELLIPSOIDS" / "NONE":
// TRIANGLE_STRIP); world2cam as assembleAllClouds takes it, or empty for vertices in the node frame (the viewer's own way: it
// applies cloud_matrices in GL).  vertices = rows of (x, y, z, rgb bits: a GL_BGRA colour); strips = (first vertex, vertex
// count) per glBegin(GL_TRIANGLE_STRIP).
struct DisplayGeometry {
  std::vector<float> vertices;
  std::vector<int64_t> strips, node_offsets, node_strip_offsets;
  std::vector<int32_t> node_types;  // RGBDFE_DISPLAY_* per node: a cloud of one row is drawn as points
};
inline int32_t displayTypeFromParameter(const std::string& cloud_display_type) {
  if (cloud_display_type == "TRIANGLES") return RGBDFE_DISPLAY_TRIANGLES;
  if (cloud_display_type == "POINTS") return RGBDFE_DISPLAY_POINTS;
  return RGBDFE_DISPLAY_TRIANGLE_STRIP;  // glviewer.cpp:708: "TRIANGLE_STRIP is default"
}
inline bool displayGeometry(const FrontEnd& fe, const std::vector<int32_t>& node_ids, const std::vector<float>& world2cam,
                            const rgbdfe_display_params& params, DisplayGeometry* out) {
  if (!world2cam.empty() && world2cam.size() != node_ids.size() * 16) return false;
  const int32_t n = (int32_t)node_ids.size();
  const float* T = world2cam.empty() ? nullptr : world2cam.data();
  out->node_offsets.assign(node_ids.size() + 1, 0);
  out->node_strip_offsets.assign(node_ids.size() + 1, 0);
  out->node_types.assign(node_ids.size(), 0);
  int64_t nv = 0, ns = 0;
  // the sizes first (RGBDFE_ERR_CAPACITY reports both; an empty stream is RGBDFE_OK), then the vertices and records
  int rc = rgbdfe_display_geometry(fe.get(), n, node_ids.data(), T, &params, nullptr, 0, &nv, out->node_offsets.data(), nullptr, 0,
                                   &ns, out->node_strip_offsets.data(), out->node_types.data());
  if (rc != RGBDFE_OK && rc != RGBDFE_ERR_CAPACITY) return false;
  out->vertices.resize((size_t)nv * 4);
  out->strips.resize((size_t)ns * 2);
  if (rc == RGBDFE_ERR_CAPACITY &&
      rgbdfe_display_geometry(fe.get(), n, node_ids.data(), T, &params, out->vertices.data(), nv, &nv, out->node_offsets.data(),
                              out->strips.data(), ns, &ns, out->node_strip_offsets.data(), out->node_types.data()) != RGBDFE_OK)
    return false;
  return true;
}

// GLViewer::paintGL without a GL context (src/glviewer.cpp:291-425): the listed nodes' display geometry rasterised on the device
// (rgbdfe_render_nodes; the contract is include/rgbdfe.h, "rendering").  world2cam as displayGeometry takes it; render_params
// from renderParams() below, or rgbdfe_render_default_params for the viewer's initial position.  Images are height x width,
// row 0 at the top: rgba 4 bytes per pixel (a screencast frame), depth as glReadPixels(GL_DEPTH_COMPONENT) gives it, ids the
// primitive's first vertex in the stream (-1: nothing drawn), node_index the position in node_ids (-1).
struct RenderedImages {
  int32_t width = 0, height = 0;
  std::vector<uint8_t> rgba;
  std::vector<float> depth;
  std::vector<int64_t> ids;
  std::vector<int32_t> node_index;
};
// The viewer's camera at a window size: setViewPoint(pose) + drawClouds' modelview + resizeGL's projection.  viewpoint_pose: 16
// doubles, column-major (a cloud matrix, follow_mode_'s last one), or NULL for no viewpoint; the helper inverts it as
// setViewPoint does (a rigid pose).
inline rgbdfe_render_params renderParams(int32_t width, int32_t height, const double* viewpoint_pose = nullptr) {
  rgbdfe_render_params p;
  rgbdfe_render_default_params(&p);
  p.width = width;
  p.height = height;
  if (viewpoint_pose) {
    double inv[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) inv[4 * c + r] = viewpoint_pose[4 * r + c];
      inv[12 + r] = -(viewpoint_pose[4 * r] * viewpoint_pose[12] + viewpoint_pose[4 * r + 1] * viewpoint_pose[13] +
                      viewpoint_pose[4 * r + 2] * viewpoint_pose[14]);
    }
    rgbdfe_render_viewer_view(0.0, 0.0, -50.0, 180.0 * 16.0, 0.0, 0.0, 1.0, inv, p.view);  // initialPosition (:137-144)
  }
  rgbdfe_render_perspective(100.0 / 180.0 * 3.14159265358979323846, (double)((float)width / (float)height), 0.1, 1e4,
                            p.projection);  // fov_ as degrees, the reference's quirk (:118, :444)
  return p;
}
inline bool render(const FrontEnd& fe, const std::vector<int32_t>& node_ids, const std::vector<float>& world2cam,
                   const rgbdfe_display_params& display_params, const rgbdfe_render_params& render_params, RenderedImages* out,
                   bool with_ids = true) {
  if (!world2cam.empty() && world2cam.size() != node_ids.size() * 16) return false;
  if (render_params.width < 1 || render_params.height < 1 || render_params.width > 4096 || render_params.height > 4096) return false;
  const size_t n = (size_t)render_params.width * (size_t)render_params.height;
  out->width = render_params.width;
  out->height = render_params.height;
  out->rgba.resize(4 * n);
  out->depth.resize(n);
  out->ids.resize(with_ids ? n : 0);
  out->node_index.resize(with_ids ? n : 0);
  return rgbdfe_render_nodes(fe.get(), (int32_t)node_ids.size(), node_ids.data(), world2cam.empty() ? nullptr : world2cam.data(),
                             &display_params, &render_params, out->rgba.data(), out->depth.data(),
                             with_ids ? out->ids.data() : nullptr, with_ids ? out->node_index.data() : nullptr) == RGBDFE_OK;
}
// GLViewer::setClickedPosition (:1127-1153) on a rendered depth image: the world point under window pixel (x, y) with y
// counted from the top as Qt does, or false where nothing was drawn (depth 1).  The depth is the pixel's own; the reference
// reads window row height - y, the row above it, and hands the same winY to gluUnProject, as this does.
inline bool clickedPosition(const RenderedImages& img, const rgbdfe_render_params& render_params, int x, int y, double pos[3]) {
  if (x < 0 || y < 0 || x >= img.width || y >= img.height) return false;
  const float win_z = img.depth[(size_t)y * (size_t)img.width + (size_t)x];
  if (win_z == 1.0f) return false;  // :1141
  return rgbdfe_render_unproject((double)(float)x, (double)((float)img.height - (float)y), (double)win_z, render_params.view,
                                 render_params.projection, img.width, img.height, pos) == RGBDFE_OK;
}

// pcl::VoxelGrid with a cubic leaf of voxelfilter_size over a device buffer of n_in rows (x, y, z, rgb bits) into another of
// `capacity` rows on the context's device (rgbdfe_voxel_filter_device): the consumer of rgbdfe_assemble_map_device's output.
// Returns the rows written, or -1 (needed: the rows that would have been; flags: RGBDFE_VOXEL_LEAF_TOO_SMALL).
inline int64_t voxelFilter(const FrontEnd& fe, const void* d_points, int64_t n_in, double voxelfilter_size, void* d_out,
                           int64_t capacity, int32_t* flags = nullptr, void* stream = nullptr, int64_t* needed = nullptr) {
  int64_t n = 0;
  const int rc = rgbdfe_voxel_filter_device(fe.get(), d_points, n_in, voxelfilter_size, d_out, capacity, &n, flags, stream);
  if (needed) *needed = n;
  return rc == RGBDFE_OK ? n : -1;
}

// ColorOctomapServer (src/ColorOctomapServer.cpp) on the device: the seam of GraphManager::renderToOctomap / saveOctomapImpl
// (src/graph_mgr_io.cpp:253-329).  insertClouds is the loop over the nodes with a valid estimate: node_ids in graph_ order,
// world2cam as assembleAllClouds takes it, max_range = the parameter "maximum_depth".  When the table is full it grows (twice
// the cells) and goes on with the clouds that are not in yet, so a false return is an error, never a dropped cell.
class OctoMap {
 public:
  OctoMap(const FrontEnd& fe, int64_t capacity_cells, const rgbdfe_octomap_params* params = nullptr)
      : map_(nullptr, rgbdfe_octomap_destroy), capacity_(capacity_cells) {
    rgbdfe_octomap* m = nullptr;
    if (rgbdfe_octomap_create(fe.get(), params, capacity_cells, &m) == RGBDFE_OK) map_.reset(m);
  }
  bool valid() const { return (bool)map_; }
  rgbdfe_octomap* get() const { return map_.get(); }
  bool reset() { return map_ && rgbdfe_octomap_reset(map_.get()) == RGBDFE_OK; }  // ColorOctomapServer::reset
  bool reserve(int64_t capacity_cells) {
    if (!map_ || rgbdfe_octomap_reserve(map_.get(), capacity_cells) != RGBDFE_OK) return false;
    capacity_ = capacity_cells;
    return true;
  }
  bool insertClouds(const std::vector<int32_t>& node_ids, const std::vector<float>& world2cam, double max_range) {
    if (!map_ || world2cam.size() != node_ids.size() * 16) return false;
    size_t at = 0;
    while (at < node_ids.size()) {
      int32_t done = 0;
      const int rc = rgbdfe_octomap_insert_nodes(map_.get(), (int32_t)(node_ids.size() - at), node_ids.data() + at,
                                                 world2cam.data() + at * 16, max_range, &done);
      if (rc == RGBDFE_OK) return true;
      if (rc != RGBDFE_ERR_CAPACITY || !reserve(capacity_ * 2)) return false;
      at += (size_t)done;
    }
    return true;
  }
  int64_t size() const {
    int64_t n = 0;
    return map_ && rgbdfe_octomap_size(map_.get(), &n) == RGBDFE_OK ? n : -1;
  }
  // the leaves in ascending key order (key, log-odds, colour)
  bool leaves(std::vector<rgbdfe_octomap_leaf>* out) const {
    const int64_t n = size();
    if (n < 0) return false;
    out->resize((size_t)n);
    int64_t got = 0;
    return rgbdfe_octomap_leaves(map_.get(), out->data(), n, &got) == RGBDFE_OK && got == n;
  }
  // every node of the octree over the leaves, inner values as updateInnerOccupancy leaves them, in depth-first pre-order
  // (the payload of an .ot file); an empty map has no nodes
  bool tree(std::vector<rgbdfe_octomap_node>* out) const {
    if (!map_) return false;
    out->clear();
    int64_t n = 0;
    int rc = rgbdfe_octomap_tree(map_.get(), nullptr, 0, &n);  // the size: RGBDFE_ERR_CAPACITY, or OK for an empty map
    if (rc == RGBDFE_OK) return true;
    if (rc != RGBDFE_ERR_CAPACITY) return false;
    out->resize((size_t)n);
    int64_t got = 0;
    return rgbdfe_octomap_tree(map_.get(), out->data(), n, &got) == RGBDFE_OK && got == n;
  }
  // the same records into device memory (room for `capacity` of them); the number of nodes, -1 on failure
  int64_t treeDevice(void* d_out, int64_t capacity, void* stream = nullptr) const {
    int64_t n = 0;
    return map_ && rgbdfe_octomap_tree_device(map_.get(), d_out, capacity, &n, stream) == RGBDFE_OK ? n : -1;
  }
  // ColorOctomapServer::render's set: the nodes of octomap_display_level `depth` with log_odds >= min_log_odds
  // (-INFINITY: all of them), in tree order; key = the node's first cell, edge = resolution * 2^(16 - depth)
  bool nodesAtDepth(int32_t depth, float min_log_odds, std::vector<rgbdfe_octomap_leaf>* out) const {
    if (!map_) return false;
    out->clear();
    int64_t n = 0;
    int rc = rgbdfe_octomap_nodes_at_depth(map_.get(), depth, min_log_odds, nullptr, 0, &n);
    if (rc == RGBDFE_OK) return true;
    if (rc != RGBDFE_ERR_CAPACITY) return false;
    out->resize((size_t)n);
    int64_t got = 0;
    return rgbdfe_octomap_nodes_at_depth(map_.get(), depth, min_log_odds, out->data(), n, &got) == RGBDFE_OK && got == n;
  }
  bool write(const std::string& path) const {  // ColorOctomapServer::save
    return map_ && rgbdfe_octomap_write(map_.get(), path.c_str()) == RGBDFE_OK;
  }
  bool read(const std::string& path) { return map_ && rgbdfe_octomap_read(map_.get(), path.c_str()) == RGBDFE_OK; }
  bool setLeaves(const std::vector<rgbdfe_octomap_leaf>& leaves) {
    return map_ && rgbdfe_octomap_set_leaves(map_.get(), leaves.data(), (int64_t)leaves.size()) == RGBDFE_OK;
  }

  // ---- the read side.  A table loaded above 3/4 refuses queries (RGBDFE_ERR_CAPACITY): the leaves are then re-housed
  // at a load of at most 0.5 and the call repeated, as insertClouds doubles a full table.
  // logodds(occupancy_threshold), what a query takes for "occupied" when it is given NAN
  bool occupiedLogOdds(float* out) const { return map_ && rgbdfe_octomap_occupied_log_odds(map_.get(), out) == RGBDFE_OK; }
  // OcTreeBaseImpl::search for points (x, y, z each): found[i] = 0 no leaf, 1 leaves[i] is the cell's leaf, 2 no valid key
  bool search(const std::vector<float>& points, std::vector<int32_t>* found, std::vector<rgbdfe_octomap_leaf>* leaves) {
    if (!map_ || points.size() % 3 != 0) return false;
    const int64_t n = (int64_t)(points.size() / 3);
    found->assign((size_t)n, 0);
    leaves->assign((size_t)n, rgbdfe_octomap_leaf{});
    return query([&] { return rgbdfe_octomap_search(map_.get(), points.data(), n, found->data(), leaves->data()); });
  }
  // OccupancyOcTreeBase::castRay for rays (origin and direction x, y, z each; max_range <= 0: no limit)
  bool castRays(const std::vector<float>& origins, const std::vector<float>& directions, bool ignore_unknown, double max_range,
                std::vector<rgbdfe_octomap_ray_hit>* hits, float occupied_log_odds = NAN) {
    if (!map_ || origins.size() % 3 != 0 || directions.size() != origins.size()) return false;
    const int64_t n = (int64_t)(origins.size() / 3);
    hits->assign((size_t)n, rgbdfe_octomap_ray_hit{});
    return query([&] {
      return rgbdfe_octomap_cast_rays(map_.get(), origins.data(), directions.data(), n, ignore_unknown ? 1 : 0, max_range,
                                      occupied_log_odds, hits->data());
    });
  }
  // the map seen from cam2world (column-major Matrix4f): rows x cols rows of a node cloud (x, y, z in the camera frame, rgb
  // bits; NaN where the pixel's ray hits nothing); status (may be NULL): the rays' RGBDFE_OCTOMAP_RAY_* per pixel
  bool viewCloud(const std::array<float, 16>& cam2world, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                 bool ignore_unknown, double max_range, std::vector<float>* cloud, std::vector<uint8_t>* status = nullptr,
                 float occupied_log_odds = NAN) {
    if (!map_ || rows < 0 || cols < 0) return false;
    const size_t n = (size_t)rows * (size_t)cols;
    cloud->assign(4 * n, 0.0f);
    if (status) status->assign(n, 0);
    return query([&] {
      return rgbdfe_octomap_view_cloud(map_.get(), cam2world.data(), fx, fy, cx, cy, rows, cols, ignore_unknown ? 1 : 0, max_range,
                                       occupied_log_odds, cloud->data(), status ? status->data() : nullptr);
    });
  }
  // the same into device memory of the map's device (d_status may be NULL); nothing is read back
  bool viewCloudDevice(const std::array<float, 16>& cam2world, double fx, double fy, double cx, double cy, int32_t rows,
                       int32_t cols, bool ignore_unknown, double max_range, void* d_cloud, void* d_status = nullptr,
                       void* stream = nullptr, float occupied_log_odds = NAN) {
    if (!map_) return false;
    return query([&] {
      return rgbdfe_octomap_view_cloud_device(map_.get(), cam2world.data(), fx, fy, cx, cy, rows, cols, ignore_unknown ? 1 : 0,
                                              max_range, occupied_log_odds, d_cloud, d_status, stream);
    });
  }

 private:
  template <class Call>
  bool query(Call call) {
    int rc = call();
    const int64_t n = size();
    if (rc == RGBDFE_ERR_CAPACITY && n >= 0 && 4 * n > 3 * capacity_ && reserve(2 * n)) rc = call();
    return rc == RGBDFE_OK;
  }
  std::unique_ptr<rgbdfe_octomap, void (*)(rgbdfe_octomap*)> map_;
  int64_t capacity_;
};

// 4x4 inverse of a column-major float matrix (the reference calls Eigen's Matrix4f::inverse(), node.cpp:1536):
// Gauss-Jordan with partial pivoting in double, rounded to float
inline std::array<float, 16> inverse4(const std::array<float, 16>& T) {
  double a[4][8];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { a[r][c] = T[c * 4 + r]; a[r][c + 4] = r == c ? 1.0 : 0.0; }
  for (int i = 0; i < 4; ++i) {
    int p = i;
    for (int r = i + 1; r < 4; ++r) if (std::fabs(a[r][i]) > std::fabs(a[p][i])) p = r;
    for (int c = 0; c < 8; ++c) std::swap(a[i][c], a[p][c]);
    const double d = a[i][i];
    for (int c = 0; c < 8; ++c) a[i][c] /= d;
    for (int r = 0; r < 4; ++r)
      if (r != i) { const double f = a[r][i]; for (int c = 0; c < 8; ++c) a[r][c] -= f * a[i][c]; }
  }
  std::array<float, 16> out;
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[c * 4 + r] = (float)a[r][c + 4];
  return out;
}

// pairwiseObservationLikelihood (src/node.cpp:1520-1554) + observation_criterion_met (src/misc.cpp:1136-1148) for a
// batch of results, as matchNodePair applies them when observability_threshold > 0 (node.cpp:1340-1343): an edge that
// fails the criterion is withdrawn (edge ids -1).  Both nodes of every edge need setPointCloud().
inline bool pairwiseObservationLikelihood(const FrontEnd& fe, std::vector<MatchingResult>& results, int emm_skip_step,
                                          double observability_threshold) {
  std::vector<int32_t> new_ids, old_ids;
  std::vector<float> T;
  std::vector<size_t> which;
  for (size_t i = 0; i < results.size(); ++i) {
    const MatchingResult& mr = results[i];
    if (mr.edge.id1 < 0) continue;
    const std::array<float, 16> inv = inverse4(mr.final_trafo);
    new_ids.push_back(mr.edge.id2); old_ids.push_back(mr.edge.id1); T.insert(T.end(), mr.final_trafo.begin(), mr.final_trafo.end());
    new_ids.push_back(mr.edge.id1); old_ids.push_back(mr.edge.id2); T.insert(T.end(), inv.begin(), inv.end());
    which.push_back(i);
  }
  if (which.empty()) return true;
  std::vector<rgbdfe_emm_counts> c(new_ids.size());
  if (rgbdfe_observation_likelihood(fe.get(), (int32_t)new_ids.size(), new_ids.data(), old_ids.data(), T.data(),
                                    emm_skip_step, c.data()) != RGBDFE_OK)
    return false;
  for (size_t k = 0; k < which.size(); ++k) {
    MatchingResult& mr = results[which[k]];
    const rgbdfe_emm_counts &a = c[2 * k], &b = c[2 * k + 1];
    mr.inlier_points = a.inliers + b.inliers;     // node.cpp:1548-1551
    mr.outlier_points = a.outliers + b.outliers;
    mr.occluded_points = a.occluded + b.occluded;
    mr.all_points = a.all + b.all;
    double quality = 0.0;
    if (!rgbdfe_observation_criterion_met(mr.inlier_points, mr.outlier_points,
                                          mr.occluded_points + mr.inlier_points + mr.outlier_points,
                                          observability_threshold, &quality))
      mr.edge.id1 = mr.edge.id2 = -1;  // node.cpp:1419-1422
  }
  return true;
}

}  // namespace rgbdslam
#endif
