// mapping_session.cpp -- TEST INFRASTRUCTURE: one section of include/rgbdfe.hpp's mapping wrappers per run, for
// tests/test_gpu_cpp_mapping.py.  Needs g++ -std=c++14, include/rgbdfe.hpp and librgbdfe.so, nothing else.
//   mapping_session <section> <input file> <output directory>      section: pairs | graph | clouds | octomap | front
// Input: the container the test writes -- "RGBDFEC1", int32 count, then per array: int32 name length, the name, int32
// element type (0 u8, 1 i32, 2 i64, 3 f32, 4 f64, 5 u16), int32 ndim, ndim x int64 shape, the bytes.
// Output: every result as <output directory>/<name>.bin (raw bytes) plus scalars.json, one JSON object of integers.
// Returns non-zero, naming the call, on any unexpected false, -1 or exception.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "rgbdfe.hpp"

using namespace rgbdslam;

namespace {

struct Blob {
  int32_t type = 0;
  std::vector<int64_t> shape;
  std::vector<uint8_t> bytes;
  template <class T> const T* as() const { return reinterpret_cast<const T*>(bytes.data()); }
  int64_t dim(size_t k) const { return shape.at(k); }
};

std::map<std::string, Blob> g_in;
std::string g_out;
std::ostringstream g_scalars;
bool g_first_scalar = true;

[[noreturn]] void fail(const std::string& what) { throw std::runtime_error(what); }
#define MUST(call) do { if (!(call)) fail(std::string("unexpected failure of ") + #call + " (line " + std::to_string(__LINE__) + ")"); } while (0)

void readInput(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) fail(std::string("cannot open ") + path);
  char magic[8];
  int32_t count = 0;
  if (std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, "RGBDFEC1", 8) != 0 || std::fread(&count, 4, 1, f) != 1) fail("bad container");
  static const size_t width[6] = {1, 4, 8, 4, 8, 2};
  for (int i = 0; i < count; ++i) {
    int32_t len = 0, ndim = 0;
    Blob b;
    if (std::fread(&len, 4, 1, f) != 1 || len < 0 || len > 255) fail("bad container: name");
    std::string name((size_t)len, '\0');
    if (len && std::fread(&name[0], 1, (size_t)len, f) != (size_t)len) fail("bad container: name");
    if (std::fread(&b.type, 4, 1, f) != 1 || std::fread(&ndim, 4, 1, f) != 1 || b.type < 0 || b.type > 5 || ndim < 0 || ndim > 8)
      fail("bad container: " + name);
    size_t n = 1;
    for (int d = 0; d < ndim; ++d) {
      int64_t s = 0;
      if (std::fread(&s, 8, 1, f) != 1 || s < 0) fail("bad container: " + name);
      b.shape.push_back(s);
      n *= (size_t)s;
    }
    b.bytes.resize(n * width[b.type]);
    if (!b.bytes.empty() && std::fread(b.bytes.data(), 1, b.bytes.size(), f) != b.bytes.size()) fail("bad container: " + name);
    g_in[name] = std::move(b);
  }
  std::fclose(f);
}

const Blob& in(const std::string& name) {
  auto it = g_in.find(name);
  if (it == g_in.end()) fail("the input has no array " + name);
  return it->second;
}
double inD(const std::string& name, size_t k = 0) { return in(name).as<double>()[k]; }
int64_t inI(const std::string& name, size_t k = 0) { return in(name).as<int64_t>()[k]; }

void put(const std::string& name, const void* data, size_t bytes) {
  const std::string path = g_out + "/" + name + ".bin";
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || (bytes && std::fwrite(data, 1, bytes, f) != bytes) || std::fclose(f) != 0) fail("cannot write " + path);
}
template <class T> void put(const std::string& name, const std::vector<T>& v) { put(name, v.data(), v.size() * sizeof(T)); }
void scalar(const std::string& name, long long v) {
  g_scalars << (g_first_scalar ? "{" : ", ") << "\"" << name << "\": " << v;
  g_first_scalar = false;
}
std::string idx(const std::string& stem, int i) { return stem + "_" + std::to_string(i); }

rgbdfe_config config(int max_nodes, int max_keypoints, int max_pairs) {
  rgbdfe_config cfg = FrontEnd::defaultConfig();
  cfg.device_id = 0;
  cfg.max_nodes = max_nodes;
  cfg.max_keypoints = max_keypoints;
  cfg.max_pairs_per_batch = max_pairs;
  return cfg;
}

// the nodes of a section: features "desc" [n, m, 32] / "xyz1" [n, m, 4] with "counts" [n] rows in use, ids 0 .. n - 1
std::vector<std::unique_ptr<Node>> makeNodes(const FrontEnd& fe) {
  const Blob &desc = in("desc"), &xyz = in("xyz1"), &counts = in("counts");
  const int64_t n = desc.dim(0), m = desc.dim(1);
  std::vector<std::unique_ptr<Node>> nodes;
  for (int64_t i = 0; i < n; ++i) {
    nodes.emplace_back(new Node(fe, (int)i, desc.as<uint8_t>() + i * m * 32, xyz.as<float>() + i * m * 4, counts.as<int32_t>()[i]));
    MUST(nodes.back()->matchable_);
  }
  return nodes;
}

// setPointCloud for node i from "depth" [n, rows, cols] (+ "rgb" [n, rows, cols, 3] if present), "K" (fx, fy, cx, cy),
// "min_depth"
void setCloud(Node* node, int64_t i, const std::string& depth_name = "depth", const std::string& rgb_name = "rgb") {
  const Blob& d = in(depth_name);
  const int rows = (int)d.dim(1), cols = (int)d.dim(2);
  const uint8_t* rgb = g_in.count(rgb_name) ? in(rgb_name).as<uint8_t>() + i * rows * cols * 3 : nullptr;
  MUST(node->setPointCloud(d.as<float>() + i * rows * cols, rows, cols, rgb, rgb ? 3 : 0, false, inD("K", 0), inD("K", 1), inD("K", 2),
                           inD("K", 3), 1.0, inD("min_depth"), 1));
}

// ---- pairs: nodeComparisons, pairwiseObservationLikelihood, icpFallback -------------------------------------------------------
void sectionPairs() {
  FrontEnd fe(config(16, 512, 64));
  std::vector<std::unique_ptr<Node>> nodes = makeNodes(fe);
  for (size_t i = 0; i < nodes.size(); ++i) setCloud(nodes[i].get(), (int64_t)i);
  GraphManager gm(fe);
  const Node* new_node = nodes.back().get();
  std::vector<const Node*> cand;
  for (int64_t k = 0; k < in("candidates").dim(0); ++k) cand.push_back(nodes[(size_t)in("candidates").as<int32_t>()[k]].get());
  std::vector<MatchingResult> results = gm.nodeComparisons(new_node, cand);
  MUST(results.size() == cand.size());
  auto dump = [&](const std::string& tag) {
    std::vector<int32_t> ids, counts;
    std::vector<float> trafos, rmse;
    std::vector<double> edge;
    std::vector<uint32_t> points;
    std::vector<int32_t> matches;
    for (const MatchingResult& mr : results) {
      ids.push_back(mr.edge.id1); ids.push_back(mr.edge.id2);
      counts.push_back((int32_t)mr.all_matches.size()); counts.push_back((int32_t)mr.inlier_matches.size());
      trafos.insert(trafos.end(), mr.ransac_trafo.begin(), mr.ransac_trafo.end());
      trafos.insert(trafos.end(), mr.final_trafo.begin(), mr.final_trafo.end());
      trafos.insert(trafos.end(), mr.icp_trafo.begin(), mr.icp_trafo.end());
      rmse.push_back(mr.rmse);
      edge.insert(edge.end(), mr.edge.transform.begin(), mr.edge.transform.end());
      edge.push_back(mr.edge.informationScale);
      points.push_back(mr.inlier_points); points.push_back(mr.outlier_points); points.push_back(mr.occluded_points);
      points.push_back(mr.all_points);
      for (const DMatch& m : mr.all_matches) { matches.push_back(m.queryIdx); matches.push_back(m.trainIdx); }
      for (const DMatch& m : mr.inlier_matches) { matches.push_back(m.queryIdx); matches.push_back(m.trainIdx); }
    }
    put(tag + "_ids", ids); put(tag + "_counts", counts); put(tag + "_trafos", trafos); put(tag + "_rmse", rmse);
    put(tag + "_edge", edge); put(tag + "_points", points); put(tag + "_matches", matches);
  };
  dump("compare");
  MUST(pairwiseObservationLikelihood(fe, results, (int)inI("emm_skip_step"), inD("observability_threshold")));
  dump("emm");
  std::vector<rgbdfe_icp_report> reports;
  const int edges = gm.icpFallback(new_node, cand, results, nullptr, &reports);
  MUST(edges >= 0);
  scalar("icp_edges", edges);
  scalar("icp_reports", (long long)reports.size());
  dump("icp");
  put("icp_reports", reports);
}

// ---- graph: the pose-graph wrappers, driven by the test's list of operations ---------------------------------------------------
enum Op { OP_NODE, OP_EDGE, OP_STRATEGY, OP_FIXED, OP_OPTIMIZE, OP_PRUNE, OP_SANITY, OP_EVALUATION, OP_TRAJECTORY, OP_TRANSFORMS,
          OP_CLOUDS, OP_ASSEMBLE };

void sectionGraph() {
  FrontEnd fe(config(80, 64, 16));
  const Blob &ops = in("ops"), &opf = in("opf"), &edges = in("edges"), &desc = in("desc"), &xyz = in("xyz1");
  const int64_t m = desc.dim(1);
  std::vector<std::unique_ptr<Node>> nodes;
  std::vector<int32_t> ids;
  GraphManager gm(fe);
  for (int64_t i = 0; i < ops.dim(0); ++i) {
    const int32_t* op = ops.as<int32_t>() + 4 * i;
    const double f0 = opf.as<double>()[2 * i];
    const int at = (int)i;
    switch (op[0]) {
      case OP_NODE: {
        const size_t k = nodes.size();
        nodes.emplace_back(new Node(fe, op[1], desc.as<uint8_t>() + k * m * 32, xyz.as<float>() + k * m * 4, (int)m));
        MUST(nodes.back()->matchable_);
        gm.nodeAdded(nodes.back().get(), op[1], false);
        ids.push_back(op[1]);
        break;
      }
      case OP_EDGE: {
        const double* e = edges.as<double>() + 19 * op[1];
        LoadedEdge3D edge;
        edge.id1 = (int)e[0];
        edge.id2 = (int)e[1];
        for (int k = 0; k < 16; ++k) edge.transform[k] = e[2 + k];
        edge.informationScale = e[18];
        MUST(gm.addEdgeToG2O(edge, op[2] != 0));
        break;
      }
      case OP_STRATEGY: MUST(gm.setPoseRelativeTo(op[1])); break;
      case OP_FIXED: MUST(gm.setFixed(op[1], op[2] != 0)); break;
      case OP_OPTIMIZE: {
        rgbdfe_pose_graph_report rep;
        const double chi2 = gm.optimizeGraph(f0, &rep);
        MUST(chi2 >= 0.0);
        std::vector<int64_t> ri{rep.iterations, rep.launches, rep.readbacks, rep.recorded};
        std::vector<double> rf{chi2, rep.chi2};
        for (int k = 0; k < rep.recorded; ++k) {
          ri.push_back(rep.it[k].trials);
          for (int t = 0; t < rep.it[k].trials; ++t) ri.push_back(rep.it[k].pcg_iterations[t]);
          rf.push_back(rep.it[k].chi2_before); rf.push_back(rep.it[k].chi2_after); rf.push_back(rep.it[k].lambda);
        }
        put(idx("report_i", at), ri);
        put(idx("report_f", at), rf);
        break;
      }
      case OP_PRUNE: {
        std::vector<uint8_t> verdicts;
        const int pruned = gm.pruneEdgesWithErrorAbove((float)f0, &verdicts);
        MUST(pruned >= 0);
        scalar(idx("pruned", at), pruned);
        put(idx("verdicts", at), verdicts);
        break;
      }
      case OP_SANITY: scalar(idx("sanity", at), gm.sanityCheck((float)f0)); break;
      case OP_EVALUATION: {
        rgbdfe_pose_graph_evaluation ev;
        std::vector<double> est;
        MUST(gm.evaluation(f0, &ev, &est, (int)ids.size()));
        std::vector<double> chi2;
        std::vector<int64_t> counts;
        for (const rgbdfe_pose_graph_round& r : ev.round) {
          chi2.push_back(r.chi2);
          counts.push_back(r.iterations); counts.push_back(r.pruned); counts.push_back(r.launches); counts.push_back(r.readbacks);
        }
        put(idx("evaluation_chi2", at), chi2);
        put(idx("evaluation_counts", at), counts);
        put(idx("estimates", at), est);
        break;
      }
      case OP_TRAJECTORY: {
        const std::string path = g_out + "/" + idx("trajectory", at) + ".txt";
        std::vector<double> stamps;
        for (size_t k = 0; k < ids.size(); ++k) stamps.push_back(1000.0 + 0.5 * (double)k);
        if (op[1] == 2) {  // unequal lists: refused, no file
          stamps.pop_back();
          scalar(idx("trajectory", at), gm.saveTrajectory(path, ids, stamps) ? 1 : 0);
          break;
        }
        const bool with = op[1] == 1;
        MUST(gm.saveTrajectory(path, ids, stamps, with ? in("base2points").as<double>() : nullptr,
                               with ? in("init_base_pose").as<double>() : nullptr, with ? "/map" : nullptr,
                               with ? "/camera" : nullptr));
        break;
      }
      case OP_TRANSFORMS: {
        std::vector<int32_t> which = ids;
        if (op[1] == 1) which.push_back(9999);  // an unknown id: empty
        put(idx("transforms", at), gm.transforms(which));
        break;
      }
      case OP_CLOUDS:
        for (int k = 0; k < op[1]; ++k) setCloud(nodes[(size_t)k].get(), k);
        break;
      case OP_ASSEMBLE: {
        std::vector<int32_t> which(ids.begin(), ids.begin() + op[1]);
        std::vector<float> cloud;
        std::vector<int64_t> offsets;
        MUST(assembleAllClouds(fe, which, gm.transforms(which), f0, false, &cloud, &offsets));
        put(idx("assembled", at), cloud);
        put(idx("assembled_offsets", at), offsets);
        break;
      }
      default: fail("unknown operation " + std::to_string(op[0]));
    }
  }
}

// ---- clouds: pointCloud, reducePointCloud, assembleAllClouds, displayGeometry ----------------------------------------------------
void putCloud(const Node& node, const std::string& name) {
  std::vector<float> cloud;
  int rows = -1, cols = -1;
  MUST(node.pointCloud(&cloud, &rows, &cols));
  put(name, cloud);
  scalar(name + "_rows", rows);
  scalar(name + "_cols", cols);
}

void putDisplay(const FrontEnd& fe, const std::vector<int32_t>& ids, const std::vector<float>& T, const rgbdfe_display_params& prm,
                const std::string& name) {
  DisplayGeometry g;
  MUST(displayGeometry(fe, ids, T, prm, &g));
  put(name + "_vertices", g.vertices);
  put(name + "_strips", g.strips);
  put(name + "_offsets", g.node_offsets);
  put(name + "_strip_offsets", g.node_strip_offsets);
  put(name + "_types", g.node_types);
}

void sectionClouds() {
  FrontEnd fe(config(16, 64, 16));
  std::vector<std::unique_ptr<Node>> nodes = makeNodes(fe);   // 0, 1: 48 x 64; 2: one row; 3: no valid point; 4: as 0
  for (int64_t i : {0, 1, 3, 4}) setCloud(nodes[(size_t)i].get(), i);
  setCloud(nodes[2].get(), 0, "depth_row", "rgb_row");
  for (int i = 0; i < 5; ++i) putCloud(*nodes[(size_t)i], idx("cloud", i));

  const Blob& T = in("world2cam");
  auto transformsOf = [&](const std::vector<int32_t>& ids) {
    std::vector<float> out;
    for (int32_t id : ids) out.insert(out.end(), T.as<float>() + 16 * id, T.as<float>() + 16 * id + 16);
    return out;
  };
  const std::vector<int32_t> listed{0, 1, 2, 0, 3};   // an id twice, the one-row cloud, the cloud without a point
  const double maximum_depth = inD("maximum_depth"), vfs = inD("voxelfilter_size");
  auto assemble = [&](const std::vector<int32_t>& ids, bool raster, double filter, const std::string& name) {
    std::vector<float> cloud;
    std::vector<int64_t> offsets;
    MUST(assembleAllClouds(fe, ids, transformsOf(ids), maximum_depth, raster, &cloud, &offsets, filter));
    put(name, cloud);
    put(name + "_offsets", offsets);
  };
  assemble(listed, false, 0.0, "assembled_compact");
  assemble(listed, true, 0.0, "assembled_raster");
  assemble({}, false, 0.0, "assembled_empty");
  assemble(listed, false, vfs, "assembled_filtered");
  {
    std::vector<float> cloud{1.f, 2.f, 3.f, 4.f};
    std::vector<int64_t> offsets{7};
    std::vector<float> bad = transformsOf(listed);
    bad.pop_back();
    scalar("assemble_bad_length", assembleAllClouds(fe, listed, bad, maximum_depth, false, &cloud, &offsets) ? 1 : 0);
    scalar("assemble_bad_untouched", cloud.size() == 4 && offsets.size() == 1 && offsets[0] == 7 ? 1 : 0);
  }

  const Blob& forms = in("display_forms");   // rows of (display type, skip step), with "display_f" rows of (threshold, maximum depth)
  const std::vector<int32_t> shown{0, 1, 2};
  for (int64_t k = 0; k < forms.dim(0); ++k) {
    rgbdfe_display_params prm;
    prm.display_type = forms.as<int32_t>()[2 * k];
    prm.visualization_skip_step = forms.as<int32_t>()[2 * k + 1];
    prm.squared_meshing_threshold = in("display_f").as<double>()[2 * k];
    prm.maximum_depth = in("display_f").as<double>()[2 * k + 1];
    putDisplay(fe, shown, {}, prm, idx("display_node", (int)k));
    putDisplay(fe, shown, transformsOf(shown), prm, idx("display_world", (int)k));
  }
  {
    DisplayGeometry g;
    rgbdfe_display_params prm{RGBDFE_DISPLAY_POINTS, 1, 0.0009, INFINITY};
    std::vector<float> bad = transformsOf(shown);
    bad.pop_back();
    scalar("display_bad_length", displayGeometry(fe, shown, bad, prm, &g) ? 1 : 0);
  }

  // reducePointCloud: an invalid size changes nothing
  scalar("reduce_zero", nodes[1]->reducePointCloud(0.0) ? 1 : 0);
  scalar("reduce_negative", nodes[1]->reducePointCloud(-1.0) ? 1 : 0);
  putCloud(*nodes[1], "cloud_1_after_invalid");
  int64_t points = -1;
  int32_t flags = -1;
  MUST(nodes[1]->reducePointCloud(vfs, &points, &flags));
  scalar("reduce_points", points);
  scalar("reduce_flags", flags);
  putCloud(*nodes[1], "cloud_1_reduced");
  MUST(nodes[4]->reducePointCloud(inD("tiny_leaf"), &points, &flags));   // a leaf too small for the extent: the flag, the cloud stays
  scalar("tiny_points", points);
  scalar("tiny_flags", flags);
  putCloud(*nodes[4], "cloud_4_after_tiny");
  MUST(nodes[3]->reducePointCloud(vfs, &points, &flags));                // no valid point: a cloud of no rows
  scalar("empty_points", points);
  scalar("empty_flags", flags);
  putCloud(*nodes[3], "cloud_3_reduced");
  // the reduced clouds (one row: drawn as points) as inputs of the two map calls
  const std::vector<int32_t> after{0, 1, 3};
  assemble(after, false, 0.0, "assembled_after");
  rgbdfe_display_params strip{RGBDFE_DISPLAY_TRIANGLE_STRIP, 1, 0.0009, INFINITY};
  putDisplay(fe, after, transformsOf(after), strip, "display_after");
}

// ---- octomap: all of class OctoMap ------------------------------------------------------------------------------------------------
int64_t capacityOf(const OctoMap& map) {
  int64_t st[2] = {0, 0};
  MUST(rgbdfe_octomap_stats(map.get(), st, 2) == RGBDFE_OK);
  return st[0];
}

void sectionOctomap() {
  FrontEnd fe(config(16, 64, 16));
  std::vector<std::unique_ptr<Node>> nodes = makeNodes(fe);
  std::vector<int32_t> ids;
  for (size_t i = 0; i < nodes.size(); ++i) { setCloud(nodes[i].get(), (int64_t)i); ids.push_back((int32_t)i); }
  const Blob& T = in("world2cam");
  const std::vector<float> world2cam(T.as<float>(), T.as<float>() + 16 * ids.size());
  rgbdfe_octomap_params prm;
  rgbdfe_octomap_default_params(&prm);
  prm.resolution = inD("resolution");
  const double max_range = inD("max_range");
  const float threshold = in("depth_threshold").as<float>()[0];

  {  // a map that failed to create: every member says so
    OctoMap bad(fe, 0, &prm);
    std::vector<rgbdfe_octomap_leaf> leaves;
    std::vector<rgbdfe_octomap_node> tree;
    std::vector<int32_t> found;
    std::vector<rgbdfe_octomap_ray_hit> hits;
    std::vector<float> cloud;
    float lo = 0.f;
    const std::vector<float> p{0.f, 0.f, 0.f}, d{1.f, 0.f, 0.f};
    const std::array<float, 16> eye{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    std::vector<int32_t> r{bad.valid(), bad.get() != nullptr, bad.reset(), bad.reserve(64), bad.insertClouds(ids, world2cam, max_range),
                           (int32_t)bad.size(), bad.leaves(&leaves), bad.tree(&tree), (int32_t)bad.treeDevice(nullptr, 0),
                           bad.nodesAtDepth(16, threshold, &leaves), bad.write(g_out + "/never.ot"), bad.read(g_out + "/never.ot"),
                           bad.setLeaves(leaves), bad.occupiedLogOdds(&lo), bad.search(p, &found, &leaves),
                           bad.castRays(p, d, false, -1.0, &hits), bad.viewCloud(eye, 1, 1, 0, 0, 1, 1, false, -1.0, &cloud),
                           bad.viewCloudDevice(eye, 1, 1, 0, 0, 1, 1, false, -1.0, nullptr)};
    put("invalid_map", r);
  }

  OctoMap map(fe, inI("capacity"), &prm);
  MUST(map.valid());
  {  // an empty map: no nodes, and that is no failure
    std::vector<rgbdfe_octomap_node> tree(3);
    std::vector<rgbdfe_octomap_leaf> level(3);
    MUST(map.tree(&tree));
    MUST(map.nodesAtDepth(14, -INFINITY, &level));
    scalar("empty_tree", (long long)tree.size());
    scalar("empty_level", (long long)level.size());
  }
  MUST(map.insertClouds(ids, world2cam, max_range));
  scalar("capacity_after_insert", capacityOf(map));
  scalar("size", map.size());
  {  // a view of 2^32 pixels is refused for its size (RGBDFE_ERR_CAPACITY), not for the table's load: no re-housing.  The C ABI
     // compares the size before it looks at the table or the output, so the pointer (it must not be null) is never used.
    const std::array<float, 16> eye{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    char never_written = 0;
    MUST(map.reserve(3 * map.size()));   // a load of 1/3, and a capacity that a re-housing to 2 n would change
    scalar("oversized_view", map.viewCloudDevice(eye, 1, 1, 0, 0, 65536, 65536, false, -1.0, &never_written) ? 1 : 0);
    scalar("capacity_after_oversized_view", capacityOf(map));
  }
  std::vector<rgbdfe_octomap_leaf> leaves;
  MUST(map.leaves(&leaves));
  put("leaves", leaves);
  std::vector<rgbdfe_octomap_node> tree;
  MUST(map.tree(&tree));
  put("tree", tree);
  for (int depth : {16, 14}) {
    std::vector<rgbdfe_octomap_leaf> level;
    MUST(map.nodesAtDepth(depth, threshold, &level));
    put(idx("level_threshold", depth), level);
    MUST(map.nodesAtDepth(depth, -INFINITY, &level));
    put(idx("level_all", depth), level);
  }
  MUST(map.write(g_out + "/map.ot"));
  {
    OctoMap second(fe, 2 * map.size() + 64, &prm);
    MUST(second.valid() && second.read(g_out + "/map.ot"));
    std::vector<rgbdfe_octomap_leaf> got;
    MUST(second.leaves(&got));
    put("leaves_read", got);
    std::vector<rgbdfe_octomap_leaf> reversed(leaves.rbegin(), leaves.rend());
    reversed.resize(reversed.size() / 2);
    MUST(second.setLeaves(reversed));
    MUST(second.leaves(&got));
    put("leaves_set", got);
  }

  // the read side on a table loaded to 1: re-housed once, to a load of 0.5
  float occupied = 0.f;
  MUST(map.occupiedLogOdds(&occupied));
  put("occupied_log_odds", &occupied, 4);
  MUST(map.reserve(map.size()));
  scalar("capacity_full", capacityOf(map));
  const Blob& pts = in("points");
  std::vector<int32_t> found;
  std::vector<rgbdfe_octomap_leaf> at;
  MUST(map.search(std::vector<float>(pts.as<float>(), pts.as<float>() + 3 * pts.dim(0)), &found, &at));
  scalar("capacity_after_search", capacityOf(map));
  put("found", found);
  put("found_leaves", at);
  const Blob &o = in("origins"), &d = in("directions");
  std::vector<rgbdfe_octomap_ray_hit> hits;
  MUST(map.castRays(std::vector<float>(o.as<float>(), o.as<float>() + 3 * o.dim(0)),
                    std::vector<float>(d.as<float>(), d.as<float>() + 3 * d.dim(0)), false, inD("ray_range"), &hits));
  scalar("capacity_after_rays", capacityOf(map));
  put("hits", hits);
  std::array<float, 16> cam2world;
  std::copy(in("cam2world").as<float>(), in("cam2world").as<float>() + 16, cam2world.begin());
  std::vector<float> view;
  std::vector<uint8_t> status;
  MUST(map.viewCloud(cam2world, inD("view", 0), inD("view", 1), inD("view", 2), inD("view", 3), (int32_t)inD("view", 4),
                     (int32_t)inD("view", 5), true, -1.0, &view, &status));
  scalar("capacity_after_view", capacityOf(map));
  put("view", view);
  put("view_status", status);
  MUST(map.leaves(&leaves));
  put("leaves_after_queries", leaves);
}

// ---- front: setDetectorType, fastDetect, the sensor-frame Node constructor -----------------------------------------------------
void putNode(const Node& node, const FrontEnd& fe, const std::string& name) {
  put(name + "_keypoints", node.feature_locations_2d_);
  put(name + "_descriptors", node.feature_descriptors_);
  put(name + "_xyz", node.feature_locations_3d_);
  scalar(name + "_features", node.featureCount());
  scalar(name + "_matchable", node.matchable_ ? 1 : 0);
  scalar(name + "_resident", rgbdfe_node_count(fe.get(), node.id_));
}

void sectionFront() {
  FrontEnd fe(config(4, 2048, 8));
  fe.setDetectorType("FAST");
  fe.setDetectorType("ORB");
  int threw = 0;
  try { fe.setDetectorType("SURF"); } catch (const std::runtime_error&) { threw = 1; }
  scalar("unknown_detector_throws", threw);
  const Blob& noise = in("noise");
  const int threshold = (int)inI("fast_threshold");
  put("fast_noise", fe.fastDetect(noise.as<uint8_t>(), nullptr, (int)noise.dim(0), (int)noise.dim(1), threshold));
  const Blob& flat = in("flat");
  put("fast_flat", fe.fastDetect(flat.as<uint8_t>(), nullptr, (int)flat.dim(0), (int)flat.dim(1), threshold));
  const int max_keypoints = (int)inI("max_keypoints");
  MUST(rgbdfe_detector_configure(fe.get(), max_keypoints, 3, 5) == RGBDFE_OK);
  const Blob &rgb = in("rgb8"), &d16 = in("depth16"), &mono = in("mono8"), &d32 = in("depth32"), &shape = in("shapes");
  const int64_t* s = shape.as<int64_t>();   // visual rows, cols; depth rows, cols
  const SensorFrame colour(rgb.as<uint8_t>(), (int)s[0], (int)s[1], (size_t)rgb.dim(1), RGBDFE_VISUAL_RGB8, d16.as<uint16_t>(), (int)s[2],
                           (int)s[3], (size_t)d16.dim(1) * 2, RGBDFE_DEPTH_16UC1);
  const Node a(fe, 0, colour, inD("K", 0), inD("K", 1), inD("K", 2), inD("K", 3), 1.0, max_keypoints);
  putNode(a, fe, "colour");
  const SensorFrame grey(mono.as<uint8_t>(), (int)s[0], (int)s[1], (size_t)mono.dim(1), RGBDFE_VISUAL_MONO8, d32.as<float>(), (int)s[2],
                         (int)s[3], (size_t)d32.dim(1) * 4, RGBDFE_DEPTH_32FC1);
  const Node b(fe, 1, grey, inD("K", 0), inD("K", 1), inD("K", 2), inD("K", 3), 1.0, max_keypoints);
  putNode(b, fe, "grey");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: mapping_session <pairs|graph|clouds|octomap|front> <input file> <output directory>\n");
    return 2;
  }
  const std::string section = argv[1];
  g_out = argv[3];
  try {
    readInput(argv[2]);
    if (section == "pairs") sectionPairs();
    else if (section == "graph") sectionGraph();
    else if (section == "clouds") sectionClouds();
    else if (section == "octomap") sectionOctomap();
    else if (section == "front") sectionFront();
    else fail("unknown section " + section);
    g_scalars << (g_first_scalar ? "{}" : "}") << "\n";
    const std::string text = g_scalars.str();
    const std::string path = g_out + "/scalars.json";
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size() || std::fclose(f) != 0) fail("cannot write " + path);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mapping_session %s: %s\n", section.c_str(), e.what());
    return 1;
  }
  return 0;
}
