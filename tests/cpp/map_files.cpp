// tests/cpp/map_files.cpp -- TEST INFRASTRUCTURE ONLY: the map-file wrappers of include/rgbdfe.hpp (rgbdfe_save_map,
// rgbdfe_save_node_clouds, rgbdfe_save_cloud_file, rgbdfe_cloud_file_info, rgbdfe_load_cloud_file), built by
// tests/test_gpu_cpp_map_files.py with plain g++ against the header and librgbdfe.so.
//   map_files dir n maximum_depth chunk_points
// reads dir/in_<k>.pcd (k < n: the clouds, organised), dir/transforms.bin (n x 16 floats) and dir/poses.bin (n x 16 doubles),
// both column-major; makes the clouds resident as nodes k and writes dir/cpp_map.pcd, dir/cpp_map.ply (compact), dir/cpp_raster
// (raster, no suffix: the name rule appends .pcd), dir/cpp_plain_%04d.* and dir/cpp_moved_%04d.* (graph ids 100 + 7 k), and
// dir/cpp_copy.ply (cloud n - 1 through the host-only writer).  One line per file call: what it reported.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rgbdfe.hpp"

template <class T>
static bool read_all(const std::string& path, std::vector<T>& out, size_t n) {
  out.resize(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  const bool ok = fread(out.data(), sizeof(T), n, f) == n;
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: map_files dir n maximum_depth chunk_points\n"); return 2; }
  const std::string dir = argv[1];
  const int32_t n = atoi(argv[2]);
  const double maximum_depth = atof(argv[3]);
  const int64_t chunk = atoll(argv[4]);
  std::vector<float> T;
  std::vector<double> P;
  if (!read_all(dir + "/transforms.bin", T, (size_t)n * 16) || !read_all(dir + "/poses.bin", P, (size_t)n * 16)) return 2;
  rgbdfe_config cfg = rgbdslam::FrontEnd::defaultConfig();
  cfg.max_nodes = 16; cfg.max_keypoints = 64; cfg.max_pairs_per_batch = 16;
  rgbdslam::FrontEnd fe(cfg);
  std::vector<int32_t> ids, graph_ids;
  std::vector<float> last;
  rgbdfe_cloud_file_header h = {};
  for (int32_t k = 0; k < n; ++k) {
    if (!rgbdslam::rgbdfe_load_cloud_file(dir + "/in_" + std::to_string(k) + ".pcd", &last, &h)) {
      fprintf(stderr, "load %d: %s\n", k, rgbdfe_last_error(nullptr));
      return 3;
    }
    if (rgbdfe_restore_node_cloud(fe.get(), k, last.data(), h.height, h.width, 40.0, 40.0, 1.0, 1.0, 1) != RGBDFE_OK) return 4;
    ids.push_back(k);
    graph_ids.push_back(100 + 7 * k);
  }
  rgbdfe_map_file_stats st;
  std::string written;
  const char* names[3] = {"/cpp_map.pcd", "/cpp_map.ply", "/cpp_raster"};
  for (int i = 0; i < 3; ++i) {
    if (!rgbdslam::rgbdfe_save_map(fe, ids, T, maximum_depth, i == 2, dir + names[i], &written, &st, chunk)) {
      fprintf(stderr, "save_map: %s\n", rgbdfe_last_error(fe.get()));
      return 5;
    }
    printf("map %s %lld %lld %d %d\n", written.substr(dir.size() + 1).c_str(), (long long)st.points, (long long)st.bytes_written,
           st.format, st.groups);
  }
  for (int moved = 0; moved < 2; ++moved) {
    int32_t nw = -1;
    if (!rgbdslam::rgbdfe_save_node_clouds(fe, ids, graph_ids, P, moved != 0, dir + (moved ? "/cpp_moved" : "/cpp_plain"), &nw)) {
      fprintf(stderr, "save_node_clouds: %s\n", rgbdfe_last_error(fe.get()));
      return 6;
    }
    printf("clouds %d %d\n", moved, nw);
  }
  if (!rgbdslam::rgbdfe_save_cloud_file(last, h.width, h.height, RGBDFE_CLOUD_FILE_PLY, dir + "/cpp_copy.ply")) return 7;
  rgbdfe_cloud_file_header back;
  if (!rgbdslam::rgbdfe_cloud_file_info(dir + "/cpp_copy.ply", &back)) return 8;
  printf("copy %d %d %d %lld\n", back.format, back.width, back.height, (long long)back.points);
  if (rgbdslam::rgbdfe_cloud_file_info(dir + "/transforms.bin", &back)) return 9;   // not a cloud file
  return 0;
}
