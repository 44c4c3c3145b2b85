// display_geometry.h -- what display_geometry.hip (kernels) and api_display.hip (host side) share: the device view of a
// batch of node clouds that become GL vertex streams, and the launch functions.  The contract is the "display geometry"
// block of include/rgbdfe.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbdfe {

// the forms (the values of include/rgbdfe.h's RGBDFE_DISPLAY_*)
constexpr int32_t kDispPoints = 0, kDispTriangles = 1, kDispStrip = 2;

constexpr uint32_t kDispBlock = 256;      // threads of an item workgroup
constexpr uint32_t kDispPerThread = 4;    // consecutive items of a thread
constexpr uint32_t kDispItemTile = kDispBlock * kDispPerThread;  // points / cells of a POINTS / TRIANGLES tile
constexpr uint32_t kDispRowTile = 64;     // strip rows of a TRIANGLE_STRIP tile: a lane per row, one wave
constexpr uint32_t kDispScanBlock = 1024; // tiles per trip of the one-workgroup scan

// One listed node.  Its items -- the points (POINTS) or cells (TRIANGLES) in the reference's loop order, x outer and y
// inner, or the visited rows (TRIANGLE_STRIP) -- are cut into tiles that never cross a node: the node owns the tiles
// [first_tile, first_tile + ceil(n_items / tile size)).  The table has n_nodes + 1 rows, the last one a sentinel whose
// first_tile is the number of tiles.
struct DispNode {
  const float4* cloud;   // h x w points, row-major
  int32_t w, h;
  int32_t type;          // the form this node is drawn in
  int32_t step;          // visualization_skip_step (TRIANGLE_STRIP)
  uint32_t n_items;
  uint32_t items_h;      // items per column: h (POINTS), h - 1 (TRIANGLES); unused for strips
  uint32_t first_tile;
  uint32_t first_row;    // TRIANGLE_STRIP: the node's first entry of row_count
  float R[9], t[3];      // as MapNode: rot (row-major) and trans of the Matrix4f
};
static_assert(sizeof(DispNode) == 88, "DispNode layout");

struct DispParams {
  float mesh_thresh;     // (float)squared_meshing_threshold
  float max_depth;       // (float)maximum_depth
  uint32_t transform;    // 0: vertices stay in the node frame
};

// each returns its number of kernel launches
// tile_count[t] = (vertices, strip records) of tile t; row_count[first_row + r] = those of strip row r.  Then one
// workgroup: tile_first[t] = the (vertices, strips) in front of tile t as two int64, tile_first[n_tiles] = the totals;
// node_first[k] = those in front of node k, node_first[n_nodes] = the totals.  have_items / have_rows: the call lists
// nodes of that kind.
int launch_display_count_scan(const DispNode* nodes, const uint32_t* tile_node, uint32_t n_nodes, uint32_t n_tiles,
                              DispParams prm, bool have_items, bool have_rows, uint2* tile_count, uint2* row_count,
                              int64_t* tile_first, int64_t* node_first, hipStream_t st);
// the vertex rows and the strip records (first vertex, vertex count; two int64 each) at the places the scan assigned
int launch_display_write(const DispNode* nodes, const uint32_t* tile_node, uint32_t n_tiles, DispParams prm, bool have_items,
                         bool have_rows, const uint2* row_count, const int64_t* tile_first, float4* vertices,
                         int64_t* strips, hipStream_t st);

}  // namespace rgbdfe
