// session.h -- what session.hip (the pack kernel) and api_session.hip (host side) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbdfe {

// one node of a read-back as the pack kernel sees it: where its rows lie in the slabs and where they go in the packed arrays
struct NodePackEntry {
  uint32_t slot;       // rows slot * max_kp .. + rows of every slab, bytes slot * stats_stride .. of the counters
  uint32_t rows;
  uint32_t first_row;  // of the node in every packed array (the prefix sum of the rows in front of it)
  uint32_t has_kp;     // the slot's KeyPoint.pt are this node's (kNodeHasKeypoints); 0: the node's kp rows are zeros
};

// A source that is NULL (a slab that was never allocated) reads as zeros; an output that is NULL is not packed.
struct NodePackArgs {
  const uint4* desc;      // d_desc (desc_units = 2: 32 bytes per row) or d_sift_f32 (desc_units = 32: 128 floats per row)
  uint32_t desc_units;    // 16-byte units per descriptor row
  const uint4* xyz;       // d_xyz
  const float2* kp;       // d_kp2d
  const uint8_t* stats;   // d_feat_stats
  uint32_t max_kp, stats_stride;
  uint4* out_desc;        // total rows x desc_units, 16-byte aligned
  uint4* out_xyz;         // total rows
  float2* out_kp;         // total rows
  uint8_t* out_stats;     // total rows (bytes: a node's first counter lands on any byte)
};

constexpr uint32_t kNodePackRows = 64;  // rows of one node a workgroup packs

// One launch for the whole table (none for n == 0 or max_rows == 0): max_rows = the largest `rows` of the table.
// Returns the number of kernel launches.
int launch_node_pack(const NodePackEntry* d_table, uint32_t n, uint32_t max_rows, const NodePackArgs& args, hipStream_t stream);

}  // namespace rgbdfe
