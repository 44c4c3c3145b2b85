// session.hip -- the read-back of resident nodes (rgbdfe_download_nodes): node_pack_kernel gathers the rows of the listed
// nodes out of the slabs (slot x max_keypoints strides) into packed arrays, node after node in the order of the list, so
// that ONE device-to-host copy per array follows whatever the number of nodes.
//
// A plain bandwidth kernel: a workgroup takes kNodePackRows rows of one node, and its lanes walk the rows' bytes in 16-byte
// units where the layout allows it -- descriptors (32 or 512 bytes per row) and 3-D locations (16) start on a 16-byte
// boundary on both sides whatever the slot and the rows in front.  KeyPoint.pt (8 bytes per row) goes 8 bytes per lane: an
// odd number of rows in front shifts a node's rows by half a unit against the slab.  The counters are bytes, and a node of
// 65 rows leaves the next node's counters on an odd byte: one byte per lane.  Neighbouring lanes touch neighbouring
// addresses on both sides.  No atomics, no LDS, no wave-level operation: every output byte has exactly one writer.
#include "session.h"

namespace rgbdfe {

namespace {

__global__ __launch_bounds__(256) void node_pack_kernel(const NodePackEntry* __restrict__ table, uint32_t n, NodePackArgs a) {
  const uint32_t tid = threadIdx.x, step = blockDim.x;
  for (uint32_t k = blockIdx.y; k < n; k += gridDim.y) {
    const NodePackEntry e = table[k];
    const uint32_t r0 = blockIdx.x * kNodePackRows;
    if (r0 >= e.rows) continue;
    const uint32_t nr = min(kNodePackRows, e.rows - r0);
    const size_t src_row = (size_t)e.slot * a.max_kp + r0, dst_row = (size_t)e.first_row + r0;
    if (a.out_desc) {
      const uint4* src = a.desc + src_row * a.desc_units;
      uint4* dst = a.out_desc + dst_row * a.desc_units;
      for (uint32_t u = tid; u < nr * a.desc_units; u += step) dst[u] = src[u];
    }
    if (a.out_xyz)
      for (uint32_t u = tid; u < nr; u += step) a.out_xyz[dst_row + u] = a.xyz[src_row + u];
    if (a.out_kp) {
      const bool have = a.kp && e.has_kp;
      for (uint32_t u = tid; u < nr; u += step) {
        float2 v;
        v.x = 0.f; v.y = 0.f;
        if (have) v = a.kp[src_row + u];
        a.out_kp[dst_row + u] = v;
      }
    }
    if (a.out_stats) {
      const size_t src = (size_t)e.slot * a.stats_stride + r0;
      for (uint32_t u = tid; u < nr; u += step) a.out_stats[dst_row + u] = a.stats ? a.stats[src + u] : (uint8_t)0;
    }
  }
}

}  // namespace

int launch_node_pack(const NodePackEntry* d_table, uint32_t n, uint32_t max_rows, const NodePackArgs& args, hipStream_t stream) {
  if (n == 0 || max_rows == 0) return 0;
  const dim3 grid((max_rows + kNodePackRows - 1) / kNodePackRows, n < 65535u ? n : 65535u);
  hipLaunchKernelGGL(node_pack_kernel, grid, dim3(256), 0, stream, d_table, n, args);
  return 1;
}

}  // namespace rgbdfe
