// api_voxel.hip -- the voxel filter: a cloud reduced to the centroids of its occupied grid cells (kernels: voxel_filter.hip),
// over a host array, a device buffer, or a node's resident cloud (Node::reducePointCloud, node.cpp:1448-1460)
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"

namespace impl {

namespace {

// what the first half of a run leaves for the second
struct VoxRun {
  bool too_small = false;  // the leaf is too small for the cloud's extent: the output is the input
  int64_t rows = 0;        // rows of the output
  int passes = 0;          // sort passes that ran
  const uint32_t* d_idx = nullptr;         // the point indices sorted by cell, index order inside a cell
  const uint32_t* d_cell_start = nullptr;  // rows + 1 entries
};

bool leaf_of(double voxelfilter_size, float* inv) {
  const float L = (float)voxelfilter_size;
  *inv = 1.0f / L;
  return L > 0.0f && std::isfinite(*inv) && *inv != 0.0f;
}

// Everything up to the number of occupied cells: two reads of 32 bytes, at most 18 launches.  ctx->mu is held.
int vox_count_cells(rgbdfe_ctx* ctx, const float4* d_in, int64_t n_in, float inv, hipStream_t st, VoxRun* run) {
  *run = VoxRun();
  if (n_in == 0) return RGBDFE_OK;
  const uint32_t n = (uint32_t)n_in;
  const size_t n_tiles = ((size_t)n + kVoxTile - 1) / kVoxTile;
  DeviceLayout lay;
  const Block b_hdr = lay.room(256), b_box = lay.room(24 * n_tiles), b_count = lay.room(4 * n_tiles),
              b_first = lay.room(4 * (n_tiles + 1));
  const SortWorkspace b_sort = sort_workspace(lay, n);
  const Block b_cells = lay.room(4 * ((size_t)n + 1));
  int rc = ensure_scratch(ctx, lay.total());
  if (rc != RGBDFE_OK) return rc;
  void* base = ctx->d_scratch;
  VoxHeader* d_hdr = at<VoxHeader>(base, b_hdr);
  float* d_box = at<float>(base, b_box);
  uint32_t* d_count = at<uint32_t>(base, b_count);
  uint32_t* d_first = at<uint32_t>(base, b_first);
  uint32_t* d_keys[2] = {at<uint32_t>(base, b_sort.keys[0]), at<uint32_t>(base, b_sort.keys[1])};
  uint32_t* d_idx[2] = {at<uint32_t>(base, b_sort.idx[0]), at<uint32_t>(base, b_sort.idx[1])};
  uint32_t* d_hist = at<uint32_t>(base, b_sort.hist);
  uint32_t* d_digits = at<uint32_t>(base, b_sort.digits);
  uint32_t* d_cells = at<uint32_t>(base, b_cells);

  launch_vox_stats(d_in, n, d_box, d_count, d_first, d_hdr, st);
  HIP_TRY(ctx, hipGetLastError());
  VoxHeader h;
  HIP_TRY(ctx, hipMemcpyAsync(&h, d_hdr, sizeof(h), hipMemcpyDeviceToHost, st));  // the first read: the box, the valid points
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (h.n_valid == 0) return RGBDFE_OK;

  // the leaf-too-small check, then the grid, as VoxelGrid::applyFilter has them
  int64_t cells_d = 1;
  for (int a = 0; a < 3; ++a) {
    const float prod = (h.max_p[a] - h.min_p[a]) * inv;
    if (prod >= 2147483648.0f) run->too_small = true;
    else if (!run->too_small) {
      cells_d *= (int64_t)prod + 1;  // each factor <= 2^31 and the product so far <= INT32_MAX: no overflow
      if (cells_d > (int64_t)INT32_MAX) run->too_small = true;
    }
  }
  if (run->too_small) {
    run->rows = n_in;
    return RGBDFE_OK;
  }
  int64_t min_b[3], div[3];
  for (int a = 0; a < 3; ++a) {
    min_b[a] = (int)floorf(h.min_p[a] * inv);
    div[a] = (int64_t)(int)floorf(h.max_p[a] * inv) - min_b[a] + 1;
  }
  VoxGrid g;
  g.inv = inv;
  for (int a = 0; a < 3; ++a) g.min_b[a] = (float)(int)min_b[a];
  g.mul1 = (uint32_t)div[0];
  g.mul2 = (uint32_t)(div[0] * div[1]);
  // div[a] can exceed the checked extent by one per axis: a grid past 2^31 cells has int32 indices that wrap to negative
  // values; the keys then carry the sign bit flipped, so that the unsigned sort gives the signed order
  const int64_t cells = div[0] * div[1] * div[2];
  const bool wraps = cells > ((int64_t)1 << 31);
  g.flip = wraps ? 0x80000000u : 0u;
  int bits = 32;
  if (!wraps)
    for (bits = 1; bits < 32 && ((int64_t)1 << bits) < cells; ++bits) {}
  run->passes = (bits + 7) / 8;

  launch_vox_keys(d_in, n, g, d_first, d_keys[0], d_idx[0], st);
  const int cur = launch_vox_sort(h.n_valid, run->passes, d_keys, d_idx, d_hist, d_digits, st);
  launch_vox_heads(d_keys[cur], h.n_valid, d_count, d_first, d_cells, d_hdr, st);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&h, d_hdr, sizeof(h), hipMemcpyDeviceToHost, st));  // the second read: the occupied cells
  HIP_TRY(ctx, hipStreamSynchronize(st));
  run->rows = (int64_t)h.n_cells;
  run->d_idx = d_idx[cur];
  run->d_cell_start = d_cells;
  return RGBDFE_OK;
}

// the output pass: the centroids, or the input as it is
int vox_emit(rgbdfe_ctx* ctx, const float4* d_in, const VoxRun& run, float4* d_out, float* d_zplane, hipStream_t st) {
  if (run.rows == 0) return RGBDFE_OK;
  if (run.too_small) {
    HIP_TRY(ctx, hipMemcpyAsync(d_out, d_in, (size_t)run.rows * sizeof(float4), hipMemcpyDeviceToDevice, st));
    return RGBDFE_OK;
  }
  launch_vox_centroids(d_in, run.d_idx, run.d_cell_start, (uint32_t)run.rows, d_out, d_zplane, st);
  HIP_TRY(ctx, hipGetLastError());
  return RGBDFE_OK;
}

int voxel_filter_common(rgbdfe_ctx* ctx, const float* h_in, const void* d_in, int64_t n_in, double voxelfilter_size, float* h_out,
                        void* d_out, bool device, int64_t capacity, int64_t* n_out, int32_t* flags, void* stream) {
  float inv = 0.f;
  if (!ctx || n_in < 0 || !n_out || capacity < 0 || (n_in > 0 && !(device ? d_in != nullptr : h_in != nullptr)) ||
      (capacity > 0 && !(device ? d_out != nullptr : h_out != nullptr)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad voxel filter arguments");
  if (!leaf_of(voxelfilter_size, &inv))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "voxelfilter_size must be positive as a float, with a finite non-zero inverse");
  if (n_in > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "voxel filter: 2^31 points or more in one call");
  if (device && n_in > 0 && capacity > 0) {
    const char *a = (const char*)d_in, *b = (const char*)d_out;
    if (a < b + (size_t)capacity * sizeof(float4) && b < a + (size_t)n_in * sizeof(float4))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "voxel filter: d_out overlaps d_points");
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  *n_out = 0;
  if (flags) *flags = 0;
  if (n_in == 0) return RGBDFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  DeviceBuffer in_stage;
  const float4* d_points = (const float4*)d_in;
  int rc = RGBDFE_OK;
  if (!device) {
    rc = in_stage.alloc(ctx, (size_t)n_in * sizeof(float4), "voxel filter: staging allocation failed");
    if (rc != RGBDFE_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(in_stage.p, h_in, (size_t)n_in * sizeof(float4), hipMemcpyHostToDevice, st));
    d_points = (const float4*)in_stage.p;
  }
  VoxRun run;
  rc = vox_count_cells(ctx, d_points, n_in, inv, st, &run);
  if (rc != RGBDFE_OK) return rc;
  *n_out = run.rows;
  if (flags && run.too_small) *flags |= RGBDFE_VOXEL_LEAF_TOO_SMALL;
  if (capacity < run.rows) return fail(ctx, RGBDFE_ERR_CAPACITY, "voxel filter: `out` is too small (*n_out rows are needed)");
  if (run.rows == 0) return RGBDFE_OK;
  OutputSink sink(device ? d_out : nullptr);
  rc = sink.ready(ctx, (size_t)run.rows * sizeof(float4), "voxel filter: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  rc = vox_emit(ctx, d_points, run, (float4*)sink.d, nullptr, st);
  if (rc != RGBDFE_OK) return rc;
  HIP_TRY(ctx, sink.finish(h_out, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));  // the scratch and the staging are this call's
  return RGBDFE_OK;
}

}  // namespace

int rgbdfe_voxel_filter(rgbdfe_ctx* ctx, const float* points, int64_t n_in, double voxelfilter_size, float* out, int64_t capacity,
                        int64_t* n_out, int32_t* flags) {
  return voxel_filter_common(ctx, points, nullptr, n_in, voxelfilter_size, out, nullptr, false, capacity, n_out, flags, nullptr);
}

int rgbdfe_voxel_filter_device(rgbdfe_ctx* ctx, const void* d_points, int64_t n_in, double voxelfilter_size, void* d_out,
                               int64_t capacity, int64_t* n_out, int32_t* flags, void* stream) {
  return voxel_filter_common(ctx, nullptr, d_points, n_in, voxelfilter_size, nullptr, d_out, true, capacity, n_out, flags, stream);
}

// Node::reducePointCloud: pc_col becomes its filtered cloud, unstructured (height 1)
int rgbdfe_reduce_node_cloud(rgbdfe_ctx* ctx, int32_t node_id, double voxelfilter_size, int64_t* n_out, int32_t* flags) {
  float inv = 0.f;
  if (!ctx || !n_out) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  if (!leaf_of(voxelfilter_size, &inv))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "voxelfilter_size must be positive as a float, with a finite non-zero inverse");
  std::lock_guard<std::mutex> g(ctx->mu);
  *n_out = 0;
  if (flags) *flags = 0;
  CloudEntry* found = resident_cloud(ctx, node_id);
  if (!found) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "no cloud for this node");
  CloudEntry& ce = *found;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  const int64_t n_in = (int64_t)ce.ch * (int64_t)ce.cw;
  VoxRun run;
  int rc = vox_count_cells(ctx, ce.d, n_in, inv, ctx->stream, &run);
  if (rc != RGBDFE_OK) return rc;
  *n_out = run.rows;
  if (run.too_small) {  // the reference's filter hands the input back: the cloud stays as it is, raster included
    if (flags) *flags |= RGBDFE_VOXEL_LEAF_TOO_SMALL;
    return RGBDFE_OK;
  }
  float4* d_new = nullptr;  // the rows and the z plane behind them, as every resident cloud has it
  const size_t rows = (size_t)run.rows;
  if (hipMalloc((void**)&d_new, (rows > 0 ? rows : 1) * (sizeof(float4) + sizeof(float))) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "cloud allocation failed");
  }
  rc = vox_emit(ctx, ce.d, run, d_new, reinterpret_cast<float*>(d_new + rows), ctx->stream);
  if (rc == RGBDFE_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RGBDFE_ERR_HIP, "voxel filter failed");
  if (rc == RGBDFE_OK) rc = wait_for_pair_lanes(ctx);  // nothing may still read the old cloud
  if (rc != RGBDFE_OK) {
    (void)hipFree(d_new);
    return rc;
  }
  (void)hipFree(ce.d);
  if (ce.d_samples) (void)hipFree(ce.d_samples);
  ce.d = d_new;
  ce.d_samples = nullptr;
  ce.samples_skip = 0;  // the cached EMM samples belonged to the structured cloud
  ce.ch = 1;
  ce.cw = (int)run.rows;
  return RGBDFE_OK;
}

}  // namespace impl
