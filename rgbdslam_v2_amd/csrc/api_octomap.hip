// api_octomap.hip -- the occupancy map: resident node clouds (or a host cloud) ray-cast one after another into a persistent
// table of leaves on the device (kernels: octomap.hip); GraphManager::renderToOctomap / saveOctomapImpl
// (graph_mgr_io.cpp:253-329) over ColorOctomapServer::insertCloudCallback (ColorOctomapServer.cpp:61-129)
// (one of the host-side translation units of librgbdfe.so; shared declarations: rgbdfe_host.h)
#include "rgbdfe_host.h"
#include "ot_parse.h"

#include <algorithm>

struct rgbdfe_octomap {
  rgbdfe_ctx* owner = nullptr;  // the handle the map was created on (a group's, for a multi-device one)
  rgbdfe_ctx* ctx = nullptr;    // the single-device context its table lives on
  rgbdfe_octomap_params prm{};
  OctoTable tb{};
  void* blob = nullptr;         // the table's one allocation
  OctoCtl* d_ctl = nullptr;
  uint32_t epoch = 0;           // of the last cloud
  int64_t n_leaves = 0;
  int64_t launches = 0;         // kernel launches of the last insert call (tools/bench_octomap.py)
  // the tree calls' workspace (octomap_tree.hip): one allocation, grown when a call needs more, freed with the map
  GrowBuffer tree_ws;
  int64_t tree_launches = 0;    // kernel launches of the last tree / depth / write call (tools/bench_octomap_tree.py)
  int64_t query_launches = 0;   // kernel launches of the last search / cast / view call (tools/bench_octomap_query.py)
};

namespace impl {

namespace {

// a table of `cap` slots in its one allocation: the keys, values and colours (cleared to 0xff bytes), then the marks (to 0)
struct TableLayout {
  DeviceLayout lay;
  Block key, value, colour, mark;
  explicit TableLayout(uint32_t cap)
      : key(lay.room(8 * (size_t)cap)), value(lay.room(4 * (size_t)cap)), colour(lay.room(4 * (size_t)cap)),
        mark(lay.room(4 * (size_t)cap)) {}
  hipError_t clear(void* blob, hipStream_t st) const {
    const hipError_t e = hipMemsetAsync(blob, 0xff, mark.off, st);
    return e != hipSuccess ? e : hipMemsetAsync(at<uint32_t>(blob, mark), 0, lay.total() - mark.off, st);
  }
};

// a table of `cap` free slots
int alloc_table(rgbdfe_ctx* ctx, uint32_t cap, OctoTable* tb, void** blob, hipStream_t st) {
  const TableLayout tl(cap);
  DeviceBuffer buf;
  const int rc = buf.alloc(ctx, tl.lay.total(), "octomap: table allocation failed");
  if (rc != RGBDFE_OK) return rc;
  if (tl.clear(buf.p, st) != hipSuccess) return fail(ctx, RGBDFE_ERR_HIP, "octomap: clearing the table failed");
  tb->key = at<unsigned long long>(buf.p, tl.key);
  tb->value = at<float>(buf.p, tl.value);
  tb->colour = at<uint32_t>(buf.p, tl.colour);
  tb->mark = at<uint32_t>(buf.p, tl.mark);
  tb->cap = cap;
  *blob = buf.p;
  buf.p = nullptr;  // the table is the caller's now
  return RGBDFE_OK;
}

bool cap_ok(int64_t capacity_cells) { return capacity_cells >= 1 && capacity_cells < ((int64_t)1 << 31); }

// the leaves into a fresh table of `cap` slots, which becomes the map's.  ctx->mu is held.
int rehouse(rgbdfe_octomap* map, uint32_t cap) {
  rgbdfe_ctx* ctx = map->ctx;
  hipStream_t st = ctx->stream;
  OctoTable nt{};
  void* nblob = nullptr;
  int rc = alloc_table(ctx, cap, &nt, &nblob, st);
  if (rc != RGBDFE_OK) return rc;
  OctoCtl ctl{};
  ctl.n_leaves = (uint32_t)map->n_leaves;
  hipError_t e = hipMemcpyAsync(map->d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    launch_octo_rehash(map->tb, nt, map->d_ctl, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&ctl, map->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess || ctl.overflow != 0) {
    (void)hipFree(nblob);
    return fail(ctx, e != hipSuccess ? RGBDFE_ERR_HIP : RGBDFE_ERR_INTERNAL, "octomap: re-housing the leaves failed");
  }
  (void)hipFree(map->blob);
  map->blob = nblob;
  map->tb = nt;
  map->epoch = 0;  // the fresh table's marks are 0
  return RGBDFE_OK;
}

struct CloudRef { const float4* d; uint32_t n; };

// the sort's buffers of an OctoScratch / a TreeScratch
template <class Scratch>
void fill_sort_pointers(void* base, const SortWorkspace& w, Scratch* s) {
  for (int i = 0; i < 2; ++i) {
    s->keys[i] = at<uint32_t>(base, w.keys[i]);
    s->idx[i] = at<uint32_t>(base, w.idx[i]);
  }
  s->hist = at<uint32_t>(base, w.hist);
  s->digits = at<uint32_t>(base, w.digits);
}

// the clouds one after another; ctx->mu is held and the device is set
int insert_clouds(rgbdfe_octomap* map, const std::vector<CloudRef>& clouds, const float* transforms, double max_range,
                  int32_t* n_done) {
  rgbdfe_ctx* ctx = map->ctx;
  hipStream_t st = ctx->stream;
  uint32_t n_max = 0;
  for (const CloudRef& c : clouds) n_max = std::max(n_max, c.n);
  const size_t n = n_max, n_tiles = (n + kVoxTile - 1) / kVoxTile;
  DeviceLayout lay;
  const Block b_hdr = lay.room(256), b_count = lay.room(4 * n_tiles), b_first = lay.room(4 * (n_tiles + 1));
  const SortWorkspace b_sort = sort_workspace(lay, n);
  const Block b_cells = lay.room(4 * (n + 1));
  int rc = ensure_scratch(ctx, lay.total());
  if (rc != RGBDFE_OK) return rc;
  OctoScratch s{};
  s.hdr = at<VoxHeader>(ctx->d_scratch, b_hdr);
  s.tile_count = at<uint32_t>(ctx->d_scratch, b_count);
  s.tile_first = at<uint32_t>(ctx->d_scratch, b_first);
  s.cell_start = at<uint32_t>(ctx->d_scratch, b_cells);
  fill_sort_pointers(ctx->d_scratch, b_sort, &s);

  // the colour rows are sorted by slot, `cap` standing for "no leaf": the passes that cover 0 .. cap
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)map->tb.cap) ++bits;
  const int passes = (bits + 7) / 8;

  const rgbdfe_octomap_params& p = map->prm;
  OctoCloud oc{};
  oc.res = p.resolution;
  oc.inv_res = 1.0 / p.resolution;
  oc.max_range = max_range;
  oc.hit = (float)log(p.prob_hit / (1.0 - p.prob_hit));
  oc.miss = (float)log(p.prob_miss / (1.0 - p.prob_miss));
  oc.clamp_min = (float)log(p.clamping_min / (1.0 - p.clamping_min));
  oc.clamp_max = (float)log(p.clamping_max / (1.0 - p.clamping_max));

  OctoCtl ctl{};
  ctl.n_leaves = (uint32_t)map->n_leaves;
  HIP_TRY(ctx, hipMemcpyAsync(map->d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, st));
  map->launches = 0;
  for (size_t k = 0; k < clouds.size(); ++k) {
    if (map->epoch >= 0x7ffffffeu) {  // 2 * epoch + 1 must fit the mark
      HIP_TRY(ctx, hipMemsetAsync(map->tb.mark, 0, 4 * (size_t)map->tb.cap, st));
      map->epoch = 0;
    }
    oc.epoch = ++map->epoch;
    rigid_of_matrix4f(transforms + k * 16, oc.R, oc.t);
    launch_octo_cloud(map->tb, map->d_ctl, clouds[k].d, clouds[k].n, oc, passes, s, st);
    map->launches += clouds[k].n == 0 ? 1 : 7 + 3 * passes;
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&ctl, map->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));  // the one read of the call
  HIP_TRY(ctx, hipStreamSynchronize(st));
  map->n_leaves = (int64_t)ctl.n_leaves;
  if (n_done) *n_done = (int32_t)ctl.n_done;
  if (ctl.overflow != 0) {
    // the cloud that did not fit left claimed keys without leaves: a fresh table of the same size holds the leaves only
    rc = rehouse(map, map->tb.cap);
    if (rc != RGBDFE_OK) return rc;
    return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: the table is full (the clouds before *n_done are in; reserve more cells)");
  }
  return RGBDFE_OK;
}

bool range_ok(double max_range) { return !std::isnan(max_range); }

}  // namespace

void rgbdfe_octomap_default_params(rgbdfe_octomap_params* p) {
  if (!p) return;
  p->resolution = 0.05;            // octomap_resolution (parameter_server.cpp:56)
  p->prob_hit = 0.9;               // octomap_prob_hit (:63)
  p->prob_miss = 0.4;              // octomap_prob_miss (:64)
  p->clamping_min = 0.001;         // octomap_clamping_min (:62)
  p->clamping_max = 0.999;         // octomap_clamping_max (:61)
  p->occupancy_threshold = 0.5;    // octomap_occupancy_threshold (:60)
}

rgbdfe_ctx* octomap_owner(rgbdfe_octomap* map) { return map ? map->owner : nullptr; }

int rgbdfe_octomap_create(rgbdfe_ctx* ctx, rgbdfe_ctx* owner, const rgbdfe_octomap_params* params, int64_t capacity_cells,
                          rgbdfe_octomap** out) {
  if (!ctx || !out) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  *out = nullptr;
  rgbdfe_octomap_params p;
  impl::rgbdfe_octomap_default_params(&p);
  if (params) p = *params;
  auto prob = [](double v) { return v > 0.0 && v < 1.0; };
  if (!(p.resolution > 0.0) || !std::isfinite(p.resolution) || !std::isfinite(1.0 / p.resolution) || !prob(p.prob_hit) ||
      !prob(p.prob_miss) || !prob(p.clamping_min) || !prob(p.clamping_max) || !(p.clamping_min <= p.clamping_max))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG,
                "octomap: resolution must be positive and finite, the probabilities inside (0, 1), clamping_min <= clamping_max");
  if (!cap_ok(capacity_cells)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "octomap: capacity_cells must lie in [1, 2^31)");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  std::unique_ptr<rgbdfe_octomap> map(new rgbdfe_octomap());
  map->owner = owner;
  map->ctx = ctx;
  map->prm = p;
  if (hipMalloc((void**)&map->d_ctl, sizeof(OctoCtl)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, RGBDFE_ERR_OUT_OF_MEMORY, "octomap: allocation failed");
  }
  int rc = alloc_table(ctx, (uint32_t)capacity_cells, &map->tb, &map->blob, ctx->stream);
  if (rc == RGBDFE_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RGBDFE_ERR_HIP, "octomap: clearing the table failed");
  if (rc != RGBDFE_OK) {
    if (map->blob) (void)hipFree(map->blob);
    (void)hipFree(map->d_ctl);
    return rc;
  }
  *out = map.release();
  return RGBDFE_OK;
}

void rgbdfe_octomap_destroy(rgbdfe_octomap* map) {
  if (!map) return;
  {
    std::lock_guard<std::mutex> g(map->ctx->mu);
    (void)hipSetDevice(map->ctx->cfg.device_id);
    (void)hipStreamSynchronize(map->ctx->stream);
    if (map->blob) (void)hipFree(map->blob);
    if (map->d_ctl) (void)hipFree(map->d_ctl);
    if (map->tree_ws.p) (void)hipFree(map->tree_ws.p);
  }
  delete map;
}

// no leaves, the same table; ctx->mu is held and the device is set
static int clear_map(rgbdfe_octomap* map) {
  rgbdfe_ctx* ctx = map->ctx;
  HIP_TRY(ctx, TableLayout(map->tb.cap).clear(map->blob, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  map->epoch = 0;
  map->n_leaves = 0;
  return RGBDFE_OK;
}

// ColorOctomapServer::reset: an empty tree with the same parameters
int rgbdfe_octomap_reset(rgbdfe_octomap* map) {
  rgbdfe_ctx* ctx = map->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  return clear_map(map);
}

int rgbdfe_octomap_reserve(rgbdfe_octomap* map, int64_t capacity_cells) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!cap_ok(capacity_cells)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "octomap: capacity_cells must lie in [1, 2^31)");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (capacity_cells < map->n_leaves) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: fewer cells than the map has leaves");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  return rehouse(map, (uint32_t)capacity_cells);
}

int rgbdfe_octomap_insert_nodes(rgbdfe_octomap* map, int32_t n_nodes, const int32_t* node_ids, const float* transforms,
                                double max_range, int32_t* n_done) {
  rgbdfe_ctx* ctx = map->ctx;
  if (n_done) *n_done = 0;
  if (n_nodes < 0 || (n_nodes > 0 && (!node_ids || !transforms)) || !range_ok(max_range))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad octomap insertion arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (n_nodes == 0) return RGBDFE_OK;
  std::vector<CloudRef> clouds((size_t)n_nodes);
  for (size_t k = 0; k < clouds.size(); ++k) {
    const CloudEntry* ce = resident_cloud(ctx, node_ids[k]);
    if (!ce) return fail(ctx, RGBDFE_ERR_UNKNOWN_NODE, "octomap: no cloud for a listed node");
    clouds[k].d = ce->d;
    clouds[k].n = (uint32_t)((size_t)ce->ch * (size_t)ce->cw);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  return insert_clouds(map, clouds, transforms, max_range, n_done);
}

int rgbdfe_octomap_insert_cloud(rgbdfe_octomap* map, const float* points, int64_t n, const float* transform, double max_range) {
  rgbdfe_ctx* ctx = map->ctx;
  if (n < 0 || (n > 0 && !points) || !transform || !range_ok(max_range))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad octomap insertion arguments");
  if (n > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: 2^31 points or more in one cloud");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  DeviceBuffer stage;
  if (n > 0) {
    const int rc = stage.alloc(ctx, (size_t)n * sizeof(float4), "octomap: staging allocation failed");
    if (rc != RGBDFE_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(stage.p, points, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  }
  std::vector<CloudRef> clouds(1);
  clouds[0].d = (const float4*)stage.p;
  clouds[0].n = (uint32_t)n;
  return insert_clouds(map, clouds, transform, max_range, nullptr);  // synchronises before `stage` goes
}

int rgbdfe_octomap_size(rgbdfe_octomap* map, int64_t* n_leaves) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!n_leaves) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  *n_leaves = map->n_leaves;
  return RGBDFE_OK;
}

int rgbdfe_octomap_stats(rgbdfe_octomap* map, int64_t* out, int32_t n_out) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!out || n_out < 0) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const int64_t v[5] = {(int64_t)map->tb.cap, map->n_leaves, map->launches, map->tree_launches, map->query_launches};
  for (int32_t i = 0; i < n_out; ++i) out[i] = i < 5 ? v[i] : 0;
  return RGBDFE_OK;
}

int rgbdfe_octomap_leaves(rgbdfe_octomap* map, rgbdfe_octomap_leaf* out, int64_t capacity, int64_t* n_out) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!n_out || capacity < 0 || (capacity > 0 && !out)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  *n_out = map->n_leaves;
  if (capacity < map->n_leaves) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: `out` is too small (*n_out records are needed)");
  if (map->n_leaves == 0) return RGBDFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  const size_t cap = map->tb.cap;
  std::vector<unsigned long long> key(cap);
  std::vector<uint32_t> value(cap), colour(cap);
  HIP_TRY(ctx, hipMemcpyAsync(key.data(), map->tb.key, 8 * cap, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(value.data(), map->tb.value, 4 * cap, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(colour.data(), map->tb.colour, 4 * cap, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<std::pair<unsigned long long, uint32_t>> order;  // (key, slot) of the leaves
  order.reserve((size_t)map->n_leaves);
  for (size_t i = 0; i < cap; ++i)
    if (key[i] != kOctoEmptyKey && value[i] != kOctoNoLeaf) order.emplace_back(key[i], (uint32_t)i);
  if ((int64_t)order.size() != map->n_leaves) return fail(ctx, RGBDFE_ERR_INTERNAL, "octomap: the leaf count and the table disagree");
  std::sort(order.begin(), order.end());
  for (size_t r = 0; r < order.size(); ++r) {
    const unsigned long long k = order[r].first;
    const uint32_t i = order[r].second;
    rgbdfe_octomap_leaf& o = out[r];
    o.key[0] = (uint16_t)(k & 0xffffu); o.key[1] = (uint16_t)((k >> 16) & 0xffffu); o.key[2] = (uint16_t)((k >> 32) & 0xffffu);
    o.zero0 = 0;
    memcpy(&o.log_odds, &value[i], 4);
    o.rgb[0] = (uint8_t)((colour[i] >> 16) & 255u); o.rgb[1] = (uint8_t)((colour[i] >> 8) & 255u); o.rgb[2] = (uint8_t)(colour[i] & 255u);
    o.zero1 = 0;
  }
  return RGBDFE_OK;
}

// ---- the tree of the leaf set: inner nodes, one depth, .ot files (kernels: octomap_tree.hip) ------------------------------

namespace {

// the workspace of a tree call over the map as it is; ctx->mu is held and the device is set
int tree_workspace(rgbdfe_octomap* map, TreeScratch* t) {
  rgbdfe_ctx* ctx = map->ctx;
  const size_t n = (size_t)map->n_leaves, cap = map->tb.cap;
  if (17 * (uint64_t)n > (uint64_t)UINT32_MAX)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: the tree of this map may have 2^32 nodes or more");
  const size_t tiles = (std::max(n, cap) + kTreeTile - 1) / kTreeTile;
  // (the sort's histogram and digit totals sit behind its pairs, in front of top / off / the levels)
  DeviceLayout lay;
  const Block b_hdr = lay.room(256), b_code = lay.room(8 * n), b_scode = lay.room(8 * n), b_slot = lay.room(4 * n);
  const SortWorkspace b_sort = sort_workspace(lay, n);
  const Block b_top = lay.room(4 * n), b_off = lay.room(4 * n);
  Block b_level[2][3];
  for (auto& level : b_level)
    for (Block& b : level) b = lay.room(4 * n);
  const Block b_count = lay.room(4 * tiles), b_first = lay.room(4 * (tiles + 1));
  const int rc = map->tree_ws.ensure(ctx, lay.total(), "octomap: tree workspace allocation failed");
  if (rc != RGBDFE_OK) return rc;
  void* base = map->tree_ws.p;
  t->hdr = at<TreeHdr>(base, b_hdr);
  t->code = at<unsigned long long>(base, b_code);
  t->scode = at<unsigned long long>(base, b_scode);
  t->slot = at<uint32_t>(base, b_slot);
  fill_sort_pointers(base, b_sort, t);
  t->top = at<uint32_t>(base, b_top);
  t->off = at<uint32_t>(base, b_off);
  for (int l = 0; l < 2; ++l) {
    t->level[l].value = at<float>(base, b_level[l][0]);
    t->level[l].colour = at<uint32_t>(base, b_level[l][1]);
    t->level[l].first = at<uint32_t>(base, b_level[l][2]);
  }
  t->tile_count = at<uint32_t>(base, b_count);
  t->tile_first = at<uint32_t>(base, b_first);
  return RGBDFE_OK;
}

// the records of the whole tree to host (h_out) or device (d_out) memory; ctx->mu is held
// (or, with `vec`, to a vector that takes the size the tree needs)
int tree_common(rgbdfe_octomap* map, rgbdfe_octomap_node* h_out, void* d_out, bool to_device, int64_t capacity, int64_t* n_nodes,
                void* stream, std::vector<rgbdfe_octomap_node>* vec = nullptr) {
  rgbdfe_ctx* ctx = map->ctx;
  *n_nodes = 0;
  map->tree_launches = 0;
  if (map->n_leaves == 0) return RGBDFE_OK;  // an empty map has no node, not even a root
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  TreeScratch t{};
  int rc = tree_workspace(map, &t);
  if (rc != RGBDFE_OK) return rc;
  const uint32_t n = (uint32_t)map->n_leaves;
  HIP_TRY(ctx, hipMemsetAsync(t.hdr, 0, sizeof(TreeHdr), st));
  int launches = launch_tree_leaves(map->tb, n, t, st);
  launches += launch_tree_chain(n, t, st);
  HIP_TRY(ctx, hipGetLastError());
  TreeHdr h{};
  HIP_TRY(ctx, hipMemcpyAsync(&h, t.hdr, sizeof(h), hipMemcpyDeviceToHost, st));  // the one read before the capacity check
  HIP_TRY(ctx, hipStreamSynchronize(st));
  map->tree_launches = launches;
  if ((int64_t)h.cnt[16] != map->n_leaves) return fail(ctx, RGBDFE_ERR_INTERNAL, "octomap: the leaf count and the table disagree");
  const int64_t total = (int64_t)h.n_nodes;
  *n_nodes = total;
  if (vec) {
    vec->resize((size_t)total);
    h_out = vec->data();
  } else if (capacity < total) {
    return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: `out` is too small (*n_nodes records are needed)");
  }
  OutputSink sink(to_device ? d_out : nullptr);
  rc = sink.ready(ctx, (size_t)total * sizeof(rgbdfe_octomap_node), "octomap: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  launches += launch_tree_levels(n, 0u, t, sink.d, st);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, sink.finish(h_out, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  map->tree_launches = launches;
  return RGBDFE_OK;
}

std::string ot_header(const rgbdfe_octomap* map, int64_t n_nodes) {
  char res[64], size[64];
  snprintf(res, sizeof(res), "%g", map->prm.resolution);
  snprintf(size, sizeof(size), "%lld", (long long)n_nodes);
  return std::string("# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                     "id ColorOcTree\nsize ") + size + "\nres " + res + "\ndata\n";
}

// `leaves` become the map's contents; ctx->mu is held
int set_leaves_locked(rgbdfe_octomap* map, const rgbdfe_octomap_leaf* leaves, int64_t n) {
  rgbdfe_ctx* ctx = map->ctx;
  if (n > (int64_t)map->tb.cap) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: more leaves than the map has cells (nothing changed)");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = ctx->stream;
  int rc = clear_map(map);
  if (rc != RGBDFE_OK || n == 0) return rc;
  std::vector<OctoLeafIn> in((size_t)n);
  for (size_t i = 0; i < in.size(); ++i) {
    const rgbdfe_octomap_leaf& l = leaves[i];
    if (l.zero0 != 0 || l.zero1 != 0 || !std::isfinite(l.log_odds))
      return fail(ctx, RGBDFE_ERR_INVALID_ARG, "octomap: a leaf with non-zero padding or a non-finite log-odds (the map is empty)");
    in[i].key = (unsigned long long)l.key[0] | ((unsigned long long)l.key[1] << 16) | ((unsigned long long)l.key[2] << 32);
    in[i].value = l.log_odds;
    in[i].colour = ((uint32_t)l.rgb[0] << 16) | ((uint32_t)l.rgb[1] << 8) | (uint32_t)l.rgb[2];
  }
  DeviceLayout lay;
  const Block b_in = lay.room(in.size() * sizeof(OctoLeafIn)), b_dup = lay.room(256);
  DeviceBuffer stage;
  rc = stage.alloc(ctx, lay.total(), "octomap: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  OctoLeafIn* d_in = at<OctoLeafIn>(stage.p, b_in);
  uint32_t* d_dup = at<uint32_t>(stage.p, b_dup);
  OctoCtl ctl{};
  uint32_t dup = 0;
  HIP_TRY(ctx, hipMemcpyAsync(d_in, in.data(), b_in.bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(d_dup, 0, 4, st));
  HIP_TRY(ctx, hipMemcpyAsync(map->d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, st));
  launch_octo_set_leaves(d_in, (uint32_t)n, map->tb, map->d_ctl, d_dup, st);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&ctl, map->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&dup, d_dup, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (dup != 0 || ctl.overflow != 0) {
    rc = clear_map(map);
    if (rc != RGBDFE_OK) return rc;
    return dup != 0 ? fail(ctx, RGBDFE_ERR_INVALID_ARG, "octomap: a key is repeated among the leaves (the map is empty)")
                    : fail(ctx, RGBDFE_ERR_INTERNAL, "octomap: a leaf found no slot");
  }
  map->n_leaves = n;
  return RGBDFE_OK;
}

}  // namespace

int rgbdfe_octomap_tree(rgbdfe_octomap* map, rgbdfe_octomap_node* out, int64_t capacity, int64_t* n_nodes) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!n_nodes || capacity < 0 || (capacity > 0 && !out)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  return tree_common(map, out, nullptr, false, capacity, n_nodes, nullptr);
}

int rgbdfe_octomap_tree_device(rgbdfe_octomap* map, void* d_out, int64_t capacity, int64_t* n_nodes, void* stream) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!n_nodes || capacity < 0 || (capacity > 0 && !d_out)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  return tree_common(map, nullptr, d_out, true, capacity, n_nodes, stream);
}

int rgbdfe_octomap_nodes_at_depth(rgbdfe_octomap* map, int32_t depth, float min_log_odds, rgbdfe_octomap_leaf* out, int64_t capacity,
                                  int64_t* n_out) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!n_out || capacity < 0 || (capacity > 0 && !out) || depth < 0 || depth > 16 || std::isnan(min_log_odds))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "octomap: bad depth query arguments (depth 0 .. 16, min_log_odds not NaN)");
  std::lock_guard<std::mutex> g(ctx->mu);
  *n_out = 0;
  map->tree_launches = 0;
  if (map->n_leaves == 0) return RGBDFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = ctx->stream;
  TreeScratch t{};
  int rc = tree_workspace(map, &t);
  if (rc != RGBDFE_OK) return rc;
  const uint32_t n = (uint32_t)map->n_leaves;
  // the nodes of a depth are at most min(leaves, 8^depth): the staging is sized before anything runs
  const uint64_t bound = depth >= 11 ? (uint64_t)n : std::min<uint64_t>(n, (uint64_t)1 << (3 * depth));
  DeviceBuffer stage;
  rc = stage.alloc(ctx, (size_t)bound * sizeof(rgbdfe_octomap_leaf), "octomap: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  HIP_TRY(ctx, hipMemsetAsync(t.hdr, 0, sizeof(TreeHdr), st));
  int launches = launch_tree_leaves(map->tb, n, t, st);
  launches += launch_tree_levels(n, (uint32_t)depth, t, nullptr, st);
  launches += launch_tree_filter(n, (uint32_t)depth, min_log_odds, t, stage.p, st);
  HIP_TRY(ctx, hipGetLastError());
  TreeHdr h{};
  HIP_TRY(ctx, hipMemcpyAsync(&h, t.hdr, sizeof(h), hipMemcpyDeviceToHost, st));  // the one read before the capacity check
  HIP_TRY(ctx, hipStreamSynchronize(st));
  map->tree_launches = launches;
  if ((int64_t)h.cnt[16] != map->n_leaves) return fail(ctx, RGBDFE_ERR_INTERNAL, "octomap: the leaf count and the table disagree");
  *n_out = (int64_t)h.n_out;
  if (capacity < *n_out) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: `out` is too small (*n_out records are needed)");
  if (h.n_out > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(out, stage.p, (size_t)h.n_out * sizeof(rgbdfe_octomap_leaf), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return RGBDFE_OK;
}

int rgbdfe_octomap_write(rgbdfe_octomap* map, const char* path) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!path) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  // the payload first: a failure on the device leaves no file behind
  std::vector<rgbdfe_octomap_node> rec;
  int64_t n_nodes = 0;
  const int rc = tree_common(map, nullptr, nullptr, false, 0, &n_nodes, nullptr, &rec);
  if (rc != RGBDFE_OK) return rc;
  const std::string head = ot_header(map, n_nodes);
  FILE* f = fopen(path, "wb");
  if (!f) return fail(ctx, RGBDFE_ERR_INVALID_ARG, std::string("octomap: cannot open for writing: ") + path);
  bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
  if (ok && !rec.empty()) ok = fwrite(rec.data(), sizeof(rgbdfe_octomap_node), rec.size(), f) == rec.size();
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    (void)remove(path);  // nothing partial stays behind under the name
    return fail(ctx, RGBDFE_ERR_INTERNAL, std::string("octomap: writing failed (the file was removed): ") + path);
  }
  return RGBDFE_OK;
}

int rgbdfe_octomap_set_leaves(rgbdfe_octomap* map, const rgbdfe_octomap_leaf* leaves, int64_t n) {
  rgbdfe_ctx* ctx = map->ctx;
  if (n < 0 || (n > 0 && !leaves)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  return set_leaves_locked(map, leaves, n);
}

int rgbdfe_octomap_read(rgbdfe_octomap* map, const char* path) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!path) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::vector<uint8_t> bytes;
  {
    FILE* f = fopen(path, "rb");
    if (!f) return fail(ctx, RGBDFE_ERR_INVALID_ARG, std::string("octomap: cannot open for reading: ") + path);
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail(ctx, RGBDFE_ERR_INTERNAL, std::string("octomap: reading failed: ") + path);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  char res[64];
  snprintf(res, sizeof(res), "%g", map->prm.resolution);
  std::vector<rgbdfe_octomap_leaf> leaves;
  std::string err;
  if (!ot_parse(bytes.data(), bytes.size(), res, &leaves, &err)) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "octomap: " + err);
  return set_leaves_locked(map, leaves.data(), (int64_t)leaves.size());
}

// ---- the read side: point lookups, ray casts, the map seen from a pose (kernels: octomap_query.hip) ----------------------

namespace {

// logodds(occupancy_threshold), checked here, where it is used
int map_occupied(rgbdfe_octomap* map, float* out) {
  const double t = map->prm.occupancy_threshold;
  if (!(t > 0.0 && t < 1.0)) return fail(map->ctx, RGBDFE_ERR_INVALID_ARG, "octomap: occupancy_threshold must lie inside (0, 1)");
  *out = (float)log(t / (1.0 - t));
  return RGBDFE_OK;
}

// the work bound of the block, then the walk's parameters; ctx->mu is held
int query_setup(rgbdfe_octomap* map, int32_t ignore_unknown, double max_range, float occupied_log_odds, OctoQuery* q) {
  rgbdfe_ctx* ctx = map->ctx;
  if (4 * map->n_leaves > 3 * (int64_t)map->tb.cap)
    return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: the table is loaded above 3/4, a query would crawl (reserve more cells first)");
  q->res = map->prm.resolution;
  q->inv_res = 1.0 / map->prm.resolution;
  q->max_range2 = max_range > 0.0 ? max_range * max_range : -1.0;
  q->ignore_unknown = ignore_unknown != 0 ? 1u : 0u;
  q->occupied = occupied_log_odds;
  return std::isnan(occupied_log_odds) ? map_occupied(map, &q->occupied) : RGBDFE_OK;
}

int view_common(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                int32_t ignore_unknown, double max_range, float occupied_log_odds, float* h_out, uint8_t* h_status, void* d_out,
                void* d_status, bool to_device, void* stream) {
  rgbdfe_ctx* ctx = map->ctx;
  const int64_t n = (int64_t)rows * (int64_t)cols;
  if (rows < 0 || cols < 0 || !transform || !range_ok(max_range) || (n > 0 && !(to_device ? d_out : (void*)h_out)))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad octomap view arguments");
  if (n > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: 2^31 pixels or more in one view");
  std::lock_guard<std::mutex> g(ctx->mu);
  map->query_launches = 0;
  if (n == 0) return RGBDFE_OK;
  OctoQuery q{};
  int rc = query_setup(map, ignore_unknown, max_range, occupied_log_odds, &q);
  if (rc != RGBDFE_OK) return rc;
  OctoView v{};
  rigid_of_matrix4f(transform, v.R, v.t);
  v.fx = (float)fx; v.fy = (float)fy; v.cx = (float)cx; v.cy = (float)cy;
  v.rows = (uint32_t)rows; v.cols = (uint32_t)cols;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = (to_device && stream) ? (hipStream_t)stream : ctx->stream;
  const bool want_status = to_device ? d_status != nullptr : h_status != nullptr;
  OutputSink cloud(to_device ? d_out : nullptr), plane(to_device ? d_status : nullptr);
  rc = cloud.ready(ctx, (size_t)n * sizeof(float4), "octomap: staging allocation failed");
  if (rc == RGBDFE_OK && want_status && !to_device) rc = plane.ready(ctx, (size_t)n, "octomap: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  launch_octo_view(map->tb, v, q, (float4*)cloud.d, want_status ? (uint8_t*)plane.d : nullptr, st);
  HIP_TRY(ctx, hipGetLastError());
  map->query_launches = 1;
  HIP_TRY(ctx, cloud.finish(h_out, st));
  if (want_status && !to_device) HIP_TRY(ctx, plane.finish(h_status, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return RGBDFE_OK;
}

}  // namespace

int rgbdfe_octomap_occupied_log_odds(rgbdfe_octomap* map, float* out) {
  rgbdfe_ctx* ctx = map->ctx;
  if (!out) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  return map_occupied(map, out);
}

int rgbdfe_octomap_search(rgbdfe_octomap* map, const float* points, int64_t n, int32_t* found, rgbdfe_octomap_leaf* leaves) {
  rgbdfe_ctx* ctx = map->ctx;
  if (n < 0 || (n > 0 && (!points || !found || !leaves))) return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad octomap search arguments");
  if (n > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: 2^31 points or more in one search");
  std::lock_guard<std::mutex> g(ctx->mu);
  map->query_launches = 0;
  if (n == 0) return RGBDFE_OK;
  OctoQuery q{};
  int rc = query_setup(map, 0, -1.0, 0.0f, &q);
  if (rc != RGBDFE_OK) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = ctx->stream;
  DeviceLayout lay;
  const Block b_pts = lay.room(12 * (size_t)n), b_found = lay.room(4 * (size_t)n), b_leaves = lay.room(16 * (size_t)n);
  DeviceBuffer stage;
  rc = stage.alloc(ctx, lay.total(), "octomap: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(at<float>(stage.p, b_pts), points, 12 * (size_t)n, hipMemcpyHostToDevice, st));
  launch_octo_search(map->tb, at<float>(stage.p, b_pts), (uint32_t)n, q.inv_res, at<int32_t>(stage.p, b_found),
                     at<uint4>(stage.p, b_leaves), st);
  HIP_TRY(ctx, hipGetLastError());
  map->query_launches = 1;
  HIP_TRY(ctx, hipMemcpyAsync(found, at<int32_t>(stage.p, b_found), 4 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(leaves, at<uint4>(stage.p, b_leaves), 16 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return RGBDFE_OK;
}

int rgbdfe_octomap_cast_rays(rgbdfe_octomap* map, const float* origins, const float* directions, int64_t n, int32_t ignore_unknown,
                             double max_range, float occupied_log_odds, rgbdfe_octomap_ray_hit* hits) {
  rgbdfe_ctx* ctx = map->ctx;
  if (n < 0 || (n > 0 && (!origins || !directions || !hits)) || !range_ok(max_range))
    return fail(ctx, RGBDFE_ERR_INVALID_ARG, "bad octomap ray cast arguments");
  if (n > (int64_t)INT32_MAX) return fail(ctx, RGBDFE_ERR_CAPACITY, "octomap: 2^31 rays or more in one call");
  std::lock_guard<std::mutex> g(ctx->mu);
  map->query_launches = 0;
  if (n == 0) return RGBDFE_OK;
  OctoQuery q{};
  int rc = query_setup(map, ignore_unknown, max_range, occupied_log_odds, &q);
  if (rc != RGBDFE_OK) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device_id));
  hipStream_t st = ctx->stream;
  DeviceLayout lay;
  const Block b_o = lay.room(12 * (size_t)n), b_d = lay.room(12 * (size_t)n),
              b_hits = lay.room(sizeof(rgbdfe_octomap_ray_hit) * (size_t)n);
  DeviceBuffer stage;
  rc = stage.alloc(ctx, lay.total(), "octomap: staging allocation failed");
  if (rc != RGBDFE_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(at<float>(stage.p, b_o), origins, 12 * (size_t)n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(at<float>(stage.p, b_d), directions, 12 * (size_t)n, hipMemcpyHostToDevice, st));
  launch_octo_cast(map->tb, at<float>(stage.p, b_o), at<float>(stage.p, b_d), (uint32_t)n, q,
                   at<rgbdfe_octomap_ray_hit>(stage.p, b_hits), st);
  HIP_TRY(ctx, hipGetLastError());
  map->query_launches = 1;
  HIP_TRY(ctx, hipMemcpyAsync(hits, at<rgbdfe_octomap_ray_hit>(stage.p, b_hits), sizeof(rgbdfe_octomap_ray_hit) * (size_t)n,
                              hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return RGBDFE_OK;
}

int rgbdfe_octomap_view_cloud(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy, int32_t rows,
                              int32_t cols, int32_t ignore_unknown, double max_range, float occupied_log_odds, float* out,
                              uint8_t* status) {
  return view_common(map, transform, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range, occupied_log_odds, out, status, nullptr,
                     nullptr, false, nullptr);
}

int rgbdfe_octomap_view_cloud_device(rgbdfe_octomap* map, const float* transform, double fx, double fy, double cx, double cy,
                                     int32_t rows, int32_t cols, int32_t ignore_unknown, double max_range, float occupied_log_odds,
                                     void* d_out, void* d_status, void* stream) {
  return view_common(map, transform, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range, occupied_log_odds, nullptr, nullptr, d_out,
                     d_status, true, stream);
}

}  // namespace impl
