"""CPU: the restatement of the map's read side (tests/octomap_query_oracle.py) held against independent arithmetic: the
leaves it must find, a float64 ray-box slab intersection over all occupied leaves, the cells insertion itself marked, and
hand-written expectations for every status and boundary of the contract (include/rgbdfe.h, "occupancy map: the read
side").  The kernels are held against this oracle in tests/test_emu_octomap_query_kernels.py and
tests/test_gpu_octomap_query.py."""
import math

import numpy as np

import octomap_oracle as oo
import octomap_query_oracle as qo

F = np.float32


def cell_of(rec):
    return tuple(int(k) - 32768 for k in rec["key"])


# ---- (a) search
def test_search_finds_every_leaf_at_its_centre_and_nothing_one_cell_into_empty_space():
    scene = qo.random_scene(seed=3, n=300, half=6)
    lv, res = scene["leaves"], scene["resolution"]
    q = qo.oracle_of(scene)
    centres = qo.points_of_keys([oo.pack(*k) for k in lv["key"]], res)
    found, recs = q.search(centres)
    assert (found == 1).all() and recs.tobytes() == lv.tobytes()
    # one cell beyond the cube's faces there is no leaf: every centre moved there along x
    out = centres.copy()
    out[:, 0] = F((6 + 0.5) * res)
    found, recs = q.search(out)
    assert (found == 0).all() and not recs["log_odds"].any() and not recs["rgb"].any()
    assert (recs["key"][:, 0] == 32768 + 6).all() and (recs["key"][:, 1:] == lv["key"][:, 1:]).all()
    # one cell to the side of each leaf, where the neighbour is empty
    have = {tuple(k) for k in lv["key"].astype(int)}
    lone = np.array([k for k in lv["key"].astype(int) if (k[0], k[1], k[2] + 1) not in have])
    assert len(lone) > 200
    side = qo.points_of_keys([oo.pack(k[0], k[1], k[2] + 1) for k in lone], res)
    found, _ = q.search(side)
    assert (found == 0).all()


# ---- (b) the first occupied cell by slab intersection
SLAB_SEED, SLAB_RES, SLAB_LEAVES, SLAB_RAYS = 21, 0.1, 400, 300
SLAB_EXCLUDED = 0   # rays set aside as ties or grazes: the recorded number (the cap is 2 % = 6)


def slab(o, d, lo, hi):
    """Entry and exit parameter of the ray o + t d (t >= 0) through the boxes [lo, hi] (n, 3); entry > exit: no hit."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    par = d == 0.0
    inside = (o >= lo) & (o <= hi)
    near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    return np.maximum(near.max(axis=1), 0.0), far.min(axis=1)


def test_the_hit_cell_is_the_first_occupied_box_of_a_float64_slab_test():
    scene = qo.random_scene(seed=SLAB_SEED, n=SLAB_LEAVES, half=8, res=SLAB_RES)
    lv, res = scene["leaves"], SLAB_RES
    q = qo.oracle_of(scene)
    occ = lv[lv["log_odds"] >= q.occupied_log_odds()]
    assert 100 < len(occ) < len(lv)
    cells = occ["key"].astype(np.float64) - 32768.0
    lo, hi = cells * res, (cells + 1.0) * res
    rng = np.random.default_rng(SLAB_SEED + 1)
    O = rng.uniform(-8 * res, 8 * res, (SLAB_RAYS, 3)).astype(np.float32)
    aim = rng.integers(0, len(occ), SLAB_RAYS)
    P = (lo[aim] + rng.uniform(0.2, 0.8, (SLAB_RAYS, 3)) * res).astype(np.float32)  # a point well inside an occupied box
    D = P - O
    hits = q.cast_rays(O, D, ignore_unknown=1, max_range=-1.0)
    margin = 1e-9 * res
    excluded = 0
    for i in range(SLAB_RAYS):
        o, d = O[i].astype(np.float64), D[i].astype(np.float64)
        unit = np.linalg.norm(d)
        e_in, x_in = slab(o, d, lo + margin, hi - margin)    # the boxes shrunk: a hit beyond doubt
        e_out, x_out = slab(o, d, lo - margin, hi + margin)  # the boxes grown: everything that is touched at all
        sure, maybe = e_in <= x_in, e_out <= x_out
        assert sure[aim[i]]
        first = np.argmin(np.where(sure, e_in, np.inf))
        others = np.delete(np.arange(len(occ)), first)
        tie = (np.where(sure, e_in, np.inf)[others] - e_in[first]) * unit < margin
        graze = (maybe & ~sure)[others] & ((e_out[others] - e_in[first]) * unit < margin)
        if tie.any() or graze.any():
            excluded += 1
            continue
        assert hits["status"][i] == qo.HIT, (i, hits[i])
        assert tuple(hits["key"][i]) == tuple(occ["key"][first]), (i, hits[i], occ[first])
        assert hits["log_odds"][i] == occ["log_odds"][first] and tuple(hits["rgb"][i]) == tuple(occ["rgb"][first])
    print("slab test: %d of %d rays excluded" % (excluded, SLAB_RAYS))
    assert excluded * 50 <= SLAB_RAYS
    assert excluded == SLAB_EXCLUDED


# ---- (c) consistency with insertion
RASTER_HITS, RASTER_RAYS = 2924, 2924   # the recorded counts of the raster below


def test_rays_towards_the_points_of_an_inserted_cloud_end_in_the_cells_insertion_marked():
    res = 0.1
    pts, T = oo.raster(64, 48), oo.translation()
    m = oo.LiteralMap(resolution=res)
    m.insert(pts, T, -1.0)
    lv = m.leaves()
    q = qo.QueryOracle(lv, resolution=res)
    occupied = {oo.pack(*l["key"]) for l in lv if l["log_odds"] >= q.occupied_log_odds()}
    R, o = oo.split_transform(T)
    fin = np.isfinite(pts[:, :3]).all(axis=1)
    X = pts[fin, :3]
    P = np.stack([((R[a, 0] * X[:, 0] + R[a, 1] * X[:, 1]) + R[a, 2] * X[:, 2]) + o[a] for a in range(3)], axis=1)  # as insertion
    D = P - o[None, :]
    hits = q.cast_rays(np.broadcast_to(o, P.shape), D, ignore_unknown=0, max_range=-1.0)
    is_hit = hits["status"] == qo.HIT
    print("insertion consistency: %d of %d rays hit; statuses %s" % (is_hit.sum(), len(P), np.unique(hits["status"], return_counts=True)))
    reach = np.linalg.norm(D.astype(np.float64), axis=1) + res * math.sqrt(3.0)
    for h, r in zip(hits[is_hit], reach[is_hit]):
        assert oo.pack(*h["key"]) in occupied
        assert np.linalg.norm(h["centre"].astype(np.float64) - o.astype(np.float64)) <= r
    assert set(np.unique(hits["status"])) <= {qo.HIT, qo.UNKNOWN}
    assert is_hit.sum() * 100 >= 99 * len(P)
    assert (int(is_hit.sum()), len(P)) == (RASTER_HITS, RASTER_RAYS)


# ---- (d) every status and boundary, by hand.  Cells are named by their index (key - 32768); planted_scene() says where
# the leaves are.  name -> (status, steps, end cell or None)
E = qo.EDGE
BY_HAND = {
    "origin occupied": (qo.HIT, 0, (-50, -50, -50)),
    "origin unknown": (qo.UNKNOWN, 0, (-60, -50, -50)),
    "origin unknown, ignored, then occupied": (qo.HIT, 10, (-50, -50, -50)),
    "origin key invalid": (qo.BAD_ORIGIN, 0, None),           # 8192.0 * 4 = 32768: key 65536
    "origin key invalid below": (qo.BAD_ORIGIN, 0, None),     # -8192.5 * 4 = -32770: key -2
    "origin nan": (qo.BAD_ORIGIN, 0, None),
    "origin inf": (qo.BAD_ORIGIN, 0, None),
    "direction zero": (qo.BAD_DIRECTION, 0, (0, 0, 0)),
    "direction nan": (qo.BAD_DIRECTION, 0, (0, 0, 0)),
    "direction inf": (qo.BAD_DIRECTION, 0, (0, 0, 0)),        # inf / inf
    "direction underflows": (qo.BAD_DIRECTION, 0, (0, 0, 0)),  # 1e-60 is 0 in float: n == 0
    "direction overflows": (qo.BAD_DIRECTION, 0, (0, 0, 0)),  # n == inf: every component divides to 0
    "direction tiny but normal": (qo.UNKNOWN, 1, (1, 0, 0)),  # 1e-15 normalises to (1, 0, 0)
    "tie xy +": (qo.HIT, 1, (20, 21, 20)),                    # tMax0 == tMax1 < tMax2: y, the later axis
    "tie xy -": (qo.HIT, 1, (20, 19, 20)),
    "tie xyz +": (qo.HIT, 1, (40, 40, 41)),                   # all equal: z
    "tie xyz -": (qo.HIT, 1, (40, 40, 39)),
    "diagonal through unknown": (qo.HIT, 6, (63, 63, 60)),    # y, x, y, x, y, x
    "threshold of the map": (qo.HIT, 5, (105, 0, 0)),         # (103, 0, 0) is one float below logodds(0.7)
    "threshold of the map as NaN": (qo.HIT, 5, (105, 0, 0)),
    "threshold of the call": (qo.HIT, 5, (100, 5, 0)),        # (100, 3, 0) is one float below 0.5
    "threshold above every leaf": (qo.OUT_OF_RANGE, 13, (100, 13, 0)),  # 12 cells are 3.0 m: equality goes on
    "threshold -inf: the free leaf is occupied": (qo.HIT, 0, (0, 0, 0)),
    "range equal goes on": (qo.OUT_OF_RANGE, 5, (0, 0, 5)),   # cell 4 is at 1.0 exactly
    "range one ulp less stops": (qo.OUT_OF_RANGE, 4, (0, 0, 4)),
    "range equal at the hit": (qo.HIT, 10, (0, 0, 10)),
    "range one ulp less at the hit": (qo.OUT_OF_RANGE, 10, (0, 0, 10)),  # the range is looked at before the cell
    "range zero": (qo.HIT, 10, (0, 0, 10)),
    "range negative": (qo.HIT, 10, (0, 0, 10)),
    "range inf": (qo.HIT, 10, (0, 0, 10)),
}
for _a in range(3):
    for _s in (1, -1):
        _c = [0, 0, 0]
        _c[_a] = 10 * _s
        BY_HAND["axis %d %+d" % (_a, _s)] = (qo.HIT, 10, tuple(_c))   # through 4 unknown cells, a free leaf, 4 unknown cells
        _c[_a] = _s
        BY_HAND["axis %d %+d, unknown stops" % (_a, _s)] = (qo.UNKNOWN, 1, tuple(_c))
        _c = [7, 7, 7]
        _c[_a] = E if _s > 0 else -E - 1
        BY_HAND["off the edge axis %d %+d" % (_a, _s)] = (qo.OUT_OF_BOUNDS, 3, tuple(_c))
        BY_HAND["off the edge at once axis %d %+d" % (_a, _s)] = (qo.OUT_OF_BOUNDS, 0, tuple(_c))


def test_every_status_and_boundary_by_hand():
    scene = qo.planted_scene()
    q = qo.oracle_of(scene)
    cells = {cell_of(l): l for l in scene["leaves"]}
    rays = qo.planted_rays()
    assert {r[0] for r in rays} == set(BY_HAND)
    seen = set()
    for name, o, d, ign, mr, thr in rays:
        O, D = qo.rays_arrays([(name, o, d)])
        h = q.cast_rays(O, D, ign, mr, thr)[0]
        status, steps, cell = BY_HAND[name]
        assert (h["status"], h["steps"]) == (status, steps), (name, h)
        seen.add(status)
        assert h["zero0"] == 0 and h["zero1"] == 0
        if cell is None:
            assert not h["key"].any() and not h["centre"].any()
        else:
            assert cell_of(h) == cell, (name, h)
            assert [float(c) for c in h["centre"]] == [(k + 0.5) * qo.PLANTED_RES for k in cell]  # exact in float
        if status == qo.HIT:
            assert h["log_odds"] == cells[cell]["log_odds"] and tuple(h["rgb"]) == tuple(cells[cell]["rgb"])
        else:
            assert h["log_odds"] == 0 and not h["rgb"].any()
    assert seen == {qo.HIT, qo.UNKNOWN, qo.OUT_OF_RANGE, qo.OUT_OF_BOUNDS, qo.BAD_ORIGIN, qo.BAD_DIRECTION}


def test_the_view_is_the_ray_cast_of_its_pixels_and_returns_to_the_camera_frame():
    """A pose without rotation, one occupied wall: pixel (v, u) sees the wall cell its ray meets, at the cell's centre
    relative to the camera; a pixel that looks past the wall is a NaN row with word 0."""
    res = 0.25
    cells = {(cx, cy, 8): (2.0, (100 + cx, 200 + cy, 30)) for cx in range(-6, 6) for cy in range(-6, 6)}
    q = qo.QueryOracle(qo.leaves_of(cells), resolution=res)
    T = oo.translation((0.125, 0.125, 0.125))
    cloud, status = q.view_cloud(T, 4.0, 4.0, 4.0, 4.0, 9, 9, ignore_unknown=1, max_range=4.0)
    assert status[4, 4] == qo.HIT  # straight ahead: the cell (0, 0, 8), 8 cells in front
    assert cloud[4, 4, :3].tolist() == [0.0, 0.0, 2.0]
    assert int(cloud.view(np.uint32)[4, 4, 3]) == (100 << 16) | (200 << 8) | 30
    assert status[0, 0] == qo.OUT_OF_RANGE and cloud.view(np.uint32)[0, 0].tolist() == [0x7fc00000] * 3 + [0]
    O = np.tile(np.asarray([[0.125, 0.125, 0.125]], np.float32), (81, 1))
    D = np.array([[(u - 4.0) / 4.0, (v - 4.0) / 4.0, 1.0] for v in range(9) for u in range(9)], np.float32)
    hits = q.cast_rays(O, D, 1, 4.0)
    assert (hits["status"] == status.reshape(-1)).all()
    seen = hits["status"] == qo.HIT
    assert 4 < seen.sum() < 81
    assert (cloud.reshape(-1, 4)[seen, :3] == hits["centre"][seen] - O[seen]).all()


def test_the_default_threshold_and_where_it_is_checked():
    assert qo.QueryOracle([], occupancy_threshold=0.5).occupied_log_odds() == 0.0
    assert qo.QueryOracle([], occupancy_threshold=0.7).occupied_log_odds() == F(math.log(0.7 / (1.0 - 0.7)))


def test_the_home_slot_of_the_wrap_scene():
    scene, ks = qo.wrap_scene()
    assert all(qo.home_slot(k, 16) in (14, 15) for k in ks) and len(set(ks)) == 9
    assert 4 * len(scene["leaves"]) <= 3 * scene["capacity"]
