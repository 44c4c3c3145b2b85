"""-m gpu: the voxel filter (include/rgbdfe.h, "voxel filter"; csrc/voxel_filter.hip) through the C ABI against the vectorised
restatement in tests/voxel_filter_oracle.py.  Every comparison is on bytes: the row count, every float's bits, every rgb word.
tests/test_oracle_voxel_filter.py shows that a byte comparison sees a wrong order inside the cells (the census)."""
import ctypes as C
import warnings

import numpy as np
import pytest

import map_assembly_oracle as mo
import voxel_filter_oracle as vo

pytestmark = pytest.mark.gpu

INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 20000)
LEAVES = (0.05, 0.25, 4.0)


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    yield f
    f.close()


def raw(fe, pts, leaf, capacity):
    """The C call as it is: (status, n_out, flags, out rows)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    out = np.full((max(capacity, 1), 4), -7.0, np.float32)
    n, flags = C.c_int64(-1), C.c_int32(-1)
    st = fe._L.rgbdfe_voxel_filter(fe._ctx, pts.ctypes.data, len(pts), float(leaf), out.ctypes.data, capacity, C.byref(n),
                                   C.byref(flags))
    return st, n.value, flags.value, out


def check(fe, pts, leaf):
    """Filters pts on the device and holds the result against the oracle; returns the oracle's info."""
    want, want_flags, info = vo.voxel_filter(pts, leaf)
    got, flags = fe.voxel_filter(pts, leaf, return_flags=True)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert flags == want_flags
    assert got.tobytes() == want.tobytes(), mo.mismatch(got, want)
    return info


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_either_side_of_a_wave_a_workgroup_and_the_tiles(fe, n, leaf):
    info = check(fe, vo.cloud(n, seed=n), leaf)
    print("n %d leaf %g: %d valid points, %d cells" % (n, leaf, info["n_valid"], len(info.get("count", ()))))


@pytest.mark.parametrize("side,leaf,lo,hi,passes", [(3.0, 0.5, 0, 2**8, 1), (3.0, 0.1, 2**8, 2**16, 2), (3.0, 0.025, 2**16, 2**24, 3),
                                                    (6.0, 0.005, 2**24, 2**31, 4)])
def test_every_number_of_sort_passes(fe, side, leaf, lo, hi, passes):
    pts = vo.cloud(4096, seed=int(side * 10), side=side)
    info = check(fe, pts, leaf)
    d = info["d"]
    assert lo < d[0] * d[1] * d[2] <= hi and lo < info["n_cells"] <= hi, (d, info["div"])  # the range this case is meant for
    assert info["passes"] == passes


def test_five_thousand_points_in_one_cell(fe):
    info = check(fe, vo.cloud(5000, seed=41, centre=(50.0, 50.0, 50.0)), 100.0)
    assert info["count"].tolist() == [info["n_valid"]] and 4000 < info["n_valid"] < 5000


def test_two_cells_whose_members_alternate(fe):
    pts = vo.cloud(9001, seed=42, side=0.5, centre=(0.5, 0.5, 0.5), nan_share=0, infs=False)
    pts[1::2, 0] += np.float32(10.0)
    info = check(fe, pts, 1.0)
    assert info["count"].tolist() == [4501, 4500]


def test_every_point_in_a_cell_of_its_own(fe):
    info = check(fe, vo.cloud(3000, seed=43, nan_share=0, infs=False), 0.005)
    assert info["count"].max() == 1 and len(info["count"]) == 3000


def test_geometry(fe):
    info = check(fe, vo.cloud(3000, seed=44, centre=(-37.3, 12.1, 100.7)), 0.25)
    assert info["min_b"][0] < 0 < info["min_b"][1]
    flat = vo.cloud(3000, seed=45)
    flat[:, 2] = np.float32(0.75)
    info = check(fe, flat, 0.25)
    assert info["d"][2] == 1 and info["div"][2] == 1
    same = np.tile(vo.cloud(1, seed=46, nan_share=0, infs=False), (1500, 1))
    info = check(fe, same, 0.25)
    assert info["count"].tolist() == [1500]
    info = check(fe, np.concatenate([vo.cloud(1100, seed=47)] * 3), 0.25)
    assert np.all(info["count"] % 3 == 0)


def test_no_valid_point_and_no_point(fe):
    bad = vo.cloud(1500, seed=48)
    bad[:, 1] = np.nan
    bad[::7, 1] = np.inf
    st, n, flags, out = raw(fe, bad, 0.25, 1500)
    assert (st, n, flags) == (0, 0, 0) and np.all(out == -7.0)
    assert check(fe, bad, 0.25)["n_valid"] == 0
    st, n, flags, _ = raw(fe, np.zeros((0, 4), np.float32), 0.25, 0)
    assert (st, n, flags) == (0, 0, 0)
    n64 = C.c_int64(-1)
    assert fe._L.rgbdfe_voxel_filter(fe._ctx, None, 0, 0.25, None, 0, C.byref(n64), None) == 0 and n64.value == 0
    assert fe.voxel_filter(np.zeros((0, 4), np.float32), 0.25).shape == (0, 4)


def test_a_leaf_too_small_returns_the_input(fe):
    pts = vo.cloud(4096, seed=60, side=6.0)
    want, want_flags, _ = vo.voxel_filter(pts, 0.004)
    assert want_flags == vo.LEAF_TOO_SMALL
    got, flags = fe.voxel_filter(pts, 0.004, return_flags=True)
    assert flags == vo.LEAF_TOO_SMALL and got.tobytes() == pts.tobytes() == want.tobytes()
    st, n, flags, _ = raw(fe, pts, 0.004, len(pts) - 1)
    assert (st, n, flags) == (CAPACITY, len(pts), vo.LEAF_TOO_SMALL)
    huge = pts.copy()
    huge[5, 0] = np.float32(3e30)  # a float product >= 2^31
    got, flags = fe.voxel_filter(huge, 1.0, return_flags=True)
    assert flags == vo.LEAF_TOO_SMALL and got.tobytes() == huge.tobytes()


def test_capacity_one_short_then_the_needed_size(fe):
    pts = vo.cloud(4097, seed=61)
    want, _, _ = vo.voxel_filter(pts, 0.25)
    st, n, flags, out = raw(fe, pts, 0.25, len(want) - 1)
    assert (st, n, flags) == (CAPACITY, len(want), 0)
    st, n, flags, out = raw(fe, pts, 0.25, len(want))
    assert (st, n, flags) == (0, len(want), 0) and out.tobytes() == want.tobytes()
    st, n, flags, out = raw(fe, pts, 0.25, len(pts))  # n_in rows always suffice
    assert (st, n) == (0, len(want)) and out[:n].tobytes() == want.tobytes() and np.all(out[n:] == -7.0)


@pytest.mark.parametrize("leaf", [0.0, -1.0, float("nan"), float("inf"), 1e-46])
def test_refused_leaves(fe, leaf):
    from rgbdslam_v2_amd._lib import RgbdfeError
    pts = vo.cloud(100, seed=62)
    assert raw(fe, pts, leaf, 100)[0] == INVALID_ARG
    assert raw(fe, pts[:0], leaf, 0)[0] == INVALID_ARG
    with pytest.raises(RgbdfeError):
        fe.voxel_filter(pts, leaf)
    n64 = C.c_int64(0)
    assert fe._L.rgbdfe_reduce_node_cloud(fe._ctx, 0, leaf, C.byref(n64), None) == INVALID_ARG


def test_refused_arguments(fe):
    L = fe._L
    pts, out, n64 = vo.cloud(8, seed=63), np.zeros((8, 4), np.float32), C.c_int64(0)
    assert L.rgbdfe_voxel_filter(fe._ctx, None, 8, 0.25, out.ctypes.data, 8, C.byref(n64), None) == INVALID_ARG
    assert L.rgbdfe_voxel_filter(fe._ctx, pts.ctypes.data, -1, 0.25, out.ctypes.data, 8, C.byref(n64), None) == INVALID_ARG
    assert L.rgbdfe_voxel_filter(fe._ctx, pts.ctypes.data, 8, 0.25, None, 8, C.byref(n64), None) == INVALID_ARG
    assert L.rgbdfe_voxel_filter(fe._ctx, pts.ctypes.data, 8, 0.25, out.ctypes.data, 8, None, None) == INVALID_ARG
    assert L.rgbdfe_voxel_filter(fe._ctx, pts.ctypes.data, 2**31, 0.25, out.ctypes.data, 8, C.byref(n64), None) == CAPACITY


def upload(fe, node_id, rows, cols, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 3.0, (rows, cols)).astype(np.float32)
    d[rng.random((rows, cols)) < 0.1] = np.nan
    rgb = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    return fe.upload_node_cloud(node_id, d, 40.0, 40.0, cols / 2.0, rows / 2.0, rgb=rgb, min_depth=0.4, cloud_skip=1,
                                return_cloud=True)


SHAPES = ((7, 9), (25, 41), (60, 80), (24, 32))  # 63, 1025, 4800, 768 points


@pytest.fixture()
def nodes(fe):
    clouds = [upload(fe, k, r, c, 70 + k) for k, (r, c) in enumerate(SHAPES)]
    assert [c.size // 4 for c in clouds] == [63, 1025, 4800, 768]
    rng = np.random.default_rng(7)
    Ts = []
    for k in range(len(clouds)):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = q.astype(np.float32)
        T[:3, 3] = rng.uniform(-1, 1, 3).astype(np.float32)
        Ts.append(T)
    yield list(range(len(clouds))), clouds, Ts
    for k in range(len(clouds)):
        fe.release_node_cloud(k)


def test_the_device_entry_writes_the_host_entrys_bytes(fe):
    import torch
    from rgbdslam_v2_amd._lib import RgbdfeError
    pts = vo.cloud(20000, seed=64)
    host = fe.voxel_filter(pts, 0.1)
    d_in = torch.from_numpy(pts).to("cuda:0")
    d_out = torch.full((len(pts), 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()  # the copies run on torch's stream, the filter on the context's
    n, flags = fe.voxel_filter_device(d_in, 0.1, d_out, return_flags=True)
    back = d_out.cpu().numpy()
    assert (n, flags) == (len(host), 0) and back[:n].tobytes() == host.tobytes()
    assert np.all(back[n:] == -7.0)  # nothing behind the filtered cloud is touched
    assert d_in.cpu().numpy().tobytes() == pts.tobytes()
    with pytest.raises(RgbdfeError):
        fe.voxel_filter_device(d_in, 0.1, d_out[:n - 1])
    with pytest.raises(RgbdfeError):  # out inside points
        fe.voxel_filter_device(d_in, 0.1, d_in[100:200])
    with pytest.raises(ValueError):
        fe.voxel_filter_device(d_in[:, :3], 0.1, d_out)


def test_assemble_then_filter_on_the_device(fe, nodes):
    import torch
    ids, clouds, Ts = nodes
    want_map, _ = mo.assemble(clouds, Ts, 2.5)
    want, _, info = vo.voxel_filter(want_map, 0.1)
    total = sum(c.size // 4 for c in clouds)
    d_map = torch.zeros((total, 4), dtype=torch.float32, device="cuda:0")
    d_out = torch.zeros((total, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    n_map = fe.assemble_map_device(ids, Ts, d_map, 2.5)
    assert n_map == len(want_map)
    n = fe.voxel_filter_device(d_map[:n_map], 0.1, d_out)
    assert n == len(want) and 0 < n < n_map and info["count"].max() > 1
    assert d_out[:n].cpu().numpy().tobytes() == want.tobytes()


def test_reduce_node_cloud(fe, nodes):
    from rgbdslam_v2_amd._lib import RgbdfeError
    ids, clouds, Ts = nodes
    structured = fe.observation_likelihood([1], [1], [np.eye(4, dtype=np.float32)])
    assert structured[0, 3] > 1  # the measurement model really runs on the structured cloud
    leaf = 0.2
    reduced = []
    for k in ids:
        before = fe.node_cloud(k)
        assert before.tobytes() == clouds[k].tobytes()
        want, _, _ = vo.voxel_filter(before, leaf)
        assert fe.reduce_node_cloud(k, leaf) == (len(want), 0)
        after = fe.node_cloud(k)
        assert after.shape == (1, len(want), 4) and after.tobytes() == want.tobytes()
        assert 0 < len(want) < before.size // 4
        reduced.append(after)
    # an unstructured cloud: inliers = all = 1 (misc.cpp:835-843), whatever the other cloud's size
    got = fe.observation_likelihood([1, 2, 0], [1, 3, 2], [np.eye(4, dtype=np.float32)] * 3)
    assert got.tolist() == [[1, 0, 0, 1]] * 3
    got_map, off = fe.assemble_map(ids, Ts, 2.5, return_offsets=True)
    want_map, want_off = mo.assemble(reduced, Ts, 2.5)
    assert np.array_equal(off, want_off) and mo.mismatch(got_map, want_map) is None and len(got_map) > 0
    # twice = the oracle twice (another leaf, so that the second pass merges cells)
    want2, _, _ = vo.voxel_filter(reduced[2], 0.5)
    assert fe.reduce_node_cloud(2, 0.5) == (len(want2), 0)
    again = fe.node_cloud(2)
    assert again.shape == (1, len(want2), 4) and again.tobytes() == want2.tobytes() and len(want2) < reduced[2].shape[1]
    # a leaf too small leaves the cloud as it is
    n_out, flags = fe.reduce_node_cloud(2, 1e-12)
    assert (n_out, flags) == (len(want2), vo.LEAF_TOO_SMALL) and fe.node_cloud(2).tobytes() == want2.tobytes()
    # the mirror of the reference: vfs <= 0 warns and does nothing
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert fe.reduce_node_cloud(2, 0.0) is None and fe.reduce_node_cloud(2, -1.0) is None
    assert len(w) == 2 and fe.node_cloud(2).tobytes() == want2.tobytes()
    # release works, and the node is unknown afterwards
    fe.release_node_cloud(3)
    n64 = C.c_int64(0)
    assert fe._L.rgbdfe_reduce_node_cloud(fe._ctx, 3, leaf, C.byref(n64), None) == UNKNOWN_NODE
    assert fe._L.rgbdfe_reduce_node_cloud(fe._ctx, 77, leaf, C.byref(n64), None) == UNKNOWN_NODE
    with pytest.raises(RgbdfeError):
        fe.reduce_node_cloud(77, leaf)
    upload(fe, 3, *SHAPES[3], seed=73)  # the fixture releases it


def test_a_reduced_cloud_of_no_points(fe):
    d = np.full((6, 8), np.nan, np.float32)
    fe.upload_node_cloud(9, d, 40.0, 40.0, 4.0, 3.0, min_depth=0.4, cloud_skip=1)
    try:
        assert fe.reduce_node_cloud(9, 0.1) == (0, 0)
        assert fe.node_cloud(9).shape == (1, 0, 4)
        got, off = fe.assemble_map([9], [np.eye(4, dtype=np.float32)], return_offsets=True)
        assert got.shape == (0, 4) and off.tolist() == [0, 0]
        assert fe.reduce_node_cloud(9, 0.1) == (0, 0)
        assert fe.observation_likelihood([9], [9], [np.eye(4, dtype=np.float32)]).tolist() == [[1, 0, 0, 1]]
    finally:
        fe.release_node_cloud(9)


def test_two_identical_calls_give_identical_bytes(fe):
    pts = vo.cloud(20000, seed=65)
    a = fe.voxel_filter(pts, 0.1, return_flags=True)
    b = fe.voxel_filter(pts, 0.1, return_flags=True)
    assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes() and len(a[0]) > 0


# ---- the later trips of block_scan_1024 (csrc/voxel_filter.hip): one workgroup covers 1024 tiles a trip and carries `base`
TILE, SORT_TILE, TRIP = 1024, 4096, 1024  # kVoxTile, kVoxSortTile, the tiles of one trip


def tiles(n, tile=TILE):
    return -(-n // tile)


def trips(n_tiles):
    return -(-n_tiles // TRIP)


def cells_starting_behind(info, at):
    """The occupied cells whose first sorted pair stands at position `at` or behind it."""
    start = np.cumsum(info["count"]) - info["count"]
    return int((start >= at).sum())


@pytest.mark.parametrize("n,side,leaf,point_trips,head_trips,passes", [
    (1048576, 3.0, 0.05, 1, 1, 3), (1048577, 3.0, 0.05, 2, 1, 3), (2097153, 3.0, 0.05, 3, 2, 3), (1048577, 6.0, 0.02, 2, 1, 4),
    (2097153, 6.0, 0.02, 3, 2, 4)])
def test_more_point_and_cell_tiles_than_one_trip_of_the_scan(fe, n, side, leaf, point_trips, head_trips, passes):
    """vox_finish_kernel scans ceil(n / 1024) tile counts, vox_head_scan_kernel ceil(n_valid / 1024): 1024 tiles are one full
    trip of block_scan_1024, 1025 a second trip of one tile, 2049 a third.  The last row is made valid, so that the one
    point of tile 1024 (2048) takes its rank from the carried base."""
    pts = vo.cloud(n, seed=n % 1000 + int(side), side=side)
    pts[n - 1, :3] = np.float32(0.125) * np.float32(side)
    assert trips(tiles(n)) == point_trips
    valid = np.isfinite(pts[:, :3]).all(axis=1)
    for trip in range(1, point_trips):  # every later trip has valid points: ranks that need the carried base
        assert valid[trip * TRIP * TILE:(trip + 1) * TRIP * TILE].any()
    info = check(fe, pts, leaf)
    assert info["passes"] == passes
    assert trips(tiles(info["n_valid"])) == head_trips
    if head_trips > 1:  # cells that start in the second trip of the head scan
        assert info["n_valid"] > TRIP * TILE and cells_starting_behind(info, TRIP * TILE) > 1000
    print("n %d leaf %g: %d tiles of points, %d valid points in %d tiles, %d cells" % (n, leaf, tiles(n), info["n_valid"],
                                                                                     tiles(info["n_valid"]), len(info["count"])))


def test_a_second_trip_from_base_zero_and_one_that_adds_nothing(fe):
    """1 049 601 points = 1026 tiles.  First no valid point in the first 1024 tiles: the second trip starts from base 0.
    Then valid points in the first 1024 tiles only: the second trip adds nothing to a base of 1 048 576."""
    n, first = 1049601, TRIP * TILE
    assert tiles(n) == 1026
    late = vo.cloud(n, seed=71)
    late[:first, 2] = np.nan
    info = check(fe, late, 0.05)
    assert 0 < info["n_valid"] <= n - first and np.isfinite(late[first:, :3]).all(axis=1).sum() == info["n_valid"]
    early = vo.cloud(n, seed=72, nan_share=0, infs=False)
    early[first:, 2] = np.nan
    info = check(fe, early, 0.05)
    assert info["n_valid"] == first and tiles(info["n_valid"]) == TRIP  # the head scan: exactly one full trip


def test_more_sort_tiles_than_one_trip_of_the_digit_scan(fe):
    """4 198 401 valid points = 1026 sort tiles of 4096 pairs: vox_digit_scan_kernel makes a second trip over every digit's
    row in each of the three passes, and the point and head scans make five.  Through both entry points."""
    import torch
    n = 4198401
    pts = vo.cloud(n, seed=73, side=6.0, nan_share=0, infs=False)
    want, want_flags, info = vo.voxel_filter(pts, 0.05)
    assert info["n_valid"] > 4194304 and tiles(info["n_valid"], SORT_TILE) == 1026 and trips(1026) == 2
    assert info["passes"] == 3 and want_flags == 0 and cells_starting_behind(info, 4 * TRIP * TILE) > 0
    d_in = torch.from_numpy(pts).to("cuda:0")
    d_out = torch.full((len(want) + 3, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()  # the copies run on torch's stream, the filter on the context's
    n_out, flags = fe.voxel_filter_device(d_in, 0.05, d_out, return_flags=True)
    back = d_out.cpu().numpy()
    assert (n_out, flags) == (len(want), 0) and np.all(back[n_out:] == -7.0)
    assert back[:n_out].tobytes() == want.tobytes(), mo.mismatch(back[:n_out], want)
    del d_in, d_out
    got, flags = fe.voxel_filter(pts, 0.05, return_flags=True)
    assert flags == 0 and got.shape == want.shape and got.tobytes() == want.tobytes(), mo.mismatch(got, want)
