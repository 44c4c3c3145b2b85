"""-m gpu: map assembly (include/rgbdfe.h, "map assembly"; csrc/map_assembly.hip) through the C ABI against the restatement
of transformAndAppendPointCloud in tests/map_assembly_oracle.py: the points, their number and the nodes' first rows.

The clouds come from upload_node_cloud(..., return_cloud=True), whose output tests/test_gpu_emm.py pins bit for bit; their
sizes (1, 63, 64, 65, 257, 1025, 1024, 4800, 768 points) sit either side of a wave, a workgroup and the kernels' tile."""
import ctypes as C

import numpy as np
import pytest

import map_assembly_oracle as mo

pytestmark = pytest.mark.gpu

DEPTHS = (2.5, np.inf, -1.0, np.nan, 0.0)
SHAPES = [((1, 1), 1), ((7, 9), 1), ((8, 8), 1), ((5, 13), 1), ((1, 257), 1), ((25, 41), 1), ((32, 32), 1), ((60, 80), 1),
          ((48, 64), 2)]
UNKNOWN_NODE, CAPACITY = -4, -5


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    yield f
    f.close()


def upload(fe, node_id, depth, cloud_skip=1, min_depth=0.4, seed=0, cx=None, cy=None):
    rows, cols = depth.shape
    rgb = np.random.default_rng(1000 + seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    cx = float(cols // 2) if cx is None else cx
    cy = float(rows // 2) if cy is None else cy
    return fe.upload_node_cloud(node_id, depth, 40.0, 40.0, cx, cy, rgb=rgb, encoding_bgr=False, depth_scaling=1.0,
                                min_depth=min_depth, cloud_skip=cloud_skip, return_cloud=True)


def random_transforms(rng, n):
    Ts = []
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = q.astype(np.float32)
        T[:3, 3] = rng.uniform(-3, 3, 3).astype(np.float32)
        Ts.append(T)
    return Ts


@pytest.fixture(scope="module")
def scene(fe):
    """Nodes 0..8: the shapes above (depth uniform in [0.3, 5], 10 % NaN, one +inf pixel, min_depth 0.4: NaN z beside finite
    x, y); node 9: one finite point.  Transforms: random rotations with translations, node 1 the identity, node 2 with a NaN."""
    rng = np.random.default_rng(31)
    clouds = []
    for k, ((rows, cols), s) in enumerate(SHAPES):
        d = rng.uniform(0.3, 5.0, (rows, cols)).astype(np.float32)
        d[rng.random((rows, cols)) < 0.1] = np.nan
        d[rng.integers(rows), rng.integers(cols)] = np.inf
        clouds.append(upload(fe, k, d, cloud_skip=s, seed=k))
    clouds.append(upload(fe, 9, np.full((1, 1), 1.5, np.float32), seed=9, cx=3.0, cy=-2.0))
    assert [c.shape[0] * c.shape[1] for c in clouds] == [1, 63, 64, 65, 257, 1025, 1024, 4800, 768, 1]
    ids = np.arange(len(clouds), dtype=np.int32)
    Ts = random_transforms(rng, len(clouds))
    Ts[1] = np.eye(4, dtype=np.float32)
    Ts[2][2, 0] = np.nan
    yield ids, clouds, Ts
    for k in ids:
        fe.release_node_cloud(int(k))


def raw(fe, ids, Ts, maximum_depth, preserve_raster, capacity):
    """The C call as it is: (status, n_out, out rows, node_offsets)."""
    ids = np.ascontiguousarray(ids, np.int32)
    T = np.ascontiguousarray(np.asarray(Ts, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
    out = np.zeros((max(capacity, 1), 4), np.float32)
    off = np.full(len(ids) + 1, -1, np.int64)
    n = C.c_int64(-1)
    st = fe._L.rgbdfe_assemble_map(fe._ctx, len(ids), ids.ctypes.data, T.ctypes.data, float(maximum_depth), int(preserve_raster),
                                   out.ctypes.data, capacity, C.byref(n), off.ctypes.data)
    return st, n.value, out, off


@pytest.mark.parametrize("preserve_raster", [False, True])
@pytest.mark.parametrize("maximum_depth", DEPTHS)
def test_assembled_map_equals_the_oracle(fe, scene, maximum_depth, preserve_raster):
    ids, clouds, Ts = scene
    want, want_off = mo.assemble(clouds, Ts, maximum_depth, preserve_raster)
    got, off = fe.assemble_map(ids, Ts, maximum_depth, preserve_raster, return_offsets=True)
    print("maximum_depth %s raster %s: %d of %d points" % (maximum_depth, preserve_raster, len(got), sum(c.size // 4 for c in clouds)))
    assert len(got) == len(want) == off[-1]
    assert np.array_equal(off, want_off)
    assert mo.mismatch(got, want) is None, mo.mismatch(got, want)
    if preserve_raster:
        clipped = mo.clipped_rows(clouds, maximum_depth)
        assert np.all(got.view(np.uint32)[clipped, :3] == mo.QNAN_BITS)
    elif maximum_depth == 2.5:  # every larger node has kept, clipped and skipped points
        kept_inf = np.diff(mo.assemble(clouds, Ts, np.inf)[1])
        for k in range(1, 9):
            assert 0 < np.diff(off)[k] < kept_inf[k] < clouds[k].size // 4, k


def test_a_node_without_kept_points_between_two_that_keep_some(fe):
    """maximum_depth = 0 keeps the points in the origin only: pixels of depth 0 under min_depth = 0."""
    rng = np.random.default_rng(5)
    clouds = []
    for k, zeros in enumerate((3, 0, 2)):
        d = rng.uniform(0.3, 5.0, (33, 37)).astype(np.float32)
        d.reshape(-1)[rng.choice(d.size, zeros, replace=False)] = 0.0
        clouds.append(upload(fe, 20 + k, d, min_depth=0.0, seed=20 + k))
    Ts = random_transforms(rng, 3)
    try:
        for raster in (False, True):
            got, off = fe.assemble_map([20, 21, 22], Ts, 0.0, raster, return_offsets=True)
            want, want_off = mo.assemble(clouds, Ts, 0.0, raster)
            assert np.array_equal(off, want_off) and mo.mismatch(got, want) is None
        got, off = fe.assemble_map([20, 21, 22], Ts, 0.0, False, return_offsets=True)
        assert off.tolist() == [0, 3, 3, 5]
        assert np.array_equal(got[:3, :3], np.tile(Ts[0][:3, 3], (3, 1)))
        only = fe.assemble_map([21], Ts[1:2], 0.0, False, return_offsets=True)  # nothing at all is kept
        assert only[0].shape == (0, 4) and only[1].tolist() == [0, 0]
    finally:
        for k in (20, 21, 22):
            fe.release_node_cloud(k)


def test_an_id_listed_twice_and_an_empty_list(fe, scene):
    ids, clouds, Ts = scene
    lst = [5, 7, 5, 0, 9, 9]
    T = [Ts[5], Ts[7], Ts[3], Ts[0], Ts[9], Ts[4]]
    for raster in (False, True):
        got, off = fe.assemble_map(lst, T, 2.5, raster, return_offsets=True)
        want, want_off = mo.assemble([clouds[i] for i in lst], T, 2.5, raster)
        assert np.array_equal(off, want_off) and mo.mismatch(got, want) is None
    got, off = fe.assemble_map([], np.zeros((0, 4, 4), np.float32), 2.5, False, return_offsets=True)
    assert got.shape == (0, 4) and off.tolist() == [0]
    st, n, _, off = raw(fe, [], np.zeros((0, 4, 4), np.float32), 2.5, 0, 0)
    assert (st, n, off.tolist()) == (0, 0, [0])


def test_refusals(fe, scene):
    from rgbdslam_v2_amd._lib import RgbdfeError
    ids, clouds, Ts = scene
    st, n, _, _ = raw(fe, [0, 77, 1], Ts[:3], 2.5, 0, 100)
    assert st == UNKNOWN_NODE
    with pytest.raises(RgbdfeError):
        fe.assemble_map([0, 77, 1], Ts[:3], 2.5)
    with pytest.raises(RgbdfeError):
        fe.node_cloud(77)
    L = fe._L
    one, T = np.zeros(1, np.int32), np.eye(4, dtype=np.float32)
    n64 = C.c_int64(0)
    buf = np.zeros(4, np.float32)
    assert L.rgbdfe_assemble_map(fe._ctx, -1, one.ctypes.data, T.ctypes.data, 1.0, 0, buf.ctypes.data, 1, C.byref(n64), None) == -1
    assert L.rgbdfe_assemble_map(fe._ctx, 1, None, T.ctypes.data, 1.0, 0, buf.ctypes.data, 1, C.byref(n64), None) == -1
    assert L.rgbdfe_assemble_map(fe._ctx, 1, one.ctypes.data, None, 1.0, 0, buf.ctypes.data, 1, C.byref(n64), None) == -1
    assert L.rgbdfe_assemble_map(fe._ctx, 1, one.ctypes.data, T.ctypes.data, 1.0, 0, None, 1, C.byref(n64), None) == -1
    assert L.rgbdfe_assemble_map(fe._ctx, 1, one.ctypes.data, T.ctypes.data, 1.0, 0, buf.ctypes.data, 1, None, None) == -1


@pytest.mark.parametrize("preserve_raster", [False, True])
def test_capacity_one_short_then_the_needed_size(fe, scene, preserve_raster):
    ids, clouds, Ts = scene
    want, want_off = mo.assemble(clouds, Ts, 2.5, preserve_raster)
    st, n, _, _ = raw(fe, ids, Ts, 2.5, preserve_raster, len(want) - 1)
    assert (st, n) == (CAPACITY, len(want))
    st, n2, out, off = raw(fe, ids, Ts, 2.5, preserve_raster, n)
    assert (st, n2) == (0, n) and np.array_equal(off, want_off)
    assert mo.mismatch(out[:n], want) is None
    # the sum of the clouds' sizes always suffices
    total = sum(c.size // 4 for c in clouds)
    st, n3, out, _ = raw(fe, ids, Ts, 2.5, preserve_raster, total)
    assert (st, n3) == (0, n) and mo.mismatch(out[:n], want) is None


def test_the_range_boundary_is_strict(fe):
    """Centre pixels (x = y = 0) of depth exactly 2.5f and the float behind it at maximum_depth = 2.5: 6.25 > 6.25 is false."""
    nxt = np.nextafter(np.float32(2.5), np.float32(np.inf))
    clouds = []
    for k, centre in enumerate((np.float32(2.5), nxt)):
        d = np.full((3, 3), 1.0, np.float32)
        d[1, 1] = centre
        clouds.append(upload(fe, 30 + k, d, seed=30 + k, cx=1.0, cy=1.0))
        assert clouds[k][1, 1, :3].tolist() == [0.0, 0.0, float(centre)]
    T = [np.eye(4, dtype=np.float32)] * 2
    try:
        got, off = fe.assemble_map([30, 31], T, 2.5, False, return_offsets=True)
        want, want_off = mo.assemble(clouds, T, 2.5, False)
        assert np.array_equal(off, want_off) and mo.mismatch(got, want) is None
        assert off.tolist() == [0, 9, 17]
        assert got[4, :3].tolist() == [0.0, 0.0, 2.5] and not (got[9:, 2] == nxt).any()
        ras = fe.assemble_map([30, 31], T, 2.5, True)
        assert ras[4, :3].tolist() == [0.0, 0.0, 2.5]
        assert np.all(ras.view(np.uint32)[9 + 4, :3] == mo.QNAN_BITS)
        assert ras.view(np.uint32)[9 + 4, 3] == clouds[1].view(np.uint32)[1, 1, 3]
    finally:
        fe.release_node_cloud(30)
        fe.release_node_cloud(31)


@pytest.mark.parametrize("preserve_raster", [False, True])
def test_assemble_map_device_writes_the_same_bytes(fe, scene, preserve_raster):
    import torch
    ids, clouds, Ts = scene
    host, host_off = fe.assemble_map(ids, Ts, 2.5, preserve_raster, return_offsets=True)
    total = sum(c.size // 4 for c in clouds)
    out = torch.full((total, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()  # the fill runs on torch's stream, the assembly on the context's
    n, off = fe.assemble_map_device(ids, Ts, out, 2.5, preserve_raster, return_offsets=True)
    assert n == len(host) and np.array_equal(off, host_off)
    back = out.cpu().numpy()
    assert back[:n].tobytes() == host.tobytes()
    assert np.all(back[n:] == -7.0)  # nothing behind the assembled cloud is touched
    from rgbdslam_v2_amd._lib import RgbdfeError
    small = torch.zeros((n - 1, 4), dtype=torch.float32, device="cuda:0")
    with pytest.raises(RgbdfeError):
        fe.assemble_map_device(ids, Ts, small, 2.5, preserve_raster)


def test_node_cloud_returns_the_resident_cloud(fe, scene):
    ids, clouds, Ts = scene
    for k in ids:
        got = fe.node_cloud(int(k))
        assert got.shape == clouds[k].shape and got.tobytes() == clouds[k].tobytes()
    rows, cols = C.c_int32(0), C.c_int32(0)
    buf = np.zeros((4799, 4), np.float32)
    assert fe._L.rgbdfe_download_node_cloud(fe._ctx, 7, buf.ctypes.data, 4799, C.byref(rows), C.byref(cols)) == CAPACITY
    assert (rows.value, cols.value) == (60, 80)


def test_node_cloud_of_the_sensor_batch_path():
    """The clouds sensor_detect_describe_batch_nodes keeps = upload_node_cloud on ingest_frame's planes of the same frames."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    from test_gpu_sensor_ingest import K, restart, sensor_frame
    from test_oracle_orb_photos import load_photos
    photos = load_photos()
    a = FrontEnd(device_id=0, max_nodes=4, max_keypoints=1024, max_pairs_per_batch=16)
    try:
        restart(a, "ORB", False)
        vis, dep = [], []
        for k in range(2):
            v, d, enc = sensor_frame(photos, k, "rgb8", "32FC1")
            vis.append(v)
            dep.append(d)
        a.sensor_detect_describe_batch_nodes(vis, dep, *K, node_ids=np.array([0, 1], np.int32), visual_encoding=enc,
                                             cloud_skip=2, cloud_encoding_bgr=False, cloud_min_depth=0.1)
        kept = [a.node_cloud(k) for k in range(2)]
        for k in range(2):
            _, _, dm = a.ingest_frame(vis[k], dep[k], enc, gray=False, mono8=False)
            want = a.upload_node_cloud(2 + k, dm, *K, rgb=vis[k], encoding_bgr=False, min_depth=0.1, cloud_skip=2,
                                       return_cloud=True)
            assert kept[k].shape == want.shape == (240, 320, 4) and kept[k].tobytes() == want.tobytes()
        T = random_transforms(np.random.default_rng(3), 2)
        got = a.assemble_map([1, 0], T, 2.1)
        assert mo.mismatch(got, mo.assemble([kept[1], kept[0]], T, 2.1)[0]) is None and 0 < len(got) < 2 * 240 * 320
    finally:
        a.close()


def test_two_identical_calls_give_identical_bytes(fe, scene):
    ids, clouds, Ts = scene
    for raster in (False, True):
        a = fe.assemble_map(ids, Ts, 2.5, raster, return_offsets=True)
        b = fe.assemble_map(ids, Ts, 2.5, raster, return_offsets=True)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


# ---- the later trips of map_scan_kernel (csrc/map_assembly.hip): 1024 tile counts a trip, then 1024 nodes' first rows a stride
MAP_TILE = 1024  # kMapTile; a tile never crosses a node


@pytest.fixture(scope="module")
def small_clouds(fe):
    """Nodes 40, 41, 42 of 1, 63 and 1025 points: one full tile is never reached, so the tiles' counts differ."""
    rng = np.random.default_rng(57)
    clouds = [upload(fe, 40, np.full((1, 1), 1.5, np.float32), seed=40)]
    for k, (rows, cols) in ((41, (7, 9)), (42, (25, 41))):
        d = rng.uniform(0.3, 5.0, (rows, cols)).astype(np.float32)
        d[rng.random((rows, cols)) < 0.1] = np.nan
        clouds.append(upload(fe, k, d, seed=k))
    assert [c.size // 4 for c in clouds] == [1, 63, 1025]
    yield clouds
    for k in (40, 41, 42):
        fe.release_node_cloud(k)


@pytest.mark.parametrize("which,n_tiles", [("1100 nodes", 1466), ("exactly 1024 tiles", 1024)])
def test_more_tiles_and_more_nodes_than_one_trip_of_the_scan(fe, small_clouds, which, n_tiles):
    """Compact mode over a list that repeats three resident clouds: more than 1024 tiles and more than 1023 nodes (the
    node_first loop takes 1024 entries a stride, the sentinel included), and once exactly 1024 tiles.  maximum_depth 2.5
    clips a part of every larger cloud."""
    rng = np.random.default_rng(58)
    if which == "1100 nodes":
        pick = np.arange(1100) % 3
    else:
        pick = np.concatenate([np.full(300, 2), np.full(212, 1), np.full(212, 0)])  # 600 + 424 tiles
    pick = rng.permutation(pick)
    clouds = [small_clouds[k] for k in pick]
    Ts = random_transforms(rng, len(pick))
    per_node = np.array([-(-(c.size // 4) // MAP_TILE) for c in clouds])
    first_tile = np.cumsum(per_node) - per_node
    assert per_node.sum() == n_tiles
    want, want_off = mo.assemble(clouds, Ts, 2.5)
    kept = np.diff(want_off)
    if which == "1100 nodes":  # kept points behind tile 1024 and nodes behind entry 1024: both loops go round again
        assert len(pick) + 1 > 1024 and kept[first_tile >= 1024].sum() > 1000 and kept[1024:].sum() > 0
        assert len({int(k) for k in kept[first_tile >= 1024]}) >= 3  # nodes, and so tiles, of different counts
    assert 0 < len(want) < mo.assemble(clouds, Ts, np.inf)[1][-1]  # the clip takes points away
    got, off = fe.assemble_map(40 + pick, Ts, 2.5, False, return_offsets=True)
    assert np.array_equal(off, want_off) and len(got) == off[-1]
    assert mo.mismatch(got, want) is None, mo.mismatch(got, want)
