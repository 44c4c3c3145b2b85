"""-m gpu: map files (include/rgbdfe.h, "map files"; csrc/api_map_files.hip, csrc/map_files.hip) through the C ABI on the scene
of tests/test_gpu_map_assembly.py -- clouds of 1, 63, 64, 65, 257, 1025, 1024, 4800, 768 and 1 points with 10 % NaN, one +inf,
a NaN transform and an identity transform.  The expected file is built here: the header of tests/cloud_file_oracle.py and the
rows of tests/map_assembly_oracle.py, packed by the oracle for PLY."""
import ctypes as C
import os

import numpy as np
import pytest

import cloud_file_oracle as co
import map_assembly_oracle as mo
from test_gpu_map_assembly import SHAPES, random_transforms, upload

pytestmark = pytest.mark.gpu

INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
CHUNKS = (1, 64, 1000, 5000, 0)
LARGEST = 4800


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    yield f
    f.close()


@pytest.fixture(scope="module")
def scene(fe):
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


@pytest.fixture(scope="module")
def expected(scene):
    """(maximum_depth, raster) -> the oracle's rows, computed once."""
    ids, clouds, Ts = scene
    return {(md, r): mo.assemble(clouds, Ts, md, r)[0] for md in (2.5, np.inf, -1.0) for r in (False, True)}


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("preserve_raster", [False, True])
@pytest.mark.parametrize("maximum_depth", [2.5, np.inf, -1.0])
@pytest.mark.parametrize("fmt", ["pcd", "ply"])
def test_saved_map_equals_header_and_oracle_rows(fe, scene, expected, tmp_path, fmt, maximum_depth, preserve_raster):
    from rgbdslam_v2_amd.frontend import read_cloud_file
    ids, clouds, Ts = scene
    want_rows = expected[(maximum_depth, preserve_raster)]
    want = co.file_bytes(want_rows, fmt)
    files = []
    for chunk in CHUNKS:
        path = str(tmp_path / ("map_%d.%s" % (chunk, fmt)))
        st = fe.save_map(path, ids, Ts, maximum_depth, preserve_raster, chunk_points=chunk)
        data = read_file(path)
        files.append(data)
        print("%s md %s raster %s chunk %d: %d points, %d groups, %d + %d scratch bytes, tables %d" %
              (fmt, maximum_depth, preserve_raster, chunk, st["points"], st["groups"], st["device_scratch_bytes"], st["pinned_bytes"],
               st["table_bytes"]))
        assert (st["path"], st["format"], st["points"], st["bytes_written"]) == (path, fmt, len(want_rows), len(data))
        bound = 2 * 16 * max(chunk if chunk else 1 << 20, LARGEST)
        assert 0 < st["device_scratch_bytes"] <= bound and 0 < st["pinned_bytes"] <= bound
        assert st["table_bytes"] < 4096 + 200 * len(ids) + 24 * sum((c.size // 4 + 1023) // 1024 + 1 for c in clouds)   # the small tables
        # chunk_points below 64 count as 64: {1, 63} {64} {65} {257} {1025} {1024} {4800} {768} {1}; 1000: the first five together
        assert st["groups"] == {1: 9, 64: 9, 1000: 5, 5000: 3, 0: 1}[chunk]
    n_diff = sum(a != b for a, b in zip(files[0], want)) + abs(len(files[0]) - len(want))
    print("bytes that differ from the oracle's file: %d of %d" % (n_diff, len(want)))
    assert files[0] == want
    assert all(f == files[0] for f in files[1:])   # the file does not depend on chunk_points
    assert files[0][-84:] == co.ply_camera(len(want_rows), 1) if fmt == "ply" else True
    # ... and is, byte for byte, what rgbdfe_assemble_map returns
    got = fe.assemble_map(ids, Ts, maximum_depth, preserve_raster)
    assert files[0] == co.file_bytes(got, fmt)
    rows, info = read_cloud_file(str(tmp_path / ("map_0.%s" % fmt)))
    back = want_rows.view(np.uint32).copy()
    if fmt == "ply":
        back[:, 3] &= 0x00FFFFFF
    assert rows.shape == (1, len(want_rows), 4) and rows.tobytes() == back.tobytes()
    assert (info["format"], info["width"], info["height"], info["points"]) == (fmt, len(want_rows), 1, len(want_rows))


@pytest.mark.parametrize("fmt", ["pcd", "ply"])
def test_an_id_listed_twice_and_groups_below_a_quad(fe, scene, tmp_path, fmt):
    ids, clouds, Ts = scene
    lst = [9, 0, 3, 3, 0, 9, 7, 9]   # single points around larger clouds: PLY groups that stay below four vertices
    T = [Ts[k] for k in lst]
    want = co.file_bytes(mo.assemble([clouds[k] for k in lst], T, np.inf, False)[0], fmt)
    for chunk in (1, 100, 0):
        path = str(tmp_path / ("twice_%d.%s" % (chunk, fmt)))
        fe.save_map(path, lst, T, np.inf, False, chunk_points=chunk)
        assert read_file(path) == want, chunk


def test_name_rule_through_save_map(fe, scene, tmp_path):
    ids, clouds, Ts = scene
    for given, written, fmt in (("a.PLY", "a.PLY", "ply"), ("a.PcD", "a.PcD", "pcd"), ("a", "a.pcd", "pcd"), ("a.ply.bak", "a.ply.bak.pcd", "pcd")):
        st = fe.save_map(str(tmp_path / given), ids[:3], Ts[:3])
        assert (st["path"], st["format"]) == (str(tmp_path / written), fmt)
        assert read_file(st["path"]) == co.file_bytes(mo.assemble(clouds[:3], Ts[:3])[0], fmt)
    assert sorted(os.listdir(tmp_path)) == ["a.PLY", "a.PcD", "a.pcd", "a.ply.bak.pcd"]


def test_no_points_no_file(fe, scene, tmp_path):
    ids, clouds, Ts = scene
    for fmt in ("pcd", "ply"):
        st = fe.save_map(str(tmp_path / ("none." + fmt)), [], np.zeros((0, 4, 4), np.float32))
        assert (st["points"], st["bytes_written"], st["groups"], st["format"]) == (0, 0, 0, fmt)
        st = fe.save_map(str(tmp_path / ("clipped." + fmt)), ids, Ts, maximum_depth=0.0)   # every point is clipped
        assert (st["points"], st["bytes_written"]) == (0, 0)
    assert os.listdir(tmp_path) == []


def test_unknown_node_and_unopenable_path(fe, scene, tmp_path):
    ids, clouds, Ts = scene
    L = fe._L
    T = np.ascontiguousarray(np.asarray(Ts[:3], np.float32).transpose(0, 2, 1))
    lst = np.array([0, 77, 1], np.int32)
    stats = C.create_string_buffer(64)
    good = str(tmp_path / "x.pcd").encode()

    def call(node_ids, path, chunk=0, n=3, written=None, cap=0):
        return L.rgbdfe_save_map(fe._ctx, n, node_ids.ctypes.data, T.ctypes.data, 2.5, 0, path, chunk, written, cap, stats)
    assert call(lst, good) == UNKNOWN_NODE
    assert call(ids[:3], str(tmp_path / "no_such_dir" / "x.pcd").encode()) == INVALID_ARG
    assert b"cannot open" in L.rgbdfe_last_error(fe._ctx)
    assert call(ids[:3], good, chunk=-1) == INVALID_ARG and call(ids[:3], good, n=-1) == INVALID_ARG
    assert call(ids[:3], None) == INVALID_ARG and call(ids[:3], b"") == INVALID_ARG
    small = C.create_string_buffer(4)
    assert call(ids[:3], good, written=small, cap=4) == CAPACITY
    assert os.listdir(tmp_path) == []
    assert call(ids[:3], good) == 0 and os.listdir(tmp_path) == ["x.pcd"]


# ---- saveIndividualCloudsToFile ---------------------------------------------------------------------------------------------
def random_poses(n, seed=3):
    rng = np.random.default_rng(seed)
    poses = []
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        P = np.eye(4)
        P[:3, :3] = q
        P[:3, 3] = rng.uniform(-3, 3, 3)
        poses.append(P)
    poses[1] = np.eye(4)
    poses[2][:3, :3] = np.diag([-1.0, -1.0, 1.0])   # a half turn: the conversion's branch without a positive trace
    return poses


@pytest.mark.parametrize("moved", [False, True])
def test_node_cloud_files(fe, scene, tmp_path, moved):
    from rgbdslam_v2_amd.frontend import read_cloud_file
    ids, clouds, Ts = scene
    poses = random_poses(len(ids))
    graph_ids = [100 + 7 * int(k) for k in ids]
    before = [fe.node_cloud(int(k)).tobytes() for k in ids]
    base = str(tmp_path / "cloud")
    assert fe.save_node_clouds(base, ids, poses, graph_ids=graph_ids, transform_individual_clouds=moved) == len(ids)
    assert sorted(os.listdir(tmp_path)) == sorted("cloud_%04d.%s" % (g, e) for g in graph_ids for e in ("pcd", "txt"))
    for k, g in zip(ids, graph_ids):
        cloud = clouds[k]
        if moved:   # pcl::transformPointCloud with the pose cast to float: raster assembly of the node alone, clip off
            rows = mo.assemble([cloud], [poses[k].astype(np.float32)], -1.0, True)[0].reshape(cloud.shape)
            assert rows.tobytes() == fe.assemble_map([k], [poses[k].astype(np.float32)], -1.0, True).tobytes()
        else:
            rows = cloud
            assert rows.tobytes() == before[k]
        vp = co.node_viewpoint(poses[k], moved)
        data = read_file("%s_%04d.pcd" % (base, g))
        assert data == co.pcd_bytes(rows, vp), (k, data[:300])
        assert ("WIDTH %d\nHEIGHT %d\n" % (cloud.shape[1], cloud.shape[0])).encode() in data
        got, info = read_cloud_file("%s_%04d.pcd" % (base, g))
        assert got.shape == cloud.shape and info["viewpoint"].tobytes() == np.array([float(co.fmt_g(v)) for v in vp], np.float32).tobytes()
        assert read_file("%s_%04d.txt" % (base, g)).decode() == co.node_txt(poses[k], moved)
    if moved:
        assert b"\nVIEWPOINT 0 0 0 0 0 0 1\n" in read_file("%s_%04d.pcd" % (base, graph_ids[0]))
        assert read_file("%s_%04d.txt" % (base, graph_ids[0])) == b"-1 0 0 0 0 -1 0 0 0 0 1 0 0 0 0 1\n"
    assert [fe.node_cloud(int(k)).tobytes() for k in ids] == before   # the resident clouds are not modified


def test_node_cloud_files_of_a_reduced_an_empty_and_an_unknown_node(fe, tmp_path):
    rng = np.random.default_rng(8)
    d = rng.uniform(0.5, 3.0, (24, 32)).astype(np.float32)
    try:
        upload(fe, 12, d, seed=12)
        upload(fe, 13, np.full((6, 8), np.nan, np.float32), seed=13)
        upload(fe, 14, d[:5, :7].copy(), seed=14)
        n = fe.reduce_node_cloud(12, 0.25)[0]
        assert 0 < n < d.size and fe.node_cloud(12).shape == (1, n, 4)
        assert fe.reduce_node_cloud(13, 0.25)[0] == 0
        poses = random_poses(3, seed=4)
        for moved in (False, True):
            base = str(tmp_path / ("r%d" % moved))
            assert fe.save_node_clouds(base, [12, 13, 14], poses, transform_individual_clouds=moved) == 2   # node 13: skipped
            data = read_file(base + "_0012.pcd")
            assert ("WIDTH %d\nHEIGHT 1\n" % n).encode() in data and len(data) == data.index(b"DATA binary\n") + 12 + 16 * n
            assert not os.path.exists(base + "_0013.pcd") and not os.path.exists(base + "_0013.txt")
            assert b"WIDTH 7\nHEIGHT 5\n" in read_file(base + "_0014.pcd") and os.path.exists(base + "_0014.txt")
        before = sorted(os.listdir(tmp_path))
        one = np.array([12, 99], np.int32)
        P = np.ascontiguousarray(np.stack(poses[:2]).transpose(0, 2, 1))
        nw = C.c_int32(-1)
        assert fe._L.rgbdfe_save_node_clouds(fe._ctx, 2, one.ctypes.data, None, P.ctypes.data, 0, str(tmp_path / "u").encode(),
                                            C.byref(nw)) == UNKNOWN_NODE and nw.value == 0
        assert fe._L.rgbdfe_save_node_clouds(fe._ctx, 1, one.ctypes.data, None, P.ctypes.data, 0,
                                            str(tmp_path / "no_such_dir" / "u").encode(), C.byref(nw)) == INVALID_ARG
        assert fe._L.rgbdfe_save_node_clouds(fe._ctx, 1, one.ctypes.data, None, None, 0, str(tmp_path / "u").encode(), C.byref(nw)) == INVALID_ARG
        assert sorted(os.listdir(tmp_path)) == before
    finally:
        for k in (12, 13, 14):
            fe.release_node_cloud(k)
