"""GPU: the map-file wrappers of include/rgbdfe.hpp (tests/cpp/map_files.cpp, plain g++ against the header and
librgbdfe.so, a child process) against the Python binding on a fresh FrontEnd: the same clouds restored as resident nodes, the
same transforms and poses -- the files of the two must be equal byte for byte.  (The binding gives the oracle's bytes:
tests/test_gpu_map_files.py.)"""
import os
import subprocess

import numpy as np
import pytest

from rgbdslam_v2_amd import _lib
from rgbdslam_v2_amd.frontend import FrontEnd, read_cloud_file, save_cloud_file
from test_gpu_map_assembly import random_transforms
from test_gpu_map_files import random_poses

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (7, 9), (25, 41), (60, 80), (1, 257))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, linked and rpath'ed as examples/cpp/Makefile does."""
    out = str(tmp_path_factory.mktemp("cpp_map_files") / "map_files")
    lib = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_files.cpp"), "-o", out, "-L" + lib, "-lrgbdfe",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_headers_files_are_the_bindings_files(exe, tmp_path):
    rng = np.random.default_rng(17)
    clouds = []
    for rows, cols in SHAPES:
        c = rng.uniform(-2.0, 2.0, (rows, cols, 4)).astype(np.float32)
        c.view(np.uint32)[..., 3] = rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
        c[rng.random((rows, cols)) < 0.1, 2] = np.nan
        clouds.append(c)
    n = len(clouds)
    Ts = random_transforms(rng, n)
    poses = random_poses(n, seed=6)
    for k, c in enumerate(clouds):
        save_cloud_file(str(tmp_path / ("in_%d.pcd" % k)), c)
    np.ascontiguousarray(np.asarray(Ts, np.float32).transpose(0, 2, 1)).tofile(tmp_path / "transforms.bin")
    np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1)).tofile(tmp_path / "poses.bin")
    r = subprocess.run([exe, str(tmp_path), str(n), "2.5", "3000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]

    ids = list(range(n))
    graph_ids = [100 + 7 * k for k in ids]
    fe = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    try:
        for k, c in enumerate(clouds):
            fe.restore_node_cloud(k, c, 40.0, 40.0, 1.0, 1.0)
        want = []
        for name, raster in (("py_map.pcd", False), ("py_map.ply", False), ("py_raster", True)):
            st = fe.save_map(str(tmp_path / name), ids, Ts, 2.5, raster, chunk_points=3000)
            want.append("map %s %d %d %d %d" % (os.path.basename(st["path"]).replace("py_", "cpp_"), st["points"], st["bytes_written"],
                                                ("pcd", "ply").index(st["format"]), st["groups"]))
            assert st["points"] > 0 and st["groups"] == 3
        for moved in (0, 1):
            want.append("clouds %d %d" % (moved, fe.save_node_clouds(str(tmp_path / ("py_moved" if moved else "py_plain")), ids, poses,
                                                                     graph_ids=graph_ids, transform_individual_clouds=bool(moved))))
    finally:
        fe.close()
    save_cloud_file(str(tmp_path / "py_copy.ply"), clouds[-1])
    want.append("copy 1 257 1 257")
    assert r.stdout.splitlines() == want
    names = sorted(os.listdir(tmp_path))
    py = [f for f in names if f.startswith("py_")]
    assert len(py) == 3 + 4 * n + 1 and "py_raster.pcd" in py
    for f in py:
        twin = tmp_path / f.replace("py_", "cpp_")
        assert twin.exists() and twin.read_bytes() == (tmp_path / f).read_bytes(), f
    assert read_cloud_file(str(tmp_path / "cpp_copy.ply"))[0].shape == (1, 257, 4)
