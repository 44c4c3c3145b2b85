"""CPU: the kernel SOURCE of csrc/octomap_query.hip run on the host (tests/emu/emu_octomap_query.cpp over the HIP-on-CPU
vocabulary of tests/emu/, one OS thread per HIP thread) against the scalar restatement in tests/octomap_query_oracle.py, on
the bytes of the search results, the hit records and the view clouds: every case of tests/test_gpu_octomap_query.py, and
the one the public interface cannot produce (a key that is claimed and is not a leaf).  The device's roundings are not what
this test sees -- that is the GPU test."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import octomap_oracle as oo
import octomap_query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_LEAF = 0xffffffff


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_octomap_query")
    lib = os.path.join(d, "libemu_octomap_query.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_octomap_query.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    table = [vp, vp, vp, u32, u32]
    L.emu_octo_search.restype = ctypes.c_int
    L.emu_octo_search.argtypes = table + [ctypes.c_double, vp, u32, vp, vp]
    L.emu_octo_cast.restype = ctypes.c_int
    L.emu_octo_cast.argtypes = table + [vp, vp, vp, u32, vp]
    L.emu_octo_view.restype = ctypes.c_int
    L.emu_octo_view.argtypes = table + [vp, vp, vp, u32, u32, vp, vp]
    return L


def entries(scene):
    """(keys, value bits, colours, capacity) of a scene's table: its leaves, then its claimed keys."""
    lv = scene["leaves"]
    key = [oo.pack(*k) for k in lv["key"]] + list(scene.get("claimed", ()))
    val = list(lv["log_odds"].view(np.uint32)) + [NO_LEAF] * len(scene.get("claimed", ()))
    col = [(int(c[0]) << 16) | (int(c[1]) << 8) | int(c[2]) for c in lv["rgb"]] + [NO_LEAF] * len(scene.get("claimed", ()))
    cap = scene.get("capacity", 2 * len(key) + 8)
    return np.array(key, np.uint64), np.array(val, np.uint32), np.array(col, np.uint32), cap


def threshold(scene, occupied):
    return float(qo.oracle_of(scene).occupied_log_odds()) if occupied is None or np.isnan(occupied) else float(occupied)


def run(emu, scene, query):
    k, v, c, cap = entries(scene)
    table = (k.ctypes.data, v.ctypes.data, c.ctypes.data, len(k), cap)
    if query[0] == "search":
        pts = np.ascontiguousarray(query[1], np.float32)
        found, leaves = np.full(len(pts), -1, np.int32), np.zeros(len(pts), qo.LEAF)
        assert emu.emu_octo_search(*table, scene["resolution"], pts.ctypes.data, len(pts), found.ctypes.data, leaves.ctypes.data) == 0
        return found, leaves
    if query[0] == "cast":
        _, O, D, ign, mr, occ = query
        O, D = np.ascontiguousarray(O, np.float32), np.ascontiguousarray(D, np.float32)
        prm = np.array([scene["resolution"], mr, threshold(scene, occ), ign], np.float64)
        hits = np.zeros(len(O), qo.HIT_REC)
        assert emu.emu_octo_cast(*table, prm.ctypes.data, O.ctypes.data, D.ctypes.data, len(O), hits.ctypes.data) == 0
        return hits
    _, T, fx, fy, cx, cy, rows, cols, ign, mr, occ = query
    T = np.ascontiguousarray(T, np.float32)
    prm = np.array([scene["resolution"], mr, threshold(scene, occ), ign], np.float64)
    intr = np.array([fx, fy, cx, cy], np.float64)
    cloud, status = np.zeros((rows, cols, 4), np.float32), np.zeros((rows, cols), np.uint8)
    assert emu.emu_octo_view(*table, prm.ctypes.data, T.ctypes.data, intr.ctypes.data, rows, cols, cloud.ctypes.data,
                             status.ctypes.data) == 0
    return cloud, status


def same(got, ref):
    if isinstance(ref, tuple):
        assert len(got) == len(ref)
        for g, r in zip(got, ref):
            same(g, r)
        return
    assert got.dtype == ref.dtype and got.shape == ref.shape
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(np.asarray([g.tobytes() != r.tobytes() for g, r in zip(got.reshape(len(got), -1), ref.reshape(len(ref), -1))]))[0]
        raise AssertionError("rows differ: %s; first: got %r, expected %r" % (bad[:8], got[bad[0]], ref[bad[0]]))


@pytest.mark.parametrize("name", list(qo.CASES))
def test_the_kernels_give_the_oracles_bytes(emu, name):
    scene, query = qo.CASES[name]
    same(run(emu, scene, query), qo.expected(name))


def test_the_tables_of_the_load_rule_at_three_quarters_and_after_the_reserve(emu):
    """The load rule itself is the host's; the kernels run on the table at exactly 3/4 and on the re-housed one."""
    lv13, queries = qo.load_rule_inputs()
    for lv, cap in ((lv13[:12], 16), (lv13, 26)):
        scene = dict(resolution=0.1, occupancy_threshold=0.5, leaves=lv, capacity=cap)
        for q in queries:
            same(run(emu, scene, q), qo.run(scene, q))


def test_the_map_of_a_cloud_seen_from_the_pose_it_was_inserted_from(emu):
    _, _, scene, query, ref = qo.raster_view()
    same(run(emu, scene, query), ref)
    assert (ref[1] == qo.HIT).sum() == 3063 and set(np.unique(ref[1])) == {qo.HIT, qo.UNKNOWN}


def test_a_claimed_key_that_is_not_a_leaf_is_no_leaf(emu):
    """The cell (3, 0, 0) is claimed and holds no leaf: search finds none, a ray stops there as unknown or, with unknown
    ignored, walks through to the occupied leaf behind it.  The same table without the claimed key gives the same bytes."""
    cells = {(0, 0, 0): (-1.0, (1, 2, 3)), (1, 0, 0): (-1.0, (4, 5, 6)), (2, 0, 0): (-1.0, (7, 8, 9)), (6, 0, 0): (2.0, (10, 11, 12))}
    scene = dict(resolution=0.25, occupancy_threshold=0.5, leaves=qo.leaves_of(cells))
    claimed = dict(scene, claimed=[oo.pack(32768 + 3, 32768, 32768)], capacity=2 * len(cells) + 8)
    plain = dict(scene, capacity=claimed["capacity"])
    pts = np.array([qo.centre_of((c, 0, 0), 0.25) for c in range(8)], np.float32)
    O, D = pts[:1], np.array([[1, 0, 0]], np.float32)
    for q in (("search", pts), ("cast", O, D, 0, -1.0, None), ("cast", O, D, 1, -1.0, None)):
        ref = qo.run(scene, q)
        same(run(emu, claimed, q), ref)
        same(run(emu, plain, q), ref)
    found, _ = run(emu, claimed, ("search", pts))
    assert list(found) == [1, 1, 1, 0, 0, 0, 1, 0]
    stop, through = run(emu, claimed, ("cast", O, D, 0, -1.0, None)), run(emu, claimed, ("cast", O, D, 1, -1.0, None))
    assert (stop["status"][0], stop["steps"][0]) == (qo.UNKNOWN, 3) and (through["status"][0], through["steps"][0]) == (qo.HIT, 6)
