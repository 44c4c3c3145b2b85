"""CPU: the kernel SOURCE of csrc/display_geometry.hip run on the host (tests/emu/emu_display.cpp over the HIP-on-CPU vocabulary
of tests/emu/, one OS thread per HIP thread) against tests/display_oracle.py: the hand-written streams of
tests/display_cases.py and clouds either side of the kernels' tiles -- counts, offsets, strip records and vertex bytes.
The device itself is tests/test_gpu_display_geometry.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import display_cases as dc
import display_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dc.hand_cases()
ITEM_TILE, ROW_TILE = 1024, 64  # kDispItemTile, kDispRowTile (csrc/display_geometry.h)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_display")
    lib = os.path.join(d, "libemu_display.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_display.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    L.emu_display.restype = ctypes.c_int
    L.emu_display_scan.restype = None
    L.emu_display_scan.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp]
    L.emu_display.argtypes = [ctypes.c_int32, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                              vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, vp]
    return L


def run(emu, clouds, prm, transforms=None, slack=3):
    """The call as api_display.hip makes it, into buffers with `slack` poisoned guard rows behind the needed sizes."""
    clouds = [np.ascontiguousarray(c, np.float32) for c in clouds]
    n = len(clouds)
    ptrs = (ctypes.c_void_p * n)(*[c.ctypes.data for c in clouds])
    hw = np.array([c.shape[:2] for c in clouds], np.int32).reshape(-1)
    T = None
    if transforms is not None:
        T = np.ascontiguousarray(np.asarray(transforms, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
    totals, first, types = np.zeros(2, np.int64), np.zeros(2 * (n + 1), np.int64), np.zeros(n, np.int32)

    def call(v, s):
        return emu.emu_display(n, ptrs, hw.ctypes.data, T.ctypes.data if T is not None else None, prm["display_type"],
                               prm["visualization_skip_step"], prm["squared_meshing_threshold"], prm["maximum_depth"],
                               v.ctypes.data, len(v) - slack, s.ctypes.data, len(s) - slack, totals.ctypes.data,
                               first.ctypes.data, types.ctypes.data)
    none_v, none_s = np.zeros((slack, 4), np.uint32), np.zeros((slack, 2), np.int64)
    sized = call(none_v, none_s)
    v = np.full((totals[0] + slack, 4), 0xDEADBEEF, np.uint32)
    s = np.full((totals[1] + slack, 2), -77, np.int64)
    launches = call(v, s)
    assert sized == (-1 if totals[0] or totals[1] else launches)
    assert np.all(v[totals[0]:] == 0xDEADBEEF) and np.all(s[totals[1]:] == -77)
    first = first.reshape(-1, 2)
    return dict(vertices=v[:totals[0]], strips=s[:totals[1]], node_offsets=first[:, 0].copy(),
                node_strip_offsets=first[:, 1].copy(), node_types=types, launches=launches)


def check(got, want):
    assert np.array_equal(got["node_types"], want["node_types"])
    assert np.array_equal(got["node_offsets"], want["node_offsets"])
    assert np.array_equal(got["node_strip_offsets"], want["node_strip_offsets"])
    assert np.array_equal(got["strips"], want["strips"])
    assert do.same_vertices(got["vertices"], want["vertices"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_written_streams(emu, case):
    got = run(emu, [case["cloud"]], case["prm"])
    assert do.same_vertices(got["vertices"], dc.rows_of(case["cloud"], case["stream"]))
    assert np.array_equal(got["strips"], case["strips"])
    check(got, do.display([case["cloud"]], case["prm"], literal=True))


def test_all_hand_cases_in_one_call_of_each_form(emu):
    """Mixed sizes and node types, an id's cloud twice in a row, with transforms; the launches do not depend on the nodes."""
    clouds = [c["cloud"] for c in CASES]
    clouds.insert(3, clouds[3])
    rng = np.random.default_rng(2)
    Ts = np.tile(np.eye(4, dtype=np.float32), (len(clouds), 1, 1))
    Ts[:, :3, :] = rng.uniform(-2, 2, (len(clouds), 3, 4))
    for t, step, launches in ((do.POINTS, 1, 3), (do.TRIANGLES, 1, 3), (do.TRIANGLE_STRIP, 1, 5), (do.TRIANGLE_STRIP, 2, 5)):
        prm = do.default_params(display_type=t, visualization_skip_step=step)
        got = run(emu, clouds, prm, Ts)
        assert got["launches"] == launches  # count (+ row count), scan, write (+ row write): rows == 1 clouds are POINTS
        assert set(got["node_types"].tolist()) == {do.POINTS, t}
        check(got, do.display(clouds, prm, Ts, literal=True))


# POINTS: w * h either side of a tile; TRIANGLES: (w - 1) * (h - 1); a cloud of more than one column per thread group
@pytest.mark.parametrize("form,shape", [(do.POINTS, (32, 32)), (do.POINTS, (31, 33)), (do.POINTS, (25, 41)),
                                        (do.TRIANGLES, (33, 33)), (do.TRIANGLES, (32, 34)), (do.TRIANGLES, (26, 42)),
                                        (do.TRIANGLES, (5, 300))])
def test_item_tiles(emu, form, shape):
    h, w = shape
    items = h * w if form == do.POINTS else (h - 1) * (w - 1)
    assert items in (ITEM_TILE, ITEM_TILE - 1, ITEM_TILE + 1, 4 * 299)
    cloud = dc.holes_and_jumps(np.random.default_rng(h * w), h, w, holes=0.2)
    prm = do.default_params(display_type=form)
    check(run(emu, [cloud], prm), do.display([cloud], prm))


# TRIANGLE_STRIP: visited rows either side of a tile (one chunk, one short, one more), steps 1 and 2
@pytest.mark.parametrize("h,step", [(65, 1), (64, 1), (66, 1), (129, 2), (131, 2)])
def test_row_tiles(emu, h, step):
    rows = len(range(0, h - step, step))
    assert rows in (ROW_TILE, ROW_TILE - 1, ROW_TILE + 1)
    cloud = dc.holes_and_jumps(np.random.default_rng(h), h, 9, holes=0.2, spacing=0.002)
    prm = do.default_params(display_type=do.TRIANGLE_STRIP, visualization_skip_step=step)
    got, want = run(emu, [cloud], prm), do.display([cloud], prm)
    assert len(want["strips"]) > rows // 2
    check(got, want)


def test_a_row_at_its_bound_and_a_row_with_nothing(emu):
    flat = dc.grid(3, 12, spacing=0.002)
    flat[2, :, 2] = np.nan  # the second visited row has no valid lower point
    prm = do.default_params(display_type=do.TRIANGLE_STRIP)
    got = run(emu, [flat], prm)
    assert got["strips"].tolist() == [[0, 22]]  # 2 * ceil((12 - 1) / 1): the stated bound of one row
    check(got, do.display([flat], prm, literal=True))


@pytest.mark.parametrize("n_tiles", [0, 1, 1024, 1025, 2100])
def test_the_scan_over_more_than_one_trip(emu, n_tiles):
    """The one-workgroup scan alone: a trip is 1024 tiles; 2100 tiles are more than two trips.  Nodes of 0 to 4 tiles."""
    rng = np.random.default_rng(n_tiles)
    counts = rng.integers(0, 6145, (n_tiles, 2), dtype=np.uint32)
    first = [0]
    while first[-1] < n_tiles:
        first.append(min(first[-1] + int(rng.integers(0, 5)), n_tiles))
    first = np.asarray(first + [n_tiles], np.uint32)  # the last node owns no tile; then the sentinel
    n_nodes = len(first) - 1
    tile_first, node_first = np.full((n_tiles + 2, 2), -1, np.int64), np.full((n_nodes + 2, 2), -1, np.int64)
    emu.emu_display_scan(counts.ctypes.data, n_tiles, first.ctypes.data, n_nodes, tile_first.ctypes.data, node_first.ctypes.data)
    want = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(counts.astype(np.int64), axis=0)])
    assert np.array_equal(tile_first[:n_tiles + 1], want) and np.all(tile_first[n_tiles + 1] == -1)
    assert np.array_equal(node_first[:n_nodes + 1], want[first]) and np.all(node_first[n_nodes + 1] == -1)


def test_stand_alone_program_under_the_address_and_undefined_sanitizers(tmp_path):
    """tests/emu/emu_display_main.cpp: the kernel source over exact-size heap blocks, built with -fsanitize=address,undefined
    (a stand-alone program with its own main: nothing is loaded into this interpreter)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "emu_display_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wno-attributes",
           "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_display_main.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the offsets
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 1000
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
