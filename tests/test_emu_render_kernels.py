"""CPU: the kernel SOURCE of csrc/render.hip run on the host (tests/emu/emu_render.cpp over the HIP-on-CPU vocabulary of
tests/emu/, one OS thread per HIP thread) against tests/render_oracle.py on the planted scenes of tests/render_cases.py: the
four images, byte for byte, in one group and in a group per node.  The clouds are tests/render_cases.cloud_of's, the streams
tests/display_oracle.py's.  The device itself is tests/test_gpu_render.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import display_oracle as do
import render_cases as rc
import render_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.cases()
CLOUDS = {k: rc.cloud_of(f) for k, f in rc.frames().items()}
IMAGES = ("rgba", "depth", "ids", "node_index")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_render")
    lib = os.path.join(d, "libemu_render.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_render.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.emu_render.restype = ctypes.c_int
    L.emu_render.argtypes = [i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    return L


def run(emu, stream, rp, group_first=None, guard=2, count=False):
    """The kernels as api_render.hip launches them, into poisoned images with `guard` rows behind them."""
    n = len(stream["node_types"])
    W, H = rp["width"], rp["height"]
    v = np.ascontiguousarray(stream["vertices"]).view(np.float32).reshape(-1, 4)
    off, soff = np.ascontiguousarray(stream["node_offsets"], np.int64), np.ascontiguousarray(stream["node_strip_offsets"], np.int64)
    strips, types = np.ascontiguousarray(stream["strips"], np.int64), np.ascontiguousarray(stream["node_types"], np.int32)
    if group_first is None:
        group_first = [0, n] if n else [0]
    gf = np.asarray(group_first, np.int32)
    view, proj = np.asarray(rp["view"], np.float64), np.asarray(rp["projection"], np.float64)
    clear = np.asarray(rp["clear_rgba"], np.uint8)
    rgba = np.full((H + guard, W, 4), 0xAB, np.uint8)
    depth = np.full((H + guard, W), -7.0, np.float32)
    ids = np.full((H + guard, W), -77, np.int64)
    node = np.full((H + guard, W), -77, np.int32)
    stats = np.full(2, 77, np.uint64)
    launches = emu.emu_render(n, v.ctypes.data, off.ctypes.data, strips.ctypes.data, soff.ctypes.data, types.ctypes.data,
                              len(gf) - 1, gf.ctypes.data, view.ctypes.data, proj.ctypes.data, W, H,
                              ro.point_size(rp["gl_point_size"]), rp["cull"], clear.ctypes.data, rgba.ctypes.data,
                              depth.ctypes.data, ids.ctypes.data, node.ctypes.data, stats.ctypes.data if count else None)
    assert launches >= 1  # (-1: a group left the queue non-empty; -2: the product kernels counted)
    assert np.all(rgba[H:] == 0xAB) and np.all(depth[H:] == -7.0) and np.all(ids[H:] == -77) and np.all(node[H:] == -77)
    return dict(rgba=rgba[:H], depth=depth[:H], ids=ids[:H], node_index=node[:H], launches=launches, tested=int(stats[0]),
                won=int(stats[1]))


def same(got, want):
    for name in IMAGES:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_planted_scene(emu, case):
    stream = do.display([CLOUDS[k] for k in case["nodes"]], case["disp"], case["transforms"])
    want = ro.render_stream(stream, case["rp"])
    case["planted"](stream, case["rp"], want)
    got = run(emu, stream, case["rp"])
    same(got, want)
    assert got["launches"] == (4 if len(stream["vertices"]) else 1)  # clear; lane pass, workgroup pass, shading
    n = len(case["nodes"])
    if n > 1:  # a group per node: the same bytes
        same(run(emu, stream, case["rp"], list(range(n + 1))), want)
    # the counting kernels (diagnostics): the same bytes, the oracle's fragments; a fragment that won on arrival may lose later
    counted = run(emu, stream, case["rp"], count=True)
    same(counted, want)
    assert counted["tested"] == want["tested"] and int(np.sum(want["ids"] >= 0)) <= counted["won"] <= want["tested"]


def test_both_passes_ran_where_the_cases_say_so():
    """The lane pass and the workgroup pass are told apart by the box alone: the cases hold boxes on both sides of
    kRenderSmallBox = 64 pixels, and points on both sides of 8 x 8."""
    boxes = set()
    for case in CASES:
        if case["name"] in ("fan_front_k7", "fan_front_k8", "guard_band_and_full_screen"):
            stream = do.display([CLOUDS[k] for k in case["nodes"]], case["disp"], case["transforms"])
            boxes |= set(rc._boxes(stream, case["rp"]))
    assert {64, 81, 48 * 32} <= boxes
    sizes = {ro.point_size(c["rp"]["gl_point_size"]) for c in CASES if c["disp"]["display_type"] == do.POINTS}
    assert {1, 2, 3, 4, 64} <= sizes


def test_stand_alone_program_under_the_address_and_undefined_sanitizers(tmp_path):
    """tests/emu/emu_render_main.cpp: the kernel source over exact-size heap blocks, built with -fsanitize=address,undefined (a
    stand-alone program with its own main: nothing is loaded into this interpreter)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "emu_render_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wno-attributes",
           "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_render_main.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the images
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
