"""CPU: sensor-frame ingest (include/rgbdfe.h, "sensor frames"; csrc/ingest.hip).

* the numpy restatement (tests/ingest_oracle.py) against what it restates: CV_RGB2GRAY's fixed-point weights against the
  real-valued luminance, resizeNN's double index table against the exact integer floor;
* the C ABI: the header declares the new entry points, the library exports them, the struct mirror has the library's size;
* the kernel's SOURCE run on the host (tests/emu/emu_ingest.cpp over the HIP-on-CPU vocabulary of tests/emu/) against the
  restatement, bit for bit: every visual encoding x depth encoding at 640x480 (the 16-byte vector instantiation), at 653x491
  with a padded visual_step (the scalar instantiation) and with a 333x250 depth image resampled to 653x491 and a 320x240 one
  to 640x480 (the gather instantiations).  The GPU runs of the same kernel: tests/test_gpu_sensor_ingest.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ingest_oracle as io
from oracle import pyoracle as po
from rgbdslam_v2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rgbdfe_sizeof_sensor_frame", "rgbdfe_ingest_frame", "rgbdfe_sensor_detect_describe",
               "rgbdfe_sensor_detect_describe_batch_nodes")


# ---- the restatement itself -------------------------------------------------------------------------------------------
def test_gray_of_keeps_gray_triples():
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(io.gray_of(np.stack([x, x, x], -1)[None]), x[None])


def test_gray_of_is_the_luminance_within_half_a_step_and_rounding():
    """All 2^24 triples: |gray - (0.299 R + 0.587 G + 0.114 B)| <= 0.51 (the weights are 14-bit roundings of these; max 0.506)."""
    worst = 0.0
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for r in range(256):
        v = np.stack([np.full_like(g, r), g, b], -1)
        lum = 0.299 * r + 0.587 * g.astype(np.float64) + 0.114 * b.astype(np.float64)
        worst = max(worst, float(np.abs(io.gray_of(v).astype(np.float64) - lum).max()))
    print("max |gray - luminance| over all triples: %.4f" % worst)
    assert worst <= 0.51


@pytest.mark.parametrize("src,dst", [(512, 640), (424, 640), (640, 1280), (480, 960), (333, 1000)])
def test_index_table_is_the_exact_floor(src, dst):
    want = np.minimum((np.arange(dst, dtype=np.int64) * src) // dst, src - 1)
    assert np.array_equal(io.index_table(dst, src), want)


def test_resize_nearest_identity_and_doubling():
    a = np.arange(12, dtype=np.uint16).reshape(3, 4)
    assert np.array_equal(io.resize_nearest(a, (3, 4)), a)
    assert np.array_equal(io.resize_nearest(a, (6, 8)), np.repeat(np.repeat(a, 2, 0), 2, 1))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_sensor_entry_points():
    hdr = open(os.path.join(ROOT, "include", "rgbdfe.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        getattr(L, sym)
    for name in ("RGBDFE_VISUAL_MONO8 0", "RGBDFE_VISUAL_RGB8  1", "RGBDFE_VISUAL_BGR8  2", "RGBDFE_DEPTH_32FC1  0",
                 "RGBDFE_DEPTH_16UC1  1"):
        assert "#define " + name in hdr, name
    assert (_lib.VISUAL_MONO8, _lib.VISUAL_RGB8, _lib.VISUAL_BGR8, _lib.DEPTH_32FC1, _lib.DEPTH_16UC1) == (0, 1, 2, 0, 1)


def test_the_struct_mirror_has_the_library_s_size_and_the_abi_version_stays():
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.rgbdfe_sizeof_sensor_frame.restype = ctypes.c_int
    L.rgbdfe_abi_version.restype = ctypes.c_int
    assert L.rgbdfe_sizeof_sensor_frame() == ctypes.sizeof(_lib.RgbdfeSensorFrame) == 48
    assert ctypes.sizeof(_lib.RgbdfeSensorCloud) == 16
    assert L.rgbdfe_abi_version() == 6


# ---- the kernel's source on the CPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_ingest")
    lib = os.path.join(d, "libemu_ingest.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-attributes", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_ingest.cpp"), "-o", lib],
                   check=True, capture_output=True, timeout=300)
    L = ctypes.CDLL(lib)
    L.emu_ingest.restype = ctypes.c_int
    L.emu_ingest.argtypes = [ctypes.POINTER(_lib.RgbdfeSensorFrame)] + [ctypes.c_void_p] * 3 + [ctypes.c_int]
    return L


SPECIAL_F32 = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 0.0, 2.549, 2.551, 2.5449998, 2.545, 0.004999, 0.005, 0.015, 1e-30,
                        3.0e7, -3.0e7, 1e38, 0.5, 10.0], np.float32)
SPECIAL_U16 = np.array([0, 499, 500, 510, 511, 5100, 5590, 5600, 5610, 65535, 1, 1000, 2000, 4999], np.uint16)


def synth_visual(rows, cols, channels, seed, pad=0):
    """Random bytes with every value present; `pad` extra bytes per row (a padded visual_step), filled with other noise."""
    rng = np.random.default_rng(seed)
    row_bytes = cols * channels
    buf = rng.integers(0, 256, (rows, row_bytes + pad), dtype=np.uint8)
    v = buf[:, :row_bytes]
    v = v if channels == 1 else v.reshape(rows, cols, 3)
    assert v.base is not None and v.strides[0] == row_bytes + pad
    return v


def synth_depth(rows, cols, encoding, seed):
    rng = np.random.default_rng(seed)
    if encoding == "16UC1":
        d = rng.integers(300, 6000, (rows, cols)).astype(np.uint16)
        d.reshape(-1)[rng.choice(d.size, 40 * len(SPECIAL_U16), replace=False)] = np.tile(SPECIAL_U16, 40)
        return d
    d = rng.uniform(0.3, 3.0, (rows, cols)).astype(np.float32)
    d.reshape(-1)[rng.choice(d.size, 40 * len(SPECIAL_F32), replace=False)] = np.tile(SPECIAL_F32, 40)
    return d


def frame_of(v, d, enc):
    from rgbdslam_v2_amd.frontend import FrontEnd
    return FrontEnd._sensor_frame(v, d, enc)


def assert_planes_equal(got, want):
    for name, a, b in zip(("gray", "mono8", "depth_m"), got, want):
        if a.dtype == np.float32:
            assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)), name + " bits"
        else:
            assert np.array_equal(a, b), name


GEOMETRIES = [
    # visual (rows, cols), depth (rows, cols), visual row padding, misaligned outputs
    ((480, 640), (480, 640), 0, 0),
    ((491, 653), (491, 653), 7, 0),
    ((491, 653), (250, 333), 7, 0),
    ((480, 640), (240, 320), 0, 0),
    ((480, 640), (480, 640), 0, 1),
]


@pytest.mark.parametrize("depth_enc", ["32FC1", "16UC1"])
@pytest.mark.parametrize("visual_enc", ["mono8", "rgb8", "bgr8"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "%dx%d_d%dx%d_pad%d_mis%d" % (g[0][1], g[0][0], g[1][1], g[1][0], g[2], g[3]))
def test_the_kernel_source_equals_the_restatement(emu, geom, visual_enc, depth_enc):
    (rows, cols), (drows, dcols), pad, mis = geom
    v = synth_visual(rows, cols, 1 if visual_enc == "mono8" else 3, 11 * rows + cols, pad)
    d = synth_depth(drows, dcols, depth_enc, 7 * drows + dcols)
    fr, keep = frame_of(v, d, None if visual_enc == "mono8" else visual_enc)
    assert fr.visual_step == cols * (1 if visual_enc == "mono8" else 3) + pad
    got = (np.full((rows, cols), 0xAA, np.uint8), np.full((rows, cols), 0xAA, np.uint8), np.full((rows, cols), -7.0, np.float32))
    assert emu.emu_ingest(ctypes.byref(fr), got[0].ctypes.data, got[1].ctypes.data, got[2].ctypes.data, mis) == 1
    assert_planes_equal(got, io.prepared_planes(v, d))


def test_the_kernel_source_with_null_outputs(emu):
    v = synth_visual(480, 640, 3, 5)
    d = synth_depth(480, 640, "16UC1", 6)
    fr, keep = frame_of(v, d, "rgb8")
    want = io.prepared_planes(v, d)
    g = np.zeros((480, 640), np.uint8)
    assert emu.emu_ingest(ctypes.byref(fr), g.ctypes.data, None, None, 0) == 1
    assert np.array_equal(g, want[0])
    m = np.zeros((480, 640), np.uint8)
    assert emu.emu_ingest(ctypes.byref(fr), None, m.ctypes.data, None, 0) == 1
    assert np.array_equal(m, want[1])


def test_rgb8_and_bgr8_frames_differ_only_by_their_channel_order():
    """The reference applies CV_RGB2GRAY to the channels as stored: a frame read as bgr8 gets the red weight on its blue
    channel.  On the colour test frames that moves >= 90 % of the gray pixels, so the rule is observable."""
    from test_oracle_orb_photos import load_photos
    P = load_photos()
    for k in range(5):
        rgb = io.colour_frame(P, k)
        bgr = np.ascontiguousarray(rgb[..., ::-1])
        assert np.mean(io.gray_of(rgb) != io.gray_of(bgr)) >= 0.90


def test_u16_holes_are_zero_metres_and_a_zero_mask():
    mono8, dm = po.depth_to_mono8(np.array([[0, 499, 500, 510, 5100, 65535]], np.uint16))
    assert dm[0, 0] == 0.0 and not np.isnan(dm).any()
    assert list(mono8[0]) == [0, 0, 0, 0, 230, 255]
