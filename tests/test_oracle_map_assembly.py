"""CPU: the two restatements of transformAndAppendPointCloud (tests/map_assembly_oracle.py) against each other -- the
vectorised one the GPU tests use, and the statement-by-statement transcription of src/misc.cpp:183-238 -- and the C ABI's
declarations.  The GPU runs: tests/test_gpu_map_assembly.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import map_assembly_oracle as mo
from rgbdslam_v2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rgbdfe_assemble_map", "rgbdfe_assemble_map_device", "rgbdfe_download_node_cloud")
DEPTHS = (2.5, np.inf, -1.0, np.nan, 0.0)
SETS = ([1], [63, 64, 65], [257, 7, 1025])


def make_cloud(rng, n):
    """n points within a few metres, 20 % with a NaN z, a few +inf coordinates, random rgb words."""
    c = np.empty((n, 4), np.float32)
    c[:, :3] = rng.uniform(-2.5, 2.5, (n, 3)).astype(np.float32)
    c[rng.random(n) < 0.2, 2] = np.nan
    for k in range(max(1, n // 50)):
        c[rng.integers(n), rng.integers(3)] = np.inf
    c.view(np.uint32)[:, 3] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return c


def make_transforms(rng, n):
    """Random rotations with translations; the second one the identity, the last one with a NaN in it."""
    Ts = []
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = q.astype(np.float32)
        T[:3, 3] = rng.uniform(-3, 3, 3).astype(np.float32)
        Ts.append(T)
    if n > 1:
        Ts[1] = np.eye(4, dtype=np.float32)
    if n > 2:
        Ts[-1][1, 2] = np.nan
    return Ts


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20)
    return [([make_cloud(rng, n) for n in sizes], make_transforms(rng, len(sizes))) for sizes in SETS]


@pytest.mark.parametrize("preserve_raster", [False, True])
@pytest.mark.parametrize("maximum_depth", DEPTHS)
def test_vectorised_equals_literal(cases, maximum_depth, preserve_raster):
    for clouds, Ts in cases:
        a, ao = mo.assemble(clouds, Ts, maximum_depth, preserve_raster)
        b, bo = mo.assemble_literal(clouds, Ts, maximum_depth, preserve_raster)
        assert mo.mismatch(a, b) is None, mo.mismatch(a, b)
        assert np.array_equal(ao, bo) and ao[-1] == len(a)
        if preserve_raster:
            sizes = [len(c) for c in clouds]
            assert ao.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
            clipped = mo.clipped_rows(clouds, maximum_depth)
            for got in (a, b):  # clipped raster points are exactly the quiet NaN, their rgb word stays
                assert np.all(got.view(np.uint32)[clipped, :3] == mo.QNAN_BITS)
            assert np.array_equal(a.view(np.uint32)[:, 3], np.concatenate(clouds).view(np.uint32)[:, 3])


def test_every_case_has_kept_clipped_and_skipped_points(cases):
    for clouds, Ts in cases[1:]:
        n = sum(len(c) for c in clouds)
        kept_clip = len(mo.assemble(clouds, Ts, 2.5)[0])
        kept_all = len(mo.assemble(clouds, Ts, np.inf)[0])
        assert 0 < kept_clip < kept_all < n
    clouds, Ts = cases[2]
    for md in (-1.0, np.nan):  # a negative or NaN range disables the clip: the same cloud as +inf
        assert mo.mismatch(mo.assemble(clouds, Ts, md)[0], mo.assemble(clouds, Ts, np.inf)[0]) is None
    assert len(mo.assemble(clouds, Ts, 0.0)[0]) == 0  # no random point sits in the origin


def test_semantics_on_hand_made_points():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    w = np.array([1, 0xFFFFFFFF, 0x7F800001, 4, 5], np.uint32).view(np.float32)
    c = np.array([[1, 2, 2, w[0]],       # range exactly 3: kept at maximum_depth = 3 (strict comparison)
                  [1, 2, 2.0000002, w[1]],  # just beyond
                  [0.5, 0.25, nan, w[2]],   # NaN z beside finite x, y: skipped, copied as it is in raster mode
                  [inf, 0, 1, w[3]],        # inf: distance inf > 9 clipped; kept at maximum_depth = +inf
                  [0, 0, 0, w[4]]], np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [10, 20, 30]
    for fn in (mo.assemble, mo.assemble_literal):
        out, off = fn([c], [T], 3.0, False)
        assert off.tolist() == [0, 2]
        assert out[:, :3].tolist() == [[11, 22, 32], [10, 20, 30]]
        assert out.view(np.uint32)[:, 3].tolist() == [1, 5]
        out, off = fn([c], [T], 3.0, True)
        bits = out.view(np.uint32)
        assert off.tolist() == [0, 5] and bits[:, 3].tolist() == c.view(np.uint32)[:, 3].tolist()
        assert np.all(bits[[1, 3], :3] == mo.QNAN_BITS)
        assert np.array_equal(bits[2], c.view(np.uint32)[2])
        out, off = fn([c], [T], np.inf, False)   # inf * inf = inf is never exceeded
        assert off.tolist() == [0, 4] and out[2, 0] == inf and np.isnan(out[2, 1:3]).all()  # 0 * inf in the other rows
        out, off = fn([c, c], [T, T], 0.0, False)  # only the origin survives a zero range
        assert off.tolist() == [0, 1, 2]


def test_header_declares_and_library_exports_the_entry_points(frontend_lib):
    hdr = open(os.path.join(ROOT, "include", "rgbdfe.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    # refusals that need no device: no context
    n = ctypes.c_int64(-1)
    assert frontend_lib.rgbdfe_assemble_map(None, 0, None, None, 1.0, 0, None, 0, ctypes.byref(n), None) == -1
    assert frontend_lib.rgbdfe_download_node_cloud(None, 0, None, 0, None, None) == -1
