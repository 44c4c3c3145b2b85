"""CPU: the host-only calls of the map files (rgbdfe_save_cloud_file, rgbdfe_cloud_file_info, rgbdfe_load_cloud_file,
rgbdfe_cloud_file_path) through the library with no device and no context, against tests/cloud_file_oracle.py."""
import ctypes as C
import os

import numpy as np
import pytest

import cloud_file_oracle as co
from test_oracle_cloud_file import cloud

INVALID_ARG, CAPACITY = -1, -5


@pytest.fixture(scope="module")
def mod(frontend_lib):
    from rgbdslam_v2_amd import frontend
    return frontend


@pytest.mark.parametrize("fmt", ["pcd", "ply"])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1025])
def test_saved_bytes_equal_the_oracles(mod, tmp_path, n, fmt):
    pts = cloud(n, n)
    vp = (0.5, -0.0, 1e-5, 123456.7, 1e20, 0.0, -1.0)
    path = str(tmp_path / ("c." + fmt))
    mod.save_cloud_file(path, pts, viewpoint=vp)
    data = open(path, "rb").read()
    assert data == co.file_bytes(pts, fmt, vp)
    got, info = mod.read_cloud_file(path)
    want, winfo = co.read(data)
    assert got.shape == (1, n, 4) and got.tobytes() == want.tobytes()
    assert {k: info[k] for k in ("format", "width", "height", "points", "header_bytes")} == \
        {k: winfo[k] for k in ("format", "width", "height", "points", "header_bytes")}
    assert info["data_bytes"] == len(data) - info["header_bytes"]
    if fmt == "pcd":
        assert info["viewpoint"].tobytes() == np.array([float(co.fmt_g(v)) for v in vp], np.float32).tobytes()
        assert got.tobytes() == pts.tobytes()                          # NaN payloads and the rgb word's top byte included
    else:
        assert np.all(got.view(np.uint32)[..., 3] >> 24 == 0)          # a vertex has three colour bytes
        assert np.array_equal(got.view(np.uint32)[0, :, :3], pts.view(np.uint32)[:, :3])
        assert mod.read_cloud_file(path, header_only=True)["viewpoint"].tolist() == [0, 0, 0, 1, 0, 0, 0]


@pytest.mark.parametrize("fmt", ["pcd", "ply"])
def test_organised_clouds(mod, tmp_path, fmt):
    pts = cloud(35, 3, shape=(5, 7))
    path = str(tmp_path / ("o." + fmt))
    mod.save_cloud_file(path, pts)
    assert open(path, "rb").read() == co.file_bytes(pts, fmt)
    got, info = mod.read_cloud_file(path)
    assert got.shape == (5, 7, 4) and (info["width"], info["height"], info["points"]) == (7, 5, 35)


def test_default_viewpoint_is_the_aggregates(mod, tmp_path):
    path = str(tmp_path / "d.pcd")
    mod.save_cloud_file(path, cloud(3))
    assert b"\nVIEWPOINT 0 0 0 1 0 0 0\n" in open(path, "rb").read()


@pytest.mark.parametrize("given, written, fmt", [("m.PLY", "m.PLY", "ply"), ("m.pcd", "m.pcd", "pcd"), ("m.PcD", "m.PcD", "pcd"),
                                                 ("m", "m.pcd", "pcd"), ("m.ply.bak", "m.ply.bak.pcd", "pcd")])
def test_name_rule(mod, given, written, fmt):
    assert mod.cloud_file_path("/some/dir/" + given) == ("/some/dir/" + written, fmt)


def test_name_rule_capacity(frontend_lib):
    L = frontend_lib
    buf = C.create_string_buffer(5)
    f = C.c_int32(-1)
    assert L.rgbdfe_cloud_file_path(b"m", buf, 5, C.byref(f)) == CAPACITY and f.value == 0   # "m.pcd" and its NUL need 6
    assert L.rgbdfe_cloud_file_path(b"m.ply", buf, 5, C.byref(f)) == CAPACITY and f.value == 1
    assert L.rgbdfe_cloud_file_path(None, buf, 5, C.byref(f)) == INVALID_ARG


def test_capacity_and_open_failures(frontend_lib, mod, tmp_path):
    L = frontend_lib
    pts = cloud(5)
    path = str(tmp_path / "five.pcd").encode()
    assert L.rgbdfe_save_cloud_file(pts.ctypes.data, 5, 1, None, 0, path) == 0
    h = mod._lib.CloudFileHeader()
    out = np.full((5, 4), 7.0, np.float32)
    assert L.rgbdfe_load_cloud_file(path, out.ctypes.data, 4, C.byref(h)) == CAPACITY and h.points == 5 and np.all(out == 7.0)
    assert b"too small" in L.rgbdfe_last_error(None)
    assert L.rgbdfe_load_cloud_file(path, out.ctypes.data, 5, C.byref(h)) == 0 and out.tobytes() == pts.tobytes()
    assert L.rgbdfe_load_cloud_file(path, None, 5, C.byref(h)) == INVALID_ARG
    missing = str(tmp_path / "no_such_dir" / "x.pcd").encode()
    assert L.rgbdfe_save_cloud_file(pts.ctypes.data, 5, 1, None, 0, missing) == INVALID_ARG
    assert b"cannot open" in L.rgbdfe_last_error(None)
    assert L.rgbdfe_cloud_file_info(missing, C.byref(h)) == INVALID_ARG
    assert L.rgbdfe_load_cloud_file(missing, out.ctypes.data, 5, C.byref(h)) == INVALID_ARG
    assert L.rgbdfe_cloud_file_info(str(tmp_path).encode(), C.byref(h)) == INVALID_ARG       # a directory
    assert L.rgbdfe_save_cloud_file(pts.ctypes.data, 5, 1, None, 2, path) == INVALID_ARG     # no such format
    assert L.rgbdfe_save_cloud_file(pts.ctypes.data, -1, 1, None, 0, path) == INVALID_ARG
    assert L.rgbdfe_save_cloud_file(None, 5, 1, None, 0, path) == INVALID_ARG
    assert L.rgbdfe_save_cloud_file(pts.ctypes.data, 1 << 16, 1 << 15, None, 0, path) == CAPACITY   # 2^31 points
    assert open(path, "rb").read() == co.pcd_bytes(pts)   # the refused calls left the file alone
    assert not os.path.exists(missing)


def test_files_of_other_layouts_are_refused(frontend_lib, mod, tmp_path):
    good = co.pcd_bytes(cloud(4))
    ply = co.ply_bytes(cloud(4))
    bad = {"short": good[:-1], "long": good + b"\0", "ascii": good.replace(b"DATA binary", b"DATA ascii"),
           "fields": good.replace(b"FIELDS x y z rgb", b"FIELDS x y z"), "empty": b"", "ply short": ply[:-1],
           "big endian": ply.replace(b"binary_little_endian", b"binary_big_endian"), "viewport": ply[:-12] + bytes(12)}
    h = mod._lib.CloudFileHeader()
    out = np.zeros((8, 4), np.float32)
    for name, data in bad.items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        assert frontend_lib.rgbdfe_cloud_file_info(str(p).encode(), C.byref(h)) == INVALID_ARG, name
        assert frontend_lib.rgbdfe_load_cloud_file(str(p).encode(), out.ctypes.data, 8, C.byref(h)) == INVALID_ARG, name
        assert frontend_lib.rgbdfe_last_error(None).startswith(b"cloud file: "), name
    assert not out.any()
