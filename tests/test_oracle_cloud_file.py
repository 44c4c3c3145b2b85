"""CPU: the oracle of the map files (tests/cloud_file_oracle.py) against itself: the writer against the independent reader,
the headers against the literals of the contract, the vectorised 15-byte packing against a scalar loop, and the text of a
viewpoint number."""
import numpy as np
import pytest

import cloud_file_oracle as co

SIZES = (0, 1, 3, 4, 5, 1025)


def cloud(n, seed=0, shape=None):
    rng = np.random.default_rng(100 + seed)
    pts = rng.standard_normal((n, 4)).astype(np.float32)
    pts.view(np.uint32)[:, 3] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)   # the top byte included
    if n > 2:
        pts[0, 0], pts[1, 2], pts[2, 1] = np.nan, np.inf, -np.inf
        pts.view(np.uint32)[n - 1, 0] = 0x7FC12345   # a NaN with a payload
    return pts if shape is None else pts.reshape(shape + (4,))


@pytest.mark.parametrize("fmt", ["pcd", "ply"])
@pytest.mark.parametrize("n", SIZES)
def test_reader_returns_what_the_writer_wrote(n, fmt):
    pts = cloud(n, n)
    data = co.file_bytes(pts, fmt)
    got, info = co.read(data)
    want = pts.view(np.uint32).copy()
    if fmt == "ply":
        want[:, 3] &= 0x00FFFFFF   # a vertex has three colour bytes
    assert got.shape == (1, n, 4) and np.array_equal(got.view(np.uint32).reshape(-1, 4), want)
    assert (info["format"], info["width"], info["height"], info["points"]) == (fmt, n, 1, n)
    assert len(data) == info["header_bytes"] + (16 * n if fmt == "pcd" else 15 * n + 84)


def test_organised_clouds_keep_their_shape():
    pts = cloud(35, 3, shape=(5, 7))
    for fmt in ("pcd", "ply"):
        got, info = co.read(co.file_bytes(pts, fmt))
        assert got.shape == (5, 7, 4) and (info["width"], info["height"]) == (7, 5)


def test_headers_are_the_literals():
    h = co.pcd_header(640, 480, (1.5, -2.0, 0.25, 1.0, 0.0, 0.0, 0.0)).decode()
    assert h == ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\n"
                 "COUNT 1 1 1 1\nWIDTH 640\nHEIGHT 480\nVIEWPOINT 1.5 -2 0.25 1 0 0 0\nPOINTS 307200\nDATA binary\n")
    assert co.pcd_header(7, 1).decode().split("\n")[8] == "VIEWPOINT 0 0 0 1 0 0 0"
    p = co.ply_bytes(cloud(3))
    text = p[:p.index(b"end_header\n") + 11].decode()
    lines = text.split("\n")
    assert lines[:4] == ["ply", "format binary_little_endian 1.0", "comment PCL generated", "element vertex 3"]
    assert lines[10] == "element camera 1" and lines[-2] == "end_header" and len(lines) == 34
    assert [ln.split()[2] for ln in lines[11:32]] == ["view_px", "view_py", "view_pz", "x_axisx", "x_axisy", "x_axisz", "y_axisx",
                                                      "y_axisy", "y_axisz", "z_axisx", "z_axisy", "z_axisz", "focal", "scalex", "scaley",
                                                      "centerx", "centery", "viewportx", "viewporty", "k1", "k2"]
    assert [ln.split()[1] for ln in lines[11:32]] == ["float"] * 17 + ["int", "int", "float", "float"]


def test_camera_record():
    cam = np.frombuffer(co.ply_camera(7, 5), "<f4")
    assert cam[:17].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0] and cam[19:].tolist() == [0, 0]
    assert np.frombuffer(co.ply_camera(7, 5), "<i4")[17:19].tolist() == [7, 5]


@pytest.mark.parametrize("n", SIZES + (64, 257))
def test_packing_against_a_scalar_loop(n):
    pts = cloud(n, 7 + n)
    assert co.pack_ply(pts) == co.pack_ply_scalar(pts) and len(co.pack_ply(pts)) == 15 * n
    if n:
        v = co.pack_ply(pts)
        w = int(pts.view(np.uint32)[n - 1, 3])
        assert v[-3:] == bytes([(w >> 16) & 255, (w >> 8) & 255, w & 255]) and v[-15:-3] == pts[n - 1, :3].tobytes()


@pytest.mark.parametrize("value, text", [(0.0, "0"), (-0.0, "-0"), (1e-5, "1e-05"), (123456.7, "123457"), (1e20, "1e+20")])
def test_viewpoint_numbers_print_as_a_stream_prints_them(value, text):
    assert co.fmt_g(value) == text
    assert co.pcd_header(1, 1, (value,) * 7).decode().split("\n")[8] == "VIEWPOINT " + " ".join([text] * 7)


def test_reader_refuses_other_files():
    good = co.pcd_bytes(cloud(4))
    for bad in (good[:-1], good + b"\0", good.replace(b"DATA binary", b"DATA ascii"), good.replace(b"x y z rgb", b"x y z"),
                co.ply_bytes(cloud(4))[:-1], co.ply_bytes(cloud(4)).replace(b"end_header\n", b"end_headers")):
        with pytest.raises((ValueError, KeyError)):
            co.read(bad)


def test_node_text_of_the_quirk_and_of_a_pose():
    assert co.node_txt(np.eye(4), True) == "-1 0 0 0 0 -1 0 0 0 0 1 0 0 0 0 1\n"
    assert co.node_viewpoint(np.eye(4), True).tolist() == [0, 0, 0, 0, 0, 0, 1]
    pose = np.eye(4)
    pose[:3, 3] = (1.5, -2.0, 0.25)
    assert co.node_txt(pose, False) == "1 0 0 1.5 0 1 0 -2 0 0 1 0.25 0 0 0 1\n"
    c, s = np.cos(0.3), np.sin(0.3)
    pose[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    vp = co.node_viewpoint(pose, False)
    assert np.allclose(vp[3:], [np.cos(0.15), 0, 0, np.sin(0.15)], atol=1e-7)
    assert np.allclose(co.quaternionf_to_rotation(*vp[3:]), pose[:3, :3], atol=1e-6)
