"""CPU: the image writers and the trajectory reader of tools/render_map.py (no device): a PNG written with zlib decodes to the
bytes that went in, a PPM holds the r, g, b, a pose line becomes the matrix of its quaternion."""
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import render_map  # noqa: E402


def read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, bits, colour, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (bits, comp, flt, lace) == (8, 0, 0, 0) and colour in (2, 6)
    ch = 4 if colour == 6 else 3
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert np.all(rows[:, 0] == 0)
    return rows[:, 1:].reshape(h, w, ch)


def test_png_and_ppm_hold_the_pixels(tmp_path):
    rng = np.random.default_rng(1)
    for shape in ((5, 7, 4), (1, 1, 4), (6, 3, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / "a.png")
        render_map.write_png(path, img)
        assert np.array_equal(read_png(path), img)
    img = rng.integers(0, 256, (4, 9, 4), dtype=np.uint8)
    render_map.write_image(str(tmp_path / "b.png"), img)
    got = read_png(str(tmp_path / "b.png"))
    assert np.array_equal(got[..., :3], img[..., :3]) and np.all(got[..., 3] == 255)
    render_map.write_image(str(tmp_path / "b.ppm"), img)
    data = open(str(tmp_path / "b.ppm"), "rb").read()
    assert data.startswith(b"P6\n9 4\n255\n") and data[len(b"P6\n9 4\n255\n"):] == img[..., :3].tobytes()


def test_trajectory_lines_become_poses(tmp_path):
    path = str(tmp_path / "t.txt")
    with open(path, "w") as f:
        f.write("# stamp tx ty tz qx qy qz qw\n0.5 1 2 3 0 0 0 1\n1.5 0 0 0 0 0.70710678118654752 0 0.70710678118654752\n")
    (s0, p0), (s1, p1) = render_map.read_trajectory(path)
    assert (s0, s1) == (0.5, 1.5) and np.array_equal(p0[:3, :3], np.eye(3)) and p0[:3, 3].tolist() == [1, 2, 3]
    assert np.allclose(p1[:3, :3], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-15)  # a quarter turn about y
