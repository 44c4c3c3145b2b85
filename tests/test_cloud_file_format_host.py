"""CPU: the map files' parser (csrc/cloud_file_format.h) as a stand-alone program (tests/emu/cloud_file_main.cpp) built with
the address and undefined-behaviour sanitizers: files written here by tests/cloud_file_oracle.py are accepted and their rows
returned; a good file cut at every length of its header and at several lengths of its data, a header field that lies, counts
that are no numbers or overflow, and a header without its last line are refused without a sanitizer report.  The program is
run directly; nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_file_oracle as co
from test_oracle_cloud_file import cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("cloud_file_format")
    exe = os.path.join(d, "cloud_file_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "cloud_file_main.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the verdicts
        subprocess.run(cmd, check=True)
    return exe


def run(prog, tmp_path, blobs):
    paths = []
    for i, b in enumerate(blobs):
        p = tmp_path / ("f%05d.bin" % i)
        p.write_bytes(b)
        paths.append(str(p))
    lines = []
    for k in range(0, len(paths), 400):   # (the command line has a length)
        r = subprocess.run([prog] + paths[k:k + 400], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines += r.stdout.splitlines()
    assert len(lines) == len(blobs)
    return lines


def ok_line(pts, fmt, data):
    rows, info = co.read(data)
    return "ok %d %d %d %d %d %d" % (("pcd", "ply").index(fmt), info["width"], info["height"], info["points"], info["header_bytes"],
                                     int(np.frombuffer(rows.tobytes(), np.uint8).sum(dtype=np.uint64)))


def test_files_of_the_two_layouts_are_accepted_and_their_rows_returned(prog, tmp_path):
    clouds = [cloud(n, n) for n in (0, 1, 3, 4, 5, 1025)] + [cloud(35, 3, shape=(5, 7))]
    vp = (0.5, -0.0, 1e-5, 123456.7, 1e20, np.inf, np.nan)
    blobs, want = [], []
    for pts in clouds:
        for fmt in ("pcd", "ply"):
            blobs.append(co.file_bytes(pts, fmt, vp))
            want.append(ok_line(pts, fmt, blobs[-1]))
    assert run(prog, tmp_path, blobs) == want


@pytest.mark.parametrize("fmt", ["pcd", "ply"])
def test_a_file_cut_anywhere_is_refused(prog, tmp_path, fmt):
    good = co.file_bytes(cloud(21, 2), fmt, (1.5, -2.0, 0.25, 1.0, 0.0, 0.0, 0.0))
    head = co.read(good)[1]["header_bytes"]
    cuts = list(range(head + 1)) + [head + 1, head + 15, head + 16, head + 17, head + 15 * 21, len(good) - 84, len(good) - 1]
    blobs = [good[:k] for k in sorted(set(k for k in cuts if 0 <= k < len(good)))] + [good + b"\0", good + good]
    lines = run(prog, tmp_path, blobs)
    assert [ln for ln in lines if not ln.startswith("bad cloud file: ")] == []
    assert run(prog, tmp_path, [good])[0].startswith("ok ")


def test_headers_that_lie_are_refused(prog, tmp_path):
    pcd = co.pcd_bytes(cloud(12, 1, shape=(3, 4)))
    ply = co.ply_bytes(cloud(12, 1))
    big = str(1 << 31).encode()
    cases = {
        "POINTS more": pcd.replace(b"POINTS 12", b"POINTS 13"), "POINTS fewer": pcd.replace(b"POINTS 12", b"POINTS 11"),
        "WIDTH": pcd.replace(b"WIDTH 4", b"WIDTH 5"), "HEIGHT": pcd.replace(b"HEIGHT 3", b"HEIGHT 2"),
        "vertex more": ply.replace(b"vertex 12", b"vertex 13"), "vertex fewer": ply.replace(b"vertex 12", b"vertex 11"),
        "vertex 2^64": ply.replace(b"vertex 12", b"vertex 18446744073709551628"),
        "SIZE": pcd.replace(b"SIZE 4 4 4 4", b"SIZE 4 4 4 8"), "TYPE": pcd.replace(b"TYPE F F F F", b"TYPE F F F U"),
        "COUNT": pcd.replace(b"COUNT 1 1 1 1", b"COUNT 1 1 1 2"), "DATA ascii": pcd.replace(b"DATA binary", b"DATA ascii"),
        "DATA compressed": pcd.replace(b"DATA binary", b"DATA binary_compressed"),
        "FIELDS": pcd.replace(b"FIELDS x y z rgb", b"FIELDS x y z rgba"), "VERSION": pcd.replace(b"VERSION 0.7", b"VERSION .7"),
        "WIDTH text": pcd.replace(b"WIDTH 4", b"WIDTH four"), "WIDTH negative": pcd.replace(b"WIDTH 4", b"WIDTH -4"),
        "WIDTH empty": pcd.replace(b"WIDTH 4", b"WIDTH "), "WIDTH blank": pcd.replace(b"WIDTH 4", b"WIDTH  4"),
        "WIDTH 2^31": pcd.replace(b"WIDTH 4", b"WIDTH " + big).replace(b"HEIGHT 3", b"HEIGHT 1").replace(b"POINTS 12", b"POINTS " + big),
        "POINTS 2^64+12": pcd.replace(b"POINTS 12", b"POINTS 18446744073709551628"),
        "WIDTH x HEIGHT wraps": pcd.replace(b"WIDTH 4", b"WIDTH 65536").replace(b"HEIGHT 3", b"HEIGHT 65536").replace(b"POINTS 12", b"POINTS 0"),
        "VIEWPOINT six": pcd.replace(b"VIEWPOINT 0 0 0 1 0 0 0", b"VIEWPOINT 0 0 0 1 0 0"),
        "VIEWPOINT text": pcd.replace(b"VIEWPOINT 0 0 0 1 0 0 0", b"VIEWPOINT 0 0 0 one 0 0 0"),
        "VIEWPOINT hex": pcd.replace(b"VIEWPOINT 0 0 0 1 0 0 0", b"VIEWPOINT 0 0 0 0x1p0 0 0 0"),
        "VIEWPOINT long": pcd.replace(b"VIEWPOINT 0 0 0 1 0 0 0", b"VIEWPOINT 0 0 0 " + b"1" * 40 + b" 0 0 0"),
        "no end_header": ply.replace(b"end_header\n", b""), "no end_header, longer": ply.replace(b"end_header\n", b"end_heade\n") + b"\0",
        "big endian": ply.replace(b"binary_little_endian", b"binary_big_endian"), "ply ascii": ply.replace(b"binary_little_endian", b"ascii"),
        "a property more": ply.replace(b"property float k2\n", b"property float k2\nproperty float k3\n"),
        "vertex text": ply.replace(b"vertex 12", b"vertex twelve"), "crlf": pcd.replace(b"\n", b"\r\n", 3),
        "viewport": ply[:-16] + bytes(4) + ply[-12:], "header only": pcd[:co.read(pcd)[1]["header_bytes"]], "empty": b"",
    }
    names = list(cases)
    for n in names:
        assert cases[n] not in (pcd, ply), n   # (every replacement took place)
    lines = run(prog, tmp_path, [cases[n] for n in names])
    for n, line in zip(names, lines):
        assert line.startswith("bad cloud file: "), (n, line)
