"""CPU: the session file's validator (csrc/session_format.h) as a stand-alone program (tests/emu/session_main.cpp) built
with the address and undefined-behaviour sanitizers: files written here from the header's description (tests/session_file.py)
are accepted, and a good file cut at every length, with a byte flipped at every offset, with a wrong version or length, with
chunks out of order and with counts that lie under a correct CRC is refused with the cause and without a sanitizer report.
The program is run directly; nothing is loaded into Python under a sanitizer."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import session_file as sf
from rgbdslam_v2_amd.candidates import PoseGraph
from rgbdslam_v2_amd.frontend import Slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = 6


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("session_format")
    exe = os.path.join(d, "session_main")
    csrc = os.path.join(ROOT, "rgbdslam_v2_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "emu", "session_main.cpp"), os.path.join(csrc, "candidates.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the verdicts
        subprocess.run(cmd, check=True)
    return exe


def run(prog, tmp_path, blobs):
    paths = []
    for i, b in enumerate(blobs):
        p = tmp_path / ("f%05d.session" % i)
        p.write_bytes(b)
        paths.append(str(p))
    lines = []
    for k in range(0, len(paths), 400):   # (the command line has a length)
        r = subprocess.run([prog] + paths[k:k + 400], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines += r.stdout.splitlines()
    assert len(lines) == len(blobs)
    return lines


def strings():
    g = PoseGraph()
    g.set_strategy("first")
    for i in range(3):
        g.add_node(i, keyframe=(i == 0))
    g.add_edge_se3(0, 1, np.eye(4), 1.0, set_estimate=True)
    g.add_edge(1, 2)
    s = Slam(None, g, min_matches=10)
    return g.serialize(), s.serialize()


def nodes_of(rows_by_id, kind=0, seed=1):
    rng = np.random.default_rng(seed)
    out = {}
    for i, rows in rows_by_id.items():
        desc = rng.integers(0, 256, (rows, 32), np.uint8) if kind == 0 else rng.standard_normal((rows, 128)).astype(np.float32)
        out[i] = dict(kind=kind, desc=desc, xyz1=rng.standard_normal((rows, 4)).astype(np.float32),
                      kp_xy=rng.standard_normal((rows, 2)).astype(np.float32) if i % 2 else None, stats=rng.integers(0, 256, rows, np.uint8))
    return out


def small_file(clouds=True):
    graph, slam = strings()
    nodes = nodes_of({4: 3, 9: 0, 11: 5})
    nodes.update(nodes_of({2: 1}, kind=2))
    cl = {4: dict(points=np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4), cloud_skip=2, fx=525.0, fy=525.0, cx=319.5, cy=239.5),
          7: dict(points=np.zeros((1, 0, 4), np.float32), cloud_skip=1, fx=1.0, fy=1.0, cx=0.0, cy=0.0)} if clouds else None
    return sf.write(8, ABI, nodes, clouds=cl, graph=graph, slam=slam)


def test_files_written_from_the_description_are_accepted(prog, tmp_path):
    graph, slam = strings()
    files = [small_file(), small_file(clouds=False),
             sf.write(130, ABI, {}),                                                       # no node at all
             sf.write(130, ABI, nodes_of({0: 0, 1: 0})),                                   # nodes without a row
             sf.write(130, ABI, {**nodes_of({5: 65, 0: 130, 7: 1}), **nodes_of({3: 64, 8: 63}, kind=1)}),
             sf.write(16, ABI, nodes_of({1: 2}), dete=sf.dete_payload(1, 300, 8, 2, 1, np.linspace(2, 90, 64)), graph=graph),
             sf.write(16, ABI, nodes_of({1: 2}), slam=slam)]
    lines = run(prog, tmp_path, files)
    assert lines == ["ok 4 9 2 1 1", "ok 4 9 0 1 1", "ok 0 0 0 0 0", "ok 2 0 0 0 0", "ok 5 323 0 0 0", "ok 1 2 0 1 0", "ok 1 2 0 0 1"], lines
    table = sf.chunk_table(files[0])[1]
    assert [t for t, _, _ in table] == sf.ORDER and sf.read(files[0])["nodes"][11]["rows"] == 5


def test_every_truncation_and_every_flipped_byte_is_refused(prog, tmp_path):
    good = small_file()
    blobs = [good[:k] for k in range(len(good))] + [good + bytes(8)]
    for k in range(len(good)):
        b = bytearray(good)
        b[k] ^= 1 << (k % 8)
        blobs.append(bytes(b))
    lines = run(prog, tmp_path, blobs)
    bad = [k for k, line in enumerate(lines) if not line.startswith("bad ")]
    # the only bytes a validator cannot see through: the padding behind a payload is checked to be zero, so none are left
    assert bad == [], (bad[:10], [lines[k] for k in bad[:3]])
    assert all(len(line) > 8 for line in lines)   # a cause is named
    flags, table = sf.chunk_table(good)
    for tag, off, n in table[:-1]:   # a flip inside a payload is that chunk's CRC mismatch
        assert lines[len(good) + 1 + off + n // 2] == "bad session file: CRC mismatch in chunk " + tag.decode(), tag


def reseal(b, table, tag):
    """The CRC of chunk `tag` recomputed over its (patched) payload."""
    off, n = next((o, n) for t, o, n in table if t == tag)
    b[off - 12:off - 8] = struct.pack("<I", zlib.crc32(bytes(b[off:off + n])))
    return bytes(b)


def test_defects_under_correct_checksums(prog, tmp_path):
    good = small_file()
    flags, table = sf.chunk_table(good)
    at = {t: o for t, o, _ in table}
    cases = {}
    b = bytearray(good); struct.pack_into("<I", b, 8, 2); cases["unknown version"] = bytes(b)
    b = bytearray(good); struct.pack_into("<Q", b, 16, len(good) + 8); cases["length field"] = bytes(b)
    b = bytearray(good); struct.pack_into("<I", b, 12, 3); cases["bad header"] = bytes(b)
    b = bytearray(good); struct.pack_into("<I", b, 12, 0); cases["CLOU chunk and the flags"] = bytes(b)
    b = bytearray(good); struct.pack_into("<I", b, at[b"NODE"], 5); cases["NODE chunk"] = reseal(b, table, b"NODE")
    b = bytearray(good); struct.pack_into("<i", b, at[b"NODE"] + 8 + 3 * 16 + 4, 7); cases["NODE chunk (a node's record)"] = reseal(b, table, b"NODE")  # has_keypoints 7
    b = bytearray(good); struct.pack_into("<i", b, at[b"NODE"] + 8 + 2 * 16 + 8, 9); cases["more rows than the CONF chunk"] = reseal(b, table, b"NODE")
    b = bytearray(good); struct.pack_into("<i", b, at[b"NODE"] + 8, 12); cases["NODE chunk (a node's record)#ids"] = reseal(b, table, b"NODE")  # ids not ascending
    b = bytearray(good); struct.pack_into("<I", b, at[b"CONF"] + 8, 1); cases["node kinds differ"] = reseal(b, table, b"CONF")
    b = bytearray(good); struct.pack_into("<i", b, at[b"DETE"] + 20, 4); cases["DETE chunk"] = reseal(b, table, b"DETE")
    b = bytearray(good); struct.pack_into("<d", b, at[b"DETE"] + 24, float("nan")); cases["threshold is not finite"] = reseal(b, table, b"DETE")
    b = bytearray(good); struct.pack_into("<i", b, at[b"CLOU"] + 8 + 4, 3); cases["CLOU chunk"] = reseal(b, table, b"CLOU")   # rows 3: more points than there are
    b = bytearray(good); struct.pack_into("<I", b, at[b"GRPH"] + 24 + 12, 9); cases["GRPH chunk"] = reseal(b, table, b"GRPH")  # n_edges, its own CRC now wrong
    swapped = sf.assemble(sf.CLOUDS, [(t, good[o:o + n]) for t, o, n in (table[1], table[0]) + tuple(table[2:-1])])
    cases["out of order"] = swapped
    cases["mandatory chunk"] = sf.assemble(0, [(t, good[o:o + n]) for t, o, n in table[:2]])
    names = list(cases)
    lines = run(prog, tmp_path, [cases[n] for n in names])
    for n, line in zip(names, lines):
        assert line.startswith("bad ") and n.split("#")[0] in line, (n, line)
