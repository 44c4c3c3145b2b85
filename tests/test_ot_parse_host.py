"""CPU: the host-side .ot reader behind rgbdfe_octomap_read (csrc/ot_parse.h) as a stand-alone program
(tests/emu/ot_parse_main.cpp) built with the address and undefined-behaviour sanitizers: files of the oracle are read back
to their leaves, and every malformed file -- each refusal of the contract, and a good file cut at every length -- is
refused with a message and without a sanitizer report."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import octomap_tree_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = dict(to.planted_sets())


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("ot_parse")
    exe = os.path.join(d, "ot_parse_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"), "-I",
           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "ot_parse_main.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the answers
        subprocess.run(cmd, check=True)
    return exe


def run(prog, tmp_path, blobs, res="0.05"):
    paths = []
    for i, b in enumerate(blobs):
        p = tmp_path / ("f%05d.ot" % i)
        p.write_bytes(b)
        paths.append(str(p))
    r = subprocess.run([prog, res] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(blobs)
    return lines


def digest(leaves):
    """The program's digest of the leaves in file order."""
    w = np.frombuffer(leaves.tobytes(), "<u8").reshape(-1, 2)
    mul = (2 * np.arange(len(w), dtype=np.uint64) + np.uint64(1))
    x = np.bitwise_xor.reduce(w * mul[:, None], axis=0) if len(w) else np.zeros(2, np.uint64)
    return "%016x" % int(x[0] ^ x[1])


def test_files_of_the_oracle_come_back_as_their_leaves(prog, tmp_path):
    names = list(PLANTED)
    blobs = [to.ot_file(to.LiteralTree(PLANTED[n]).records(), 0.05) for n in names] + [to.header(0, 0.05)]
    lines = run(prog, tmp_path, blobs)
    for n, line in zip(names, lines):
        leaves = PLANTED[n]
        in_file_order = leaves[np.argsort(to.path_codes(leaves["key"]), kind="stable")]
        assert line == "ok %d %s" % (len(leaves), digest(in_file_order)), n
    assert lines[-1] == "ok 0 %016x" % 0


def test_every_refusal_names_its_reason(prog, tmp_path):
    rec = to.LiteralTree(PLANTED["eight siblings"]).records()
    good = to.ot_file(rec, 0.05)
    pruned = rec[:16].copy()
    pruned["children"][15] = 0
    deep = rec.copy()
    deep["children"][16] = 1
    bad = [(good.replace(b"id ColorOcTree", b"id OcTree"), "id"), (good.replace(b"res 0.05", b"res 0.1"), "res"),
           (good[:-8], "truncated"), (good.replace(b"size 24", b"size 25"), "size"), (good.replace(b"size 24", b"size 23"), "size"),
           (good + b"\0" * 8, "size"), (to.ot_file(pruned, 0.05), "pruned"), (to.ot_file(deep, 0.05), "depth 16"),
           (good.replace(b"# Octomap OcTree file", b"# Octomap OcTree fila"), "first line"), (good.replace(b"size 24", b"size x"), "size"),
           (b"", "first line"), (good.replace(b"size 24\n", b""), "size")]
    lines = run(prog, tmp_path, [b for b, _ in bad])
    for (_, word), line in zip(bad, lines):
        assert line.startswith("refused: ") and word in line, (word, line)
    assert run(prog, tmp_path, [good], res="0.1")[0].startswith("refused: ") and run(prog, tmp_path, [good])[0].startswith("ok 8 ")


def test_a_good_file_cut_at_every_length_is_refused(prog, tmp_path):
    good = to.ot_file(to.LiteralTree(PLANTED["hierarchical average"]).records(), 0.05)
    lines = run(prog, tmp_path, [good[:k] for k in range(len(good))])
    assert all(l.startswith("refused: ") for l in lines)
