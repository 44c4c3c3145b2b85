"""CPU: the layout type behind the host code's device scratch and staging (csrc/device_layout.h) as a stand-alone program
(tests/emu/device_layout_main.cpp) built with the address and undefined-behaviour sanitizers: every block is 256-aligned and
written end to end into a heap block of exactly the layout's total, the uploaded blocks sit in the staging vector at their own
offsets, the sort workspace follows launch_vox_sort's rule, and rgbdfe_project_to_3d's blocks land where its hand-written
sums put them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("device_layout")
    exe = os.path.join(d, "device_layout_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
           os.path.join(ROOT, "tests", "emu", "device_layout_main.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the answers
        subprocess.run(cmd, check=True)
    return exe


def up(b):
    return (b + 255) // 256 * 256


def run(prog, *args):
    """(blocks as (offset, bytes), total, the staging vector or None)"""
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    blocks = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("block ")]
    total = [int(l.split()[1]) for l in lines if l.startswith("total ")]
    assert len(total) == 1 and "written ok" in lines, r.stdout[-2000:]
    staged = [bytes.fromhex(l[len("staged "):]) for l in lines if l.startswith("staged")]
    return blocks, total[0], staged[0] if staged else None


def check_carving(blocks, sizes, total):
    """256-aligned, in the order of the requests, disjoint, each as large as its rounded request, the last ends at the total"""
    assert [b for _, b in blocks] == list(sizes)
    at = 0
    for off, b in blocks:
        assert off % 256 == 0 and off == at
        at += up(b)
    assert total == at


@pytest.mark.parametrize("sizes", [(1,), (256,), (257, 1, 255, 512, 3), (24, 16, 12, 48, 256), (100000, 7), ()])
def test_blocks_are_aligned_disjoint_and_end_at_the_total(prog, sizes):
    blocks, total, staged = run(prog, "layout", *["r%d" % s for s in sizes])
    check_carving(blocks, sizes, total)
    assert staged == b""


def test_a_zero_byte_block_takes_no_room(prog):
    with_zero, total_z, _ = run(prog, "layout", "r10", "r0", "r300", "r0", "r0", "r1")
    without, total, _ = run(prog, "layout", "r10", "r300", "r1")
    check_carving(with_zero, (10, 0, 300, 0, 0, 1), total_z)
    assert [b for b in with_zero if b[1]] == without and total_z == total
    assert run(prog, "layout", "r0")[1] == 0 and run(prog, "layout", "p0", "r0")[1:] == (0, b"")


def test_uploaded_blocks_are_staged_at_their_own_offsets(prog):
    sizes = (5, 256, 0, 300, 1)
    blocks, total, staged = run(prog, "layout", *["p%d" % s for s in sizes], "r1000", "r3")
    check_carving(blocks, sizes + (1000, 3), total)
    expect = b"".join(bytes([i + 1]) * s + b"\0" * (up(s) - s) for i, s in enumerate(sizes))
    assert staged == expect and len(staged) == blocks[len(sizes)][0]  # the uploaded prefix ends where the working blocks begin


@pytest.mark.parametrize("n", [0, 1, 4096, 4097])
def test_the_sort_workspace_follows_the_rule_of_launch_vox_sort(prog, n):
    blocks, total, _ = run(prog, "sort", n)
    tiles = (n + 4095) // 4096
    sizes = (4 * n, 4 * n, 4 * n, 4 * n, 4 * 256 * tiles, 1024)
    check_carving(blocks, sizes, total)
    assert total == 4 * up(4 * n) + up(4 * 256 * tiles) + 1024  # what api_voxel.hip wrote out: 4 * b_pairs + b_hist + b_digits


def test_project_to_3d_keeps_its_offsets(prog):
    n_kp, rows, cols = 3, 2, 2   # rgbdfe_project_to_3d: keypoints, depth image, kept indices, points, the counter block
    blocks, total, _ = run(prog, "layout", "r%d" % (n_kp * 8), "r%d" % (rows * cols * 4), "r%d" % (n_kp * 4), "r%d" % (n_kp * 16), "r256")
    assert [off for off, _ in blocks] == [0, 256, 512, 768, 1024] and total == 1280
