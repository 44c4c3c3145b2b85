"""CPU: the source of cloud_pack_ply_kernel (csrc/map_files.hip) run on the host (tests/emu/emu_map_files.cpp over the
HIP-on-CPU vocabulary of tests/emu/, one OS thread per HIP thread) against the numpy packing of tests/cloud_file_oracle.py:
sizes either side of a quad, a wave, a workgroup and the kernel's tile, with and without a carry, into a poisoned slot."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_file_oracle as co
from test_oracle_cloud_file import cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_map_files")
    lib = os.path.join(d, "libemu_map_files.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_map_files.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.emu_cloud_pack_ply.restype = u32
    L.emu_cloud_pack_ply.argtypes = [vp, u32, vp, u32, ctypes.c_int, vp, vp]
    L.emu_ply_pack_tile.restype = u32
    return L


def pack(emu, carry, body, final):
    """Runs the kernel; checks the slot and the carry; returns (packed rows, the vertex bytes, the rows left over)."""
    rows = np.concatenate([carry, body])
    total = len(rows)
    packed = total if final else total & ~3
    words = (15 * packed + 3) // 4
    slot = np.full(4 * words + 64, POISON, np.uint8)
    carry_out = np.full((3, 4), np.float32(-7.0))
    carry_in = np.ascontiguousarray(np.concatenate([carry, np.full((3 - len(carry), 4), np.float32(9.0))]))   # rows behind n_carry: never read
    body = np.ascontiguousarray(body)
    got = emu.emu_cloud_pack_ply(carry_in.ctypes.data, len(carry), body.ctypes.data if len(body) else None, len(body), int(final),
                                 slot.ctypes.data, carry_out.ctypes.data)
    assert got == packed
    data = slot.tobytes()
    assert data[:15 * packed] == co.pack_ply(rows[:packed])
    assert data[15 * packed:4 * words] == bytes(4 * words - 15 * packed)           # up to the end of the last whole word: zeros
    assert data[4 * words:] == bytes([POISON]) * 64                                 # behind it: untouched
    left = total - packed
    assert carry_out[:left].tobytes() == rows[packed:].tobytes()
    assert np.all(carry_out[left:] == np.float32(-7.0))
    return packed, data[:15 * packed], rows[packed:]


def sizes(emu):
    t = emu.emu_ply_pack_tile()
    return [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1]


def test_the_last_group_packs_every_row(emu):
    assert emu.emu_ply_pack_tile() == 1024
    for n in sizes(emu):
        pack(emu, np.zeros((0, 4), np.float32), cloud(n, n), final=True)


def test_a_group_in_the_middle_packs_whole_quads_and_carries_the_rest(emu):
    for n in sizes(emu):
        for c in (0, 1, 3):
            pack(emu, cloud(c, 50 + c), cloud(n, n), final=False)


def test_carry_into_the_last_group(emu):
    for n in (0, 1, 4, 1024, 2049):
        pack(emu, cloud(3, 9), cloud(n, n), final=True)


def test_groups_chained_through_their_carries_give_the_vertices_of_the_whole(emu):
    pts = cloud(1024 + 700, 4)
    cuts = [0, 1, 2, 2, 7, 70, 1094, 1095, len(pts)]   # a group of no row, groups that stay below a quad, one over a tile
    carry = np.zeros((0, 4), np.float32)
    out = b""
    for g in range(len(cuts) - 1):
        _, data, carry = pack(emu, carry, pts[cuts[g]:cuts[g + 1]], final=(g == len(cuts) - 2))
        out += data
    assert out == co.pack_ply(pts)
