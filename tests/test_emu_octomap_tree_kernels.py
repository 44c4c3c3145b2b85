"""CPU: the kernel SOURCE of csrc/octomap_tree.hip run on the host (tests/emu/emu_octomap_tree.cpp over the HIP-on-CPU
vocabulary of tests/emu/, one OS thread per HIP thread) against tests/octomap_tree_oracle.py, on the bytes of the node
records and of one depth's records.  The radix sort of voxel_filter.hip cannot run there and is replaced by a host
stand-in; the device itself is tests/test_gpu_octomap_tree.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import octomap_oracle as oo
import octomap_tree_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = to.planted_sets()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_octomap_tree")
    lib = os.path.join(d, "libemu_octomap_tree.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_octomap_tree.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    L.emu_octomap_tree.restype = ctypes.c_int
    L.emu_octomap_tree.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_float] + \
        [ctypes.c_void_p] * 3
    return L


def run(emu, leaves, cap, depth, thr, seed=0):
    """(records, the records of `depth`, TreeHdr::cnt, launches) with the leaves in random slots of a table of cap."""
    rng = np.random.default_rng(seed)
    key = np.full(cap, 0xffffffffffffffff, np.uint64)
    value = np.full(cap, 0xffffffff, np.uint32)
    colour = np.full(cap, 0xffffffff, np.uint32)
    slots = rng.permutation(cap)[:len(leaves)]
    k = leaves["key"].astype(np.uint64)
    key[slots] = k[:, 0] | (k[:, 1] << np.uint64(16)) | (k[:, 2] << np.uint64(32))
    value[slots] = leaves["log_odds"].view(np.uint32)
    c = leaves["rgb"].astype(np.uint32)
    colour[slots] = (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    claimed = rng.permutation(np.setdiff1d(np.arange(cap), slots))[:3]  # claimed keys without a leaf are no leaves
    key[claimed] = np.uint64(5) + claimed.astype(np.uint64)
    rec = np.zeros(17 * len(leaves) + 1, to.NODE)
    level = np.zeros(len(leaves) + 1, oo.LEAF)
    n_nodes, n_level, cnt = ctypes.c_uint32(0), ctypes.c_uint32(0), np.zeros(17, np.uint32)
    launches = emu.emu_octomap_tree(key.ctypes.data, value.ctypes.data, colour.ctypes.data, cap, len(leaves), rec.ctypes.data,
                                    ctypes.byref(n_nodes), depth, thr, level.ctypes.data, ctypes.byref(n_level), cnt.ctypes.data)
    assert launches > 0
    assert not rec[n_nodes.value:].tobytes().strip(b"\0") and not level[n_level.value:].tobytes().strip(b"\0")
    return rec[:n_nodes.value], level[:n_level.value], cnt, launches


# one run per set (a run starts some 150 launches of up to 1024 OS threads each, ten seconds): three of the rule sets,
# and the two random sets that stop one element into a second wave and a second tile; the depth of the query changes
KEPT = {"one leaf": 16, "eight siblings": 15, "white subtree": 13, "random 257": 1, "random 1025": 12}
SETS = [(n, l, KEPT[n]) for n, l in PLANTED if n in KEPT]


@pytest.mark.parametrize("name,leaves,depth", SETS, ids=[s[0] for s in SETS])
def test_the_kernels_give_the_literal_trees_bytes(emu, name, leaves, depth):
    lit = to.LiteralTree(leaves)
    want = lit.records()
    lv = lit.at_depth(depth)
    thr = np.sort(lv["log_odds"])[len(lv) // 2]
    rec, level, cnt, launches = run(emu, leaves, len(leaves) + (7 if depth & 1 else 0), depth, thr, seed=depth)
    assert rec.tobytes() == want.tobytes()
    assert level.tobytes() == lv[lv["log_odds"] >= thr].tobytes()
    assert [int(c) for c in cnt] == [len(lit.at_depth(d)) for d in range(17)]
    assert launches == 3 + 20 + 3 + 1 + 48  # gather, sorts and arrange, chain, leaf records, levels: whatever the size
