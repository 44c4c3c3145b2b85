"""CPU: the kernel SOURCE of csrc/octomap.hip run on the host (tests/emu/emu_octomap.cpp over the HIP-on-CPU vocabulary of
tests/emu/, one OS thread per HIP thread: the lanes of a workgroup race for the table's slots) against the scalar
restatement in tests/octomap_oracle.py, on the bytes of the sorted leaf records.  The radix sort of voxel_filter.hip cannot
run there and is replaced by a host stand-in; the device's roundings are not what this test sees -- that is
tests/test_gpu_octomap.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import octomap_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY, NO_LEAF = np.uint64(0xffffffffffffffff), np.uint32(0xffffffff)
CASES = {c[0]: c for c in oo.cases()}
NAMES = ["n 1 res 0.05 range -1", "n 65 res 0.05 range 2.8", "n 257 res 0.1 range -1", "n 1025 res 0.1 range 2.8",
         "n 3072 res 0.4 range -1", "n 3072 res 0.4 range 2.8", "planted res 0.05 range -1", "planted res 0.05 range 2.5",
         "planted res 0.25 range -1", "planted res 0.25 range 2.5", "all invalid", "empty",
         "other probabilities", "5000 in one cell", "two cells alternating", "white sequence", "far point into a free cell",
         "rigid 0", "rigid 1"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_octomap")
    lib = os.path.join(d, "libemu_octomap.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_octomap.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    L.emu_octomap.restype = ctypes.c_int
    L.emu_octomap.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                              ctypes.c_uint32] + [ctypes.c_void_p] * 4
    return L


def run(emu, case, cap, rehash=0):
    """(leaf records, (overflow, n_done, n_leaves)) of a case through the kernels."""
    _, prm, ins = case
    m = oo.LiteralMap(**prm)  # for the parameters as the host derives them
    mr = {float(i[2]) for i in ins}
    assert len(mr) == 1  # one range per call, as in the C ABI
    pts = np.ascontiguousarray(np.concatenate([np.asarray(i[0], np.float32).reshape(-1, 4) for i in ins] + [np.zeros((1, 4), np.float32)]))
    counts = np.array([len(i[0]) for i in ins], np.int32)
    Ts = np.ascontiguousarray(np.stack([np.asarray(i[1], np.float32) for i in ins]))
    p = np.array([m.res, mr.pop(), m.hit, m.miss, m.cmin, m.cmax], np.float64)
    n = max(cap, rehash)
    key, value, colour, ctl = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(3, np.uint32)
    slots = emu.emu_octomap(pts.ctypes.data, counts.ctypes.data, len(ins), Ts.ctypes.data, p.ctypes.data, cap, rehash,
                            key.ctypes.data, value.ctypes.data, colour.ctypes.data, ctl.ctypes.data)
    key, value, colour = key[:slots], value[:slots], colour[:slots]
    leaf = (key != EMPTY) & (value != NO_LEAF)
    recs = oo.records([(int(k), v, ((c >> 16) & 255, (c >> 8) & 255, c & 255))
                       for k, v, c in zip(key[leaf], value[leaf].view(np.float32), colour[leaf].astype(np.int64))])
    return recs, tuple(int(v) for v in ctl)


@pytest.mark.parametrize("name", NAMES)
def test_the_kernels_give_the_oracles_bytes(emu, name):
    case = CASES[name]
    ref = oo.run(case).leaves()
    got, ctl = run(emu, case, len(ref) + len(ref) // 4 + 8)
    assert ctl == (0, len(case[2]), len(ref))
    assert got.tobytes() == ref.tobytes()


def test_a_full_table_a_cloud_that_does_not_fit_and_the_move_to_another_table(emu):
    a, b = oo.cloud(255, seed=7), oo.cloud(257, seed=8)
    T0, T1 = oo.translation(), oo.shifted(oo.translation(), 0.7)
    one = ("one", dict(resolution=0.1), [(a, T0, 2.8)])
    two = ("two", dict(resolution=0.1), [(a, T0, 2.8), (b, T1, 2.8), (a, T0, 2.8)])
    ref1, ref2 = oo.run(one).leaves(), oo.run(two).leaves()
    assert len(ref2) > len(ref1)
    got, ctl = run(emu, two, len(ref2))  # filled to the last slot: the probes wrap around the end
    assert ctl == (0, 3, len(ref2)) and got.tobytes() == ref2.tobytes()
    # the second cloud does not fit: it and the third change nothing, and only the leaves move to the next table
    got, ctl = run(emu, two, (len(ref1) + len(ref2)) // 2)
    assert ctl == (1, 1, len(ref1)) and got.tobytes() == ref1.tobytes()
    got, ctl = run(emu, two, (len(ref1) + len(ref2)) // 2, rehash=len(ref1))
    assert ctl == (1, 1, len(ref1)) and got.tobytes() == ref1.tobytes()
    got, ctl = run(emu, two, len(ref2) + 5, rehash=3 * len(ref2))
    assert ctl == (0, 3, len(ref2)) and got.tobytes() == ref2.tobytes()
