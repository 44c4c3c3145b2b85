"""CPU: the source of node_pack_kernel (csrc/session.hip) run on the host (tests/emu/emu_session.cpp over the HIP-on-CPU
vocabulary of tests/emu/, one OS thread per HIP thread) against a numpy gather, on the shapes of tests/test_gpu_session.py:
130 rows per slot (a slot's counters end inside a word, the counter stride is 132), nodes of 0, 1, 63, 64, 65 and 130 rows
in slots out of order, so that the rows in front of a node are odd (KeyPoint.pt half a 16-byte unit off) and the counters
of a node start on every byte of a word."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_KP, STRIDE, N_SLOTS = 130, 132, 24
POISON = 0xA5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_session")
    lib = os.path.join(d, "libemu_session.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_session.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.emu_node_pack.restype = ctypes.c_int
    L.emu_node_pack.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp, u32, u32, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def slabs():
    """Every byte of every slab random, the rows beyond a node's included: a gather that reads a wrong row shows."""
    rng = np.random.default_rng(11)
    rows = N_SLOTS * MAX_KP
    return {"orb": rng.integers(0, 256, (rows, 32), np.uint8), "f32": rng.standard_normal((rows, 128)).astype(np.float32),
            "xyz": rng.standard_normal((rows, 4)).astype(np.float32), "kp": rng.standard_normal((rows, 2)).astype(np.float32),
            "stats": rng.integers(1, 256, (N_SLOTS, STRIDE), np.uint8)}


def ptr(a):
    return None if a is None else a.ctypes.data


def pack(emu, slabs, nodes, desc="orb", outputs=("desc", "xyz", "kp", "stats"), have_kp_slab=True, have_stats_slab=True, tail=7):
    """nodes: (slot, rows, has_kp) in list order.  Returns nothing: asserts every packed array against the gather, and that
    the `tail` rows behind the total keep their poison."""
    first = np.concatenate([[0], np.cumsum([r for _, r, _ in nodes])]).astype(np.int64)
    total = int(first[-1])
    table = np.array([[s, r, first[i], k] for i, (s, r, k) in enumerate(nodes)], np.uint32).reshape(-1, 4)
    src = slabs[desc]
    width = {"desc": src.shape[1] * src.itemsize, "xyz": 16, "kp": 8, "stats": 1}
    out = {k: (np.full((total + tail) * width[k], POISON, np.uint8) if k in outputs else None) for k in width}
    launches = emu.emu_node_pack(ptr(table), len(nodes), max([r for _, r, _ in nodes], default=0), ptr(src),
                                 src.shape[1] * src.itemsize // 16, ptr(slabs["xyz"]), ptr(slabs["kp"]) if have_kp_slab else None,
                                 ptr(slabs["stats"]) if have_stats_slab else None, MAX_KP, STRIDE, ptr(out["desc"]), ptr(out["xyz"]),
                                 ptr(out["kp"]), ptr(out["stats"]))
    assert launches == (1 if total else 0)   # one launch whatever the number of nodes
    want = {k: [] for k in width}
    for s, r, k in nodes:
        sl = slice(s * MAX_KP, s * MAX_KP + r)
        want["desc"].append(src[sl].tobytes())
        want["xyz"].append(slabs["xyz"][sl].tobytes())
        want["kp"].append(slabs["kp"][sl].tobytes() if (k and have_kp_slab) else bytes(8 * r))
        want["stats"].append(slabs["stats"][s, :r].tobytes() if have_stats_slab else bytes(r))
    for k in outputs:
        got = out[k].tobytes()
        assert got[:total * width[k]] == b"".join(want[k]), k
        assert got[total * width[k]:] == bytes([POISON]) * (tail * width[k]), k + ": written beyond the last row"


# ids 5, 0, 23, 7, 11, 2 of the GPU test, asked for in neither id nor slot order
ORB_NODES = [(9, 65, 1), (23, 0, 0), (0, 130, 1), (4, 1, 0), (17, 63, 1), (2, 64, 0)]


def test_orb_nodes_every_array(emu, slabs):
    pack(emu, slabs, ORB_NODES)


@pytest.mark.parametrize("outputs", [("desc",), ("xyz",), ("kp",), ("stats",), ("desc", "stats"), ("xyz", "kp"), ()])
def test_null_outputs_are_left_out(emu, slabs, outputs):
    pack(emu, slabs, ORB_NODES, outputs=outputs)


def test_slabs_never_allocated_read_as_zeros(emu, slabs):
    pack(emu, slabs, ORB_NODES, have_kp_slab=False, have_stats_slab=False)


def test_float_nodes(emu, slabs):
    pack(emu, slabs, [(3, 65, 1), (21, 1, 0), (8, 64, 1)], desc="f32")


def test_one_node_of_every_size(emu, slabs):
    for rows in (1, 63, 64, 65, 130):
        pack(emu, slabs, [(N_SLOTS - 1, rows, 1)])


def test_a_node_listed_twice_and_a_list_of_empty_nodes(emu, slabs):
    pack(emu, slabs, [(6, 65, 1), (6, 65, 1), (1, 3, 0)])
    pack(emu, slabs, [(6, 0, 1), (1, 0, 0)])
    pack(emu, slabs, [])
