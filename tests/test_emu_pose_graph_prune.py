"""CPU: the source of pg_prune_kernel (csrc/pose_graph.hip) run on the host (tests/emu/emu_pose_graph_prune.cpp over the
HIP-on-CPU vocabulary of tests/emu/, one OS thread per HIP thread) against tests/pose_graph_eval_oracle.py: the verdict bytes,
the count, the patched measurements and information matrices and the active gates; then pg_edges_kernel on the patched
arrays, whose gate must leave rho 0 in a removed edge's place of the chi2 tree and write no record for it."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_graph_eval_oracle as pe
import pose_graph_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPO_SEQUENTIAL, TOPO_BOTH_JOINED = 1, 2


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_pose_graph_prune")
    lib = os.path.join(d, "libemu_pose_graph_prune.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_pose_graph_prune.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    L.emu_pose_graph_prune.restype = ctypes.c_int
    L.emu_pose_graph_prune.argtypes = [ctypes.c_int32] * 2 + [ctypes.c_void_p] * 5 + [ctypes.c_double] + [ctypes.c_void_p] * 4
    return L


def device_arrays(g):
    ei, ej, ZR, Zt, Om = g.arrays()
    E = len(ei)
    edge_ij = np.ascontiguousarray(np.stack([ei, ej], axis=1).astype(np.int32))
    edge_in = np.ascontiguousarray(np.concatenate([ZR.reshape(E, 9), Zt, Om.reshape(E, 36)], axis=1))
    degree = np.bincount(np.concatenate([ei, ej]), minlength=g.n)
    topo = (np.where(np.abs(ei - ej) == 1, TOPO_SEQUENTIAL, 0) | np.where((degree[ei] > 1) & (degree[ej] > 1), TOPO_BOTH_JOINED, 0))
    est = np.ascontiguousarray(np.concatenate([g.R.reshape(g.n, 9), g.t], axis=1))
    return edge_ij, edge_in, np.array(g.active, np.int32), topo.astype(np.uint8), est


def run(emu, g, thresh):
    edge_ij, edge_in, active, topo, est = device_arrays(g)
    E = len(g.ei)
    verdict = np.full(E, 77, np.uint8)
    head = np.full((E, 9), -7.0)
    count, chi2 = ctypes.c_int32(-1), ctypes.c_double(-1.0)
    p = lambda a: a.ctypes.data
    launches = emu.emu_pose_graph_prune(g.n, E, p(edge_ij), p(edge_in), p(active), p(topo), p(est), float(np.float32(thresh)),
                                        p(verdict), ctypes.byref(count), p(head), ctypes.byref(chi2))
    assert launches == 3
    return dict(edge_in=edge_in, active=active, verdict=verdict, count=count.value, head=head, chi2=chi2.value)


def check(emu, g, thresh):
    got = run(emu, g, thresh)              # from g as it is ...
    count, verdicts = pe.prune_edges(g, thresh)   # ... then the oracle moves g on
    assert got["count"] == count and got["verdict"].tobytes() == verdicts.tobytes()
    _, want_in, want_active, _, _ = device_arrays(g)
    assert got["edge_in"].tobytes() == want_in.tobytes() and got["active"].tobytes() == want_active.tobytes()
    # the per-edge kernel on the patched arrays
    errs = pe.edge_errors(g)
    lin_rho = pe.over_slots(g, pe.active_view(g)[1], po.edge_terms(pe.active_view(g)[0], g.R, g.t, False)["rho"]
                            if any(g.active) else [])
    on = np.array(g.active, bool)
    assert got["head"][on, 6].tobytes() == errs["chi2"][on].tobytes() and got["head"][on, 7].tobytes() == lin_rho[on].tobytes()
    assert (got["head"][~on] == -7.0).all()   # no record written
    assert np.float64(got["chi2"]).tobytes() == pe.chi2(g).tobytes()
    return count


@pytest.mark.parametrize("name", [c[0] for c in pe.VERDICT_CASES])
def test_the_prune_kernel_gives_the_oracles_bytes(emu, name):
    g, _, calls = pe.verdict_case(name)
    for thresh, count, _ in calls:
        assert check(emu, g, thresh) == count


@pytest.mark.parametrize("s", [5.0, 1.0, 0.25])
def test_the_threshold_is_strict(emu, s):
    assert check(emu, pe.threshold_graph(s), s) == 0
    assert check(emu, pe.threshold_graph(np.nextafter(s, 10.0)), s) == 1


def test_removed_slots_at_the_ends_of_the_trees_leaves(emu):
    g = pe.slots_graph_129()
    assert check(emu, g, 5.0) == 4 and [e for e in range(129) if not g.active[e]] == list(pe.SLOTS_129)
    assert check(emu, g, 0.25) >= 0   # a second call passes the inactive slots by
