"""CPU: the kernel SOURCE of csrc/icp.hip run on the host (tests/emu/emu_icp.cpp over the HIP-on-CPU vocabulary of
tests/emu/, one OS thread per HIP thread) against tests/icp_oracle.py: the valid-row compaction and the gather of
filterCloud, one iteration of every planted case (the correspondences, the working copy, the increment, the record) and the
whole job, driven in the chunks api_icp.hip uses -- bytes equal to the oracle's.  The device itself is
tests/test_gpu_icp.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = io.planted_cases()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("emu_icp")
    lib = os.path.join(d, "libemu_icp.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-attributes",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "emu_icp.cpp"), "-o", lib],
                   check=True)
    L = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    L.emu_icp_filter.restype = ctypes.c_int
    L.emu_icp_filter.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_int32, vp, vp]
    L.emu_icp_job.restype = ctypes.c_int
    L.emu_icp_job.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int32, vp] + [ctypes.c_double] * 3 + [ctypes.c_int32] * 2 + [vp] * 5
    return L


def emu_filter(emu, cloud, desired_size):
    cloud = np.ascontiguousarray(cloud, np.float32)
    n = len(cloud)
    n_valid = emu.emu_icp_filter(cloud.ctypes.data, n, None, 0, 0, None, None)
    pos = io.sample_positions(n_valid, desired_size).astype(np.uint32)
    rows, idx = np.zeros((len(pos) + 1, 4), np.float32), np.zeros(len(pos) + 1, np.uint32)
    pos_arg = np.append(pos, 0).astype(np.uint32)
    out = []
    for poison in (0, 1):
        assert emu.emu_icp_filter(cloud.ctypes.data, n, pos_arg.ctypes.data, len(pos), poison, rows.ctypes.data,
                                  idx.ctypes.data) == n_valid
        out.append(rows[:len(pos)].copy())
    return n_valid, idx[:len(pos)], out[0], out[1]


def emu_job(emu, S, T, G, prm, limit):
    S, T = np.ascontiguousarray(S, np.float32), np.ascontiguousarray(T, np.float32)
    ns, nt = len(S), len(T)
    G = np.eye(4, dtype=np.float32) if G is None else np.asarray(G, np.float32)
    G12 = np.ascontiguousarray(np.concatenate([G[:3, :3].reshape(9), G[:3, 3]]).astype(np.float32))
    rec = np.zeros(29)
    nn_j, nn_d2, P = np.full(ns + 1, -7, np.int32), np.zeros(ns + 1, np.float32), np.zeros((ns + 1, 4), np.float32)
    chunks = ctypes.c_int32(0)
    launches = emu.emu_icp_job(S.ctypes.data, ns, T.ctypes.data, nt, G12.ctypes.data, prm["max_correspondence_distance"],
                               prm["transformation_epsilon"], prm["euclidean_fitness_epsilon"], prm["max_iterations"], limit,
                               rec.ctypes.data, nn_j.ctypes.data, nn_d2.ctypes.data, P.ctypes.data, ctypes.byref(chunks))
    return dict(mse=rec[0], R=rec[1:10].astype(np.float32).reshape(3, 3), t=rec[10:13].astype(np.float32),
                FR=rec[13:22].astype(np.float32).reshape(3, 3), Ft=rec[22:25].astype(np.float32), done=int(rec[25]),
                state=int(rec[26]), k=int(rec[27]), c=int(rec[28]), nn_j=nn_j[:ns], nn_d2=nn_d2[:ns], P=P[:ns],
                launches=launches, chunks=chunks.value)


def same(a, b, dtype):
    return np.asarray(a, dtype).tobytes() == np.asarray(b, dtype).tobytes()


def expected_chunks(k):
    """Record reads of a job that stops at iteration k under chunks of 2, 4, 8, 16, 16 ..."""
    done, chunk, reads = 0, 2, 0
    while done < k:
        done += chunk
        reads += 1
        chunk = min(2 * chunk, 16)
    return reads, done


@pytest.mark.parametrize("name", ["desired_size above |V|", "desired_size far below |V|", "non-finite rows", "sizes 257 x 1"])
def test_compaction_and_gather_give_filter_clouds_rows(emu, name):
    case = CASES[name]
    for cloud in (case["source"], case["target"]):
        idx, rows = io.filter_cloud(cloud, case["params"]["desired_size"])
        n_valid, got_idx, got_rows, poisoned = emu_filter(emu, cloud, case["params"]["desired_size"])
        assert n_valid == int((~np.isnan(np.asarray(cloud)[:, 2])).sum())
        assert np.array_equal(got_idx, idx) and same(got_rows, rows, np.float32)
        assert same(poisoned, io.poisoned(rows), np.float32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_iteration_gives_the_oracles_bytes(emu, name):
    case = CASES[name]
    prm = case["params"]
    ref = io.reference(name, trace=True)
    _, S = io.filter_cloud(case["source"], prm["desired_size"])
    _, T = io.filter_cloud(case["target"], prm["desired_size"])
    got = emu_job(emu, io.poisoned(S), io.poisoned(T), case["G"], prm, 1)
    assert got["k"] == 1 and got["launches"] == (2 if len(S) else 1)
    first = io.align_sampled(S, T, case["G"], True, **dict(prm, max_iterations=1)) if ref["iterations"] > 1 else ref
    assert same(got["nn_j"], first["nn_j"], np.int32) and same(got["nn_d2"], first["nn_d2"], np.float32)
    assert got["c"] == first["c"] and same(got["mse"], first["mse"], np.float64)
    if first["trace"]:
        tr = first["trace"][0]
        assert same(got["P"], tr["P"], np.float32)   # the working copy G S; the increment is applied at the next load
        assert same(got["R"], tr["R"], np.float32) and same(got["t"], tr["t"], np.float32)
        assert same(got["FR"], first["T"][:3, :3], np.float32) and same(got["Ft"], first["T"][:3, 3], np.float32)
        state = ref["trace"][0]["state"]   # under the case's own max_iterations
        assert got["state"] == state and got["done"] == (1 if state else 0)
    else:
        assert got["state"] == io.NO_CORRESPONDENCES and got["done"] == 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_whole_job_gives_the_oracles_bytes(emu, name):
    case = CASES[name]
    prm = case["params"]
    ref = io.reference(name)
    _, S = io.filter_cloud(case["source"], prm["desired_size"])
    _, T = io.filter_cloud(case["target"], prm["desired_size"])
    got = emu_job(emu, io.poisoned(S), io.poisoned(T), case["G"], prm, prm["max_iterations"])
    assert (got["state"], got["k"], got["c"], got["done"]) == (ref["state"], ref["iterations"], ref["c"], 1)
    assert same(got["mse"], ref["mse"], np.float64)
    assert same(got["nn_j"], ref["nn_j"], np.int32) and same(got["nn_d2"], ref["nn_d2"], np.float32)
    if ref["converged"]:
        assert same(got["FR"], ref["T"][:3, :3], np.float32) and same(got["Ft"], ref["T"][:3, 3], np.float32)
    reads, enqueued = expected_chunks(ref["iterations"])
    enqueued = min(enqueued, prm["max_iterations"])
    assert got["chunks"] == reads and got["launches"] == enqueued * (2 if len(S) else 1)
