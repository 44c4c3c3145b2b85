"""CPU: the parts of include/rgbdfe.hpp that need no device -- inverse4, toMatchingResult, displayTypeFromParameter -- through
tests/cpp/header_host_main.cpp, built twice: plain, and as a stand-alone program with the address and undefined-behaviour
sanitizers (nothing of it is loaded into Python, nothing runs on a GPU).

inverse4 is compared with numpy.linalg.inv in float64 under a bound that is derived, not measured: per entry
|got - inv64| <= 2^-24 |inv64| + 64 kappa 2^-53 max|inv64|.  The first term is the final rounding to float; the second is the
error of an elimination in double with partial pivoting, kappa eps relative to the largest entry, with a margin of 64.  The
inputs have kappa < 1e6, so that the second term stays below the rounding of the largest entry (64e6 2^-53 < 2^-24)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("header_host_" + request.param) / "header_host_main")
    cmd = ["g++", "-std=c++14", "-O1", "-g", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "header_host_main.cpp"), "-o", exe]
    if request.param == "sanitized":
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def inverse_inputs():
    """(name, 4 x 4 float32 (row, column)) pairs."""
    rng = np.random.default_rng(41)
    out = [("identity", np.eye(4, dtype=np.float32))]
    for k in range(40):   # rigid transforms: random rotations, translations of up to 10 m
        T = np.eye(4)
        T[:3, :3] = rotation(rng)
        T[:3, 3] = rng.uniform(-10, 10, 3)
        out.append(("rigid %d" % k, T.astype(np.float32)))
    # row r has its entry in column r - 1 (cyclically): the pivot of every elimination step sits below the diagonal, so each
    # of the three steps that can swap rows does
    P = np.zeros((4, 4), np.float32)
    for c, v in enumerate((2.0, 3.0, 5.0, 7.0)):
        P[(c + 1) % 4, c] = v
    out.append(("permutation", P))
    A = np.eye(4)
    A[:3, :3] = rotation(rng) @ np.diag([0.5, 2.0, 3.0]) @ rotation(rng)
    A[:3, 3] = [4.0, -7.0, 1.5]
    out.append(("scaled affine", A.astype(np.float32)))
    return out


def test_inverse4(prog, tmp_path):
    cases = inverse_inputs()
    mats = np.stack([m for _, m in cases])
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(mats.transpose(0, 2, 1)).tofile(inp)   # column-major
    run(prog, "inverse", inp, outp)
    got = np.fromfile(outp, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)
    assert len(got) == len(cases)
    for (name, m), g in zip(cases, got):
        m64 = m.astype(np.float64)
        kappa = np.linalg.cond(m64)
        assert kappa < 1e6 and 64 * kappa * 2.0 ** -53 < 2.0 ** -24, (name, kappa)
        want = np.linalg.inv(m64)
        bound = 2.0 ** -24 * np.abs(want) + 64 * kappa * 2.0 ** -53 * np.abs(want).max()
        err = np.abs(g.astype(np.float64) - want)
        assert (err <= bound).all(), (name, float((err - bound).max()))
    assert np.array_equal(got[0], np.eye(4, dtype=np.float32))
    # the inverse of a rigid transform is (R^T, -R^T t): a transposed result would not pass the bound, and would not be this
    R, t = mats[1][:3, :3].astype(np.float64), mats[1][:3, 3].astype(np.float64)
    assert np.abs(got[1][:3, 3] - (-R.T @ t)).max() < 1e-5 and np.abs(got[1][3, :3]).max() == 0


def test_to_matching_result(prog):
    recs = {r["name"]: r for r in (json.loads(l) for l in run(prog, "records").splitlines())}
    assert list(recs) == ["no edge", "edge", "float distances", "full"]
    eye = np.eye(4).reshape(16).tolist()
    f32 = lambda v: float(np.float32(v))
    r = recs["no edge"]
    assert (r["id1"], r["id2"], r["rmse"], r["info"]) == (-1, -1, 0.5, 0.0)   # informationScale only with an edge
    assert r["all"] == [[5, 1, -1, 0.0], [6, 2, -1, 0.5], [7, 3, -1, f32(255 / 256)]]
    assert r["inliers"] == [[5, 1, 0.0], [7, 3, f32(255 / 256)]]
    assert r["ransac"] == r["final"] == [float(i + 1) for i in range(16)]
    assert r["icp"] == eye and r["edge"] == eye and r["points"] == [0, 0, 0, 0]
    r = recs["edge"]
    trafo = [f32(np.float32(0.1) * np.float32(i + 1)) for i in range(16)]
    assert (r["id1"], r["id2"], r["rmse"], r["info"]) == (3, 9, 0.25, 123.5)
    assert r["all"] == [[1000 + m, 2000 - m, -1, f32(m / 256)] for m in range(70)]
    assert r["inliers"] == [[1000 + m, 2000 - m, f32(m / 256)] for m in (63, 64, 69)]   # either side of the mask word's end
    # (%.9g identifies a float: read back as float32)
    assert [f32(v) for v in r["ransac"]] == [f32(v) for v in r["final"]] == trafo and r["icp"] == eye
    assert r["edge"] == trafo   # the float values as doubles (node.cpp:1339), printed with %.17g
    r = recs["float distances"]
    assert r["all"] == [[1000 + m, 2000 - m, -1, 0.5 + 0.25 * m] for m in range(70)]
    assert r["inliers"] == [[1000 + m, 2000 - m, 0.5 + 0.25 * m] for m in (63, 64, 69)]
    r = recs["full"]
    assert len(r["all"]) == len(r["inliers"]) == 320   # RGBDFE_MAX_MATCHES
    assert r["all"] == [[m, 65535 - m, -1, f32((m & 255) / 256)] for m in range(320)]
    assert r["inliers"] == [a[:2] + a[3:] for a in r["all"]]


def test_display_type_from_parameter(prog):
    # RGBDFE_DISPLAY_POINTS 0, _TRIANGLES 1, _TRIANGLE_STRIP 2; anything else is a strip (glviewer.cpp:708)
    assert run(prog, "display").split() == ["0", "1", "2", "2"]
