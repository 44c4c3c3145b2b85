"""CPU: tests/render_oracle.py (the restatement the renderer is held against) against independent arithmetic.

* coverage and the fill rule against fractions.Fraction point-in-triangle tests on the snapped coordinates: fans of triangles
  around a vertex on a pixel centre, edges through centres, slivers, zero-area triangles; every sample inside a fan is covered
  exactly once;
* depth and colour against their closed forms in exact rational arithmetic on a slanted quad, with w = 1 and with perspective;
* the camera helpers against numpy compositions of the same elementary matrices, and the library's own helpers
  (csrc/render_camera.h compiled on the host, tests/emu/render_camera_host.cpp) against the Python ones, byte for byte;
* unproject(project(p)) against a numpy.linalg route: the one tolerance of the renderer's tests."""
import ctypes
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import display_oracle as do
import render_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vert(xw, yw, zw=0.5, w=1.0, word=0):
    return dict(ok_w=True, ok_z=True, in_xy=True, xw=float(xw), yw=float(yw), zw=float(zw), w=float(w), word=word)


# ---- coverage

def side(ax, ay, bx, by, px, py):
    """exact: > 0 when p is to the left of a -> b"""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def classify(X, Y, sx, sy):
    """'in' / 'edge' / 'out' of the sample against the closed counter-clockwise triangle, in exact integers"""
    s = [side(X[a], Y[a], X[b], Y[b], sx, sy) for a, b in ((0, 1), (1, 2), (2, 0))]
    if all(v > 0 for v in s):
        return "in"
    return "edge" if all(v >= 0 for v in s) else "out"


def fan_check(centre, ring, W=24, H=20, closed=True):
    """Triangles (centre, ring[i], ring[i + 1]), counter-clockwise.  Returns the number of samples that lay on a spoke or on
    the centre (each of which must have been covered exactly once)."""
    n = len(ring)
    tris = []
    for i in range(n if closed else n - 1):
        s = ro.triangle_setup([vert(*centre), vert(*ring[i]), vert(*ring[(i + 1) % n])], cull=1)
        if s is not None:
            tris.append(s)
    cx, cy = ro.snap(centre[0]), ro.snap(centre[1])
    spokes = [(ro.snap(r[0]), ro.snap(r[1])) for r in ring]
    shared = 0
    for py in range(H):
        for px in range(W):
            sx, sy = 256 * px + 128, 256 * py + 128
            covered = [ro.edge_values(X, Y, px, py)[1] for X, Y, _ in tris]
            kinds = [classify(X, Y, sx, sy) for X, Y, _ in tris]
            for c, k in zip(covered, kinds):
                assert not (k == "in" and not c) and not (k == "out" and c)
            assert sum(covered) <= 1, "a sample was covered twice"
            if "in" in kinds:
                assert sum(covered) == 1
                continue
            # on the centre, or strictly inside a spoke both of whose triangles exist: inside the fan, so exactly once
            on_spoke = (sx, sy) == (cx, cy) and closed
            for i, (rx, ry) in enumerate(spokes):
                inner = closed or 0 < i < n - 1
                if inner and side(cx, cy, rx, ry, sx, sy) == 0 and (sx, sy) not in ((cx, cy), (rx, ry)):
                    t = Fraction((sx - cx) * (rx - cx) + (sy - cy) * (ry - cy), (rx - cx) ** 2 + (ry - cy) ** 2)
                    on_spoke = on_spoke or 0 < t < 1
            if on_spoke and kinds.count("edge") >= 2:
                shared += 1
                assert sum(covered) == 1, "a sample on a shared edge belongs to exactly one triangle"
    return shared


def test_fan_around_a_vertex_on_a_pixel_centre_edges_through_centres():
    centre = (10.5, 9.5)
    ring = [(16.5, 9.5), (16.5, 15.5), (10.5, 15.5), (4.5, 15.5), (4.5, 9.5), (4.5, 3.5), (10.5, 3.5), (16.5, 3.5)]
    assert fan_check(centre, ring) >= 1 + 8 * 5  # the centre and five centres per spoke


def test_random_fans_and_slivers():
    rng = np.random.default_rng(5)
    shared = 0
    for trial in range(12):
        centre = (10.5, 9.5) if trial % 2 else (float(rng.integers(8 * 256, 12 * 256)) / 256, float(rng.integers(7 * 256, 11 * 256)) / 256)
        k = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * math.pi, k))
        if trial % 3 == 0:
            ang[1] = ang[0] + 1e-3  # a sliver
        if np.max(np.diff(np.concatenate([ang, [ang[0] + 2 * math.pi]]))) >= math.pi:
            continue  # (not a fan around the centre)
        rad = rng.uniform(2.0, 8.0, k)
        ring = [(centre[0] + r * math.cos(a), centre[1] + r * math.sin(a)) for r, a in zip(rad, ang)]
        shared += fan_check(centre, ring)
    assert shared >= 6


def test_zero_area_and_back_faces():
    collinear = [vert(2.5, 2.5), vert(6.5, 6.5), vert(10.5, 10.5)]
    assert ro.triangle_setup(collinear, cull=0) is None and ro.triangle_setup(collinear, cull=1) is None
    same_after_snapping = [vert(2.5, 2.5), vert(2.5 + 1e-4, 2.5), vert(2.5, 2.5 + 1e-4)]
    assert ro.triangle_setup(same_after_snapping, cull=0) is None
    cw = [vert(2.5, 2.5), vert(2.5, 9.5), vert(9.5, 2.5)]
    assert ro.triangle_setup(cw, cull=1) is None
    X, Y, order = ro.triangle_setup(cw, cull=0)
    assert order == [0, 2, 1] and (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]) > 0
    # the same pixels from either side
    front = ro.triangle_setup([cw[0], cw[2], cw[1]], cull=1)
    for py in range(12):
        for px in range(12):
            assert ro.edge_values(X, Y, px, py)[1] == ro.edge_values(front[0], front[1], px, py)[1]


def test_snapping_ties_go_up_and_the_point_footprints():
    assert ro.snap(1.0 + 0.5 / 256) == 257 and ro.snap(1.0 + 0.49 / 256) == 256 and ro.snap(-1.0 - 0.5 / 256) == -256
    assert [ro.point_size(s) for s in (0.2, 1.0, 1.49, 1.5, 2.5, 64.4, 1000.0)] == [1, 1, 1, 2, 3, 64, 64]
    # odd sizes are centred on the pixel that holds the point, even sizes on the nearest pixel corner
    assert ro.point_span(5.25, 1, 100) == (5, 5) and ro.point_span(5.75, 3, 100) == (4, 6)
    assert ro.point_span(5.25, 2, 100) == (4, 5) and ro.point_span(5.5, 2, 100) == (5, 6) and ro.point_span(5.75, 4, 100) == (4, 7)
    assert ro.point_span(0.5, 3, 100) == (0, 1) and ro.point_span(99.5, 3, 100) == (98, 99) and ro.point_span(100.0, 1, 100) == (100, 99)


# ---- depth and colour on a slanted quad

def quad_stream(zs, words):
    """the cell (0, 0)-(1, 1) as pointCloud2GLTriangleList sends it: (pi, pl, pj), (pi, pk, pl)"""
    pts = {"i": (0.0, 0.0), "j": (1.0, 0.0), "k": (0.0, 1.0), "l": (1.0, 1.0)}
    rows = np.zeros((6, 4), np.float32)
    for r, name in enumerate("iljikl"):
        rows[r, :2] = pts[name]
        rows[r, 2] = zs[name]
        rows.view(np.uint32)[r, 3] = words[name]
    return dict(vertices=rows.view(np.uint32), node_offsets=np.array([0, 6]), strips=np.zeros((0, 2), np.int64),
                node_strip_offsets=np.array([0, 0]), node_types=np.array([do.TRIANGLES], np.int32))


def exact_fragment(rp, rows, px, py):
    """depth and colour of the fragment at (px, py) of the triangle with these three rows, in exact rational arithmetic from the
    oracle's projected vertices; None when the sample is not covered"""
    verts = [ro.project(r, rp) for r in rows]
    X, Y, order = ro.triangle_setup(verts, rp["cull"])
    verts = [verts[i] for i in order]
    e, inside = ro.edge_values(X, Y, px, py)
    if not inside:
        return None
    z = sum(Fraction(ei) * Fraction(v["zw"]) for ei, v in zip(e, verts)) / sum(e)
    q = [Fraction(ei) / Fraction(v["w"]) for ei, v in zip(e, verts)]
    cols = []
    for shift in (16, 8, 0):
        c = sum(qi * ((v["word"] >> shift) & 255) for qi, v in zip(q, verts)) / sum(q)
        cols.append(c)
    return z, cols


@pytest.mark.parametrize("perspective", [False, True])
def test_depth_and_colour_on_a_slanted_quad(perspective):
    zs = {"i": 1.0, "j": 1.5, "k": 1.25, "l": 2.0}
    words = {"i": 0x102030, "j": 0xF01000, "k": 0x00FF40, "l": 0x8040FF}
    W, H = (64, 64) if perspective else (40, 32)
    if perspective:
        view, proj = ro.sensor_camera(50.0, 50.0, 4.5, 4.5, W, H, 0.1, 100.0)
    else:
        view = ro.identity()
        proj = [0.0] * 16
        proj[0], proj[12], proj[5], proj[13], proj[10], proj[14], proj[15] = 2 * 30.0 / W, 2 * 4.5 / W - 1, -2 * 24.0 / H, 2 * 27.5 / H - 1, 0.5, -0.75, 1.0
    rp = ro.default_render_params(width=W, height=H, view=view, projection=proj)
    stream = quad_stream(zs, words)
    out = ro.render_stream(stream, rp)
    rows = stream["vertices"]
    checked = ties = 0
    for r in range(H):
        for px in range(W):
            prim = int(out["ids"][r, px])
            if prim < 0:
                continue
            z, cols = exact_fragment(rp, rows[prim:prim + 3], px, H - 1 - r)
            # the exact value rounded to float32, give or take the double evaluation's last bits
            assert abs(Fraction(float(out["depth"][r, px])) - z) <= Fraction(1, 2 ** 24) * max(z, Fraction(1, 4)) * Fraction(1001, 1000)
            for ch, c in enumerate(cols):
                want = math.floor(c + Fraction(1, 2))
                if abs((c + Fraction(1, 2)) - round(c + Fraction(1, 2))) < Fraction(1, 10 ** 9):
                    ties += 1  # on a rounding tie the double evaluation may fall either way
                    assert abs(int(out["rgba"][r, px, ch]) - want) <= 1
                else:
                    assert int(out["rgba"][r, px, ch]) == min(max(want, 0), 255)
            assert out["rgba"][r, px, 3] == 255
            checked += 1
    assert checked > 300 and ties < checked // 10
    assert len(set(out["ids"].ravel().tolist()) - {-1}) == 2  # both triangles of the cell
    if perspective:  # screen-space depth is not linear in eye depth: the quad's middle is nearer the far corner's value
        assert len(np.unique(out["depth"][out["ids"] >= 0])) > 50


def test_perspective_correct_colour_differs_from_screen_space():
    """A triangle seen at a slant: halfway along an edge in the image is not halfway along it in the world."""
    verts = [vert(2.5, 2.5, w=1.0, word=0x000000), vert(22.5, 2.5, w=4.0, word=0xFF0000), vert(2.5, 22.5, w=1.0, word=0x000000)]
    X, Y, order = ro.triangle_setup(verts, cull=1)
    e, inside = ro.edge_values(X, Y, 12, 3)
    assert inside
    q = [float(e[i]) / verts[i]["w"] for i in range(3)]
    red = (q[1] * 255.0) / ((q[0] + q[1]) + q[2])
    screen = e[1] * 255.0 / sum(e)
    assert 40 < red < 70 and 115 < screen < 130  # (1/4 . 1/2) / (1/2 + 1/8) = 1/5 of 255 against ~1/2


# ---- the camera helpers

def np_of(m):
    return np.asarray(m, np.float64).reshape(4, 4).T


def test_perspective_is_glu_perspective():
    for fovy, aspect, n, f in ((ro.REFERENCE_FOVY, 640.0 / 480.0, 0.1, 1e4), (60.0, 1.5, 0.5, 50.0)):
        cot = 1.0 / math.tan(math.radians(fovy) / 2.0)
        want = np.array([[cot / aspect, 0, 0, 0], [0, cot, 0, 0], [0, 0, (f + n) / (n - f), 2 * f * n / (n - f)], [0, 0, -1, 0]])
        got = np_of(ro.perspective(fovy, aspect, n, f))
        assert np.allclose(got, want, rtol=1e-14, atol=0) and np.array_equal(got == 0, want == 0)
    # the reference's quirk: 100 / 180 * pi DEGREES is a field of view of 1.745 degrees
    assert abs(math.degrees(2 * math.atan(1.0 / ro.perspective()[5])) - 1.7453) < 1e-3


def test_viewer_view_is_translate_rotate_rotate_rotate_viewpoint():
    def rot(deg, axis):
        a = math.radians(float(np.float32(deg)))
        c, s = math.cos(a), math.sin(a)
        R = np.eye(4)
        i, j = (axis + 1) % 3, (axis + 2) % 3
        R[i, i] = R[j, j] = c
        R[j, i], R[i, j] = s, -s
        return R
    rng = np.random.default_rng(3)
    V = np.eye(4)
    V[:3, :] = rng.uniform(-1, 1, (3, 4))
    for args in ((0.0, 0.0, -50.0, 180 * 16.0, 0.0, 0.0, 1.0), (0.3, -1.2, -7.0, 37 * 16.0, -123 * 16.0, 16.0 * 44.9, 1.0),
                 (1.0, 2.0, 3.0, 100.0, 200.0, -300.0, 2.5)):
        T = np.eye(4)
        T[:3, 3] = np.float32(args[:3])
        steps = [int((r / 16.0) / args[6]) * args[6] for r in args[3:6]]
        want = T @ rot(steps[0], 0) @ rot(steps[1], 1) @ rot(steps[2], 2) @ V
        got = np_of(ro.viewer_view(*args, viewpoint=ro.column_major(V)))
        assert np.allclose(got, want, rtol=0, atol=1e-13)
    # the default: half a turn about x, 50 back; one product per entry, so the order of the sums cannot matter
    a = math.pi
    want = np.array([[1, 0, 0, 0], [0, math.cos(a), -math.sin(a), 0], [0, math.sin(a), math.cos(a), -50.0], [0, 0, 0, 1]])
    assert np.array_equal(np_of(ro.viewer_view()), want)
    assert (int((44.9 * 16 / 16.0) / 1.0), int((-44.9 * 16 / 16.0) / 1.0)) == (44, -44)  # the steps truncate towards zero


def test_sensor_camera_puts_a_sensor_point_on_its_pixel():
    rng = np.random.default_rng(4)
    fx, fy, cx, cy, W, H = 525.0, 520.0, 319.5, 239.5, 640, 480
    for trial in range(3):
        pose = np.eye(4)
        if trial:
            A = rng.normal(size=(3, 3))
            Q, _ = np.linalg.qr(A)
            pose[:3, :3] = Q * np.sign(np.linalg.det(Q))
            pose[:3, 3] = rng.uniform(-2, 2, 3)
        view, proj = ro.sensor_camera(fx, fy, cx, cy, W, H, 0.1, 1e4, ro.column_major(pose) if trial else None)
        rp = ro.default_render_params(width=W, height=H, view=view, projection=proj)
        for _ in range(50):
            p = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.5, 8.0)])
            world = (pose[:3, :3] @ p + pose[:3, 3]).astype(np.float32)
            ps = np.linalg.inv(pose) @ np.append(world.astype(np.float64), 1.0)  # the float32 world point back in the sensor frame
            row = np.zeros(4, np.uint32)
            row[:3] = world.view(np.uint32)
            v = ro.project(row, rp)
            assert abs(v["xw"] - (fx * ps[0] / ps[2] + cx + 0.5)) < 1e-9 and abs((H - v["yw"]) - (fy * ps[1] / ps[2] + cy + 0.5)) < 1e-9
            assert abs(v["w"] - ps[2]) < 1e-12 and 0.0 < v["zw"] < 1.0


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    lib = os.path.join(tmp_path_factory.mktemp("render_camera"), "librender_camera_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "emu", "render_camera_host.cpp"), "-o", lib], check=True)
    L = ctypes.CDLL(lib)
    d, vp, i = ctypes.c_double, ctypes.c_void_p, ctypes.c_int
    L.host_perspective.argtypes = [d, d, d, d, vp]
    L.host_viewer_view.argtypes = [d] * 7 + [vp, vp]
    L.host_sensor_camera.argtypes = [d, d, d, d, i, i, d, d, vp, vp, vp]
    L.host_unproject.argtypes = [d, d, d, vp, vp, i, i, vp]
    L.host_unproject.restype = i
    for f in (L.host_perspective, L.host_viewer_view, L.host_sensor_camera):
        f.restype = None
    return L


def same_bytes(buf, want):
    return np.asarray(buf, np.float64).tobytes() == np.asarray(want, np.float64).tobytes()


def test_the_librarys_helpers_equal_the_python_ones(host):
    rng = np.random.default_rng(6)
    out, out2, out3 = np.zeros(16), np.zeros(16), np.zeros(3)
    for trial in range(40):
        fovy, aspect, n = rng.uniform(0.5, 120), rng.uniform(0.5, 2.5), rng.uniform(0.01, 1.0)
        f = n + rng.uniform(1, 1e4)
        host.host_perspective(fovy, aspect, n, f, out.ctypes.data)
        assert same_bytes(out, ro.perspective(fovy, aspect, n, f))
        args = [rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-60, 0)] + list(rng.uniform(-360 * 16, 360 * 16, 3)) + [rng.choice([1.0, 0.5, 2.5])]
        V = np.eye(4)
        V[:3, :] = rng.uniform(-1, 1, (3, 4))
        vp_ = np.asarray(ro.column_major(V))
        host.host_viewer_view(*args, vp_.ctypes.data if trial % 4 else None, out.ctypes.data)
        view = ro.viewer_view(*args, viewpoint=list(vp_) if trial % 4 else None)
        assert same_bytes(out, view)
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = Q, rng.uniform(-3, 3, 3)
        pose_ = np.asarray(ro.column_major(pose))
        W, H = int(rng.integers(1, 4097)), int(rng.integers(1, 4097))
        k = [rng.uniform(100, 900), rng.uniform(100, 900), rng.uniform(0, W), rng.uniform(0, H)]
        host.host_sensor_camera(*k, W, H, n, f, pose_.ctypes.data if trial % 3 else None, out.ctypes.data, out2.ctypes.data)
        sv, sp = ro.sensor_camera(*k, W, H, n, f, list(pose_) if trial % 3 else None)
        assert same_bytes(out, sv) and same_bytes(out2, sp)
        proj = np.asarray(ro.perspective(fovy, aspect, n, f))
        x, y, z = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0, 1)
        for v_, p_ in ((np.asarray(view), proj), (np.asarray(sv), np.asarray(sp))):
            ok = host.host_unproject(x, y, z, v_.ctypes.data, p_.ctypes.data, W, H, out3.ctypes.data)
            want = ro.unproject(x, y, z, list(v_), list(p_), W, H)
            assert ok == 1 and same_bytes(out3, want)
    singular = np.zeros(16)
    before = out3.copy()
    assert host.host_unproject(1.0, 1.0, 0.5, singular.ctypes.data, proj.ctypes.data, 8, 8, out3.ctypes.data) == 0
    assert ro.unproject(1.0, 1.0, 0.5, list(singular), list(proj), 8, 8) is None and np.array_equal(out3, before)


# Measured over this test's points: the worst distance between unproject(project(p)) and the numpy.linalg route is
# UNPROJECT_WORST (metres, for points 0.5 m to 8 m from the sensor); the test asserts 100 times that.
UNPROJECT_WORST = 1.34e-14
UNPROJECT_BOUND = 100 * UNPROJECT_WORST


def test_unproject_of_project_against_a_linalg_route():
    """setClickedPosition's round trip: a world point to window coordinates (the chain of the contract, with the depth rounded
    to float32 as the depth image holds it), back through unproject, against numpy.linalg.inv on the same window coordinates."""
    rng = np.random.default_rng(8)
    W, H = 640, 480
    pose = np.eye(4)
    c, s = math.cos(0.4), math.sin(0.4)
    pose[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    pose[:3, 3] = (0.5, -0.2, 1.0)
    view, proj = ro.sensor_camera(525.0, 525.0, 319.5, 239.5, W, H, 0.1, 1e4, ro.column_major(pose))
    rp = ro.default_render_params(width=W, height=H, view=view, projection=proj)
    inv = np.linalg.inv(np_of(proj) @ np_of(view))
    worst = 0.0
    for _ in range(500):
        p = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), 1.0]) * rng.uniform(0.5, 8.0)
        world = (pose[:3, :3] @ p + pose[:3, 3]).astype(np.float32)
        row = np.zeros(4, np.uint32)
        row[:3] = world.view(np.uint32)
        v = ro.project(row, rp)
        assert v["in_xy"] and v["ok_z"]
        depth = float(np.float32(v["zw"]))
        got = np.asarray(ro.unproject(v["xw"], v["yw"], depth, view, proj, W, H))
        o = inv @ np.array([v["xw"] / W * 2 - 1, v["yw"] / H * 2 - 1, depth * 2 - 1, 1.0])
        worst = max(worst, float(np.max(np.abs(got - o[:3] / o[3]))))
    print("unproject against numpy.linalg: worst %.3e, bound %.3e" % (worst, UNPROJECT_BOUND))
    assert worst <= UNPROJECT_BOUND
