"""CPU: the restatements of display geometry (tests/display_oracle.py: GLViewer::pointCloud2GLPoints, pointCloud2GLTriangleList
and pointCloud2GLStrip, src/glviewer.cpp) against streams written out by hand (tests/display_cases.py) and against each
other, and the PLY writer of tools/export_mesh.py read back.  The device is tests/test_gpu_display_geometry.py, the kernel
source on the host tests/test_emu_display_kernels.py.  All comparisons are on bytes."""
import os
import sys

import numpy as np
import pytest

import display_cases as dc
import display_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dc.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_written_streams(case):
    want = dc.rows_of(case["cloud"], case["stream"])
    for node in (do.node_literal, do.node_fast):
        rows, strips, _ = node(case["cloud"], case["prm"])
        assert do.same_vertices(rows, want), (node.__name__, rows, want)
        assert np.array_equal(strips, case["strips"]), (node.__name__, strips)


def test_the_named_cases_are_all_there():
    names = {c["name"] for c in CASES}
    assert {"3x2 strip", "2x2 strip", "2x2 triangles", "flip start", "x++ visits an odd column", "broken by a depth jump",
            "broken by an invalid ul", "broken by an invalid ll", "one-vertex strip", "max_depth is a test on z", "NaN z at 1 m",
            "pi in the origin, inf ratios", "all in the origin, NaN ratios", "running ul in the origin",
            "ratio equal to the threshold", "ratio one float above the threshold", "negative threshold", "rows == 1"} <= names


def test_node_types():
    by = {c["name"]: c for c in CASES}
    assert do.node_literal(by["negative threshold"]["cloud"], by["negative threshold"]["prm"])[2] == do.POINTS
    assert do.node_literal(by["rows == 1"]["cloud"], by["rows == 1"]["prm"])[2] == do.POINTS
    assert do.node_literal(by["3x2 strip"]["cloud"], by["3x2 strip"]["prm"])[2] == do.TRIANGLE_STRIP
    assert do.node_literal(by["2x2 triangles"]["cloud"], by["2x2 triangles"]["prm"])[2] == do.TRIANGLES


def test_colour_quirk_of_line_886():
    """The second vertex of a running step: ll's coordinates, ul's rgb word."""
    cloud = dc.grid(2, 3)
    words = cloud.view(np.uint32)
    assert len(np.unique(words[..., 3])) == 6
    rows, _, _ = do.node_literal(cloud, do.default_params(display_type=do.TRIANGLE_STRIP))
    assert rows[3, :3].tobytes() == words[1, 1, :3].tobytes()
    assert rows[3, 3] == words[0, 1, 3] != words[1, 1, 3]
    assert rows[1, 3] == words[1, 0, 3]  # the start's ll has its own colour (:843)


def test_ratio_at_the_threshold_is_exact():
    by = {c["name"]: c for c in CASES}
    c = by["ratio equal to the threshold"]["cloud"]
    pi, pl = c[0, 0], c[1, 1]
    assert do.sq_dist(pi, pl) / do.sq_dist(pi, do.ORIGIN) == np.float32(0.25)
    pl = by["ratio one float above the threshold"]["cloud"][1, 1]
    assert do.sq_dist(pi, pl) / do.sq_dist(pi, do.ORIGIN) > np.float32(0.25)


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("shape", [(7, 11), (8, 10), (5, 4)])
def test_flat_clouds_reach_the_stated_bounds(step, shape):
    """All valid and flat: every visited row is one strip over every visited column, two vertices a column -- the bound
    include/rgbdfe.h states: Y = ceil((rows - step) / step), X = ceil((cols - step) / step), 2 X Y vertices."""
    h, w = shape
    cloud = dc.grid(h, w, spacing=0.002)
    prm = do.default_params(display_type=do.TRIANGLE_STRIP, visualization_skip_step=step)
    rows, strips, _ = do.node_literal(cloud, prm)
    Y, X = -(-(h - step) // step), -(-(w - step) // step)
    assert len(rows) == 2 * X * Y and len(strips) == Y
    assert np.array_equal(strips, np.stack([np.arange(Y) * 2 * X, np.full(Y, 2 * X)], 1))
    stream = []
    for y in range(0, h - step, step):
        for x in range(0, w - step, step):
            stream += [(x, y), (x, y + step) if x == 0 else (x, y + step, x, y)]
    assert do.same_vertices(rows, dc.rows_of(cloud, stream))
    fast = do.node_fast(cloud, prm)
    assert do.same_vertices(fast[0], rows) and np.array_equal(fast[1], strips)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fast_forms_equal_the_literal_loops(seed):
    """23 x 17 clouds with 30 % holes, planted jumps, a point in the origin and an infinite z."""
    rng = np.random.default_rng(seed)
    cloud = dc.holes_and_jumps(rng, 17, 23)
    seen = 0
    for md in (np.inf, 1.8):
        for t, steps in ((do.POINTS, [1]), (do.TRIANGLES, [1]), (do.TRIANGLE_STRIP, [1, 2, 3])):
            for step in steps:
                prm = do.default_params(display_type=t, visualization_skip_step=step, maximum_depth=md)
                lit, fast = do.node_literal(cloud, prm), do.node_fast(cloud, prm)
                assert do.same_vertices(fast[0], lit[0]), (t, step, md)
                assert np.array_equal(fast[1], lit[1]) and fast[2] == lit[2] == t
                seen += md == np.inf and len(lit[0]) > 0 and (t != do.TRIANGLE_STRIP or len(lit[1]) > 1)
    assert seen == 5  # without the depth limit every form emits something and the strips break


def test_the_call_concatenates_nodes_and_transforms_like_map_assembly():
    import map_assembly_oracle as mo
    rng = np.random.default_rng(5)
    clouds = [dc.holes_and_jumps(rng, 6, 9), dc.grid(1, 5), dc.holes_and_jumps(rng, 9, 7)]
    Ts = []
    for k in range(3):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = q, rng.uniform(-2, 2, 3)
        Ts.append(T)
    prm = do.default_params(display_type=do.TRIANGLE_STRIP)
    plain, moved = do.display(clouds, prm, literal=True), do.display(clouds, prm, Ts, literal=True)
    assert plain["node_types"].tolist() == [do.TRIANGLE_STRIP, do.POINTS, do.TRIANGLE_STRIP]
    assert plain["node_offsets"][-1] == len(plain["vertices"]) and plain["node_strip_offsets"][1] == plain["node_strip_offsets"][2]
    for key in ("node_offsets", "strips", "node_strip_offsets"):
        assert np.array_equal(plain[key], moved[key])
    assert np.array_equal(plain["strips"][:, 0] >= 0, np.ones(len(plain["strips"]), bool))
    # the middle node: all valid points, so its vertices are the assembled map's rows
    want, _ = mo.assemble([clouds[1]], [Ts[1]], np.inf, True)
    a, b = plain["node_offsets"][1:3]
    assert do.same_vertices(moved["vertices"][a:b], want.view(np.uint32))
    fast = do.display(clouds, prm, Ts)
    assert do.same_vertices(fast["vertices"], moved["vertices"])


def test_ply_writer_read_back(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import export_mesh as em
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(9)
    cloud = dc.holes_and_jumps(rng, 8, 9, holes=0.1)
    rows, _, _ = do.node_fast(cloud, do.default_params(display_type=do.TRIANGLES))
    assert len(rows) >= 6 and len(rows) % 3 == 0
    path = str(tmp_path / "m.ply")
    assert em.write_ply(path, rows.view(np.float32)) == (len(rows), len(rows) // 3)
    head = open(path, "rb").read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(rows))
    v, f = em.read_ply(path)
    xyz = np.stack([v["x"], v["y"], v["z"]], 1)
    assert xyz.tobytes() == np.ascontiguousarray(rows[:, :3]).tobytes()
    assert np.array_equal(v["blue"], rows[:, 3] & 0xFF) and np.array_equal(v["green"], (rows[:, 3] >> 8) & 0xFF)
    assert np.array_equal(v["red"], (rows[:, 3] >> 16) & 0xFF)
    assert np.all(f["n"] == 3) and np.array_equal(np.stack([f["i"], f["j"], f["k"]], 1).reshape(-1), np.arange(len(rows)))
    with pytest.raises(ValueError):
        em.write_ply(path, rows[:4].view(np.float32))
