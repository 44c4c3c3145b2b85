"""Small clouds whose display streams are written out by hand from src/glviewer.cpp, shared by tests/test_oracle_display.py
(the oracle against the hand streams) and tests/test_emu_display_kernels.py (the kernel source against both).

A stream is a list of vertices (px, py) or (px, py, cx, cy): x, y, z of the point in column px, row py with the rgb word of
the point in column cx, row cy (its own unless given).  Strips are [first vertex, vertex count]."""
import numpy as np

import display_oracle as do

NAN = np.float32(np.nan)


def grid(h, w, spacing=0.01, z=1.0):
    """Point (column x, row y) = (spacing * x, spacing * y, z), every rgb word different."""
    pts = np.zeros((h, w, 4), np.float32)
    pts[..., 0] = (np.arange(w, dtype=np.float32) * np.float32(spacing))[None, :]
    pts[..., 1] = (np.arange(h, dtype=np.float32) * np.float32(spacing))[:, None]
    pts[..., 2] = z
    pts.view(np.uint32)[..., 3] = 0x00A00000 + 0x101 * (np.arange(h * w, dtype=np.uint32).reshape(h, w) + 1)
    return pts


def rows_of(cloud, stream):
    words = np.ascontiguousarray(cloud, np.float32).view(np.uint32)
    out = np.zeros((len(stream), 4), np.uint32)
    for k, v in enumerate(stream):
        px, py = v[0], v[1]
        cx, cy = (v[2], v[3]) if len(v) == 4 else (px, py)
        out[k, :3] = words[py, px, :3]
        out[k, 3] = words[cy, cx, 3]
    return out


def _case(name, cloud, stream, strips, **prm):
    return dict(name=name, cloud=cloud, prm=do.default_params(**prm), stream=stream,
                strips=np.asarray(strips, np.int64).reshape(-1, 2))


def hand_cases():
    S, T, P = do.TRIANGLE_STRIP, do.TRIANGLES, do.POINTS
    cases = []
    # :801-847 starts with ul, ll of column 0; :855-888 sends ul, ll of column 1, ll in ul's colour; :896 ends the strip
    cases.append(_case("3x2 strip", grid(2, 3), [(0, 0), (0, 1), (1, 0), (1, 1, 1, 0)], [[0, 4]], display_type=S))
    # the last visited column pair never closes a quad
    cases.append(_case("2x2 strip", grid(2, 2), [(0, 0), (0, 1)], [[0, 2]], display_type=S))
    # (pi, pl, pj) then (pi, pk, pl)
    cases.append(_case("2x2 triangles", grid(2, 2), [(0, 0), (1, 1), (1, 0), (0, 0), (0, 1), (1, 1)], [], display_type=T))
    # ul invalid, lr valid: the lower point first (:824-847); then ul = the lower right, ll = the upper right, whose left
    # neighbour is the NaN point: a NaN ratio is not greater (:881)
    c = grid(2, 3)
    c[0, 0, 2] = NAN
    cases.append(_case("flip start", c, [(0, 1), (1, 1), (1, 0, 1, 1)], [[0, 3]], display_type=S))
    # the same in a cloud of two columns: a strip of one vertex
    c = grid(2, 2)
    c[0, 0, 2] = NAN
    cases.append(_case("one-vertex strip", c, [(0, 1)], [[0, 1]], display_type=S))
    # step 2, ul and lr of column 0 invalid: x++ (:829), the next visited column is 3; a strip starts there and the row ends
    c = grid(3, 7, spacing=0.005)
    c[0, 0, 2] = NAN
    c[2, 2, 2] = NAN
    cases.append(_case("x++ visits an odd column", c, [(3, 0), (3, 2)], [[0, 2]], display_type=S, visualization_skip_step=2))
    # a running strip: columns 0, 1 run; column 2 breaks it; column 3 starts the next, the row ends at column 4
    c = grid(2, 5)
    c[:, 2, 2] = 2.0
    cases.append(_case("broken by a depth jump", c, [(0, 0), (0, 1), (1, 0), (1, 1, 1, 0), (3, 0), (3, 1)], [[0, 4], [4, 2]],
                       display_type=S))
    c = grid(2, 5)
    c[0, 2, 2] = NAN
    cases.append(_case("broken by an invalid ul", c, [(0, 0), (0, 1), (1, 0), (1, 1, 1, 0), (3, 0), (3, 1)], [[0, 4], [4, 2]],
                       display_type=S))
    c = grid(2, 5)  # ul of column 2 is sent before ll is found invalid (:864-867, :889-892)
    c[1, 2, 2] = NAN
    cases.append(_case("broken by an invalid ll", c, [(0, 0), (0, 1), (1, 0), (1, 1, 1, 0), (2, 0), (3, 0), (3, 1)],
                       [[0, 5], [5, 2]], display_type=S))
    # max_depth 1.5 between z = 1 and z = 2; the point (1, 0, 1.4) has range 1.72 > 1.5 and stays: the test is on z
    c = grid(2, 2)
    c[1, 0, 2] = 2.0
    c[0, 1, :3] = (1.0, 0.0, 1.4)
    cases.append(_case("max_depth is a test on z", c, [(0, 0), (1, 0), (1, 1)], [], display_type=P, maximum_depth=1.5))
    # createXYZRGBPointCloud's finite x, y "at 1 m" beside a NaN z
    c = grid(2, 2)
    c[0, 1, :3] = (0.3, 0.2, NAN)
    cases.append(_case("NaN z at 1 m", c, [(0, 0), (0, 1), (1, 1)], [], display_type=P))
    # pi in the origin: depth 0, d / 0 = inf > t (:1020): nothing
    c = grid(2, 2)
    c[0, 0, :3] = 0.0
    cases.append(_case("pi in the origin, inf ratios", c, [], [], display_type=T))
    # all four in the origin: 0 / 0 = NaN is neither > t (:1020 passes) nor <= t (:1025, :1033 fail): nothing
    c = grid(2, 2)
    c[..., :3] = 0.0
    cases.append(_case("all in the origin, NaN ratios", c, [], [], display_type=T))
    # a running step whose ul is in the origin beside a left neighbour in the origin: 0 / 0 = NaN is not > t (:857), the
    # vertex is sent.  Threshold 2: the start's ratios |ur|^2 / |ur|^2 = 1 pass.
    c = grid(2, 3)
    c[0, 0, 2] = NAN
    c[1, 0, :3] = 0.0
    c[1, 1, :3] = 0.0
    cases.append(_case("running ul in the origin", c, [(0, 1), (1, 1), (1, 0, 1, 1)], [[0, 3]], display_type=S,
                       squared_meshing_threshold=2.0))
    # threshold 0.25, pi = (0, 0, 1), the others (0, 0, 1.5): 0.25 / 1 <= 0.25 keeps both triangles
    c = grid(2, 2)
    c[..., :2] = 0.0
    c[..., 2] = 1.5
    c[0, 0, 2] = 1.0
    tri = [(0, 0), (1, 1), (1, 0), (0, 0), (0, 1), (1, 1)]
    cases.append(_case("ratio equal to the threshold", c, tri, [], display_type=T, squared_meshing_threshold=0.25))
    c = c.copy()
    c[1, 1, 2] = np.nextafter(np.float32(1.5), np.float32(2))  # pl one float further: > 0.25 (:1020)
    cases.append(_case("ratio one float above the threshold", c, [], [], display_type=T, squared_meshing_threshold=0.25))
    # glviewer.cpp:697: a negative threshold, or a cloud of one row, is drawn as points whatever was asked
    cases.append(_case("negative threshold", grid(2, 2), [(0, 0), (0, 1), (1, 0), (1, 1)], [], display_type=T,
                       squared_meshing_threshold=-1.0))
    cases.append(_case("rows == 1", grid(1, 3), [(0, 0), (1, 0), (2, 0)], [], display_type=S))
    return cases


def holes_and_jumps(rng, h, w, holes=0.3, jumps=4, spacing=0.004):
    """A slanted plane with NaN-z holes, a few columns / rows pushed back by a depth jump, one point in the origin and one
    infinite z."""
    c = grid(h, w, spacing=spacing, z=1.0)
    c[..., 2] += (rng.uniform(0, 0.002, (h, w)) + 0.001 * np.arange(w)[None, :]).astype(np.float32)
    for _ in range(jumps):
        if rng.random() < 0.5:
            c[:, rng.integers(w):, 2] += np.float32(0.5)
        else:
            c[rng.integers(h):, :, 2] += np.float32(0.5)
    c[rng.random((h, w)) < holes, 2] = NAN
    c[rng.integers(h), rng.integers(w), :3] = 0.0
    c[rng.integers(h), rng.integers(w), 2] = np.inf
    c.view(np.uint32)[..., 3] = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32)
    return c
