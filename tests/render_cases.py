"""The planted scenes of the renderer's tests (tests/test_emu_render_kernels.py on the host, tests/test_gpu_render.py on the
device): small clouds, a camera per case, and what each case is there to hit -- checked on the oracle's own intermediate values
(`planted`), so a case that stops hitting its edge fails instead of passing for nothing.

A frame is (depth [h, w] float32, rgb [h, w, 3] uint8, fx, fy, cx, cy, min_depth); `cloud_of` restates
createXYZRGBPointCloud at cloud_skip 1 (csrc/emm.hip, create_cloud_kernel) for the host tests, the GPU tests upload the frame
and render what the device made of it.  The grid frames have fx = fy = 1 and depths that are small dyadic numbers, so their
points are exact: x = u - cx, y = v - cy at depth 1.

`window_camera` is an affine camera (w = 1) that puts a point at x_w = kx x + ox, y_w = ky y + oy, z_w = kz z + oz.  ky < 0
shows the meshes from the front (the sensor's y points down, the window's up)."""
import numpy as np

import display_oracle as do
import render_oracle as ro

f32 = np.float32
MESH = 1e3  # squared_meshing_threshold under which the unit grids mesh


def frame(depth, seed, fx=1.0, fy=1.0, cx=None, cy=None, min_depth=0.4):
    depth = np.ascontiguousarray(depth, np.float32)
    h, w = depth.shape
    rgb = np.random.default_rng(3000 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return dict(depth=depth, rgb=rgb, fx=fx, fy=fy, cx=float(w // 2) if cx is None else cx, cy=float(h // 2) if cy is None else cy,
                min_depth=min_depth)


def cloud_of(fr):
    """create_cloud_kernel at cloud_skip 1, depth_scaling 1, rgb8: [h, w, 4] float32"""
    d = fr["depth"]
    h, w = d.shape
    fxinv, fyinv = f32(1.0 / fr["fx"]), f32(1.0 / fr["fy"])
    u = (np.arange(w, dtype=np.float32) - f32(fr["cx"]))[None, :].repeat(h, 0)
    v = (np.arange(h, dtype=np.float32) - f32(fr["cy"]))[:, None].repeat(w, 1)
    with np.errstate(invalid="ignore"):
        ok = d >= f32(fr["min_depth"])
        x = np.where(ok, (u * d).astype(np.float32) * fxinv, (u.astype(np.float64) * 1.0 * np.float64(fxinv)).astype(np.float32))
        y = np.where(ok, (v * d).astype(np.float32) * fyinv, (v.astype(np.float64) * 1.0 * np.float64(fyinv)).astype(np.float32))
    out = np.empty((h, w, 4), np.float32)
    out[..., 0], out[..., 1], out[..., 2] = x, y, np.where(ok, d, np.nan)
    rgb = fr["rgb"].astype(np.uint32)
    words = rgb[..., 2] | (rgb[..., 1] << 8) | (rgb[..., 0] << 16)
    words[0, 0] = 0  # the first point's colour is never written (misc.cpp:536)
    out.view(np.uint32)[..., 3] = words
    return out


def window_camera(W, H, kx, ox, ky, oy, kz=0.25, oz=0.25):
    """(view, projection) with w = 1: x_w = kx x + ox (up to the rounding of the chain the contract states)"""
    p = [0.0] * 16
    p[0], p[12] = 2.0 * kx / W, 2.0 * ox / W - 1.0
    p[5], p[13] = 2.0 * ky / H, 2.0 * oy / H - 1.0
    p[10], p[14] = 2.0 * kz, 2.0 * oz - 1.0
    p[15] = 1.0
    return ro.identity(), p


def translation(x=0.0, y=0.0, z=0.0):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (x, y, z)
    return T


def rp_of(W, H, cam, **kw):
    return ro.default_render_params(width=W, height=H, view=cam[0], projection=cam[1], **kw)


def disp(form, step=1, thresh=MESH):
    return do.default_params(display_type=form, visualization_skip_step=step, squared_meshing_threshold=thresh)


# ---- the frames: id -> frame
def frames():
    rng = np.random.default_rng(91)
    flat = np.ones((3, 4), np.float32)
    dip = flat.copy()
    dip[1, 1] = 0.5                       # one vertex nearer than the others
    holes = np.ones((5, 6), np.float32)   # strips of one, two and more vertices
    holes[2, 3] = holes[3, 2] = np.nan
    holes[3, 4] = 0.25                    # under min_depth: NaN z beside finite x, y
    slope = (1.0 + 0.125 * np.arange(6)[None, :] + 0.0625 * np.arange(5)[:, None]).astype(np.float32)
    row = np.ones((1, 5), np.float32)
    big = (1.5 + 0.004 * np.arange(11)[None, :] + rng.uniform(0, 0.004, (66, 11))).astype(np.float32)
    big[rng.random((66, 11)) < 0.1] = np.nan
    big[rng.random((66, 11)) < 0.03] = 0.2
    return {0: frame(flat, 0), 1: frame(dip, 1), 2: frame(holes, 2), 3: frame(slope, 3), 4: frame(row, 4, cy=0.0),
            5: frame(big, 5, fx=40.0, fy=40.0), 6: frame(np.full((4, 4), np.nan, np.float32), 6)}


def _verts(stream, rp):
    rows = np.ascontiguousarray(stream["vertices"]).view(np.uint32).reshape(-1, 4)
    return [ro.project(r, rp) for r in rows]


def _boxes(stream, rp):
    """pixel count of the box of every triangle that is set up"""
    v, out = _verts(stream, rp), []
    for kind, prim, at, node in ro.primitives(stream):
        if kind != "triangle":
            continue
        s = ro.triangle_setup([v[i] for i in at], rp["cull"])
        if s is not None:
            x0, x1, y0, y1 = ro.pixel_box(s[0], s[1], rp["width"], rp["height"])
            out.append(max(x1 - x0 + 1, 0) * max(y1 - y0 + 1, 0))
    return out


def case(name, nodes, dp, rp, transforms=None, planted=None):
    return dict(name=name, nodes=list(nodes), disp=dp, rp=rp, transforms=transforms, planted=planted or (lambda s, rp, out: None))


def cases():
    """Every case: dict(name, nodes (frame ids), disp, rp, transforms (list of 4 x 4 float32 or None), planted(stream, rp, oracle
    images))."""
    out = []
    front = lambda W, H, k, **kw: window_camera(W, H, k, W / 2 + 0.5, -k, H / 2 + 0.5, **kw)  # grid vertices on pixel centres
    behind = lambda W, H, k, **kw: window_camera(W, H, k, W / 2 + 0.5, k, H / 2 + 0.5, **kw)

    # -- depth test: two points per pixel, the nearer wins whichever is listed first; equal depths: the earlier
    cam = front(32, 24, 4)
    near, far = translation(z=-0.25), translation(z=0.5)
    n0 = 12  # points of frame 0

    def first_node_wins(s, rp, o):
        assert set(np.unique(o["node_index"])) == {-1, 0} and np.all(o["ids"][o["ids"] >= 0] < n0)

    def second_node_wins(s, rp, o):
        assert set(np.unique(o["node_index"])) == {-1, 1} and np.all(o["ids"][o["ids"] >= 0] >= n0)
    out.append(case("depth_near_first", [0, 0], disp(do.POINTS), rp_of(32, 24, cam), [near, far], first_node_wins))
    out.append(case("depth_near_second", [0, 0], disp(do.POINTS), rp_of(32, 24, cam), [far, near], second_node_wins))
    out.append(case("depth_equal_earlier_wins", [0, 0], disp(do.POINTS), rp_of(32, 24, cam), [far, far], first_node_wins))

    # -- point clipping: a point one float step inside and one outside each of the six planes.  x_w = 16 x + 16 maps x in
    # [-1, 1] onto the viewport; z_w = z - 1 maps z in [1, 2] onto the depth range.  The watched point is (sx, sy, 1) of frame 0.
    cam = window_camera(32, 24, 16.0, 16.0, 12.0, 12.0, kz=1.0, oz=-1.0)
    up, down = lambda v: float(np.nextafter(f32(v), f32(np.inf))), lambda v: float(np.nextafter(f32(v), f32(-np.inf)))
    planes = [("x_hi", 0, 1.0, 1.0, +1), ("x_lo", 0, -1.0, -1.0, -1), ("y_hi", 1, 1.0, 1.0, +1), ("y_lo", 1, -1.0, -1.0, -1),
              ("z_near", 2, 1.0, 1.0, -1), ("z_far", 2, 1.0, 2.0, +1)]
    for pname, axis, coord, plane, outward in planes:
        for side in ("in", "out"):
            target = (up(plane) if outward > 0 else down(plane)) if side == "out" else (down(plane) if outward > 0 else up(plane))
            t = [0.0, 0.0, 0.0]
            t[axis] = target - coord
            # keep the watched point inside the other planes: it sits at (1 | -1, 0, 1) or (0, 1 | -1, 1) or (0, 0, .)
            watch = [0.0, 0.0, 1.0]
            watch[axis] = coord

            def planted(s, rp, o, axis=axis, target=target, watch=watch, side=side):
                rows = np.ascontiguousarray(s["vertices"]).view(np.float32).reshape(-1, 4)
                want = list(watch)
                want[axis] = target
                hit = [i for i, r in enumerate(rows) if [float(r[0]), float(r[1]), float(r[2])] == [float(f32(c)) for c in want]]
                assert len(hit) == 1, "the watched point is not where the case puts it"
                v = ro.project(np.ascontiguousarray(s["vertices"]).view(np.uint32).reshape(-1, 4)[hit[0]], rp)
                assert (v["ok_w"] and v["ok_z"] and v["in_xy"]) == (side == "in")
                if not (axis == 0 and target > 1.0) and not (axis == 1 and target > 1.0):  # (x_w = W and y_w = H own no pixel)
                    assert (hit[0] in o["ids"]) == (side == "in")
            out.append(case("clip_%s_%s" % (pname, side), [0], disp(do.POINTS), rp_of(32, 24, cam), [translation(*t)], planted))

    # -- point sizes 1..4 at x_w, y_w fractions .25, .5, .75 (64 x 32: every step of the chain is exact)
    for n in (1, 2, 3, 4):
        for frac in (0.25, 0.5, 0.75):
            cam = window_camera(64, 32, 8.0, 32.0 + frac, -8.0, 16.0 + frac)

            def planted(s, rp, o, frac=frac, n=n):
                vs = [v for v in _verts(s, rp) if v["ok_w"]]
                assert vs and all(v["xw"] % 1.0 == frac and v["yw"] % 1.0 == frac for v in vs)
                assert int(np.sum(o["ids"] >= 0)) == 12 * n * n  # the footprints are disjoint (8 pixels apart) and inside
            out.append(case("point_size_%d_frac_%g" % (n, frac), [0], disp(do.POINTS), rp_of(64, 32, cam, gl_point_size=float(n)),
                            None, planted))

    # -- size 3 at each border: the points of frame 0 on the first and last pixel columns and rows of 64 x 33
    cam = window_camera(64, 33, 21.0, 42.5, -16.0, 16.5)

    def at_the_borders(s, rp, o):
        vs = _verts(s, rp)
        assert {int(v["xw"]) for v in vs} >= {0, 63} and {int(v["yw"]) for v in vs} == {0, 16, 32}
        assert int(np.sum(o["ids"] >= 0)) < 12 * 9  # footprints were cut
    out.append(case("point_size_3_borders", [0], disp(do.POINTS), rp_of(64, 33, cam, gl_point_size=3.0), None, at_the_borders))
    out.append(case("point_size_64", [0], disp(do.POINTS), rp_of(64, 33, cam, gl_point_size=200.0), None,
                    lambda s, rp, o: None))  # clamped to 64: every point goes through the workgroup pass

    # -- triangles: the fan around the inner grid vertices, vertices on pixel centres, edges through centres
    def covered_once(s, rp, o):
        assert o["tested"] == int(np.sum(o["ids"] >= 0)) > 0  # no pixel was offered twice
    for k, W, H in ((7, 48, 32), (8, 48, 32)):  # boxes of 8 x 8 = 64 pixels (the lane pass) and 9 x 9 (the workgroup pass)
        def planted(s, rp, o, k=k):
            covered_once(s, rp, o)
            assert set(_boxes(s, rp)) == {(k + 1) * (k + 1)}
            assert int(np.sum(o["ids"] >= 0)) == (3 * k) * (2 * k)  # a 3 k x 2 k pixel mesh, each edge sample owned once
        out.append(case("fan_front_k%d" % k, [0], disp(do.TRIANGLES), rp_of(W, H, front(W, H, k)), None, planted))
    for cull in (1, 0):
        for side, cam_of in (("front", front), ("behind", behind)):
            def planted(s, rp, o, cull=cull, side=side):
                drawn = int(np.sum(o["ids"] >= 0))
                assert (drawn > 0) == (side == "front" or cull == 0)
                if drawn:
                    covered_once(s, rp, o)
            out.append(case("cull%d_%s" % (cull, side), [3], disp(do.TRIANGLES), rp_of(48, 40, cam_of(48, 40, 6), cull=cull), None,
                            planted))

    def nothing_drawn(s, rp, o):
        assert len(s["vertices"]) > 0 and np.all(o["ids"] == -1) and o["tested"] == 0
    out.append(case("zero_area", [0], disp(do.TRIANGLES), rp_of(32, 24, window_camera(32, 24, 0.0, 16.5, -6.0, 12.5), cull=0), None,
                    nothing_drawn))

    # -- a vertex in front of the near plane: every triangle that uses it is absent, the others are there
    cam = front(48, 32, 8, kz=1.0, oz=-0.75)  # z_w = z - 0.75: z = 1 is inside, the dip at z = 0.5 is not

    def dip_is_absent(s, rp, o):
        vs = _verts(s, rp)
        bad = {i for i, v in enumerate(vs) if not v["ok_z"]}
        assert bad
        tris = [(prim, at) for kind, prim, at, node in ro.primitives(s)]
        gone = {prim for prim, at in tris if bad & set(at)}
        assert gone and len(gone) < len(tris)
        assert not (gone & set(o["ids"].ravel().tolist())) and (set(o["ids"].ravel().tolist()) - {-1})
    out.append(case("near_plane_vertex", [1], disp(do.TRIANGLES), rp_of(48, 32, cam), None, dip_is_absent))

    # -- a vertex beyond the guard band; the triangles left cover the whole image
    cam = window_camera(48, 32, 10000.0, 2524.5, -10000.0, 5016.5)

    def guard_band(s, rp, o):
        vs = _verts(s, rp)
        assert any(abs(v["xw"]) > ro.GUARD for v in vs) and any(abs(v["xw"]) <= ro.GUARD for v in vs)
        assert np.all(o["ids"] == o["ids"][0, 0]) and o["ids"][0, 0] >= 0 and max(_boxes(s, rp)) == 48 * 32  # one triangle, every pixel
    out.append(case("guard_band_and_full_screen", [0], disp(do.TRIANGLES), rp_of(48, 32, cam), None, guard_band))

    # -- strips: records of one, two and more vertices, even and odd triangles, visualization_skip_step 2
    def strip_lengths(s, rp, o):
        counts = set(s["strips"][:, 1].tolist())
        assert {1, 2} <= counts and max(counts) >= 5
        ids = set(o["ids"].ravel().tolist()) - {-1}
        parity = {(i - int(a)) % 2 for a, c in s["strips"] for i in ids if a <= i < a + c}
        assert parity == {0, 1}
    for cull in (1, 0):
        out.append(case("strips_cull%d" % cull, [2], disp(do.TRIANGLE_STRIP), rp_of(64, 48, front(64, 48, 8), cull=cull), None,
                        strip_lengths))
    out.append(case("strips_step_2", [3, 2], disp(do.TRIANGLE_STRIP, step=2), rp_of(64, 48, front(64, 48, 8), cull=0),
                    [translation(), translation(z=0.125)]))

    # -- mixed forms: the one-row cloud is POINTS inside a TRIANGLES call; repeated ids; an all-invalid cloud between them
    def mixed(s, rp, o):
        assert s["node_types"].tolist() == [do.TRIANGLES, do.POINTS, do.TRIANGLES, do.TRIANGLES, do.TRIANGLES]
        assert {0, 1, 4} <= set(np.unique(o["node_index"]).tolist())
    out.append(case("mixed_forms", [3, 4, 6, 0, 3], disp(do.TRIANGLES), rp_of(64, 48, front(64, 48, 8), gl_point_size=2.0),
                    [translation(), translation(z=-0.5), translation(), translation(x=-1.0, z=-0.25), translation(y=1.0, z=0.25)],
                    mixed))
    out.append(case("no_transforms", [3, 4], disp(do.TRIANGLE_STRIP), rp_of(40, 36, front(40, 36, 5))))
    out.append(case("no_nodes", [], disp(do.POINTS), rp_of(33, 25, front(33, 25, 5), clear_rgba=(9, 8, 7, 6))))

    # -- perspective: the sensor's own camera from a pose beside the cloud, every form (perspective-correct colour, w != 1)
    pose = np.eye(4)
    c, s_ = np.cos(0.2), np.sin(0.2)
    pose[:3, :3] = [[c, 0, s_], [0, 1, 0], [-s_, 0, c]]
    pose[:3, 3] = (-0.4, 0.05, 0.3)
    for form, step in ((do.POINTS, 1), (do.TRIANGLES, 1), (do.TRIANGLE_STRIP, 1), (do.TRIANGLE_STRIP, 2)):
        cam = ro.sensor_camera(60.0, 60.0, 47.5, 31.5, 96, 64, 0.1, 1e4, ro.column_major(pose))


        def drawn(s, rp, o):
            assert {0, 1} <= set(np.unique(o["node_index"]).tolist()) and o["tested"] > o["won"] > 100
        out.append(case("perspective_form%d_step%d" % (form, step), [5, 5], disp(form, step, thresh=0.01),
                        rp_of(96, 64, cam, cull=0, gl_point_size=2.0), [translation(), translation(x=-0.1, y=0.2, z=0.05)], drawn))
    return out
