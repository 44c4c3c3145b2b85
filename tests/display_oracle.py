"""Oracle of display geometry (include/rgbdfe.h, "display geometry"; csrc/display_geometry.hip): GLViewer::addPointCloud's
choice (src/glviewer.cpp:693-711) among pointCloud2GLPoints (:955-987), pointCloud2GLTriangleList (:989-1042) and
pointCloud2GLStrip (:776-906), with setGLColor in its plain form (:91-93), applied to a list of node clouds.

Restatements that tests/test_oracle_display.py holds against each other:

* ``gl_points`` / ``gl_triangle_list`` / ``gl_strip``  the three functions as literal Python loops over a recorder of the GL
  calls, the reference line beside each branch, one float32 rounding per operation;
* ``points_fast`` / ``triangles_fast``                 vectorised numpy, for the larger inputs of the GPU tests;
* ``strip_fast``                                       the strip machine over vectorised predicates (every distance test for
  every column at once; the walk itself stays a loop, as the visited columns depend on the data).

The contract is restated, not pinned on the reference's compiled code: building glviewer.cpp needs Qt, GL and a recipe
under oracle/, and the functions are first-party float code whose statements can be read off one by one.

Clouds are float32 arrays [rows, cols, 4] (x, y, z, rgb bits); transforms are 4 x 4 matrices in the row-major numpy sense
(the Matrix4f), or None for the node frame; the rgb column is only ever moved as a 32-bit word.  A vertex is (x, y, z of the
glVertex3f call, rgb word of the point the preceding setGLColor call was given)."""
import numpy as np

POINTS, TRIANGLES, TRIANGLE_STRIP = 0, 1, 2
f32 = np.float32
ORIGIN = (f32(0), f32(0), f32(0))


def default_params(**kw):
    """parameter_server.cpp:151, :139, :148, :38"""
    p = dict(display_type=POINTS, visualization_skip_step=1, squared_meshing_threshold=0.0009, maximum_depth=np.inf)
    p.update(kw)
    return p


class Recorder:
    """What a display list receives: glBegin / glColor3ub (as the rgb word) / glVertex3f / glEnd."""

    def __init__(self):
        self.vertices = []   # (x, y, z, word)
        self.strips = []     # [first vertex, vertex count] per glBegin(GL_TRIANGLE_STRIP)
        self.word = None

    def begin_strip(self):
        self.strips.append([len(self.vertices), 0])

    def end_strip(self):
        self.strips[-1][1] = len(self.vertices) - self.strips[-1][0]

    def color(self, p):      # setGLColor(p)
        self.word = p[3]

    def vertex(self, x, y, z):
        self.vertices.append((x, y, z, self.word))


def _pt(pts, words, x, y):
    """pc->points[x + y * w] as (x, y, z, rgb word)"""
    return (pts[y, x, 0], pts[y, x, 1], pts[y, x, 2], words[y, x, 3])


def valid_xyz(p, max_depth):
    """:44-47"""
    if max_depth < p[2]:
        return False
    return bool(np.isfinite(p[2]) and np.isfinite(p[1]) and np.isfinite(p[0]))


def sq_dist(p1, p2):
    """:768-773"""
    dx = f32(p1[0] - p2[0])
    dy = f32(p1[1] - p2[1])
    dz = f32(p1[2] - p2[2])
    return f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))


def _cloud(cloud):
    pts = np.ascontiguousarray(cloud, np.float32)
    assert pts.ndim == 3 and pts.shape[2] == 4
    return pts, pts.view(np.uint32)


def gl_points(cloud, prm, gl):
    """:955-987"""
    pts, words = _cloud(cloud)
    max_depth = f32(prm["maximum_depth"])  # :972
    h, w = pts.shape[:2]
    for x in range(w):  # :975
        for y in range(h):  # :976
            p = _pt(pts, words, x, y)
            if not valid_xyz(p, max_depth):  # :979
                continue
            gl.color(p)
            gl.vertex(p[0], p[1], p[2])


def _draw_triangle(gl, p1, p2, p3):
    """:214-223"""
    for p in (p1, p2, p3):
        gl.color(p)
        gl.vertex(p[0], p[1], p[2])


def gl_triangle_list(cloud, prm, gl):
    """:989-1042"""
    pts, words = _cloud(cloud)
    mesh_thresh = f32(prm["squared_meshing_threshold"])  # :997
    max_depth = f32(prm["maximum_depth"])  # :1007
    h, w = pts.shape[:2]
    with np.errstate(all="ignore"):
        for x in range(w - 1):  # :1010
            for y in range(h - 1):  # :1011
                pi = _pt(pts, words, x, y)
                if not valid_xyz(pi, max_depth):  # :1016
                    continue
                depth = sq_dist(pi, ORIGIN)  # :1017
                pl = _pt(pts, words, x + 1, y + 1)  # one right-down
                if not valid_xyz(pl, max_depth) or f32(sq_dist(pi, pl) / depth) > mesh_thresh:  # :1020
                    continue
                pj = _pt(pts, words, x + 1, y)  # one right
                if (valid_xyz(pj, max_depth) and f32(sq_dist(pi, pj) / depth) <= mesh_thresh
                        and f32(sq_dist(pj, pl) / depth) <= mesh_thresh):  # :1024-1026
                    _draw_triangle(gl, pi, pl, pj)  # :1028
                pk = _pt(pts, words, x, y + 1)  # one down
                if (valid_xyz(pk, max_depth) and f32(sq_dist(pi, pk) / depth) <= mesh_thresh
                        and f32(sq_dist(pk, pl) / depth) <= mesh_thresh):  # :1032-1034
                    _draw_triangle(gl, pi, pk, pl)  # :1035


def gl_strip(cloud, prm, gl):
    """:776-906"""
    pts, words = _cloud(cloud)
    mesh_thresh = f32(prm["squared_meshing_threshold"])  # :784
    max_depth = f32(prm["maximum_depth"])  # :785
    strip_on, flip = False, False  # :794
    h, w = pts.shape[:2]
    step = int(prm["visualization_skip_step"])  # :797
    with np.errstate(all="ignore"):
        y = 0
        while y < h - step:  # :798
            x = 0
            while x < w - step:  # :799
                if not strip_on:  # :801
                    ll = _pt(pts, words, x, y + step)
                    if not valid_xyz(ll, max_depth):  # :803
                        x += step
                        continue
                    ur = _pt(pts, words, x + step, y)
                    if not valid_xyz(ur, max_depth):  # :805
                        x += step
                        continue
                    ul = _pt(pts, words, x, y)
                    if valid_xyz(ul, max_depth):  # :808
                        depth = sq_dist(ul, ORIGIN)
                        if (f32(sq_dist(ul, ll) / depth) <= mesh_thresh and  # :810
                                f32(sq_dist(ul, ll) / depth) <= mesh_thresh and  # :811, the same test again
                                f32(sq_dist(ur, ll) / depth) <= mesh_thresh):  # :812
                            gl.begin_strip()
                            strip_on = True
                            flip = False
                            gl.color(ul)  # :818
                            gl.vertex(ul[0], ul[1], ul[2])  # :821
                    if not strip_on:  # :824
                        lr = _pt(pts, words, x + step, y + step)
                        if not valid_xyz(lr, max_depth):  # :826
                            x += 1  # :829
                            x += step
                            continue
                        else:
                            depth = sq_dist(ur, ORIGIN)  # :832
                            if (f32(sq_dist(ur, ll) / depth) <= mesh_thresh and
                                    f32(sq_dist(lr, ll) / depth) <= mesh_thresh and
                                    f32(sq_dist(ur, lr) / depth) <= mesh_thresh):  # :833-835
                                gl.begin_strip()
                                strip_on = True
                                flip = True
                    if strip_on:  # :842
                        gl.color(ll)
                        gl.vertex(ll[0], ll[1], ll[2])
                    x += step
                    continue  # :848
                else:
                    yu = y + step if flip else y  # :853-854
                    ul = _pt(pts, words, x, yu)
                    ul_left = _pt(pts, words, x - step, yu)  # *(ul-step)
                    if valid_xyz(ul, max_depth):  # :855
                        depth = sq_dist(ul, ORIGIN)
                        if f32(sq_dist(ul, ul_left) / depth) > mesh_thresh:  # :857
                            gl.end_strip()
                            strip_on = False
                            x += step
                            continue
                        gl.color(ul)  # :864
                        gl.vertex(ul[0], ul[1], ul[2])  # :867
                    else:
                        gl.end_strip()  # :869
                        strip_on = False
                        x += step
                        continue
                    yl = y if flip else y + step  # :875-876
                    ll = _pt(pts, words, x, yl)
                    ll_left = _pt(pts, words, x - step, yl)  # *(ll-step)
                    if valid_xyz(ll, max_depth):  # :877
                        depth = sq_dist(ll, ORIGIN)
                        if (f32(sq_dist(ul, ll) / depth) > mesh_thresh or
                                f32(sq_dist(ul, ul_left) / depth) > mesh_thresh or
                                f32(sq_dist(ll, ll_left) / depth) > mesh_thresh):  # :879-881
                            gl.end_strip()
                            strip_on = False
                            x += step
                            continue
                        gl.color(ul)  # :886: ul's colour on ll's vertex
                        gl.vertex(ll[0], ll[1], ll[2])  # :888
                    else:
                        gl.end_strip()  # :890
                        strip_on = False
                        x += step
                        continue
                x += step
            if strip_on:  # :896
                gl.end_strip()
            strip_on = False
            y += step


def node_type(cloud, prm):
    """:697-711 (ELLIPSOIDS and NONE are not served)"""
    if np.asarray(cloud).shape[0] <= 1 or prm["squared_meshing_threshold"] < 0:  # !isOrganized(): height == 1
        return POINTS
    return int(prm["display_type"])


def _rows(vertices):
    out = np.zeros((len(vertices), 4), np.uint32)
    for k, v in enumerate(vertices):
        out[k, :3] = np.array(v[:3], np.float32).view(np.uint32)
        out[k, 3] = v[3]
    return out


def node_literal(cloud, prm):
    """One node's (vertex rows as uint32 [n, 4], strips [m, 2] relative to the node's first vertex, type)."""
    t = node_type(cloud, prm)
    gl = Recorder()
    (gl_points, gl_triangle_list, gl_strip)[t](cloud, prm, gl)
    return _rows(gl.vertices), np.asarray(gl.strips, np.int64).reshape(-1, 2), t


# ---- the faster forms -------------------------------------------------------------------------------------------------

def _valid(pts, max_depth):
    with np.errstate(all="ignore"):
        return ~(max_depth < pts[..., 2]) & np.isfinite(pts[..., 2]) & np.isfinite(pts[..., 1]) & np.isfinite(pts[..., 0])


def _sq(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _sq0(a):
    return _sq(a, np.zeros(4, np.float32))


def points_fast(cloud, prm):
    pts, words = _cloud(cloud)
    v = _valid(pts, f32(prm["maximum_depth"]))
    return np.ascontiguousarray(words.transpose(1, 0, 2)[v.T])


def triangles_fast(cloud, prm):
    pts, words = _cloud(cloud)
    h, w = pts.shape[:2]
    if w < 2 or h < 2:
        return np.zeros((0, 4), np.uint32)
    t, md = f32(prm["squared_meshing_threshold"]), f32(prm["maximum_depth"])
    v = _valid(pts, md)
    with np.errstate(all="ignore"):
        pi, pj, pk, pl = pts[:-1, :-1], pts[:-1, 1:], pts[1:, :-1], pts[1:, 1:]
        depth = _sq0(pi)
        go = v[:-1, :-1] & v[1:, 1:] & ~(_sq(pi, pl) / depth > t)
        first = go & v[:-1, 1:] & (_sq(pi, pj) / depth <= t) & (_sq(pj, pl) / depth <= t)
        second = go & v[1:, :-1] & (_sq(pi, pk) / depth <= t) & (_sq(pk, pl) / depth <= t)
    wi, wj, wk, wl = words[:-1, :-1], words[:-1, 1:], words[1:, :-1], words[1:, 1:]
    six = np.stack([wi, wl, wj, wi, wk, wl], axis=2).transpose(1, 0, 2, 3)  # [x, y, vertex, 4]
    keep = np.stack([first] * 3 + [second] * 3, axis=2).transpose(1, 0, 2)
    return np.ascontiguousarray(six[keep])


def strip_fast(cloud, prm):
    pts, words = _cloud(cloud)
    h, w = pts.shape[:2]
    step = int(prm["visualization_skip_step"])
    t, md = f32(prm["squared_meshing_threshold"]), f32(prm["maximum_depth"])
    ys = np.arange(0, h - step, step)
    if len(ys) == 0 or w <= step:
        return np.zeros((0, 4), np.uint32), np.zeros((0, 2), np.int64)
    nx = w - step
    U, L = pts[ys], pts[ys + step]  # upper and lower rows of every visited row
    vU, vL = _valid(U, md), _valid(L, md)
    with np.errstate(all="ignore"):
        ul, ll, ur, lr = U[:, :nx], L[:, :nx], U[:, step:], L[:, step:]
        d_ul, d_ur = _sq0(ul), _sq0(ur)
        start_a = (_sq(ul, ll) / d_ul <= t) & (_sq(ur, ll) / d_ul <= t)
        start_b = (_sq(ur, ll) / d_ur <= t) & (_sq(lr, ll) / d_ur <= t) & (_sq(ur, lr) / d_ur <= t)
        run = {}
        for flip, (A, B) in ((False, (U, L)), (True, (L, U))):  # A: the row of `ul`, B: the row of `ll`
            m = max(nx - step, 0)  # the columns that have a neighbour `step` to the left
            a, b = A[:, step:step + m], B[:, step:step + m]
            al, bl = A[:, :m], B[:, :m]
            da, db = _sq0(a), _sq0(b)
            cut_a = _sq(a, al) / da > t
            cut_b = (_sq(a, b) / db > t) | (_sq(a, al) / db > t) | (_sq(b, bl) / db > t)
            pad = np.zeros((len(ys), step), bool)
            run[flip] = (np.concatenate([pad, cut_a], 1).tolist(), np.concatenate([pad, cut_b], 1).tolist())
    vU, vL, start_a, start_b = vU.tolist(), vL.tolist(), start_a.tolist(), start_b.tolist()
    idx, col, strips = [], [], []  # a vertex = (flat index of its xyz, flat index of its colour)
    for r, y in enumerate(ys.tolist()):
        up, lo = y * w, (y + step) * w
        vu, vl, sa, sb = vU[r], vL[r], start_a[r], start_b[r]
        on, flip, x = False, False, 0
        while x < nx:
            if not on:
                if vl[x] and vu[x + step]:
                    if vu[x] and sa[x]:
                        strips.append([len(idx), 0])
                        on, flip = True, False
                        idx.append(up + x)
                        col.append(up + x)
                    if not on:
                        if not vl[x + step]:
                            x += 1
                        elif sb[x]:
                            strips.append([len(idx), 0])
                            on, flip = True, True
                    if on:
                        idx.append(lo + x)
                        col.append(lo + x)
            else:
                a, b = (lo, up) if flip else (up, lo)
                va, vb = (vl, vu) if flip else (vu, vl)
                cut_a, cut_b = run[flip]
                if va[x] and not cut_a[r][x]:
                    idx.append(a + x)
                    col.append(a + x)
                    if vb[x] and not cut_b[r][x]:
                        idx.append(b + x)
                        col.append(a + x)
                    else:
                        on = False
                else:
                    on = False
                if not on:
                    strips[-1][1] = len(idx) - strips[-1][0]
            x += step
        if on:
            strips[-1][1] = len(idx) - strips[-1][0]
    flat = words.reshape(-1, 4)
    out = flat[np.asarray(idx, np.int64)].copy() if idx else np.zeros((0, 4), np.uint32)
    if idx:
        out[:, 3] = flat[np.asarray(col, np.int64), 3]
    return out, np.asarray(strips, np.int64).reshape(-1, 2)


def node_fast(cloud, prm):
    t = node_type(cloud, prm)
    none = np.zeros((0, 2), np.int64)
    if t == POINTS:
        return points_fast(cloud, prm), none, t
    if t == TRIANGLES:
        return triangles_fast(cloud, prm), none, t
    return strip_fast(cloud, prm) + (t,)


def transformed(rows, T):
    """map assembly's arithmetic on vertex rows (uint32 [n, 4]): ((T0 x + T1 y) + T2 z) + T3 per row, the word as it is"""
    T = np.asarray(T, np.float32).reshape(4, 4)
    p = rows.view(np.float32)
    out = rows.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            v = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
            out[:, r] = v.astype(np.float32).view(np.uint32)
    return out


def display(clouds, prm, transforms=None, literal=False):
    """The whole call: dict(vertices uint32 [n, 4], node_offsets, strips int64 [m, 2] into the whole stream,
    node_strip_offsets, node_types).  A cloud object that is listed more than once is worked out once."""
    parts, strips, off, soff, types, memo = [], [], [0], [0], [], {}
    for k, cloud in enumerate(clouds):
        if id(cloud) not in memo:
            memo[id(cloud)] = (node_literal if literal else node_fast)(cloud, prm)
        rows, st, t = memo[id(cloud)]
        if transforms is not None:
            rows = transformed(rows, transforms[k])
        st = st.copy()
        st[:, 0] += off[-1]
        parts.append(rows)
        strips.append(st)
        off.append(off[-1] + len(rows))
        soff.append(soff[-1] + len(st))
        types.append(t)
    return dict(vertices=np.concatenate(parts) if parts else np.zeros((0, 4), np.uint32),
                node_offsets=np.asarray(off, np.int64),
                strips=np.concatenate(strips) if strips else np.zeros((0, 2), np.int64),
                node_strip_offsets=np.asarray(soff, np.int64), node_types=np.asarray(types, np.int32))


def same_vertices(got, want):
    """Bytes: got as float32 or uint32 [n, 4]."""
    got = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    return got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()
