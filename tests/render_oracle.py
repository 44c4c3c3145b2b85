"""Oracle of rendering (include/rgbdfe.h, "rendering"; csrc/render.hip, csrc/render_camera.h): a literal scalar restatement of
the contract on top of tests/display_oracle.py.  The primitives of the display-geometry stream are drawn one after the other in
stream order with a plain GL_LESS depth test; every operation behind the float32 vertex row is a Python float (IEEE double, one
rounding per operation), coverage is Python integers.  tests/test_oracle_render.py holds it against independent arithmetic.

Matrices are lists of 16 floats, column-major (element (row, column) at [4 * column + row]).  Images are H x W, row 0 at the
top: rgba uint8 [H, W, 4], depth float32, ids int64, node_index int32."""
import math

import numpy as np

import display_oracle as do

GUARD = 16384.0
PI = 3.14159265358979323846
REFERENCE_FOVY = 100.0 / 180.0 * PI  # fov_ (glviewer.cpp:118), radians handed to gluPerspective as degrees (:444)


# ---- the camera helpers (csrc/render_camera.h)

def identity():
    return [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


def mat_mul(a, b):
    r = [0.0] * 16
    for c in range(4):
        for i in range(4):
            r[4 * c + i] = ((a[i] * b[4 * c] + a[4 + i] * b[4 * c + 1]) + a[8 + i] * b[4 * c + 2]) + a[12 + i] * b[4 * c + 3]
    return r


def perspective(fovy=REFERENCE_FOVY, aspect=float(np.float32(640) / np.float32(480)), z_near=0.1, z_far=1e4):
    """gluPerspective; fovy in degrees"""
    rad = fovy / 2.0 * PI / 180.0
    cot = math.cos(rad) / math.sin(rad)
    m = [0.0] * 16
    m[0] = cot / aspect
    m[5] = cot
    m[10] = -(z_far + z_near) / (z_far - z_near)
    m[11] = -1.0
    m[14] = -(2.0 * z_far * z_near) / (z_far - z_near)
    return m


def axis_rotation(angle_deg, axis):
    """glRotatef about a coordinate axis"""
    a = float(np.float32(angle_deg)) * PI / 180.0
    c, s = math.cos(a), math.sin(a)
    m = identity()
    i, j = (axis + 1) % 3, (axis + 2) % 3
    m[4 * i + i] = c
    m[4 * j + j] = c
    m[4 * i + j] = s
    m[4 * j + i] = -s
    return m


def viewer_view(x_tra=0.0, y_tra=0.0, z_tra=-50.0, x_rot=180.0 * 16.0, y_rot=0.0, z_rot=0.0, rotation_stepping=1.0,
                viewpoint=None):
    """drawClouds' modelview (glviewer.cpp:356-377); the defaults are initialPosition's (:137-144)"""
    t = identity()
    t[12], t[13], t[14] = float(np.float32(x_tra)), float(np.float32(y_tra)), float(np.float32(z_tra))
    for axis, rot in enumerate((x_rot, y_rot, z_rot)):
        steps = int((rot / 16.0) / rotation_stepping)
        t = mat_mul(t, axis_rotation(steps * rotation_stepping, axis))
    if viewpoint is not None:
        t = mat_mul(t, [float(v) for v in viewpoint])
    return t


def sensor_camera(fx, fy, cx, cy, W, H, z_near=0.1, z_far=1e4, pose=None):
    """(view, projection): the sensor's own pinhole, z forward and y down, at the rigid pose"""
    inv = identity()
    if pose is not None:
        pose = [float(v) for v in pose]
        for r in range(3):
            for c in range(3):
                inv[4 * c + r] = pose[4 * r + c]
            inv[12 + r] = -((pose[4 * r] * pose[12] + pose[4 * r + 1] * pose[13]) + pose[4 * r + 2] * pose[14])
    view = [0.0] * 16
    for c in range(4):
        view[4 * c] = inv[4 * c]
        view[4 * c + 1] = -inv[4 * c + 1]
        view[4 * c + 2] = -inv[4 * c + 2]
        view[4 * c + 3] = inv[4 * c + 3]
    p = [0.0] * 16
    p[0] = 2.0 * fx / W
    p[5] = 2.0 * fy / H
    p[8] = 1.0 - 2.0 * (cx + 0.5) / W
    p[9] = 2.0 * (cy + 0.5) / H - 1.0
    p[10] = -(z_far + z_near) / (z_far - z_near)
    p[11] = -1.0
    p[14] = -(2.0 * z_far * z_near) / (z_far - z_near)
    return view, p


def unproject(x, y, depth, view, projection, W, H):
    """gluUnProject; None when projection . view is singular"""
    a = mat_mul(projection, view)
    m = [[a[4 * c + r] for c in range(4)] + [1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for k in range(4):
        p = k
        for r in range(k + 1, 4):
            if abs(m[r][k]) > abs(m[p][k]):
                p = r
        if m[p][k] == 0.0:
            return None
        if p != k:
            m[k], m[p] = m[p], m[k]
        d = m[k][k]
        for c in range(8):
            m[k][c] = m[k][c] / d
        for r in range(4):
            if r == k:
                continue
            f = m[r][k]
            for c in range(8):
                m[r][c] = m[r][c] - f * m[k][c]
    v = [x / W * 2.0 - 1.0, y / H * 2.0 - 1.0, depth * 2.0 - 1.0, 1.0]
    o = [((m[r][4] * v[0] + m[r][5] * v[1]) + m[r][6] * v[2]) + m[r][7] * v[3] for r in range(4)]
    if o[3] == 0.0:
        return None
    return [o[0] / o[3], o[1] / o[3], o[2] / o[3]]


def column_major(M):
    """a numpy 4 x 4 matrix (row-major sense) as the 16-list the helpers take"""
    return [float(v) for v in np.asarray(M, np.float64).reshape(4, 4).T.reshape(-1)]


# ---- the rasteriser

def default_render_params(**kw):
    p = dict(width=640, height=480, view=viewer_view(), projection=perspective(), gl_point_size=1.0, cull=1,
             clear_rgba=(3, 3, 3, 3), max_vertices_in_flight=0)
    p.update(kw)
    return p


def project(row, rp):
    """A vertex row (4 uint32 words) through the camera: dict(ok_w, ok_z, in_xy, xw, yw, zw, w, word), or ok_w False alone."""
    x, y, z = (float(v) for v in np.asarray(row[:3], np.uint32).view(np.float32))
    V, P, W, H = rp["view"], rp["projection"], rp["width"], rp["height"]
    e = [((V[r] * x + V[4 + r] * y) + V[8 + r] * z) + V[12 + r] for r in range(4)]
    q = [((P[r] * e[0] + P[4 + r] * e[1]) + P[8 + r] * e[2]) + P[12 + r] * e[3] for r in range(4)]
    w = q[3]
    if not (w > 0.0 and w <= 1.7976931348623157e308):
        return dict(ok_w=False)
    return dict(ok_w=True, ok_z=-w <= q[2] <= w, in_xy=(-w <= q[0] <= w) and (-w <= q[1] <= w),
                xw=(q[0] / w + 1.0) * float(W) / 2.0, yw=(q[1] / w + 1.0) * float(H) / 2.0, zw=q[2] / w / 2.0 + 0.5, w=w,
                word=int(row[3]), clip=q)


def point_size(gl_point_size):
    return int(min(max(math.floor(gl_point_size + 0.5), 1.0), 64.0))


def point_span(c, n, size):
    """the pixels [lo, hi] a point of size n at window coordinate c covers, cut at [0, size)"""
    s = math.floor(c) - (n - 1) // 2 if n & 1 else math.floor(c + 0.5) - n // 2
    return max(int(s), 0), min(int(s) + n - 1, size - 1)


def snap(c):
    return int(math.floor(c * 256.0 + 0.5))


def edge_owns(dx, dy):
    return dy < 0 or (dy == 0 and dx < 0)


def triangle_setup(verts, cull):
    """verts: three project() results.  None when the triangle draws nothing, else (X, Y, order): the snapped coordinates and
    the vertices' order, counter-clockwise."""
    for v in verts:
        if not (v["ok_w"] and v["ok_z"] and abs(v["xw"]) <= GUARD and abs(v["yw"]) <= GUARD):
            return None
    X, Y, order = [snap(v["xw"]) for v in verts], [snap(v["yw"]) for v in verts], [0, 1, 2]
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area == 0 or (area < 0 and cull):
        return None
    if area < 0:
        X[1], X[2], Y[1], Y[2], order = X[2], X[1], Y[2], Y[1], [0, 2, 1]
    return X, Y, order


def pixel_box(X, Y, W, H):
    """the pixels whose centre lies in the box of the snapped vertices, cut at the viewport: (x0, x1, y0, y1), inclusive"""
    return (max((min(X) + 127) >> 8, 0), min((max(X) - 128) >> 8, W - 1), max((min(Y) + 127) >> 8, 0), min((max(Y) - 128) >> 8, H - 1))


def edge_values(X, Y, px, py):
    """(e0, e1, e2, covered) at the centre of pixel (px, py)"""
    sx, sy = 256 * px + 128, 256 * py + 128
    e, inside = [], True
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = X[b] - X[a], Y[b] - Y[a]
        v = dx * (sy - Y[a]) - dy * (sx - X[a])
        e.append(v)
        inside = inside and (v > 0 or (v == 0 and edge_owns(dx, dy)))
    return e, inside


def _channels(word):
    return ((word >> 16) & 255, (word >> 8) & 255, word & 255)  # r, g, b of the GL_BGRA word


class Canvas:
    def __init__(self, rp):
        self.W, self.H = rp["width"], rp["height"]
        self.rgba = np.empty((self.H, self.W, 4), np.uint8)
        self.rgba[:] = np.asarray(rp["clear_rgba"], np.uint8)
        self.depth = np.ones((self.H, self.W), np.float32)
        self.ids = np.full((self.H, self.W), -1, np.int64)
        self.node_index = np.full((self.H, self.W), -1, np.int32)
        self.tested = self.won = 0

    def fragment(self, px, py, z, rgb, prim, node):
        r = self.H - 1 - py
        self.tested += 1
        if z < self.depth[r, px]:  # GL_LESS
            self.won += 1
            self.depth[r, px] = z
            self.rgba[r, px] = (rgb[0], rgb[1], rgb[2], 255)
            self.ids[r, px] = prim
            self.node_index[r, px] = node


def draw_point(cv, rp, row, prim, node):
    v = project(row, rp)
    if not (v["ok_w"] and v["ok_z"] and v["in_xy"]):
        return
    n = point_size(rp["gl_point_size"])
    x0, x1 = point_span(v["xw"], n, cv.W)
    y0, y1 = point_span(v["yw"], n, cv.H)
    z = np.float32(v["zw"])
    for py in range(y0, y1 + 1):
        for px in range(x0, x1 + 1):
            cv.fragment(px, py, z, _channels(v["word"]), prim, node)


def draw_triangle(cv, rp, rows, prim, node):
    verts = [project(r, rp) for r in rows]
    if not all(v["ok_w"] for v in verts):
        return
    setup = triangle_setup(verts, rp["cull"])
    if setup is None:
        return
    X, Y, order = setup
    verts = [verts[i] for i in order]
    x0, x1, y0, y1 = pixel_box(X, Y, cv.W, cv.H)
    cols = [_channels(v["word"]) for v in verts]
    for py in range(y0, y1 + 1):
        for px in range(x0, x1 + 1):
            e, inside = edge_values(X, Y, px, py)
            if not inside:
                continue
            e0, e1, e2 = float(e[0]), float(e[1]), float(e[2])
            z = np.float32(((e0 * verts[0]["zw"] + e1 * verts[1]["zw"]) + e2 * verts[2]["zw"]) / ((e0 + e1) + e2))
            q = [e0 / verts[0]["w"], e1 / verts[1]["w"], e2 / verts[2]["w"]]
            den = (q[0] + q[1]) + q[2]
            rgb = []
            for ch in range(3):
                c = ((q[0] * cols[0][ch] + q[1] * cols[1][ch]) + q[2] * cols[2][ch]) / den
                rgb.append(int(min(max(math.floor(c + 0.5), 0.0), 255.0)))
            cv.fragment(px, py, z, rgb, prim, node)


def primitives(stream):
    """(kind, first vertex = id, vertex indices, node) of the whole stream, in stream order"""
    off, types, strips, soff = stream["node_offsets"], stream["node_types"], stream["strips"], stream["node_strip_offsets"]
    out = []
    for k, t in enumerate(types):
        a, b = int(off[k]), int(off[k + 1])
        if t == do.POINTS:
            out += [("point", v, (v,), k) for v in range(a, b)]
        elif t == do.TRIANGLES:
            out += [("triangle", v, (v, v + 1, v + 2), k) for v in range(a, b - 2, 3)]
        else:
            for s, cnt in strips[int(soff[k]):int(soff[k + 1])]:
                s, cnt = int(s), int(cnt)
                for i in range(cnt - 2):
                    out.append(("triangle", s + i, (s + i, s + i + 1, s + i + 2) if i % 2 == 0 else (s + i + 1, s + i, s + i + 2), k))
    return out


def render_stream(stream, rp):
    """The images of a display-geometry stream (display_oracle.display's dict): dict(rgba, depth, ids, node_index, tested, won)"""
    rows = np.ascontiguousarray(stream["vertices"]).view(np.uint32).reshape(-1, 4)
    cv = Canvas(rp)
    for kind, prim, at, node in primitives(stream):
        if kind == "point":
            draw_point(cv, rp, rows[at[0]], prim, node)
        else:
            draw_triangle(cv, rp, [rows[i] for i in at], prim, node)
    return dict(rgba=cv.rgba, depth=cv.depth, ids=cv.ids, node_index=cv.node_index, tested=cv.tested, won=cv.won)


def render(clouds, disp_prm, rp, transforms=None):
    return render_stream(do.display(clouds, disp_prm, transforms), rp)
