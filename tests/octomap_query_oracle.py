"""The read side of the occupancy map (include/rgbdfe.h, "occupancy map: the read side"), restated on the CPU.

A scalar transcription: one np.float32 / Python-float operation per operation of the contract, the leaves in a dict, rays
walked one at a time.  It works on the 16-byte leaf records octomap_oracle.LiteralMap.leaves() gives (and
rgbdfe_octomap_leaves, rgbdfe_octomap_set_leaves take), and gives its results as the records of the C ABI; the tests
compare bytes.  cases() are the inputs the emulation test and the GPU test share; expected() is computed once per case.

The octomap library is not on this machine: nothing here is pinned against it."""
import functools
import math

import numpy as np

import octomap_oracle as oo

F = np.float32
DBL_MAX = oo.DBL_MAX
MAX_STEPS = oo.MAX_STEPS
LEAF = oo.LEAF
HIT_REC = np.dtype([("status", "<i4"), ("steps", "<u4"), ("key", "<u2", (3,)), ("zero0", "<u2"), ("centre", "<f4", (3,)),
                    ("log_odds", "<f4"), ("rgb", "u1", (3,)), ("zero1", "u1")])
assert HIT_REC.itemsize == 36
HIT, UNKNOWN, OUT_OF_RANGE, OUT_OF_BOUNDS, BAD_ORIGIN, BAD_DIRECTION, STEP_LIMIT = range(1, 8)
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def finite(v):
    return bool(np.isfinite(v))


class QueryOracle:
    def __init__(self, leaves, resolution=0.05, occupancy_threshold=0.5):
        self.res = float(resolution)
        self.inv = 1.0 / self.res
        self.threshold = float(occupancy_threshold)
        self.leaf = {}  # packed key -> (float32 log-odds, (r, g, b))
        for l in np.asarray(leaves, LEAF).reshape(-1):
            self.leaf[oo.pack(*l["key"])] = (F(l["log_odds"]), tuple(int(c) for c in l["rgb"]))

    def occupied_log_odds(self):
        assert 0.0 < self.threshold < 1.0
        return oo.logodds(self.threshold)

    def key1(self, c):
        v = self.inv * float(c)
        if not math.isfinite(v):
            return None
        k = math.floor(v) + 32768
        return k if 0 <= k < 65536 else None

    def key(self, p):
        if not all(finite(c) for c in p):
            return None
        k = [self.key1(c) for c in p]
        return None if None in k else k

    def centre(self, k):
        return (float(k - 32768) + 0.5) * self.res

    # ---- search
    def search(self, points):
        pts = np.asarray(points, np.float32).reshape(-1, 3)
        found, recs = np.zeros(len(pts), np.int32), np.zeros(len(pts), LEAF)
        for i, p in enumerate(pts):
            k = self.key(p)
            if k is None:
                found[i] = 2
                continue
            recs["key"][i] = k
            leaf = self.leaf.get(oo.pack(*k))
            if leaf is not None:
                found[i] = 1
                recs["log_odds"][i] = leaf[0]
                recs["rgb"][i] = leaf[1]
        return found, recs

    # ---- castRay
    def ray(self, o, d, ignore_unknown, max_range, occupied):
        """(status, steps, key or None, (log-odds, rgb) or None) of one ray; o, d: three np.float32 each."""
        k = self.key(o)
        if k is None:
            return BAD_ORIGIN, 0, None, None
        leaf = self.leaf.get(oo.pack(*k))
        if leaf is not None:
            if leaf[0] >= occupied:
                return HIT, 0, k, leaf
        elif not ignore_unknown:
            return UNKNOWN, 0, k, None
        n = math.sqrt(float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if not n > 0.0:
            return BAD_DIRECTION, 0, k, None
        fn = F(n)
        u = [d[a] / fn for a in range(3)]
        if not all(finite(c) for c in u):
            return BAD_DIRECTION, 0, k, None
        step = [1 if u[a] > 0 else (-1 if u[a] < 0 else 0) for a in range(3)]
        if step == [0, 0, 0]:
            return BAD_DIRECTION, 0, k, None
        tM, tD = [DBL_MAX] * 3, [DBL_MAX] * 3
        for a in range(3):
            if step[a] != 0:
                border = self.centre(k[a]) + (float(step[a]) * self.res) * 0.5
                tM[a] = (border - float(o[a])) / float(u[a])
                tD[a] = self.res / abs(float(u[a]))
        k = list(k)
        c = [F(self.centre(k[a])) for a in range(3)]
        range2 = max_range * max_range if max_range > 0.0 else -1.0
        for it in range(MAX_STEPS):
            a = (0 if tM[0] < tM[2] else 2) if tM[0] < tM[1] else (1 if tM[1] < tM[2] else 2)
            if (step[a] < 0 and k[a] == 0) or (step[a] > 0 and k[a] == 65535):
                return OUT_OF_BOUNDS, it, k, None
            k[a] += step[a]
            tM[a] += tD[a]
            c[a] = F(self.centre(k[a]))
            if range2 >= 0.0:
                q = [c[b] - o[b] for b in range(3)]
                s = (float(q[0] * q[0]) + float(q[1] * q[1])) + float(q[2] * q[2])
                if s > range2:
                    return OUT_OF_RANGE, it + 1, k, None
            leaf = self.leaf.get(oo.pack(*k))
            if leaf is not None:
                if leaf[0] >= occupied:
                    return HIT, it + 1, k, leaf
            elif not ignore_unknown:
                return UNKNOWN, it + 1, k, None
        return STEP_LIMIT, MAX_STEPS, k, None

    def _occupied(self, occupied_log_odds):
        if occupied_log_odds is None or math.isnan(float(occupied_log_odds)):
            return self.occupied_log_odds()
        return F(occupied_log_odds)

    def cast_rays(self, origins, directions, ignore_unknown=False, max_range=-1.0, occupied_log_odds=None):
        O = np.asarray(origins, np.float32).reshape(-1, 3)
        D = np.asarray(directions, np.float32).reshape(-1, 3)
        occ = self._occupied(occupied_log_odds)
        out = np.zeros(len(O), HIT_REC)
        with np.errstate(all="ignore"):
            for i in range(len(O)):
                st, steps, k, leaf = self.ray(O[i], D[i], bool(ignore_unknown), float(max_range), occ)
                out["status"][i], out["steps"][i] = st, steps
                if k is not None:
                    out["key"][i] = k
                    out["centre"][i] = [F(self.centre(k[a])) for a in range(3)]
                if st == HIT:
                    out["log_odds"][i] = leaf[0]
                    out["rgb"][i] = leaf[1]
        return out

    # ---- the map seen from a pose
    def view_cloud(self, T, fx, fy, cx, cy, rows, cols, ignore_unknown=False, max_range=-1.0, occupied_log_odds=None):
        """T: column-major Matrix4f (16 floats).  -> (cloud [rows, cols, 4] float32, status [rows, cols] uint8)."""
        R, o = oo.split_transform(T)
        fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
        occ = self._occupied(occupied_log_odds)
        cloud = np.zeros((rows, cols, 4), np.float32)
        cloud[:, :, :3] = QNAN
        status = np.zeros((rows, cols), np.uint8)
        words = cloud.view(np.uint32)
        with np.errstate(all="ignore"):
            for v in range(rows):
                for u in range(cols):
                    x, y = (F(u) - cx) / fx, (F(v) - cy) / fy
                    d = [(R[a, 0] * x + R[a, 1] * y) + R[a, 2] for a in range(3)]
                    st, _, k, leaf = self.ray(o, d, bool(ignore_unknown), float(max_range), occ)
                    status[v, u] = st
                    if st == HIT:
                        q = [F(self.centre(k[a])) - o[a] for a in range(3)]
                        for c in range(3):
                            cloud[v, u, c] = (R[0, c] * q[0] + R[1, c] * q[1]) + R[2, c] * q[2]
                        words[v, u, 3] = (leaf[1][0] << 16) | (leaf[1][1] << 8) | leaf[1][2]
        return cloud, status


# ---------------------------------------------------------------------------------------------- the table, for the tests
def home_slot(key, cap):
    """The slot a packed key's probe run starts at (the 64-bit finaliser of MurmurHash3, scaled to cap)."""
    m = (1 << 64) - 1
    h = key
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & m
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & m
    h ^= h >> 33
    return ((h >> 32) * cap) >> 32


def keys_with_home(cap, homes, n, start=oo.pack(32768, 32768, 32768)):
    """The first n packed keys from `start` on (x ascending) whose home slot in a table of `cap` slots is in `homes`."""
    out, k = [], start
    while len(out) < n:
        if home_slot(k, cap) in homes:
            out.append(k)
        k += 1
    return out


# ---------------------------------------------------------------------------------------------- inputs
def leaves_of(cells, res=None):
    """{(cx, cy, cz) cell index: (log-odds, (r, g, b))} -> LEAF records."""
    return oo.records([(oo.pack(c[0] + 32768, c[1] + 32768, c[2] + 32768), F(v), rgb) for c, (v, rgb) in cells.items()])


def centre_of(cell, res):
    return [F((c + 0.5) * res) for c in cell]


PLANTED_RES = 0.25           # a power of two: centres, diagonals and range ends are exact in float, so the ties are
PLANTED_THRESHOLD = 0.7
EDGE = 32767                 # cell index of key 65535; -32768 is key 0


def planted_scene():
    """One map for every branch of the contract; the cells are named by their index (key - 32768)."""
    thr = oo.logodds(PLANTED_THRESHOLD)
    below = np.nextafter(thr, F(-10.0))
    occ, free = F(2.0), F(-1.0)
    cells = {}
    col = iter(range(1, 1 << 20, 7919))

    def put(cell, v):
        c = next(col) * 97 & 0xffffff
        cells[tuple(cell)] = (v, ((c >> 16) & 255, (c >> 8) & 255, c & 255))

    put((0, 0, 0), free)                         # the common origin: a free leaf
    for a in range(3):                           # axis-parallel rays: a free leaf on the way, then an occupied one
        for s in (1, -1):
            e = [0, 0, 0]
            e[a] = 5 * s
            put(e, free)
            e[a] = 10 * s
            put(e, occ)
    # ties: from (20, 20, 20) in x and y, from (40, 40, 40) in all three, in both directions: the later axis moves first
    put((20, 20, 20), free)
    put((21, 20, 20), occ), put((20, 21, 20), occ)
    put((19, 20, 20), occ), put((20, 19, 20), occ)
    put((40, 40, 40), free)
    for s in (1, -1):
        put((40 + s, 40, 40), occ), put((40, 40 + s, 40), occ), put((40, 40, 40 + s), occ)
    put((63, 63, 60), occ)                       # a longer diagonal from the unknown cell (60, 60, 60)
    # the threshold: the map's own (NaN) and a per-call one (0.5)
    put((100, 0, 0), free)
    put((103, 0, 0), below), put((105, 0, 0), thr), put((107, 0, 0), occ)
    put((100, 3, 0), np.nextafter(F(0.5), F(0.0))), put((100, 5, 0), F(0.5)), put((100, 7, 0), occ)
    put((-50, -50, -50), occ)                    # an origin inside an occupied cell
    # the edges of the key range: free leaves three cells in, on each axis at both ends
    for a in range(3):
        for end in (EDGE, -EDGE - 1):
            e = [7, 7, 7]
            e[a] = end - 3 if end > 0 else end + 3
            put(e, free)
    return dict(resolution=PLANTED_RES, occupancy_threshold=PLANTED_THRESHOLD, leaves=leaves_of(cells))


def planted_rays():
    """[(name, origin, direction, ignore_unknown, max_range, occupied_log_odds or None)] on planted_scene()."""
    r = PLANTED_RES
    C = lambda *cell: centre_of(cell, r)
    o0 = C(0, 0, 0)
    nan, inf = F(np.nan), F(np.inf)
    out = []
    out.append(("origin occupied", C(-50, -50, -50), (1, 0, 0), 0, -1.0, None))
    out.append(("origin unknown", C(-60, -50, -50), (1, 0, 0), 0, -1.0, None))
    out.append(("origin unknown, ignored, then occupied", C(-60, -50, -50), (1, 0, 0), 1, -1.0, None))
    out.append(("origin key invalid", (F(8192.0), 0, 0), (1, 0, 0), 1, -1.0, None))
    out.append(("origin key invalid below", (0, F(-8192.5), 0), (1, 0, 0), 1, -1.0, None))
    out.append(("origin nan", (0, nan, 0), (1, 0, 0), 1, -1.0, None))
    out.append(("origin inf", (0, 0, -inf), (1, 0, 0), 1, -1.0, None))
    out.append(("direction zero", o0, (0, 0, 0), 0, -1.0, None))
    out.append(("direction nan", o0, (0, nan, 1), 0, -1.0, None))
    out.append(("direction inf", o0, (inf, 0, 0), 0, -1.0, None))
    out.append(("direction underflows", o0, (F(1e-30), F(-1e-30), 0), 0, -1.0, None))
    out.append(("direction overflows", o0, (F(1e30), 0, 0), 0, -1.0, None))
    out.append(("direction tiny but normal", o0, (F(1e-15), 0, 0), 0, 1.5, None))
    for a in range(3):
        for s in (1, -1):
            d = [0, 0, 0]
            d[a] = s * 3
            out.append(("axis %d %+d" % (a, s), o0, d, 1, -1.0, None))
            out.append(("axis %d %+d, unknown stops" % (a, s), o0, d, 0, -1.0, None))
    out.append(("tie xy +", C(20, 20, 20), (1, 1, 0), 1, -1.0, None))
    out.append(("tie xy -", C(20, 20, 20), (-2, -2, 0), 1, -1.0, None))
    out.append(("tie xyz +", C(40, 40, 40), (1, 1, 1), 1, -1.0, None))
    out.append(("tie xyz -", C(40, 40, 40), (-1, -1, -1), 1, -1.0, None))
    out.append(("diagonal through unknown", C(60, 60, 60), (1, 1, 0), 1, -1.0, None))
    out.append(("threshold of the map", C(100, 0, 0), (1, 0, 0), 1, -1.0, None))
    out.append(("threshold of the map as NaN", C(100, 0, 0), (1, 0, 0), 1, -1.0, float("nan")))
    out.append(("threshold of the call", C(100, 0, 0), (0, 1, 0), 1, -1.0, 0.5))
    out.append(("threshold above every leaf", C(100, 0, 0), (0, 1, 0), 1, 3.0, 2.5))
    out.append(("threshold -inf: the free leaf is occupied", o0, (0, 0, 1), 1, -1.0, -np.inf))
    # the range: from the exact centre of (0, 0, 0) along +z the squared distance to cell j is (j / 4)^2 exactly
    one_less = math.nextafter(1.0, 0.0)
    out.append(("range equal goes on", o0, (0, 0, 1), 1, 1.0, None))           # OUT_OF_RANGE at cell 5
    out.append(("range one ulp less stops", o0, (0, 0, 1), 1, one_less, None))  # OUT_OF_RANGE at cell 4
    out.append(("range equal at the hit", o0, (0, 0, 1), 1, 2.5, None))        # HIT at cell 10
    out.append(("range one ulp less at the hit", o0, (0, 0, 1), 1, math.nextafter(2.5, 0.0), None))
    out.append(("range zero", o0, (0, 0, 1), 1, 0.0, None))
    out.append(("range negative", o0, (0, 0, 1), 1, -3.0, None))
    out.append(("range inf", o0, (0, 0, 1), 1, math.inf, None))
    for a in range(3):
        for end in (EDGE, -EDGE - 1):
            s = 1 if end > 0 else -1
            e = [7, 7, 7]
            e[a] = end - 3 * s
            d = [0, 0, 0]
            d[a] = s
            out.append(("off the edge axis %d %+d" % (a, s), C(*e), d, 1, -1.0, None))
            e[a] = end
            d[(a + 1) % 3] = F(0.001)
            out.append(("off the edge at once axis %d %+d" % (a, s), C(*e), d, 1, -1.0, None))
    return out


def rays_arrays(rays):
    O = np.array([[F(c) for c in r[1]] for r in rays], np.float32)
    D = np.array([[F(c) for c in r[2]] for r in rays], np.float32)
    return O, D


def random_scene(seed=11, n=600, half=12, res=0.1, threshold=0.5):
    """n leaves at random cells of a cube of (2 * half)^3 cells around the origin, about half of them occupied."""
    rng = np.random.default_rng(seed)
    cells = {}
    while len(cells) < n:
        c = tuple(int(v) for v in rng.integers(-half, half, 3))
        w = int(rng.integers(0, 1 << 24))
        cells[c] = (F(rng.uniform(-2.0, 3.5)), ((w >> 16) & 255, (w >> 8) & 255, w & 255))
    return dict(resolution=res, occupancy_threshold=threshold, leaves=leaves_of(cells))


def random_rays(n, seed, half=12, res=0.1):
    rng = np.random.default_rng(seed)
    O = rng.uniform(-half * res, half * res, (n, 3)).astype(np.float32)
    D = rng.normal(size=(n, 3)).astype(np.float32)
    D[::7, int(seed) % 3] = 0.0  # some rays in a coordinate plane
    return O, D


def look_at(eye, target, roll=0.0):
    """Column-major Matrix4f camera -> world: +z from eye towards target, rolled about it."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = math.cos(roll), math.sin(roll)
    x, y = c * x + s * y, -s * x + c * y
    T = np.eye(4, dtype=np.float32)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return np.ascontiguousarray(T.T).reshape(16)


def wrap_scene(cap=16):
    """Six leaves whose home slots are the last two of a table of `cap` slots: the probe runs wrap past its end."""
    ks = keys_with_home(cap, (cap - 2, cap - 1), 9)
    leaves = oo.records([(k, F(1.0 + i), (i, 2 * i, 3 * i)) for i, k in enumerate(ks[:6])])
    return dict(resolution=0.1, occupancy_threshold=0.5, leaves=leaves, capacity=cap), ks


def points_of_keys(keys, res):
    """The float centres of packed keys."""
    return np.array([[F((((k >> (16 * a)) & 0xffff) - 32768 + 0.5) * res) for a in range(3)] for k in keys], np.float32)


VIEW_SHAPES = ((1, 1), (8, 8), (9, 7), (65, 3), (64, 48))


def cases():
    """[(name, scene, query)]: scene = dict(resolution, occupancy_threshold, leaves[, capacity][, claimed]); query =
    ("search", points) | ("cast", origins, directions, ignore_unknown, max_range, occupied_log_odds or None) |
    ("view", T, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range, occupied_log_odds or None)."""
    out = []
    ps = planted_scene()
    # every planted ray in a call of its own parameters: rays grouped by (ignore_unknown, max_range, threshold)
    groups = {}
    for r in planted_rays():
        groups.setdefault((r[3], r[4], None if r[5] is None else repr(float(r[5]))), []).append(r)
    for (ign, mr, _), rays in groups.items():
        O, D = rays_arrays(rays)
        out.append(("planted rays ign %d range %r thr %r (%d)" % (ign, mr, rays[0][5], len(rays)), ps,
                    ("cast", O, D, ign, mr, rays[0][5])))
    lv = ps["leaves"]
    pts = points_of_keys([oo.pack(*k) for k in lv["key"]], PLANTED_RES)
    shifted = pts + np.asarray([0.0, 0.0, 1000 * PLANTED_RES], np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 8192.0], [-8192.5, 0, 0], [8191.875, -8192.0, 0]], np.float32)
    out.append(("planted search", ps, ("search", np.concatenate([pts, shifted, bad]))))
    rs = random_scene()
    for n in (1, 63, 64, 65, 257):
        O, D = random_rays(n, seed=100 + n)
        out.append(("random rays %d" % n, rs, ("cast", O, D, 0, -1.0, None)))
        out.append(("random rays %d ignoring unknown" % n, rs, ("cast", O, D, 1, 1.7, 1.0)))
        P = np.concatenate([O, points_of_keys([oo.pack(*k) for k in rs["leaves"]["key"][:n]], 0.1)])
        out.append(("random search %d" % len(P), rs, ("search", P)))
    ws, ks = wrap_scene()
    out.append(("wrapping probe runs", ws, ("search", points_of_keys(ks, 0.1))))
    O = points_of_keys(ks[6:], 0.1)  # from unknown cells whose probe runs wrap, along +x through the others
    out.append(("wrapping probe runs, rays", ws, ("cast", O, np.tile(np.asarray([[1, 0, 0]], np.float32), (len(O), 1)), 1, 5.0, None)))
    # views: a tilted pose outside the cube looking in, a pose inside an occupied cell, a pose looking out of the map
    occ_cell = rs["leaves"]["key"][np.argmax(rs["leaves"]["log_odds"])].astype(np.int64) - 32768
    poses = {"tilted": look_at((2.9, -2.3, 1.7), (0.1, 0.05, -0.1), roll=0.3),
             "inside an occupied cell": look_at([(c + 0.4) * 0.1 for c in occ_cell], (0.0, 0.0, 0.0), roll=-0.2),
             "looking out": look_at((2.9, -2.3, 1.7), (6.0, -5.0, 4.0), roll=0.1)}
    ranges = {"tilted": 5.5, "inside an occupied cell": 6.0, "looking out": 2.0}  # (a ray that meets nothing walks this far)
    for rows, cols in VIEW_SHAPES:
        f = 1.2 * cols
        for pname, T in poses.items():
            out.append(("view %dx%d %s" % (rows, cols, pname), rs,
                        ("view", T, max(f, 4.0), max(f, 4.0) * 1.05, cols / 2 - 0.5, rows / 2 - 0.25, rows, cols, 1,
                         ranges[pname], None)))
    out.append(("view 9x7 unknown stops", rs, ("view", poses["tilted"], 9.0, 9.0, 3.0, 4.0, 9, 7, 0, -1.0, 0.25)))
    return out


def load_rule_inputs():
    """(13 leaves, queries): in a table of 16 slots the first 12 leaves are exactly 3/4 (accepted), all 13 one too many."""
    rng = np.random.default_rng(5)
    cells = {}
    while len(cells) < 13:
        cells[tuple(int(v) for v in rng.integers(-3, 3, 3))] = (float(rng.uniform(0.5, 2.0)), (len(cells), 7, 9))
    lv13 = leaves_of(cells)
    O, D = random_rays(65, seed=9, half=3, res=0.1)
    P = np.concatenate([O, points_of_keys([oo.pack(*k) for k in lv13["key"]], 0.1)])
    T = look_at((0.9, -0.8, 0.6), (0.0, 0.0, 0.0), roll=0.2)
    return lv13, (("search", P), ("cast", O, D, 1, 1.5, None), ("view", T, 10.0, 10.0, 4.0, 3.0, 7, 9, 1, 2.5, None))


@functools.lru_cache(maxsize=None)
def raster_view():
    """End to end: (points, T, leaves, view query, expected view) of the 64 x 48 raster inserted at 0.1 m and seen from the
    pose it was inserted from, with the raster's intrinsics."""
    res, w, h, fx = 0.1, 64, 48, 52.5
    pts, T = oo.raster(w, h), oo.rigid(41)
    lit = oo.LiteralMap(resolution=res)
    lit.insert(pts, T, -1.0)
    lv = lit.leaves()
    query = ("view", T, fx, fx, w / 2 - 0.5, h / 2 - 0.5, h, w, 0, -1.0, None)
    scene = dict(resolution=res, occupancy_threshold=0.5, leaves=lv)
    return pts, T, scene, query, run(scene, query)


def oracle_of(scene):
    return QueryOracle(scene["leaves"], scene["resolution"], scene["occupancy_threshold"])


def run(scene, query):
    q = oracle_of(scene)
    if query[0] == "search":
        return q.search(query[1])
    if query[0] == "cast":
        return q.cast_rays(*query[1:])
    return q.view_cloud(*query[1:])


@functools.lru_cache(maxsize=None)
def _expected(name):
    scene, query = CASES[name]
    return run(scene, query)


def expected(name):
    """The oracle's result of a case, computed once."""
    return _expected(name)


CASES = {c[0]: (c[1], c[2]) for c in cases()}
