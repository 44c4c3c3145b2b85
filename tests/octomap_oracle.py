"""The occupancy map of include/rgbdfe.h ("occupancy map"), restated twice on the CPU.

LiteralMap is a scalar transcription: one np.float32 / Python-float operation per operation of the contract, a dict of
leaves, rays walked one at a time.  LockstepMap has another organisation: all rays of a cloud advance together in numpy
arrays, the leaves live in sorted arrays, and the colours are applied in rounds (the m-th sample of every cell at once).
Both give their leaves as the 16-byte records of rgbdfe_octomap_leaves, in its order; the tests compare bytes.

The octomap library is not on this machine: neither class is pinned against it."""
import math
import sys

import numpy as np

F = np.float32
DBL_MAX = sys.float_info.max
MAX_STEPS = 3 * 65536
LEAF = np.dtype([("key", "<u2", (3,)), ("zero0", "<u2"), ("log_odds", "<f4"), ("rgb", "u1", (3,)), ("zero1", "u1")])
assert LEAF.itemsize == 16
DEFAULTS = dict(resolution=0.05, prob_hit=0.9, prob_miss=0.4, clamping_min=0.001, clamping_max=0.999)


def logodds(p):
    return F(math.log(p / (1.0 - p)))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def split_transform(T):
    """Column-major Matrix4f (16 floats) -> (R 3x3, t 3) float32."""
    M = np.asarray(T, np.float32).reshape(4, 4).T
    return M[:3, :3].copy(), M[:3, 3].copy()


def pack(k0, k1, k2):
    return int(k0) | (int(k1) << 16) | (int(k2) << 32)


def records(items):
    """[(packed key, log-odds, (r, g, b))] -> LEAF records in ascending packed key."""
    items = sorted(items, key=lambda it: it[0])
    out = np.zeros(len(items), LEAF)
    for i, (k, v, c) in enumerate(items):
        out["key"][i] = (k & 0xffff, (k >> 16) & 0xffff, (k >> 32) & 0xffff)
        out["log_odds"][i] = v
        out["rgb"][i] = c
    return out


# ---------------------------------------------------------------------------------------------- the literal transcription
class LiteralMap:
    def __init__(self, **kw):
        self.p = params(**kw)
        self.res = float(self.p["resolution"])
        self.inv = 1.0 / self.res
        self.hit, self.miss = logodds(self.p["prob_hit"]), logodds(self.p["prob_miss"])
        self.cmin, self.cmax = logodds(self.p["clamping_min"]), logodds(self.p["clamping_max"])
        self.leaf = {}  # packed key -> [float32 log-odds, [r, g, b]]
        self.stats = {}

    def reset(self):
        self.leaf = {}

    def key1(self, c):
        v = self.inv * float(c)
        if not math.isfinite(v):
            return None
        k = math.floor(v) + 32768
        return k if 0 <= k < 65536 else None

    def key(self, p):
        k = [self.key1(c) for c in p]
        return None if None in k else k

    def norm(self, d):
        return math.sqrt(float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))

    def ray(self, o, e, free, st):
        ko, ke = self.key(o), self.key(e)
        if ko is None or ke is None or ko == ke:
            return
        free.add(pack(*ko))
        st["visits"] += 1
        d = [e[a] - o[a] for a in range(3)]
        length = F(self.norm(d))
        u = [d[a] / length for a in range(3)]
        step = [1 if u[a] > 0 else (-1 if u[a] < 0 else 0) for a in range(3)]
        tM, tD = [DBL_MAX] * 3, [DBL_MAX] * 3
        for a in range(3):
            if step[a] != 0:
                border = (float(ko[a] - 32768) + 0.5) * self.res + float(F(step[a] * self.res * 0.5))
                tM[a] = (border - float(o[a])) / float(u[a])
                tD[a] = self.res / abs(float(u[a]))
        k = list(ko)
        for _ in range(MAX_STEPS):
            a = (0 if tM[0] < tM[2] else 2) if tM[0] < tM[1] else (1 if tM[1] < tM[2] else 2)
            k[a] = (k[a] + step[a]) & 0xffff
            tM[a] += tD[a]
            if k == ke:
                return
            if min(tM[0], min(tM[1], tM[2])) > float(length):
                st["early_stops"] += 1
                return
            free.add(pack(*k))
            st["visits"] += 1

    def insert(self, pts, T, max_range=-1.0, colour_order="index"):
        pts = np.asarray(pts, np.float32).reshape(-1, 4)
        R, o = split_transform(T)
        max_range = float(max_range)
        st = dict(visits=0, early_stops=0)
        free, occ, rows = set(), set(), []
        with np.errstate(all="ignore"):
            for i in range(len(pts)):
                x, y, z = pts[i, 0], pts[i, 1], pts[i, 2]
                if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                    continue
                p = [((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + o[a] for a in range(3)]
                if not all(np.isfinite(c) for c in p):
                    continue
                rows.append((i, p))
                d = [p[a] - o[a] for a in range(3)]
                norm = self.norm(d)
                if max_range < 0.0 or norm <= max_range:
                    self.ray(o, p, free, st)
                    k = self.key(p)
                    if k is not None:
                        occ.add(pack(*k))
                else:
                    fn, fm = F(norm), F(max_range)
                    e = [o[a] + (d[a] / fn) * fm for a in range(3)]
                    self.ray(o, e, free, st)
        st["both"] = len(free & occ)
        free -= occ
        st["free"], st["occupied"] = len(free), len(occ)
        for cells, lo in ((free, self.miss), (occ, self.hit)):
            for k in cells:
                leaf = self.leaf.setdefault(k, [F(0.0), [255, 255, 255]])
                v = F(leaf[0] + lo)
                if v < self.cmin:
                    v = self.cmin
                if v > self.cmax:
                    v = self.cmax
                leaf[0] = v
        # colours
        samples = {}
        for i, p in rows:
            k = self.key(p)
            if k is not None and pack(*k) in self.leaf:
                samples.setdefault(pack(*k), []).append(i)
        st["multi_colour_cells"] = sum(1 for v in samples.values() if len(v) >= 2)
        w = pts.view(np.uint32)[:, 3]
        for k, members in samples.items():
            if colour_order == "reversed":
                members = members[::-1]
            c = self.leaf[k][1]
            for i in members:
                new = [int(w[i] >> 16) & 255, int(w[i] >> 8) & 255, int(w[i]) & 255]
                if c != [255, 255, 255]:
                    c = [(c[a] + new[a]) // 2 for a in range(3)]
                else:
                    c = new
            self.leaf[k][1] = c
        self.stats = st
        return st

    def leaves(self):
        return records([(k, v[0], v[1]) for k, v in self.leaf.items()])

    def __len__(self):
        return len(self.leaf)


# ---------------------------------------------------------------------------------------------- all rays in lockstep
class LockstepMap:
    def __init__(self, **kw):
        self.p = params(**kw)
        self.res = float(self.p["resolution"])
        self.inv = 1.0 / self.res
        self.hit, self.miss = logodds(self.p["prob_hit"]), logodds(self.p["prob_miss"])
        self.cmin, self.cmax = logodds(self.p["clamping_min"]), logodds(self.p["clamping_max"])
        self.reset()

    def reset(self):
        self.keys = np.zeros(0, np.uint64)  # ascending
        self.val = np.zeros(0, np.float32)
        self.col = np.zeros((0, 3), np.int64)
        self.early_stops = 0  # rays that took the min(tMax) > length exit, over all insertions
        self.visits = 0       # free cells with repeats, over all insertions

    def keys_of(self, P):
        """P (n, 3) float32 -> keys (n, 3) int64, valid (n,)."""
        v = self.inv * P.astype(np.float64)
        k = np.floor(v) + 32768.0
        ok = np.all((k >= 0.0) & (k < 65536.0), axis=1)  # NaN and inf fail
        return np.where(ok[:, None], k, 0.0).astype(np.int64), ok

    @staticmethod
    def packed(K):
        K = K.astype(np.uint64)
        return K[:, 0] | (K[:, 1] << np.uint64(16)) | (K[:, 2] << np.uint64(32))

    @staticmethod
    def norms(D):
        return np.sqrt(((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]).astype(np.float64))

    def rays(self, o, E):
        """Free cells (packed, with repeats) of the rays o -> E[i]."""
        n = len(E)
        O = np.broadcast_to(o, (n, 3))
        KO, oko = self.keys_of(np.ascontiguousarray(O))
        KE, oke = self.keys_of(E)
        live = oko & oke & np.any(KO != KE, axis=1)
        out = [self.packed(KO[live])]
        D = E - O
        length = self.norms(D).astype(np.float32)
        U = D / length[:, None]
        step = (U > 0).astype(np.int64) - (U < 0).astype(np.int64)
        U64 = U.astype(np.float64)
        border = ((KO - 32768).astype(np.float64) + 0.5) * self.res + (step * self.res * 0.5).astype(np.float32).astype(np.float64)
        moving = step != 0
        tM = np.where(moving, (border - O.astype(np.float64)) / np.where(moving, U64, 1.0), DBL_MAX)
        tD = np.where(moving, self.res / np.where(moving, np.abs(U64), 1.0), DBL_MAX)
        K = KO.copy()
        L = length.astype(np.float64)
        rows = np.arange(n)
        for _ in range(MAX_STEPS):
            if not live.any():
                break
            a = np.where(tM[:, 0] < tM[:, 1], np.where(tM[:, 0] < tM[:, 2], 0, 2), np.where(tM[:, 1] < tM[:, 2], 1, 2))
            r = rows[live]
            K[r, a[r]] = (K[r, a[r]] + step[r, a[r]]) & 0xffff
            tM[r, a[r]] = tM[r, a[r]] + tD[r, a[r]]
            live = live & np.any(K != KE, axis=1)
            early = live & (tM.min(axis=1) > L)
            self.early_stops += int(early.sum())
            live = live & ~early
            out.append(self.packed(K[live]))
        out = np.concatenate(out)
        self.visits += len(out)
        return out

    def insert(self, pts, T, max_range=-1.0):
        pts = np.asarray(pts, np.float32).reshape(-1, 4)
        R, o = split_transform(T)
        max_range = float(max_range)
        with np.errstate(all="ignore"):
            X = pts[:, :3]
            fin = np.isfinite(X).all(axis=1)
            idx = np.nonzero(fin)[0]
            X = X[idx]
            P = np.stack([((R[a, 0] * X[:, 0] + R[a, 1] * X[:, 1]) + R[a, 2] * X[:, 2]) + o[a] for a in range(3)], axis=1)
            fin = np.isfinite(P).all(axis=1)
            idx, P = idx[fin], np.ascontiguousarray(P[fin])
            D = P - o[None, :]
            norm = self.norms(D)
            near = np.full(len(P), True) if max_range < 0.0 else norm <= max_range
            E = P.copy()
            far = ~near
            E[far] = o[None, :] + (D[far] / norm[far].astype(np.float32)[:, None]) * F(max_range)
            free = np.unique(self.rays(o, E))
            KP, okp = self.keys_of(P)
            occ = np.unique(self.packed(KP[okp & near]))
        free = np.setdiff1d(free, occ, assume_unique=True)
        # the leaves, old and new, in one sorted array
        allk = np.union1d(self.keys, np.union1d(free, occ))
        val = np.zeros(len(allk), np.float32)
        col = np.full((len(allk), 3), 255, np.int64)
        at = np.searchsorted(allk, self.keys)
        val[at], col[at] = self.val, self.col
        for cells, lo in ((free, self.miss), (occ, self.hit)):
            at = np.searchsorted(allk, cells)
            val[at] = np.minimum(np.maximum(val[at] + lo, self.cmin), self.cmax)
        # colours: the m-th sample of every cell, round by round
        pk = self.packed(KP[okp])
        rows = idx[okp]
        at = np.searchsorted(allk, pk)
        at[at == len(allk)] = 0
        has = allk[at] == pk if len(allk) else np.zeros(len(pk), bool)
        at, rows = at[has], rows[has]
        order = np.argsort(at, kind="stable")
        at, rows = at[order], rows[order]
        first = np.r_[True, at[1:] != at[:-1]] if len(at) else np.zeros(0, bool)
        start = np.nonzero(first)[0]
        rank = np.arange(len(at)) - np.repeat(start, np.diff(np.r_[start, len(at)]))
        w = pts.view(np.uint32)[:, 3].astype(np.int64)
        new_all = np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], axis=1)
        m = 0
        while len(at) and (rank == m).any():
            sel = rank == m
            cell, new = at[sel], new_all[rows[sel]]
            is_set = (col[cell] != 255).any(axis=1)
            col[cell] = np.where(is_set[:, None], (col[cell] + new) // 2, new)
            m += 1
        self.keys, self.val, self.col = allk, val, col

    def leaves(self):
        out = np.zeros(len(self.keys), LEAF)
        out["key"][:, 0] = self.keys & np.uint64(0xffff)
        out["key"][:, 1] = (self.keys >> np.uint64(16)) & np.uint64(0xffff)
        out["key"][:, 2] = (self.keys >> np.uint64(32)) & np.uint64(0xffff)
        out["log_odds"] = self.val
        out["rgb"] = self.col
        return out

    def __len__(self):
        return len(self.keys)


# ---------------------------------------------------------------------------------------------- inputs
ORIGIN = (0.013, -0.021, 0.007)


def translation(t=ORIGIN):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = np.asarray(t, np.float32)
    return np.ascontiguousarray(T.T).reshape(16)  # column-major


def rigid(seed, spread=0.5):
    """A random rigid transform as a column-major Matrix4f."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R.astype(np.float32)
    T[:3, 3] = rng.uniform(-spread, spread, 3).astype(np.float32)
    return np.ascontiguousarray(T.T).reshape(16)


def rgb_words(rng, n):
    return rng.integers(0, 1 << 24, n, dtype=np.uint32)


def with_rgb(xyz, rgb):
    pts = np.zeros((len(xyz), 4), np.float32)
    pts[:, :3] = xyz
    pts.view(np.uint32)[:, 3] = rgb
    return pts


def raster(w=64, h=48, seed=0, fx=52.5, lo=2.0, hi=3.5, holes=True):
    """A w x h depth raster as createXYZRGBPointCloud leaves it: depth lo..hi m, a few rows without depth (NaN z beside
    finite x, y, or all NaN)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(lo, hi, (h, w)).astype(np.float32)
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    x = (u - F(w / 2 - 0.5)) / F(fx) * z
    y = (v - F(h / 2 - 0.5)) / F(fx) * z
    pts = with_rgb(np.stack([x, y, z], axis=-1).reshape(-1, 3), rgb_words(rng, w * h))
    if holes:
        n = w * h
        k = max(1, n // 40)
        pts[rng.choice(n, k, replace=False), 2] = np.nan
        pts[rng.choice(n, k, replace=False), :3] = np.nan
    return pts


def cloud(n, seed=0, **kw):
    """The first n rows of a raster that has at least n."""
    w = 64
    h = max(1, -(-n // w))
    return raster(w, h, seed=seed, **kw)[:n].copy()


# Of the first hundred seeds from 1000 on, this is the one whose 64 x 48 raster has a ray that leaves through the
# min(tMax) > length exit (at resolutions 0.05 and 0.1, range off).  At random the exit is taken by about 3 rays in a
# million (2 of 1.8 million measured): the end point must lie within float rounding of a cell face.
RASTER_SEED = 1006


def full_raster():
    return raster(64, 48, seed=RASTER_SEED)


def planted(res):
    """(points, transform): the rays the contract's branches need, seen from the centre of cell (3, -2, 5).  With a
    power-of-two resolution the centre, the diagonal ends and the range ends are exact in float, so the tMax ties are."""
    c = [(k + 0.5) * res for k in (3, -2, 5)]
    nxt = np.nextafter(F(2.5), F(10.0))
    xyz = [
        (0.1 * res, 0.0, 0.0),                      # origin and end in one cell
        (1.25, 0.0, 0.0), (0.0, -1.25, 0.0), (0.0, 0.0, 2.0),  # axis-aligned: two zero steps
        (0.0, 0.0, 1.0),                            # its end cell lies on the ray before it: occupied wins
        (1.5, 1.5, 0.0), (1.25, 1.25, 1.25), (-1.25, 1.25, -1.25),  # two-way and three-way ties
        (-0.7, -1.1, -0.4), (-1.0, -1.0, -1.0),     # negative directions
        (0.0, 0.0, 2.5), (0.0, 0.0, nxt), (0.0, -2.5, 0.0), (0.0, -nxt, 0.0),  # at the range and one ulp beyond
        (33000.0 * res, 0.3, 0.2), (3e38, 0.0, 0.0),  # keys out of the 16-bit range
        (0.3, 0.2, np.nan), (np.nan, 0.2, 1.0), (np.inf, 0.2, 1.0), (0.3, -np.inf, 1.0), (0.3, 0.2, np.inf),
        (0.4, 0.3, 1.7),
    ]
    rng = np.random.default_rng(5)
    return with_rgb(np.asarray(xyz, np.float32), rgb_words(rng, len(xyz))), translation(c)


def one_cell(n=5000, seed=3, res=0.4):
    """n points inside one cell, random colours."""
    rng = np.random.default_rng(seed)
    xyz = np.asarray([0.4 * 2 + 0.02, 0.4 * 1 + 0.02, 0.4 * 5 + 0.02], np.float32) + rng.uniform(0, 0.35, (n, 3)).astype(np.float32)
    return with_rgb(xyz, rgb_words(rng, n))


def two_cells(n=400, seed=4):
    pts = one_cell(n, seed)
    pts[1::2, 0] += F(0.4)
    return pts


def white_sequence():
    """Samples of one cell: white on an unset leaf leaves it unset, so the average starts again behind it."""
    rgb = np.array([0xffffff, 0xffffff, 0x0a141e, 0xffffff, 0xc86432, 0xfefefe, 0xffffff], np.uint32)
    xyz = np.tile(np.asarray([[0.9, 0.5, 2.1]], np.float32), (len(rgb), 1))
    return with_rgb(xyz, rgb)


def far_into_free():
    """Resolution 0.4, max_range 3.15, origin 0: the second row lies beyond the range, inside cell (0, 0, 7), which the
    first row's ray leaves free on its way to (1, 0, 7)."""
    return with_rgb(np.asarray([(0.41, 0.1, 3.1), (0.05, 0.05, 3.18)], np.float32), np.array([0x112233, 0x445566], np.uint32))


def shifted(T, dz):
    T = np.array(T, np.float32)
    T[14] += F(dz)
    return T


def cases():
    """(name, params, [(points, transform, max_range), ...]): every input family of the GPU test, each a list of
    insertions into one map."""
    out = []
    T0 = translation()
    for res in (0.05, 0.1, 0.4):
        for mr in (-1.0, 2.8):
            for n in (1, 63, 64, 65, 255, 256, 257, 1025, 3072):
                out.append(("n %d res %g range %g" % (n, res, mr), dict(resolution=res), [(full_raster() if n == 3072 else cloud(n, seed=n), T0, mr)]))
    for res in (0.05, 0.25):
        for mr in (-1.0, 2.5):
            pts, T = planted(res)
            out.append(("planted res %g range %g" % (res, mr), dict(resolution=res), [(pts, T, mr)]))
    bad = cloud(64, seed=15)
    bad[:, 1] = np.nan
    out.append(("all invalid", {}, [(bad, T0, -1.0)]))
    out.append(("empty", {}, [(np.zeros((0, 4), np.float32), T0, -1.0)]))
    out.append(("empty between", {}, [(cloud(65, seed=1), T0, -1.0), (np.zeros((0, 4), np.float32), T0, -1.0),
                                      (cloud(63, seed=2), T0, 2.8)]))
    a = cloud(257, seed=21, holes=False)
    T1 = shifted(T0, 1.0)
    out.append(("clamping", {}, [(a, T0, -1.0)] * 20 + [(a, T1, -1.0)] * 20 + [(a, T0, -1.0)] * 5))
    out.append(("other probabilities", dict(prob_hit=0.7, prob_miss=0.45, clamping_min=0.12, clamping_max=0.97),
                [(cloud(255, seed=22), T0, 2.8)] * 4 + [(cloud(255, seed=22), T1, 2.8)] * 4))
    I = translation((0.0, 0.0, 0.0))
    out.append(("5000 in one cell", dict(resolution=0.4), [(one_cell(), I, -1.0)]))
    out.append(("two cells alternating", dict(resolution=0.4), [(two_cells(), I, -1.0)]))
    out.append(("white sequence", dict(resolution=0.4), [(white_sequence(), I, -1.0), (white_sequence()[2:], I, -1.0)]))
    out.append(("far point into a free cell", dict(resolution=0.4), [(far_into_free(), I, 3.15)]))
    for k in range(3):
        out.append(("rigid %d" % k, dict(resolution=0.1), [(cloud(300 + 7 * k, seed=30 + k), rigid(40 + k), 2.8)]))
    return out


def run(case, cls=None):
    """The map of a case after its insertions."""
    _, prm, ins = case
    m = (cls or LiteralMap)(**prm)
    for pts, T, mr in ins:
        m.insert(pts, T, mr)
    return m
