"""A plain numpy restatement of observationLikelihood (misc.cpp:814-969), written from the reference's text and
independently of oracle/rgbd_oracle.c, and the planted scenes that tests/test_oracle_emm_reference.py and
tests/test_gpu_emm.py share (every builder is deterministic).

The restatement evaluates math.erf for every sample: no boundary constant enters.  The transform and the projection run
in float32 in the reference's order (pcl::transformPointCloud on a non-dense cloud leaves a point with a non-finite
coordinate untouched), round(float d) is floor(double(d) + 0.5), the 5 x 5 window is clipped to the raster and sampled
with step 2, good beats occluded beats bad.

A scene is a dict: K = (fx, fy, cx, cy) of the depth images, cloud_skip, min_depth, depth_cov, nodes = {id: depth image},
calls = [(emm_skip_step, [(new id, old id, T 4x4 row-major new -> old), ...]), ...] and, where the builder knows them,
expect = [counts per job] per call."""
import math

import numpy as np

F32 = np.float32
GOOD, BAD, OCCLUDED, NONE = 0, 1, 2, -1       # a point's class; the counts are (good, bad, occluded, all)
_erf = np.frompyfunc(math.erf, 1, 1)


# ---- the reference --------------------------------------------------------------------------------------------------------
def observation_likelihood(new_cloud, old_cloud, T, fx, fy, cx, cy, cloud_skip, skip_step, depth_cov):
    """(counts uint32[4], detail) with detail = dict of per-sampled-point arrays: cls, pz, inside, xc, yc, n_samples."""
    ch, cw = old_cloud.shape[:2]
    if skip_step <= 0 or ch <= 1 or cw <= 1:                       # :831, :835
        return np.array([1, 0, 0, 1], np.uint32), None
    T = np.asarray(T, F32)
    s = F32(cloud_skip)
    fx, fy, cx, cy = F32(fx) / s, F32(fy) / s, F32(cx) / s, F32(cy) / s      # :859-862, floats
    pts = np.asarray(new_cloud, F32)[::skip_step, ::skip_step].reshape(-1, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        px = np.where(fin, ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3], x).astype(F32)
        py = np.where(fin, ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3], y).astype(F32)
        pz = np.where(fin, ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3], z).astype(F32)
        alive = ~np.isnan(pz) & ~(pz < 0)                           # :878-879
        rx = np.floor(((px / pz) * fx + cx).astype(np.float64) + 0.5)     # round(), :804-807
        ry = np.floor(((py / pz) * fy + cy).astype(np.float64) + 0.5)
        inside = alive & (rx >= 0) & (rx < cw) & (ry >= 0) & (ry < ch)    # :883-888 (a non-finite centre is outside)
    xc = np.where(inside, rx, 0).astype(np.int64)
    yc = np.where(inside, ry, 0).astype(np.int64)
    startx, starty = np.maximum(0, xc - 2), np.maximum(0, yc - 2)
    endx, endy = np.minimum(cw, xc + 3), np.minimum(ch, yc + 3)
    sigma = math.sqrt(cloud_skip * depth_cov + cloud_skip * depth_cov)    # :903-907
    old_z = np.asarray(old_cloud, F32)[:, :, 2]
    good = np.zeros(len(pts), bool)
    occluded, bad = good.copy(), good.copy()
    n_samples = np.zeros(len(pts), np.int64)
    for j in range(3):
        for k in range(3):
            oy, ox = starty + 2 * j, startx + 2 * k
            sampled = inside & (oy < endy) & (ox < endx)
            oz = old_z[np.where(sampled, oy, 0), np.where(sampled, ox, 0)]
            sampled &= ~np.isnan(oz)                                # :900
            idx = np.flatnonzero(sampled)
            if len(idx) == 0:
                continue
            n_samples[idx] += 1
            arg = (oz[idx].astype(np.float64) - pz[idx].astype(np.float64)) / (sigma * 1.41421)
            p = 0.5 * (1 + _erf(arg).astype(np.float64))           # cdf(), :809-812
            lo, mid = p < 0.001, ~(p < 0.001) & (p < 0.999)
            occluded[idx[lo]] = True
            good[idx[mid]] = True
            bad[idx[~lo & ~mid]] = True
    cls = np.where(good, GOOD, np.where(occluded, OCCLUDED, np.where(bad, BAD, NONE)))
    counts = np.array([(cls == GOOD).sum(), (cls == BAD).sum(), (cls == OCCLUDED).sum(), len(pts)], np.uint32)
    return counts, dict(cls=cls, pz=pz, inside=inside, xc=xc, yc=yc, n_samples=n_samples)


def division_boundary(q, denom):
    """The smallest double d with d / denom >= q (denom > 0): what the host hands the kernel instead of a division."""
    c = q * denom
    while c / denom >= q:
        c = math.nextafter(c, -math.inf)
    while c / denom < q:
        c = math.nextafter(c, math.inf)
    return c


def emm_denominator(cloud_skip, depth_cov):
    return math.sqrt(cloud_skip * depth_cov + cloud_skip * depth_cov) * 1.41421


def run_scene(scene, create_point_cloud):
    """[(counts [n, 4], [detail per job]) per call] of the reference over the scene's clouds."""
    K = scene["K"]
    clouds = {i: create_point_cloud(d, *K, min_depth=scene["min_depth"], cloud_skip=scene["cloud_skip"])
              for i, d in scene["nodes"].items()}
    out = []
    for skip_step, jobs in scene["calls"]:
        res = [observation_likelihood(clouds[n], clouds[o], T, *K, scene["cloud_skip"], skip_step, scene["depth_cov"])
               for n, o, T in jobs]
        out.append((np.array([r[0] for r in res], np.uint32).reshape(-1, 4), [r[1] for r in res]))
    return out, clouds


# ---- builders -------------------------------------------------------------------------------------------------------------
def _translation(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4, dtype=F32)
    T[0, 3], T[1, 3], T[2, 3] = tx, ty, tz
    return T


def _scene(name, K, nodes, calls, cloud_skip=1, depth_cov=1e-4, expect=None, **extra):
    return dict(name=name, K=K, cloud_skip=cloud_skip, min_depth=0.01, depth_cov=depth_cov, nodes=nodes, calls=calls,
                expect=expect, **extra)


def _depth_boundary(target, denom):
    """A double near the depth difference at which cdf crosses `target` (bisection over math.erf): input selection only."""
    lo, hi = -1.0, 1.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if 0.5 * (1 + math.erf(mid / denom)) >= target:
            hi = mid
        else:
            lo = mid
    return hi


BINADES = tuple(range(-3, 4))


def _adjacent(c, k):
    c = F32(c)
    for _ in range(abs(k)):
        c = np.nextafter(c, F32(np.inf if k > 0 else -np.inf))
    return c


def boundary(cloud_skip=1, depth_cov=1e-4, binades=BINADES):
    """Per binade pz = 1.37 * 2^e: a new node with one valid pixel (x = y = 0) and an old node whose valid pixels lie on a
    lattice of pitch 5 -- row 2 holds the 7 adjacent floats around fl(pz + d_lo), row 7 those around fl(pz + d_hi).  One job
    per site: the translation moves the projection onto the site, so every job counts exactly one point whose class is the
    class of one old sample."""
    s = cloud_skip
    ch, cw, yc0, xc0 = 10, 35, 4, 17
    K = (32.0 * s, 32.0 * s, float(xc0 * s), float(yc0 * s))
    denom = emm_denominator(s, depth_cov)
    d = (_depth_boundary(0.001, denom), _depth_boundary(0.999, denom))
    nodes, jobs, windows = {}, [], []
    for b, e in enumerate(binades):
        pz = F32(1.37 * 2.0 ** e)
        new = np.full((ch * s, cw * s), np.nan, F32)
        new[yc0 * s, xc0 * s] = pz
        old = np.full((ch * s, cw * s), np.nan, F32)
        for side, row in ((0, 2), (1, 7)):
            win = []
            for k in range(7):
                col = 2 + 5 * k
                old[row * s, col * s] = _adjacent(F32(float(pz) + d[side]), k - 3)
                win.append(len(jobs))
                jobs.append((2 * b, 2 * b + 1, _translation(F32((col - xc0) * float(pz) / 32.0), F32((row - yc0) * float(pz) / 32.0))))
            windows.append(dict(binade=e, side=side, jobs=win, row=row))
        nodes[2 * b], nodes[2 * b + 1] = new, old
    return _scene("boundary_skip%d_cov%g" % (s, depth_cov), K, nodes, [(1, jobs)], cloud_skip=s, depth_cov=depth_cov,
                  windows=windows, d=d)


def census_boundary(scene, result):
    """Every job counts one point with one old sample; every window of 7 adjacent floats holds both classes, with one flip."""
    counts, details = result[0]
    flips = []
    for w in scene["windows"]:
        cls = []
        for k, j in enumerate(w["jobs"]):
            det = details[j]
            live = np.flatnonzero(det["inside"])
            assert len(live) == 1 and det["n_samples"][live[0]] == 1
            assert (det["yc"][live[0]], det["xc"][live[0]]) == (w["row"], 2 + 5 * k)
            cls.append(int(det["cls"][live[0]]))
            assert counts[j, :3].sum() == 1
        lower, upper = (OCCLUDED, GOOD) if w["side"] == 0 else (GOOD, BAD)
        flip = cls.index(upper)
        assert 0 < flip < 7 and cls == [lower] * flip + [upper] * (7 - flip), (w, cls)
        assert 2 <= flip <= 5                                       # within one step of the window's centre
        flips.append(flip)
    return flips


_HOT_Z = {GOOD: 1.0, OCCLUDED: 0.5, BAD: 1.5}       # old depths against a new point at 1 m (the boundaries are +-0.044 m)


def _hot_counts(cls, total):
    c = [0, 0, 0, total]
    if cls != NONE:
        c[cls] = 1
    return c


def one_hot():
    """A centre well inside a 12 x 16 raster.  27 jobs: one of the 9 sample positions valid, holding a good, occluded or bad
    depth; 16 jobs: one valid depth at a position of the 5 x 5 window that step 2 skips (counts nothing); priorities."""
    ch, cw, yc, xc = 12, 16, 6, 8
    K = (16.0, 16.0, float(xc), float(yc))
    new = np.full((ch, cw), np.nan, F32)
    new[yc, xc] = 1.0
    nodes, jobs, expect = {0: new}, [], []

    def add(points, cls):
        old = np.full((ch, cw), np.nan, F32)
        for (dy, dx), c in points:
            old[yc + dy, xc + dx] = _HOT_Z[c]
        nodes[len(nodes)] = old
        jobs.append((0, len(nodes) - 1, np.eye(4, dtype=F32)))
        expect.append(_hot_counts(cls, ch * cw))

    sampled = [(dy, dx) for dy in (-2, 0, 2) for dx in (-2, 0, 2)]
    for p in sampled:
        for c in (GOOD, OCCLUDED, BAD):
            add([(p, c)], c)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if (dy, dx) not in sampled:
                add([((dy, dx), GOOD)], NONE)
    for dy, dx in ((-3, 0), (3, 0), (0, -3), (0, 3), (-4, -4), (4, 4)):        # just outside the window
        add([((dy, dx), GOOD)], NONE)
    first, mid, last = sampled[0], sampled[4], sampled[8]
    add([(first, OCCLUDED), (last, BAD)], OCCLUDED)
    add([(first, BAD), (last, OCCLUDED)], OCCLUDED)
    add([(first, GOOD), (last, BAD)], GOOD)
    add([(first, BAD), (last, GOOD)], GOOD)
    add([(first, GOOD), (mid, OCCLUDED)], GOOD)
    add([(first, OCCLUDED), (mid, BAD), (last, GOOD)], GOOD)
    add([(p, BAD) for p in sampled[:8]] + [(last, OCCLUDED)], OCCLUDED)
    add([], NONE)
    return _scene("one_hot", K, nodes, [(1, jobs)], expect=[expect])


EDGE_RASTERS = ((8, 9), (9, 8))


def raster_edge(ch, cw):
    """Centres at 0, 1, 2, cw-3, cw-2, cw-1 crossed with the same rows.  Per centre one job per sample position the clipped
    window keeps: that position holds a bad or an occluded depth, the other kept positions are NaN and EVERY other pixel of
    the raster holds a good depth -- among them the pixels a clamped or unclipped load would read.  One more job per centre
    with all kept positions NaN counts nothing."""
    K = (16.0, 16.0, 0.0, 0.0)
    new = np.full((ch, cw), np.nan, F32)
    new[0, 0] = 1.0
    nodes, jobs, expect, kept_sizes = {0: new}, [], [], []
    edge = lambda n: (0, 1, 2, n - 3, n - 2, n - 1)
    for yc in edge(ch):
        for xc in edge(cw):
            ys = list(range(max(0, yc - 2), min(ch, yc + 3), 2))
            xs = list(range(max(0, xc - 2), min(cw, xc + 3), 2))
            kept = [(y, x) for y in ys for x in xs]
            kept_sizes.append(len(kept))
            T = _translation(xc / 16.0, yc / 16.0)
            for h, hot in enumerate(kept + [None]):
                old = np.full((ch, cw), _HOT_Z[GOOD], F32)
                for y, x in kept:
                    old[y, x] = np.nan
                cls = NONE
                if hot is not None:
                    cls = BAD if (h + yc + xc) % 2 else OCCLUDED
                    old[hot] = _HOT_Z[cls]
                nodes[len(nodes)] = old
                jobs.append((0, len(nodes) - 1, T))
                expect.append(_hot_counts(cls, ch * cw))
    return _scene("raster_edge_%dx%d" % (ch, cw), K, nodes, [(1, jobs)], expect=[expect], kept_sizes=kept_sizes)


def half_pixel():
    """fx = fy = 16, cx = cy = 0, z = 1: the projection is exactly 16 * translation.  k + 0.5 rounds up; -0.5 lands at 0 and
    its float predecessor outside; cw - 0.5 lands outside and its predecessor at cw - 1; pz = +0.0, -0.0 and < 0."""
    ch, cw = 8, 12
    K = (16.0, 16.0, 0.0, 0.0)
    new = np.full((ch, cw), np.nan, F32)
    new[0, 0] = 1.0
    all_good = np.full((ch, cw), 1.0, F32)
    nodes, jobs, expect = {0: new, 1: all_good}, [], []

    def add(old_id, T, hit):
        jobs.append((0, old_id, T))
        expect.append([int(hit), 0, 0, ch * cw])

    v16 = lambda v: F32(v) / F32(16)       # exact: a power of two
    pred = lambda v: np.nextafter(F32(v), F32(-np.inf))
    for k in (2, 5, 8):
        # only column k + 3 is valid: sampled from the centre k + 1 (k - 1, k + 1, k + 3), not from the centre k
        col = np.full((ch, cw), np.nan, F32); col[:, k + 3] = 1.0
        nodes[len(nodes)] = col
        add(len(nodes) - 1, _translation(v16(k + 0.5), v16(2)), True)
        add(len(nodes) - 1, _translation(v16(pred(k + 0.5)), v16(2)), False)
    for k in (2, 4):
        row = np.full((ch, cw), np.nan, F32); row[k + 3, :] = 1.0
        nodes[len(nodes)] = row
        add(len(nodes) - 1, _translation(v16(2), v16(k + 0.5)), True)
        add(len(nodes) - 1, _translation(v16(2), v16(pred(k + 0.5))), False)
    for axis, n in ((0, cw), (1, ch)):
        for v, hit in ((-0.5, True), (pred(-0.5), False), (n - 0.5, False), (pred(n - 0.5), True)):
            t = [v16(3), v16(3)]
            t[axis] = v16(v)
            add(1, _translation(*t), hit)
    add(1, _translation(v16(3), v16(3), -1.0), False)               # pz = 1 - 1 = +0.0
    Tm = _translation(v16(3), v16(3))
    Tm[2] = [-1.0, -1.0, -0.0, -0.0]                                # pz = (-0 + -0) + -0 + -0 = -0.0 (x = y = +0)
    add(1, Tm, False)
    add(1, _translation(0.0, 0.0, -1.0), False)                     # 0 / 0
    add(1, _translation(v16(3), v16(3), -2.0), False)               # behind the camera
    add(1, _translation(v16(3), v16(3)), True)
    return _scene("half_pixel", K, nodes, [(1, jobs)], expect=[expect])


SIZES = ((2, 2), (2, 3), (3, 2), (5, 7), (15, 17), (16, 16), (16, 17), (33, 31), (32, 32), (25, 41))
SKIP_STEPS = (1, 2, 3, 8, 40)


def _dense(rng, ch, cw):
    d = rng.uniform(1.0, 1.25, (ch, cw)).astype(F32)
    d[rng.random((ch, cw)) < 0.1] = np.nan
    return d


def _wobble(rng, tz=0.0):
    a = rng.normal(0, 0.03)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    T[:3, 3] = rng.normal(0, 0.04, 3) + [0, 0, tz]
    return T.astype(F32)


def sizes(ch, cw, seed=0):
    """Dense random depth with 10 % NaN at one cloud size, every emm skip step: the sampled totals of the family (1, 255,
    256, 272, 1023, 1024, 1025, ...) lie either side of a wave and of the block's 256-lane stride."""
    rng = np.random.default_rng(seed * 100003 + ch * 64 + cw)
    K = (float(cw), float(cw), (cw - 1) / 2, (ch - 1) / 2)
    nodes = {0: _dense(rng, ch, cw), 1: _dense(rng, ch, cw)}
    jobs = [(0, 1, _wobble(rng)), (1, 0, _wobble(rng, 0.1)), (0, 1, _wobble(rng, -0.1)), (0, 0, np.eye(4, dtype=F32))]
    totals = [(-(-ch // k)) * (-(-cw // k)) for k in SKIP_STEPS]
    return _scene("sizes_%dx%d" % (ch, cw), K, nodes, [(k, jobs) for k in SKIP_STEPS], totals=totals)


def many_jobs(seed=0):
    """1, 2 and 257 jobs in one call over a 16 x 17 cloud."""
    rng = np.random.default_rng(seed)
    ch, cw = 16, 17
    K = (float(cw), float(cw), (cw - 1) / 2, (ch - 1) / 2)
    nodes = {0: _dense(rng, ch, cw), 1: _dense(rng, ch, cw)}
    jobs = [((i % 2), 1 - (i % 2), _wobble(rng, rng.normal(0, 0.06))) for i in range(257)]
    return _scene("many_jobs", K, nodes, [(1, jobs[:1]), (1, jobs[:2]), (1, jobs)])


def all_scenes():
    global _SCENES
    if _SCENES is None:
        _SCENES = [boundary(1), boundary(2), boundary(1, 2.5e-5, binades=(0, -2)), one_hot()] + \
                  [raster_edge(*r) for r in EDGE_RASTERS] + [half_pixel()] + [sizes(*s) for s in SIZES] + [many_jobs()]
    return _SCENES


_SCENES = None
