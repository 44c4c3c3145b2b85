"""A plain float64 restatement of the two SIFT stages that are compared within a tolerance -- orientation assignment and
the 4 x 4 x 8 descriptor -- with the planted images and keypoint lists that
tests/test_oracle_sift_features.py (CPU, against the compiled reference) and tests/test_gpu_sift_features.py (the HIP
kernels) share.  numpy only.

Organisation: the REFERENCE's, not the kernels' -- one loop per candidate for the orientation, one loop per (feature, cell)
for the descriptor, cell (i, j) collecting the pixels with |a - i| < 1 and |b - j| < 1 weighted (1 - |a - i|)(1 - |b - j|)
-- so that a misreading of the wave-per-feature kernels cannot repeat itself here.

Arithmetic: everything continuous is float64 on the float32 values the stage is handed (plane, candidate record or
feature).  The DISCRETE decisions -- the window's bounds, the disc test, the direction bin, the descriptor's scan window --
are evaluated in float32 in the operations the stage is specified with, and every one reports its margin, from which
`stable` says whether a candidate's outcome can depend on the last bits of a float32 implementation at all."""
import numpy as np

F = np.float32
PI32 = F(3.14159265358979323846)
TWO_PI = 2.0 * 3.14159265358979323846
DOG_LEVELS, LEVELS, DIR_BINS = 5, 8, 36
NO_PEAK = 0xFFFF
SIGMA0 = F(F(1.6) * np.power(F(2.0), F(1.0) / F(DOG_LEVELS)))          # "-d 5": 1.6 * 2^(1/5)
LEVEL_RATIO = np.power(F(2.0), F(1.0) / F(DOG_LEVELS))
HALF_STEP = np.power(F(2.0), F(0.5) / F(DOG_LEVELS))
CELL_SCALES = 3.0                                                      # a descriptor cell's side in units of the scale
EPS_BIN = 1e-5        # bins: ~4 x (a 2-ulp atan2f at pi = 4.8e-7 rad = 2.7e-6 bins, plus the product's rounding at 18: 1e-6)
EPS_DISC = 1e-6       # relative distance from the disc's edge
BIN_CODES = 65535.0 / DIR_BINS

# The compiled float32 reference's largest relative L2 deviation from this restatement over every planted input, measured
# by tests/test_oracle_sift_features.py::test_reference_deviation_is_the_recorded_one (which fails when the figure moves),
# and the tolerance tests/test_gpu_sift_features.py derives from it: 8 x, for the kernel's 3e-7 rad arctangent, its 1-ulp
# rcp / exp2 / sqrt and the 2^-31 fixed-point grid over a correctly rounded float32 evaluation (errors per vote, which do
# not add coherently).
REF_DEVIATION = 3.9e-6
DESC_TOL = 8 * REF_DEVIATION
DESC_ATOL = 1e-6      # rows whose norm is below 1e-3


def relative_deviation(got, want):
    """Relative L2 of a descriptor row against `want` (float64); a row of norm < 1e-3 counts by its largest absolute
    difference on the scale DESC_ATOL : DESC_TOL."""
    n = np.linalg.norm(want)
    if n >= 1e-3:
        return np.linalg.norm(got - want) / n
    return np.abs(got - want).max() * (DESC_TOL / DESC_ATOL)


def level_sigma(j):
    return F(SIGMA0 * np.power(F(2.0), F(j) / F(DOG_LEVELS)))


class Level:
    """A Gaussian plane [h, w] (w: the padded width every stage addresses) and its central differences in float64."""

    def __init__(self, plane):
        self.plane = np.ascontiguousarray(plane, np.float32)
        p = self.plane.astype(np.float64)
        self.h, self.w = p.shape
        self.gh = np.zeros_like(p)
        self.gv = np.zeros_like(p)
        self.gh[:, 1:-1] = p[:, 2:] - p[:, :-2]
        self.gv[1:-1, :] = p[2:, :] - p[:-2, :]
        self.len = 0.5 * np.sqrt(self.gh * self.gh + self.gv * self.gv)
        self.dir = np.where(self.len == 0.0, 0.0, np.arctan2(self.gv, self.gh))


def _floor_margin(v64):
    return abs(v64 - np.round(v64))


def window(cx, cy, reach, w, h):
    """Pixels whose centre lies within `reach` of the point by the floor of the edges (float32), one pixel off the border.
    Returns (c0, r0, cols, rows), the sides the plane cuts (l, r, t, b) and the smallest margin of an uncut edge."""
    lo_c, hi_c = F(cx - reach), F(cx + reach)
    lo_r, hi_r = F(cy - reach), F(cy + reach)
    fl = [int(np.floor(v)) for v in (lo_c, hi_c, lo_r, hi_r)]
    cut = (fl[0] < 1, fl[1] > w - 2, fl[2] < 1, fl[3] > h - 2)
    exact = (float(cx) - float(reach), float(cx) + float(reach), float(cy) - float(reach), float(cy) + float(reach))
    margin = min([_floor_margin(e) for e, c in zip(exact, cut) if not c] or [1.0])
    c0, r0 = max(1, fl[0]), max(1, fl[2])
    cols = max(0, min(w - 2, fl[1]) - c0 + 1)
    rows = max(0, min(h - 2, fl[3]) - r0 + 1)
    return (c0, r0, cols, rows), cut, margin


def _smooth(v, third):
    for _ in range(6):
        v = third * ((np.roll(v, 1) + v) + np.roll(v, -1))
    return v


def _smoothing_matrix():
    m = (np.eye(DIR_BINS) + np.roll(np.eye(DIR_BINS), 1, axis=1) + np.roll(np.eye(DIR_BINS), -1, axis=1)) * float(F(1.0 / 3.0))
    return np.linalg.matrix_power(m, 6)


_SMOOTHING = _smoothing_matrix()      # smooth = _SMOOTHING @ raw (symmetric)


def _refine(v, b):
    vl, vr = v[(b - 1) % DIR_BINS], v[(b + 1) % DIR_BINS]
    turn = (b + 0.5 * ((vr - vl) / (v[b] + v[b] - vr - vl)) + 0.5) / DIR_BINS
    if turn < 0.0:
        turn += 1.0
    return int(np.floor(turn * 65535.0)) & 0xFFFF


def orientation(level, rec, sigma):
    """Orientation assignment of one candidate (x, y, sign, dx, dy, ds) of the DoG level whose gradients come from `level`
    and whose nominal scale is `sigma`.  Returns a dict: the point and scale, the window, the raw and smoothed 36-bin
    histograms, the peak set, the two best peaks in rank order, their 16-bit codes, the number of orientations the list
    reshaping makes of them, and the stability verdict with its margins."""
    x, y, _, dx, dy, ds = [F(v) for v in rec]
    cx, cy = F(F(x + F(0.5)) + dx), F(F(y + F(0.5)) + dy)
    scale64 = float(sigma) * float(LEVEL_RATIO) ** float(ds)
    scale = F(scale64)
    disc = F(abs(scale) * F(3.0))                     # twice the damping's 1.5 scales
    disc2 = F(F(disc * disc) + F(0.5))
    spread = scale64 * 1.5
    damp = -0.5 / (spread * spread)
    (c0, r0, cols, rows), cut, win_margin = window(cx, cy, disc, level.w, level.h)
    out = dict(cx=cx, cy=cy, scale=scale, window=(c0, r0, cols, rows), cut=cut, pixels=cols * rows)
    raw = np.zeros(DIR_BINS)
    bin_margin, disc_margin = 1.0, 1.0
    if cols * rows > 0:
        cc, rr = np.meshgrid(np.arange(c0, c0 + cols), np.arange(r0, r0 + rows))
        ox32 = (cc.astype(np.float32) + F(0.5)) - cx
        oy32 = (rr.astype(np.float32) + F(0.5)) - cy
        d2_32 = (ox32 * ox32).astype(np.float32) + (oy32 * oy32).astype(np.float32)
        inside = ~(d2_32 >= disc2)
        ox, oy = (cc + 0.5) - float(cx), (rr + 0.5) - float(cy)
        d2 = ox * ox + oy * oy
        disc2_64 = float(disc) * float(disc) + 0.5
        glen, gdir = level.len[r0:r0 + rows, c0:c0 + cols], level.dir[r0:r0 + rows, c0:c0 + cols]
        gh, gv = level.gh[r0:r0 + rows, c0:c0 + cols], level.gv[r0:r0 + rows, c0:c0 + cols]
        weight = glen * np.exp(d2 * damp)
        prod32 = (gdir.astype(np.float32) * F(F(18.0) / PI32)).astype(np.float32)
        bins = np.floor(prod32).astype(np.int64)
        bins = np.where(bins < 0, bins + DIR_BINS, bins)
        raw = np.bincount(bins[inside], weights=weight[inside], minlength=DIR_BINS + 1)[:DIR_BINS + 1]
        assert raw[DIR_BINS] == 0.0
        raw = raw[:DIR_BINS]
        votes = weight > 0
        near = votes & (np.abs(d2 - disc2_64) < 4 * EPS_DISC * disc2_64)          # whichever side float32 put them
        if near.any():
            disc_margin = float((np.abs(d2 - disc2_64) / disc2_64)[near].min())
        voting = inside & votes & (gh != 0) & (gv != 0)
        if voting.any():
            t = gdir[voting] * (18.0 / np.pi)
            bin_margin = float(np.abs(t - np.round(t)).min())
    third = float(F(1.0 / 3.0))
    v = _smooth(raw, third)
    top = v.max()
    thr = float(F(0.8)) * top
    vl, vr = np.roll(v, 1), np.roll(v, -1)
    peaks = np.flatnonzero((v > thr) & (v > vl) & (v > vr)) if top > 0 else np.zeros(0, np.int64)
    order = sorted(peaks.tolist(), key=lambda b: (-v[b], b))
    best = order[:2]
    codes = [_refine(v, b) for b in best] + [NO_PEAK] * (2 - len(best))
    n_orient = 0 if codes[0] == NO_PEAK else (2 if codes[1] != NO_PEAK and codes[1] != codes[0] else 1)
    # ---- can a float32 evaluation decide differently?  eps_v = (pixels + 32) 2^-24 relative, applied where the error arises:
    # a RAW bin is a float sum of at most `pixels` non-negative terms (worst case pixels * 2^-24 relative) and reaches the
    # decisions through the smoothing, which is linear, so a decision value  L . smooth = (L S) . raw  can move by
    # eps_raw * |L S| . raw; the 32 * 2^-24 -- the weights' own rounding, the 18 roundings of the six smoothing passes, the
    # decision's arithmetic -- is taken adversarially on every SMOOTHED bin the decision reads: + eps_s * |L| . smooth.
    eps_raw, eps_s = cols * rows * 2.0 ** -24, 32 * 2.0 ** -24
    eps_v = eps_raw + eps_s
    def slack(L):
        return eps_raw * (np.abs(L @ _SMOOTHING) @ raw) + eps_s * (np.abs(L) @ v)
    reasons, loose = [], []
    if bin_margin < EPS_BIN:
        reasons.append("bin")
    if disc_margin < EPS_DISC:
        reasons.append("disc")
    if win_margin < 1e-5:
        reasons.append("window")
    if top > 0:
        eye = np.eye(DIR_BINS)
        over = eye.copy()
        over[:, int(np.argmax(v))] -= float(F(0.8))
        tests = [over, eye - np.roll(eye, -1, axis=1), eye - np.roll(eye, 1, axis=1)]     # v - 0.8 top, v - left, v - right
        value = np.stack([L @ v for L in tests])
        room = np.stack([slack(L) for L in tests])
        surely_not = (value < -room).any(axis=0)
        surely = (value > room).all(axis=0)
        loose = np.flatnonzero(~surely_not).tolist()
        if (~surely_not & ~surely).any():
            reasons.append("peak")
        for hi, lo in zip(order, order[1:3]):                                         # the ranking of the first two peaks
            L = eye[hi] - eye[lo]
            if not L @ v > slack(L):
                reasons.append("rank")
        for b in best:
            l, r = (b - 1) % DIR_BINS, (b + 1) % DIR_BINS
            Ln, Ld = eye[r] - eye[l], 2 * eye[b] - eye[r] - eye[l]
            num, den, dnum, dden = Ln @ v, Ld @ v, slack(Ln), slack(Ld)
            if den <= dden or 0.5 * (dnum / (den - dden) + abs(num) * dden / (den * (den - dden))) * BIN_CODES > 1.0:
                reasons.append("code")
    # loose: every bin a float32 evaluation could call a peak (the bound on what an unstable candidate may return)
    out.update(raw=raw, smooth=v, peaks=peaks, best=best, codes=codes, n_orient=n_orient, stable=not reasons,
               reasons=reasons, eps_v=eps_v, loose_bins=loose,
               margins=dict(bin=bin_margin, disc=disc_margin, window=win_margin))
    return out


def descriptor_window(shape, feat):
    """The descriptor stage's scan window (float32, as specified): the bounding box of the rotated support |a|, |b| < 2.5
    around the feature, cut one pixel off the plane's border.  (c0, r0, cols, rows); empty when cols * rows == 0."""
    h, w = shape
    fx, fy, fs, fw = [F(v) for v in feat]
    cell = F(abs(F(fs * F(CELL_SCALES))))
    sn, cs = F(np.sin(np.float64(fw))), F(np.cos(np.float64(fw)))
    reach = F(F(F(2.5) * cell) * F(abs(cs) + abs(sn)))
    return window(fx, fy, reach, w, h)[0]


def descriptor(level, feat):
    """The 128 unnormalised values of one feature (x, y, scale, direction) in level coordinates: rows of 8 directions for
    cell (i, j) at index (j * 4 + i) * 8, i along the feature's direction."""
    fx, fy, fs, fw = [float(F(v)) for v in feat]
    cell = abs(fs * CELL_SCALES)
    sn, cs = np.sin(fw), np.cos(fw)
    out = np.zeros(128)
    if not (cell > 0 and np.isfinite(cell)):
        return out
    ext = cell * (abs(cs) + abs(sn))                  # half the side of a cell support's bounding box
    for j in range(4):
        for i in range(4):
            ci, cj = i - 1.5, j - 1.5
            px, py = fx + cell * (cs * ci - sn * cj), fy + cell * (sn * ci + cs * cj)    # the cell's centre in the plane
            c_lo, c_hi = max(1, int(np.floor(px - ext - 0.5)) - 1), min(level.w - 2, int(np.ceil(px + ext - 0.5)) + 1)
            r_lo, r_hi = max(1, int(np.floor(py - ext - 0.5)) - 1), min(level.h - 2, int(np.ceil(py + ext - 0.5)) + 1)
            if c_hi < c_lo or r_hi < r_lo:
                continue
            cc, rr = np.meshgrid(np.arange(c_lo, c_hi + 1), np.arange(r_lo, r_hi + 1))
            ox, oy = (cc + 0.5) - fx, (rr + 0.5) - fy
            a, b = (cs * ox + sn * oy) / cell, (cs * oy - sn * ox) / cell
            da, db = np.abs(a - ci), np.abs(b - cj)
            m = (da < 1.0) & (db < 1.0)
            if not m.any():
                continue
            a, b, da, db = a[m], b[m], da[m], db[m]
            glen, gdir = level.len[r_lo:r_hi + 1, c_lo:c_hi + 1][m], level.dir[r_lo:r_hi + 1, c_lo:c_hi + 1][m]
            vote = glen * np.exp(-0.125 * (a * a + b * b)) * (1.0 - da) * (1.0 - db)
            o = np.mod((fw - gdir) * (4.0 / np.pi), 8.0)
            o = np.where(o >= 8.0, 0.0, o)
            oi = np.floor(o)
            fo = o - oi
            d0 = oi.astype(np.int64) % 8
            hist = np.bincount(d0, weights=vote * (1.0 - fo), minlength=8) + np.bincount((d0 + 1) % 8, weights=vote * fo, minlength=8)
            out[(j * 4 + i) * 8:(j * 4 + i) * 8 + 8] = hist
    return out


def sum_bound(feat):
    """What the kernel sizes its fixed-point grid by: no bin's sum reaches (cell + 2)^2."""
    cell = abs(float(F(feat[2])) * CELL_SCALES)
    return (cell + 2.0) ** 2


# ---- host-side list arithmetic (float32 exactly as the list code runs) -------------------------------------------------------

def octave_scale(octave, octave_min=-1):
    return F(2.0 ** (octave + octave_min))


def candidate_key_xy(rec, octave, octave_min=-1):
    """The image position the reshaped list reports for a candidate (float32 expressions of the list code)."""
    oss = octave_scale(octave, octave_min)
    cx = F(F(F(rec[0]) + F(0.5)) + F(rec[3]))
    cy = F(F(F(rec[1]) + F(0.5)) + F(rec[4]))
    return F(F(oss * F(cx - F(0.5))) + F(0.5)), F(F(oss * F(cy - F(0.5))) + F(0.5))


def code_direction(code):
    """The level-frame direction the list code makes of a 16-bit code."""
    return F((TWO_PI / 65535.0) * int(code))


def key_orientation_code(o):
    """The 16-bit code behind a reported orientation o = fmod(2 pi - direction, 2 pi): (code, distance from the grid in codes)."""
    c = np.mod(TWO_PI - float(o), TWO_PI) * (65535.0 / TWO_PI)
    k = int(np.round(c))
    return k % 65535, abs(c - k)


def keypoint_to_key(x, y, size, angle_deg):
    """cv::KeyPoint -> SiftKey as the wrapper converts: s = size / 12, o = angle / 180 * 3.1415927 (double, stored float)."""
    return F(x), F(y), F(np.float64(F(size)) / 12.0), F(np.float64(F(angle_deg)) / 180.0 * 3.1415927)


def assign_levels(keys, octave_num, octave_min=-1):
    """The keypoint list's scale bands: for keys [n, 4] = (x, y, s, o) returns per key (octave, dog level, feature in level
    coordinates) or None for a key no band takes, and the smallest relative distance of a scale from a band edge.
    (A key two bands take keeps the last, as the product does; the planted lists keep off the edges.)"""
    n = len(keys)
    got = [None] * n
    edge = 1.0
    octave_sigma = octave_scale(0, octave_min)
    for i in range(octave_num):
        for j in range(DOG_LEVELS):
            level_sg = F(level_sigma(j) * octave_sigma)
            lo, hi = F(level_sg / HALF_STEP), F(level_sg * HALF_STEP)
            for k in range(n):
                x, y, s, o = [F(v) for v in keys[k]]
                edge = min(edge, abs(float(s) / float(lo) - 1.0), abs(float(s) / float(hi) - 1.0))
                if (s >= lo and s < hi) or (s < lo and i == 0 and j == 0) or (s > hi and i == octave_num - 1 and j == DOG_LEVELS - 1):
                    feat = (F(F(F(x - F(0.5)) / octave_sigma) + F(0.5)), F(F(F(y - F(0.5)) / octave_sigma) + F(0.5)),
                            F(s / octave_sigma), F(np.fmod(TWO_PI - np.float64(o), TWO_PI)))
                    got[k] = (i, j, feat)
        octave_sigma = F(octave_sigma * F(2.0))
    return got, edge


# ---- planted images (seeded; uint8) ---------------------------------------------------------------------------------------

def _background(h, w, amp=14.0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return amp * np.sin(0.37 * x + 0.23 * y + 0.4) + 0.7 * amp * np.sin(-0.19 * x + 0.31 * y + 1.3)


def generic(h=120, w=160, seed=31, blobs=100, bg=14.0, amp=(40.0, 90.0), aniso=(1.3, 2.2), s1r=(1.2, 5.0)):
    """Anisotropic Gaussian blobs at random sub-pixel positions and non-axis angles -- several with their centres 2 .. 6
    pixels from each border and in each corner -- over two oblique sinusoids, so that no pixel of a plane is flat or has
    an exactly axis-aligned gradient."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 118.0 + _background(h, w, bg)
    pos = [(rng.uniform(8, w - 8), rng.uniform(8, h - 8)) for _ in range(blobs - 24)]
    for _ in range(3):
        pos += [(rng.uniform(2, 6), rng.uniform(8, h - 8)), (w - rng.uniform(2, 6), rng.uniform(8, h - 8)),
                (rng.uniform(8, w - 8), rng.uniform(2, 6)), (rng.uniform(8, w - 8), h - rng.uniform(2, 6))]
        pos += [(rng.uniform(2, 6), rng.uniform(2, 6)), (w - rng.uniform(2, 6), rng.uniform(2, 6)),
                (rng.uniform(2, 6), h - rng.uniform(2, 6)), (w - rng.uniform(2, 6), h - rng.uniform(2, 6))]
    for px, py in pos:
        th = rng.uniform(0.1, 1.45) + (np.pi / 2) * rng.integers(0, 4)
        s1 = rng.uniform(*s1r)
        s2 = s1 * rng.uniform(*aniso)
        u = np.cos(th) * (x - px) + np.sin(th) * (y - py)
        v = -np.sin(th) * (x - px) + np.cos(th) * (y - py)
        img += rng.choice([-1.0, 1.0]) * rng.uniform(*amp) * np.exp(-0.5 * ((u / s1) ** 2 + (v / s2) ** 2))
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def corners(h=120, w=160, seed=32, bg=0.35, blur=(0.9, 2.2), size=(6.0, 11.0)):
    """Blurred L-shaped corners (a bright quadrant under a round envelope) at random non-axis angles: two dominant
    gradient directions at each, hence two orientations per keypoint."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 96.0 + bg * _background(h, w)
    def step(t):
        return 0.5 * (1.0 + np.tanh(1.2 * t))
    for gy in range(4):
        for gx in range(6):
            px, py = 14 + gx * 26.5 + rng.uniform(-4, 4), 14 + gy * 30.5 + rng.uniform(-4, 4)
            th = rng.uniform(0.12, 1.45) + (np.pi / 2) * rng.integers(0, 4)
            blur_k = rng.uniform(*blur)
            size_k = rng.uniform(*size)
            u = np.cos(th) * (x - px) + np.sin(th) * (y - py)
            v = -np.sin(th) * (x - px) + np.cos(th) * (y - py)
            img += rng.uniform(70, 130) * step(u / blur_k) * step(v / blur_k) * np.exp(-0.5 * ((x - px) ** 2 + (y - py) ** 2) / size_k ** 2)
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def blocks17(h=120, w=160, seed=33, block=6.0):
    """A random 0 / 255 block pattern turned by 17 degrees: the largest gradients an 8-bit image holds, no exact symmetry."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    th = np.deg2rad(17.0)
    u = np.cos(th) * (x - 80.3) + np.sin(th) * (y - 60.7)
    v = -np.sin(th) * (x - 80.3) + np.cos(th) * (y - 60.7)
    table = rng.integers(0, 2, (64, 64), dtype=np.uint8)
    img = table[(np.floor(v / block).astype(np.int64) + 32) % 64, (np.floor(u / block).astype(np.int64) + 32) % 64] * 255
    return np.ascontiguousarray(img.astype(np.uint8))


IMAGES = {
    "generic": lambda: generic(),
    "corners": lambda: corners(),
    "blocks17": lambda: blocks17(),
    "strip": lambda: generic(36, 100, seed=34, blobs=40),
}
DETECT_IMAGES = ("generic", "corners", "blocks17", "strip")
BATCH_IMAGES = ("generic", "corners", "blocks17", "generic")


# ---- planted keypoint lists for the describe path ---------------------------------------------------------------------------

def band_scale(octave, j, where=0.0, octave_min=-1):
    """A scale inside band (octave, j): where = -1 .. 1 from the lower to the upper edge (geometric), 0 the centre."""
    return float(level_sigma(j)) * 2.0 ** (octave + octave_min) * float(HALF_STEP) ** where


def describe_lists(h, w, octave_num, seed=41, heavy=False):
    """name -> [n, 4] rows of (x, y, size, angle in degrees), cv::KeyPoint fields.  No scale on a band edge, none <= 0."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    lists = {}
    # angles: 0, the smallest direction above 0, pi and its float neighbours, just under a full turn, a full turn
    a180 = f32(180.0)
    angles = [0.0, 2e-43, float(np.finfo(f32).tiny) * 60, float(np.nextafter(a180, f32(0))), 180.0, float(np.nextafter(a180, f32(360))),
              180.00003, float(np.nextafter(f32(360.0), f32(0))), 359.99, 360.0, 90.0, 270.0, 37.0, 217.0, 323.0]
    rows = []
    for k, ang in enumerate(angles):
        for o, j in ((0, 1), (1, 3), (2, 2)):
            if o < octave_num:
                rows.append((w * (0.3 + 0.05 * (k % 9)), h * (0.35 + 0.04 * (k % 7)), 12.0 * band_scale(o, j, 0.3), ang))
    lists["angles"] = rows
    # positions within 0.5 .. 3 pixels of every border and corner, fine to coarse: strips and empty windows
    rows = []
    for o in range(octave_num):
        for j in (0, 4):
            s = 12.0 * band_scale(o, j, -0.4)
            for d in (0.5, 1.2, 3.0):
                ang = rng.uniform(5, 355)
                rows += [(d, h * 0.47, s, ang), (w - d, h * 0.53, s, ang + 20), (w * 0.41, d, s, ang + 40), (w * 0.59, h - d, s, ang + 60),
                         (d, d, s, ang + 80), (w - d, d, s, ang + 100), (d, h - d, s, ang + 120), (w - d, h - d, s, ang + 140)]
    rows = [(x, y, s, a % 360.0) for x, y, s, a in rows]
    lists["borders"] = [rows[i] for i in rng.permutation(len(rows))]
    # one keypoint (two) in every band, interleaved; then a list that leaves bands empty in between
    bands = [(o, j) for o in range(octave_num) for j in range(DOG_LEVELS)]
    def inside(o, j, where):
        return (rng.uniform(0.15, 0.85) * w, rng.uniform(0.2, 0.8) * h, 12.0 * band_scale(o, j, where), rng.uniform(1, 359))
    rows = [inside(o, j, wh) for o, j in bands for wh in (-0.7, 0.6)]
    lists["all_bands"] = [rows[i] for i in rng.permutation(len(rows))]
    rows = [inside(o, j, 0.2) for o, j in bands[::3] for _ in range(3)]
    lists["sparse_bands"] = [rows[i] for i in rng.permutation(len(rows))]
    # below the first band (down to a cell under one pixel), above the last (the window covers the coarsest plane)
    lo, hi = band_scale(0, 0, -1.0), band_scale(octave_num - 1, DOG_LEVELS - 1, 1.0)
    rows = [(rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h, 12.0 * s, rng.uniform(1, 359))
            for s in (0.9 * lo, 0.5 * lo, 0.11 * lo, 1.1 * hi, 2.0 * hi, 6.0 * hi, 40.0 * hi)]
    lists["extremes"] = rows + [inside(1, 2, 0.0)]
    # cells of 0.6 and 0.15 pixels a quarter and half a pixel inside every border and corner: windows of one row or column,
    # and windows with no pixel at all (a zero row)
    rows = []
    for s, d in ((0.11 * lo, 0.25), (0.11 * lo, 0.5), (0.03 * lo, 0.5), (0.03 * lo, 0.25)):
        for ang in (0.0, 91.0, 203.0):
            rows += [(d, h * 0.37, 12.0 * s, ang), (w - d, h * 0.61, 12.0 * s, ang), (w * 0.43, d, 12.0 * s, ang), (w * 0.57, h - d, 12.0 * s, ang),
                     (d, d, 12.0 * s, ang), (w - d, h - d, 12.0 * s, ang)]
    lists["slivers"] = [rows[i] for i in rng.permutation(len(rows))]
    if heavy:   # the largest cells each octave admits
        rows = [(rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h, 12.0 * band_scale(o, DOG_LEVELS - 1, 0.98), rng.uniform(1, 359))
                for o in range(octave_num) for _ in range(4)]
        lists["largest_cells"] = rows
    return {k: np.array(v, np.float64).astype(np.float32) for k, v in lists.items()}


DESCRIBE_IMAGES = ("generic", "blocks17")


# ---- a whole frame's detection path through the restatement -----------------------------------------------------------------

def restate_orientations(planes, candidates, octave_num):
    """planes(o, l) -> Gaussian plane, candidates(o, j) -> [n, 6]: the restatement of every candidate of a frame in list
    order (octave 0 level 0 first, raster order inside a level).  Returns (records, levels): records of dict(octave, level,
    rec, ori), levels[(o, j)] the Level the stage reads for DoG level j of octave o."""
    records, levels = [], {}
    for o in range(octave_num):
        for j in range(DOG_LEVELS):
            cand = candidates(o, j)
            if len(cand) == 0:
                continue
            levels[(o, j)] = Level(planes(o, j + 1))
            sg = level_sigma(j)
            for rec in cand:
                records.append(dict(octave=o, level=j, rec=rec, ori=orientation(levels[(o, j)], rec, sg)))
    return records, levels


def walk_features(records, xy, octave_min=-1):
    """Match a frame's reported features (image positions [n, 2], list order) to its candidates: a candidate owns the next
    0 .. 2 features that sit at its position.  Returns per record the list of feature rows; every feature must be owned."""
    owned, at = [], 0
    for r in records:
        kx, ky = candidate_key_xy(r["rec"], r["octave"], octave_min)
        mine = []
        while len(mine) < 2 and at < len(xy) and xy[at][0] == kx and xy[at][1] == ky:
            mine.append(at)
            at += 1
        owned.append(mine)
    assert at == len(xy), "features that belong to no candidate: row %d of %d" % (at, len(xy))
    return owned


def circular_code_distance(a, b):
    d = abs(int(a) - int(b)) % 65535
    return min(d, 65535 - d)
