"""TEST INFRASTRUCTURE: the literal statement of the "ICP fallback" contract of include/rgbdfe.h:
filterCloud and icpAlignment (icp.cpp:20-89) for icp_method "icp".  One numpy operation per operation of the contract,
float32 where the contract says float and float64 where it says double; numpy's element-wise operations round once per
element, so an array expression is the scalar expression for every row.  The SVD is oracle/pyoracle.svd3 as it is.

Also here: the room-corner rasters and the planted cases the CPU, emulation and GPU tests share."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402

F4, F8 = np.float32, np.float64
LEAF = 64
NO_CORRESPONDENCES, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE = 1, 2, 3, 4, 5
STATE_NAMES = {1: "NO_CORRESPONDENCES", 2: "ITERATIONS", 3: "TRANSFORM", 4: "ABS_MSE", 5: "REL_MSE"}
DBL_MAX = np.finfo(F8).max


def default_params(**kw):
    p = dict(max_correspondence_distance=0.05, max_iterations=50, transformation_epsilon=1e-8,
             euclidean_fitness_epsilon=1.0, desired_size=10000)
    p.update(kw)
    return p


# ---- filterCloud -------------------------------------------------------------------------------------------------------
def sample_positions(n_valid, desired_size):
    """icp.cpp:34-38: the positions in the list of valid rows, through the float recurrence."""
    step = F4(n_valid) / F4(desired_size)
    if step < F4(1.0):
        step = F4(1.0)
    pos = []
    i = F4(0.0)
    while i < F4(n_valid):
        pos.append(int(i))
        i = F4(i + step)
    return np.array(pos, np.int64)


def filter_cloud(cloud, desired_size):
    """Returns (indices, rows)."""
    cloud = np.ascontiguousarray(cloud, F4).reshape(-1, 4)
    valid = np.flatnonzero(~np.isnan(cloud[:, 2]))
    idx = valid[sample_positions(len(valid), desired_size)] if len(valid) else np.zeros(0, np.int64)
    return idx.astype(np.int32), cloud[idx].copy()


def poisoned(rows):
    """The named deviation: a sampled row with a non-finite x or y takes part in nothing."""
    rows = rows.copy()
    bad = ~(np.isfinite(rows[:, 0]) & np.isfinite(rows[:, 1]))
    rows[bad, 0:3] = np.nan
    return rows


# ---- the pieces of an iteration -----------------------------------------------------------------------------------------
def transformed(R, t, P):
    """((R0 x + R1 y) + R2 z) + t per row, float."""
    R, t = np.asarray(R, F4).reshape(3, 3), np.asarray(t, F4)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    out = P.copy()
    for a in range(3):
        out[:, a] = ((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a]
    return out


def correspondences(P, T, block=512):
    """j(i) and d2(i): the first minimum over ascending j under a strict <, starting from +inf without an index."""
    n, m = len(P), len(T)
    nn_j = np.full(n, -1, np.int32)
    nn_d2 = np.full(n, np.inf, F4)
    if m == 0:
        return nn_j, nn_d2
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, n, block):
            p = P[i0:i0 + block]
            dx = p[:, None, 0] - T[None, :, 0]
            dy = p[:, None, 1] - T[None, :, 1]
            dz = p[:, None, 2] - T[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(np.isnan(d2), F4(np.inf), d2)   # a NaN is never < the running minimum
            j = np.argmin(d2, axis=1)                     # the first of equal minima
            best = d2[np.arange(len(p)), j]
            has = best < F4(np.inf)
            nn_j[i0:i0 + block] = np.where(has, j, -1)
            nn_d2[i0:i0 + block] = best
    return nn_j, nn_d2


def tree_sums(v):
    """v: [n, q] float64.  Each column through the tree: leaves of 64 consecutive values (zero padded) halved 32 .. 1; leaf k
    added into accumulator k % 64 in ascending k; the 64 accumulators halved the same way."""
    v = np.asarray(v, F8)
    n, q = v.shape
    leaves = -(-n // LEAF)
    x = np.zeros((leaves * LEAF, q), F8)
    x[:n] = v
    x = x.reshape(leaves, LEAF, q)
    s = LEAF // 2
    while s >= 1:
        x = x[:, :s] + x[:, s:2 * s]
        s //= 2
    part = x[:, 0] if leaves else np.zeros((0, q), F8)
    acc = np.zeros((LEAF, q), F8)
    for k0 in range(0, leaves, LEAF):
        chunk = part[k0:k0 + LEAF]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    s = LEAF // 2
    while s >= 1:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def det3(m):
    m = np.asarray(m, F4).reshape(9)
    h0 = m[0] * (m[4] * m[8] - m[5] * m[7])
    h1 = m[1] * (m[3] * m[8] - m[5] * m[6])
    h2 = m[2] * (m[3] * m[7] - m[4] * m[6])
    return (h0 - h1) + h2


def increment(sums):
    """H, the SVD, R and t from the seventeen sums.  Returns (R [3, 3] float32, t [3] float32, reflected)."""
    cd = sums[0]
    m_P = np.array([F4(sums[2 + a] / cd) for a in range(3)], F4)
    m_T = np.array([F4(sums[5 + a] / cd) for a in range(3)], F4)
    H = np.empty((3, 3), F4)
    for a in range(3):
        for b in range(3):
            H[a, b] = F4((sums[8 + 3 * a + b] - (sums[5 + a] * sums[2 + b]) / cd) / cd)
    U, _, V = pyoracle.svd3(H)
    reflected = bool(det3(U) * det3(V) < F4(0.0))
    s22 = F4(-1.0) if reflected else F4(1.0)
    R = np.empty((3, 3), F4)
    for i in range(3):
        for j in range(3):
            us2 = U[i, 2] * s22
            R[i, j] = (U[i, 0] * V[j, 0] + U[i, 1] * V[j, 1]) + us2 * V[j, 2]
    t = np.empty(3, F4)
    for i in range(3):
        rm = (R[i, 0] * m_P[0] + R[i, 1] * m_P[1]) + R[i, 2] * m_P[2]
        t[i] = m_T[i] - rm
    return R, t, reflected


def row_values(P, T, nn_j, nn_d2, maxdist2):
    kept = (nn_j >= 0) & ~(nn_d2.astype(F8) > maxdist2)
    v = np.zeros((len(P), 17), F8)
    Tj = T[np.where(kept, nn_j, 0)].astype(F8) if len(T) else np.zeros((len(P), 4), F8)
    Pd = P.astype(F8)
    v[:, 0] = 1.0
    v[:, 1] = nn_d2.astype(F8)
    v[:, 2:5] = Pd[:, 0:3]
    v[:, 5:8] = Tj[:, 0:3]
    for a in range(3):
        for b in range(3):
            v[:, 8 + 3 * a + b] = Tj[:, a] * Pd[:, b]
    v[~kept] = 0.0
    return v, kept


# ---- icpAlignment --------------------------------------------------------------------------------------------------------
def align_sampled(S, T, G=None, trace=False, **params):
    """The alignment of two SAMPLED clouds.  G: a 4 x 4 numpy matrix (row-major; None = identity).  Returns a dict: T (4 x 4
    float32: F if converged, else G's values), converged, state, iterations, c, mse, nn_j, nn_d2 (of the last iteration),
    reflected (an iteration took the s = -1 branch); with trace also the per-iteration records."""
    prm = default_params(**params)
    G = np.eye(4, dtype=F4) if G is None else np.asarray(G, F4).reshape(4, 4).copy()
    S, T = poisoned(np.ascontiguousarray(S, F4).reshape(-1, 4)), poisoned(np.ascontiguousarray(T, F4).reshape(-1, 4))
    maxdist2 = F8(prm["max_correspondence_distance"]) * F8(prm["max_correspondence_distance"])
    teps, feps = F8(prm["transformation_epsilon"]), F8(prm["euclidean_fitness_epsilon"])
    with np.errstate(all="ignore"):
        P = transformed(G[:3, :3], G[:3, 3], S)
        FR, Ft = G[:3, :3].copy(), G[:3, 3].copy()
        mse_prev = DBL_MAX
        out = dict(converged=0, state=0, iterations=0, c=0, mse=F8(0.0), reflected=False, trace=[])
        k = 0
        while True:
            k += 1
            nn_j, nn_d2 = correspondences(P, T)
            v, kept = row_values(P, T, nn_j, nn_d2, maxdist2)
            sums = tree_sums(v) if len(P) else np.zeros(17, F8)
            c = int(sums[0])
            out.update(iterations=k, c=c, nn_j=nn_j, nn_d2=nn_d2)
            if c < 3:
                out.update(state=NO_CORRESPONDENCES, converged=0, mse=(sums[1] / sums[0]) if c > 0 else F8(0.0))
                break
            mse = sums[1] / sums[0]
            R, t, reflected = increment(sums)
            out["reflected"] = out["reflected"] or reflected
            P_before = P
            P = transformed(R, t, P)
            FRn, Ftn = np.empty((3, 3), F4), np.empty(3, F4)
            for a in range(3):
                for b in range(3):
                    FRn[a, b] = (R[a, 0] * FR[0, b] + R[a, 1] * FR[1, b]) + R[a, 2] * FR[2, b]
                Ftn[a] = ((R[a, 0] * Ft[0] + R[a, 1] * Ft[1]) + R[a, 2] * Ft[2]) + t[a]
            FR, Ft = FRn, Ftn
            cos_angle = F8(0.5) * (((F8(R[0, 0]) + F8(R[1, 1])) + F8(R[2, 2])) - F8(1.0))
            tx, ty, tz = F8(t[0]), F8(t[1]), F8(t[2])
            t2 = (tx * tx + ty * ty) + tz * tz
            diff = abs(mse - mse_prev)
            state = 0
            if k >= prm["max_iterations"]:
                state = ITERATIONS
            elif cos_angle >= F8(1.0) - teps and t2 <= teps:
                state = TRANSFORM
            elif diff < F8(1e-12):
                state = ABS_MSE
            elif diff / mse_prev < feps:
                state = REL_MSE
            out.update(mse=mse)
            if trace:
                out["trace"].append(dict(k=k, c=c, mse=mse, R=R, t=t, kept=kept, sums=sums, state=state, P=P_before, nn_j=nn_j,
                                         nn_d2=nn_d2, T=T, reflected=reflected))
            mse_prev = mse
            if state:
                out.update(state=state, converged=1)
                break
    if out["converged"]:
        Tm = np.eye(4, dtype=F4)
        Tm[:3, :3], Tm[:3, 3] = FR, Ft
        out["T"] = Tm
    else:
        out["T"] = G.copy()
    return out


def align_clouds(source, target, G=None, trace=False, **params):
    """filterCloud on both clouds, then the alignment; n_source / n_target are the sample counts."""
    prm = default_params(**params)
    _, S = filter_cloud(source, prm["desired_size"])
    _, T = filter_cloud(target, prm["desired_size"])
    out = align_sampled(S, T, G, trace, **prm)
    out.update(n_source=len(S), n_target=len(T))
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def rigid(rot_vec, trans):
    """4 x 4 float64 from a rotation vector (radians) and a translation (metres)."""
    r = np.asarray(rot_vec, F8)
    th = np.linalg.norm(r)
    K = np.zeros((3, 3))
    if th > 0:
        a = r / th
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = trans
    return M


def moved(cloud, M):
    """cloud's rows moved rigidly by M (float64 arithmetic, rounded once); the fourth word as it is."""
    out = np.ascontiguousarray(cloud, F4).copy()
    out[:, :3] = (out[:, :3].astype(F8) @ M[:3, :3].T + M[:3, 3]).astype(F4)
    return out


_CORNER_AXES = rigid([0.55, -0.7, 0.2], [0, 0, 0])[:3, :3]   # the corner's three plane normals, all facing the camera
_CORNER_AT = np.array([0.1, 0.15, 2.6])


def room_corner(cols=64, rows=48, pose=None, holes=0, seed=0):
    """A cols x rows raster of a room corner (three mutually orthogonal planes meeting 2.6 m in front of the camera), as a
    pinhole camera at `pose` (4 x 4, camera-to-world; None = the origin) sees it: rows of (x, y, z, rgb bits) in the
    camera's frame, row-major over the image.  holes: that many rows get a NaN z (no depth)."""
    f = cols * 0.9
    u, v = np.meshgrid(np.arange(cols, dtype=F8), np.arange(rows, dtype=F8))
    d = np.stack([(u - (cols - 1) / 2) / f, (v - (rows - 1) / 2) / f, np.ones_like(u)], axis=-1).reshape(-1, 3)
    pose = np.eye(4) if pose is None else np.asarray(pose, F8)
    o = pose[:3, 3]
    dw = d @ pose[:3, :3].T
    depth = np.full(len(d), np.inf)
    for a in range(3):
        n = _CORNER_AXES[:, a]
        denom = dw @ n
        lam = ((_CORNER_AT - o) @ n) / np.where(denom == 0, 1, denom)
        hit = o + lam[:, None] * dw
        inside = np.ones(len(d), bool)
        for b in range(3):   # the planes are the three faces of the octant that opens towards the camera
            if b != a:
                inside &= (hit - _CORNER_AT) @ _CORNER_AXES[:, b] <= 1e-9
        ok = (denom != 0) & (lam > 0) & inside
        depth = np.where(ok & (lam < depth), lam, depth)
    cloud = np.zeros((len(d), 4), F4)
    cloud[:, :3] = (d * depth[:, None]).astype(F4)
    cloud[~np.isfinite(depth), :3] = np.nan
    rgb = (np.arange(len(d), dtype=np.uint32) * np.uint32(2654435761)) & np.uint32(0x00FFFFFF)
    cloud[:, 3] = rgb.view(F4)
    if holes:
        rng = np.random.default_rng(seed)
        cloud[rng.choice(len(d), holes, replace=False), 2] = np.nan
    return cloud


# ---- planted cases -------------------------------------------------------------------------------------------------------
def _pose(mv):
    return rigid([0.01 * mv, -0.008 * mv, 0.005 * mv], [0.02 * mv, 0.01 * mv, -0.015 * mv])


FULL_LOOP = dict(euclidean_fitness_epsilon=1e-9, transformation_epsilon=1e-12)


def _threshold_pairs():
    """Exact coordinates: with G = identity P = S bit for bit, so d2 is what the rows say.  Row 0 meets its target at d2 ==
    0.0625f == 0.25 * 0.25, row 1 at the next float above it; rows 2 .. 4 meet theirs at distance 0."""
    dy = F4(2.0 ** -13.5)
    S = np.zeros((5, 4), F4)
    T = np.zeros((5, 4), F4)
    S[:, 0] = [0.0, 10.0, 20.0, 20.0, 20.0]
    S[:, 1] = [0.0, 0.0, 0.0, 3.0, 0.0]
    S[:, 2] = [1.0, 1.0, 1.0, 1.0, 4.0]
    T[:] = S
    T[0, 0] = 0.25
    T[1, 0], T[1, 1] = 10.25, dy
    return S, T


def _three_pairs(c):
    """70 source rows on a line, 10 m apart from every target row but for the first c, which have a target 1 cm away."""
    S = np.zeros((70, 4), F4)
    S[:, 0] = np.arange(70) * 0.5
    S[:, 1] = (np.arange(70) % 3) * 0.25
    S[:, 2] = 1.0 + ((np.arange(70) ** 2) % 5) * 0.125   # (the first three rows are not collinear)
    T = S[:c].copy()
    T[:, 2] += F4(0.01)
    far = S[40:45].copy()
    far[:, 1] += F4(10.0)
    return S, np.concatenate([T, far])


def _mirrored():
    """The target is the source mirrored in x, pair by pair: the best orthogonal map is a reflection, so det(U) det(V) < 0
    and the increment is the rotation that flips the weakest direction too."""
    rng = np.random.default_rng(5)
    S = np.zeros((12, 4), F4)
    S[:, 0] = rng.uniform(-0.2, 0.2, 12)
    S[:, 1] = np.arange(12) * 0.5
    S[:, 2] = 2.0 + rng.uniform(-0.05, 0.05, 12)
    T = S.copy()
    T[:, 0] = -S[:, 0]
    return S, T


def planted_cases():
    """name -> dict(source, target, G (None = identity), params, expect = (state, iterations)).  The expectations
    were derived with this oracle on these inputs and are asserted by tests/test_oracle_icp.py."""
    c = room_corner()
    cases = {}

    def add(name, source, target, expect, G=None, **params):
        cases[name] = dict(source=source, target=target, G=G, params=default_params(**params), expect=expect)

    small = room_corner(48, 36)
    add("source = target, 48 x 36", small, small, (TRANSFORM, 1))
    add("source = target, 64 x 48", c, c, (ABS_MSE, 2))
    M = rigid(np.array([0, 0.6, 0.8]) * 0.003, np.array([0, 0.6, 0.8]) * 0.01)
    add("3 mrad, 1 cm", c, moved(c, M), (TRANSFORM, 2), euclidean_fitness_epsilon=1e-9)
    M = rigid([0.006, 0.0064, 0.0048], [0.018, 0.0192, 0.0144])
    add("defaults, 10 mrad, 3 cm", c, moved(c, M), (REL_MSE, 2))
    add("full loop, abs mse in the second chunk", c, moved(c, np.linalg.inv(_pose(1))), (ABS_MSE, 5), **FULL_LOOP)
    add("full loop, abs mse in the third chunk", c, moved(c, np.linalg.inv(_pose(1.5))), (ABS_MSE, 7), **FULL_LOOP)
    add("full loop, abs mse in the fourth chunk", c, moved(c, np.linalg.inv(_pose(5))), (ABS_MSE, 15),
        max_correspondence_distance=0.25, **FULL_LOOP)
    add("full loop, transform in the fourth chunk", c, room_corner(pose=_pose(2)), (TRANSFORM, 19), **FULL_LOOP)
    add("full loop, to the iteration limit", c, room_corner(pose=_pose(2.5)), (ITERATIONS, 50), **FULL_LOOP)
    # the same three ends on 32 x 24 rasters: short enough for the kernel emulation to run the whole job; the last one ends
    # inside a chunk that max_iterations cuts short (2 + 4 + 8 + 16 = 30, then 10 instead of 16)
    s32 = room_corner(32, 24)
    wide = dict(max_correspondence_distance=0.25, **FULL_LOOP)
    add("32 x 24, abs mse in the fourth chunk", s32, moved(s32, np.linalg.inv(_pose(10))), (ABS_MSE, 19), **wide)
    add("32 x 24, transform in the fourth chunk", s32, room_corner(32, 24, pose=_pose(5)), (TRANSFORM, 27), **wide)
    add("32 x 24, to an iteration limit of 40", s32, room_corner(32, 24, pose=_pose(7)), (ITERATIONS, 40), max_iterations=40, **wide)
    add("max_iterations 1", c, moved(c, np.linalg.inv(_pose(1))), (ITERATIONS, 1), max_iterations=1, **FULL_LOOP)
    G = rigid([0.3, -0.2, 0.1], [0.5, -0.25, 0.125]).astype(F4)
    add("target 10 m away", c, moved(c, rigid([0, 0, 0], [10, 0, 0])), (NO_CORRESPONDENCES, 1), G=G)
    S, T = _three_pairs(3)
    add("exactly 3 correspondences", S, T, (ITERATIONS, 1), max_iterations=1)
    S, T = _three_pairs(2)
    add("only 2 correspondences", S, T, (NO_CORRESPONDENCES, 1))
    S, T = _threshold_pairs()
    add("d2 at the threshold and one float above", S, T, (ITERATIONS, 1), max_correspondence_distance=0.25, max_iterations=1)
    half = moved(c, np.linalg.inv(_pose(1)))
    add("duplicated target rows", c, np.concatenate([half, half]), (ABS_MSE, 5), desired_size=7000, **FULL_LOOP)
    S, T = _mirrored()
    add("reflection", S, T, (ITERATIONS, 2), max_correspondence_distance=0.5, max_iterations=2, **FULL_LOOP)
    for ns, nt in ((1, 3072), (63, 3072), (64, 65), (65, 64), (511, 513), (512, 512), (513, 511), (257, 1), (255, 256)):
        end = (NO_CORRESPONDENCES, 1) if ns == 1 else (ITERATIONS, 3)   # one row cannot give three pairs
        add("sizes %d x %d" % (ns, nt), half[:ns], c[:nt], end, max_iterations=3, **FULL_LOOP)
    nan = c.copy()
    nan[:, 2] = np.nan
    add("all-NaN source", nan, c, (NO_CORRESPONDENCES, 1))
    add("all-NaN target", c, nan, (NO_CORRESPONDENCES, 1))
    holes = room_corner(holes=700, seed=2)
    add("desired_size above |V|", holes, moved(c, np.linalg.inv(_pose(1))), (ITERATIONS, 4), desired_size=5000, max_iterations=4, **FULL_LOOP)
    add("desired_size = |V|", c, half, (ITERATIONS, 4), desired_size=3072, max_iterations=4, **FULL_LOOP)
    add("desired_size far below |V|", c, half, (TRANSFORM, 2), desired_size=100, max_correspondence_distance=0.25, max_iterations=6, **FULL_LOOP)
    add("non-identity guess", c, moved(c, _pose(6)), (TRANSFORM, 2), G=_pose(5.8).astype(F4), **FULL_LOOP)
    bad = half.copy()
    bad[5, 0], bad[70, 1], bad[300, 0], bad[301, 2] = np.inf, np.nan, -np.inf, np.inf
    badt = c.copy()
    badt[9, 0], badt[10, 1], badt[11, 2] = np.nan, np.inf, -np.inf
    add("non-finite rows", bad, badt, (ITERATIONS, 3), max_iterations=3, **FULL_LOOP)
    return cases


_REFERENCE = {}


def reference(name, trace=False):
    """The oracle's result for a planted case, computed once."""
    key = (name, trace)
    if key not in _REFERENCE:
        case = planted_cases()[name]
        _REFERENCE[key] = align_clouds(case["source"], case["target"], case["G"], trace, **case["params"])
    return _REFERENCE[key]


def corner_depth(cols=64, rows=48, pose=None, holes=0, seed=0):
    """The depth image (rows x cols float32, NaN = no depth) and the intrinsics (fx, fy, cx, cy) of room_corner's camera:
    what rgbdfe_upload_node_cloud takes to build the same raster as a resident node cloud."""
    z = room_corner(cols, rows, pose, holes, seed)[:, 2].reshape(rows, cols).copy()
    return z, (cols * 0.9, cols * 0.9, (cols - 1) / 2, (rows - 1) / 2)


# the resident-cloud batch of tests/test_gpu_icp.py: node -> (cols, rows, pose scale or None), and the jobs (source, target,
# guess pose scale or None).  One call, one set of parameters; the jobs differ in size and end in different chunks.
BATCH_NODES = {11: (64, 48, None), 12: (64, 48, 2.0), 20: (48, 36, None), 31: (32, 24, 5.0), 30: (32, 24, None), 40: (32, 24, 7.0)}
BATCH_JOBS = [(11, 12, None), (12, 11, None), (11, 11, None), (30, 31, None), (31, 30, None), (20, 11, None), (11, 12, 1.9),
              (30, 40, None), (30, 31, None)]
BATCH_PARAMS = dict(max_correspondence_distance=0.25, max_iterations=40, **FULL_LOOP)
