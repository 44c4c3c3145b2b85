"""TEST INFRASTRUCTURE: the literal restatement of the pose-graph optimiser's contract (include/rgbdfe.h, "pose-graph
optimisation") in numpy: Levenberg-Marquardt over SE(3) edges with a Huber kernel, solved by block-Jacobi
preconditioned conjugate gradients.  Every floating-point operation is an elementwise + - * / sqrt on float64 in the
contract's order (no @, dot or sum where the order matters: arrays run over edges / vertices / blocks, never over the terms
of a sum), so the device's results can be compared byte for byte.  Vertices are 0 .. n - 1 (the library's: ascending node
id), edges are in insertion order."""
import math

import numpy as np

TILE = 64            # the width of the reduction tree's leaves (values per workgroup)
PCG_TOL = 1e-6       # stop when r' M^-1 r <= PCG_TOL (absolute)
MAX_TRIALS = 10
F8 = np.float64


# ---- small fixed-order pieces -----------------------------------------------------------------------------------------
def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def tree_sum(v):
    """The one reduction tree: leaves of TILE consecutive values (zero padded) halved 32, 16, .. 1; the leaf sums go
    round-robin into TILE accumulators (leaf k into k % TILE, in ascending k), which are halved the same way."""
    v = np.asarray(v, F8).ravel()
    m = max(1, -(-len(v) // TILE))
    x = np.zeros(m * TILE, F8)
    x[:len(v)] = v
    x = x.reshape(m, TILE)
    s = TILE // 2
    while s >= 1:
        x = x[:, :s] + x[:, s:2 * s]
        s //= 2
    part = x[:, 0]
    rounds = -(-m // TILE)
    p = np.zeros(rounds * TILE, F8)
    p[:m] = part
    p = p.reshape(rounds, TILE)
    acc = np.zeros(TILE, F8)
    for k in range(rounds):
        acc = acc + p[k]
    s = TILE // 2
    while s >= 1:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return F8(acc[0])


def quat_from_rot(R):
    """(x, y, z, w) of rotation matrices R[..., 3, 3]: the four-branch conversion, normalised, w >= 0."""
    R = np.asarray(R, F8)
    r = lambda a, b: R[..., a, b]
    with np.errstate(all="ignore"):
        tr = (r(0, 0) + r(1, 1)) + r(2, 2)
        s = np.sqrt(tr + 1.0)
        w0 = 0.5 * s
        s2 = 0.5 / s
        cand = [((r(2, 1) - r(1, 2)) * s2, (r(0, 2) - r(2, 0)) * s2, (r(1, 0) - r(0, 1)) * s2, w0)]
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            s = np.sqrt(((r(i, i) - r(j, j)) - r(k, k)) + 1.0)
            q = [None] * 3
            q[i] = 0.5 * s
            s2 = 0.5 / s
            w = (r(k, j) - r(j, k)) * s2
            q[j] = (r(j, i) + r(i, j)) * s2
            q[k] = (r(k, i) + r(i, k)) * s2
            cand.append((q[0], q[1], q[2], w))
    i1 = r(1, 1) > r(0, 0)
    dmax = np.where(i1, r(1, 1), r(0, 0))
    i2 = r(2, 2) > dmax
    branch = np.where(tr > 0.0, 0, np.where(i2, 3, np.where(i1, 2, 1)))
    out = [np.choose(branch, [c[n] for c in cand]) for n in range(4)]
    x, y, z, w = out
    nrm = np.sqrt(((x * x + y * y) + z * z) + w * w)
    x, y, z, w = x / nrm, y / nrm, z / nrm, w / nrm
    neg = w < 0.0
    return (np.where(neg, -x, x), np.where(neg, -y, y), np.where(neg, -z, z), np.where(neg, -w, w)), branch


def rot_from_update(v0, v1, v2):
    """fromVectorMQT's rotation: w = 1 - |v|^2; w < 0: identity, else the matrix of (v, sqrt(w))."""
    w = 1.0 - ((v0 * v0 + v1 * v1) + v2 * v2)
    ident = w < 0.0
    with np.errstate(invalid="ignore"):
        w = np.sqrt(w)
    tx, ty, tz = 2.0 * v0, 2.0 * v1, 2.0 * v2
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * v0, tx * v1, tx * v2
    tyy, tyz, tzz = ty * v1, ty * v2, tz * v2
    R = np.empty(np.shape(v0) + (3, 3), F8)
    R[..., 0, 0] = 1.0 - (tyy + tzz)
    R[..., 0, 1] = txy - twz
    R[..., 0, 2] = txz + twy
    R[..., 1, 0] = txy + twz
    R[..., 1, 1] = 1.0 - (txx + tzz)
    R[..., 1, 2] = tyz - twx
    R[..., 2, 0] = txz - twy
    R[..., 2, 1] = tyz + twx
    R[..., 2, 2] = 1.0 - (txx + tyy)
    R[ident] = np.eye(3)
    return R


def apply_update(R, t, d):
    """X <- X * fromVectorMQT(d) for arrays of poses (R[n,3,3], t[n,3]) and updates d[n,6]; no re-orthogonalisation."""
    Rd = rot_from_update(d[:, 3], d[:, 4], d[:, 5])
    Rn = np.empty_like(R)
    tn = np.empty_like(t)
    for a in range(3):
        for b in range(3):
            Rn[:, a, b] = dot3(R[:, a, 0], R[:, a, 1], R[:, a, 2], Rd[:, 0, b], Rd[:, 1, b], Rd[:, 2, b])
        tn[:, a] = dot3(R[:, a, 0], R[:, a, 1], R[:, a, 2], d[:, 0], d[:, 1], d[:, 2]) + t[:, a]
    return Rn, tn


# ---- the graph --------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, n):
        self.n = n
        self.R = np.tile(np.eye(3), (n, 1, 1))
        self.t = np.zeros((n, 3))
        self.fixed = np.zeros(n, bool)
        self.ei, self.ej, self.ZR, self.Zt, self.Om = [], [], [], [], []

    def set_estimate(self, v, T):
        T = np.asarray(T, F8).reshape(4, 4)
        self.R[v] = T[:3, :3]
        self.t[v] = T[:3, 3]

    def estimate(self, v):
        T = np.eye(4)
        T[:3, :3] = self.R[v]
        T[:3, 3] = self.t[v]
        return T

    def add_edge(self, i, j, Z, Om, set_estimate=False):
        Z = np.asarray(Z, F8).reshape(4, 4)
        self.ei.append(i); self.ej.append(j)
        self.ZR.append(Z[:3, :3].copy()); self.Zt.append(Z[:3, 3].copy())
        self.Om.append(np.asarray(Om, F8).reshape(6, 6).copy())
        if set_estimate:  # X2 = X1 * Z
            R1, t1 = self.R[i], self.t[i]
            Rn = np.empty((3, 3)); tn = np.empty(3)
            for a in range(3):
                for b in range(3):
                    Rn[a, b] = dot3(R1[a, 0], R1[a, 1], R1[a, 2], Z[0, b], Z[1, b], Z[2, b])
                tn[a] = dot3(R1[a, 0], R1[a, 1], R1[a, 2], Z[0, 3], Z[1, 3], Z[2, 3]) + t1[a]
            self.R[j], self.t[j] = Rn, tn

    def arrays(self):
        E = len(self.ei)
        return (np.array(self.ei, np.int64), np.array(self.ej, np.int64), np.array(self.ZR, F8).reshape(E, 3, 3),
                np.array(self.Zt, F8).reshape(E, 3), np.array(self.Om, F8).reshape(E, 6, 6))


class Plan:
    """Built once per call: the free-vertex index map, and the distinct off-diagonal block positions in the order the
    edges first touch them (row = the smaller free index), with the edges that feed each (and whether transposed)."""

    def __init__(self, g):
        self.free_of = np.full(g.n, -1, np.int64)
        self.free_of[~g.fixed] = np.arange(int((~g.fixed).sum()))
        self.verts = np.flatnonzero(~g.fixed)
        self.nf = len(self.verts)
        self.blocks = []      # (row, col)
        self.feeds = []       # per block: [(edge, transposed)]
        index = {}
        for e, (i, j) in enumerate(zip(g.ei, g.ej)):
            fi, fj = self.free_of[i], self.free_of[j]
            if fi < 0 or fj < 0 or fi == fj:
                continue
            key = (min(fi, fj), max(fi, fj))
            if key not in index:
                index[key] = len(self.blocks)
                self.blocks.append(key)
                self.feeds.append([])
            self.feeds[index[key]].append((e, fi > fj))


def edge_terms(g, R, t, jacobians=True):
    """Per edge: e[E,6], chi2 = e'Oe, rho, w = rho', and with jacobians Ji, Jj[E,6,6] and the products
    Hii, Hij, Hjj (w * J'OJ) and bi, bj (-w * J'Oe)."""
    ei, ej, ZR, Zt, Om = g.arrays()
    E = len(ei)
    Ri, ti, Rj, tj = R[ei], t[ei], R[ej], t[ej]
    Ra = np.empty((E, 3, 3)); ta = np.empty((E, 3)); RD = np.empty((E, 3, 3)); tD = np.empty((E, 3))
    d = [tj[:, k] - ti[:, k] for k in range(3)]
    for a in range(3):
        for b in range(3):
            Ra[:, a, b] = dot3(Ri[:, 0, a], Ri[:, 1, a], Ri[:, 2, a], Rj[:, 0, b], Rj[:, 1, b], Rj[:, 2, b])
        ta[:, a] = dot3(Ri[:, 0, a], Ri[:, 1, a], Ri[:, 2, a], d[0], d[1], d[2])
    d = [ta[:, k] - Zt[:, k] for k in range(3)]
    for a in range(3):
        for b in range(3):
            RD[:, a, b] = dot3(ZR[:, 0, a], ZR[:, 1, a], ZR[:, 2, a], Ra[:, 0, b], Ra[:, 1, b], Ra[:, 2, b])
        tD[:, a] = dot3(ZR[:, 0, a], ZR[:, 1, a], ZR[:, 2, a], d[0], d[1], d[2])
    (qx, qy, qz, qw), branch = quat_from_rot(RD)
    e = np.stack([tD[:, 0], tD[:, 1], tD[:, 2], qx, qy, qz], axis=1)
    Oe = np.empty((E, 6))
    for a in range(6):
        acc = Om[:, a, 0] * e[:, 0]
        for k in range(1, 6):
            acc = acc + Om[:, a, k] * e[:, k]
        Oe[:, a] = acc
    chi2 = e[:, 0] * Oe[:, 0]
    for k in range(1, 6):
        chi2 = chi2 + e[:, k] * Oe[:, k]
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        inl = chi2 <= 1.0
        rho = np.where(inl, chi2, 2.0 * sq - 1.0)
        w = np.where(inl, 1.0, 1.0 / sq)
    out = dict(e=e, chi2=chi2, rho=rho, w=w, branch=branch)
    if not jacobians:
        return out
    Ji = np.zeros((E, 6, 6)); Jj = np.zeros((E, 6, 6))
    # Q = w I + [u]x  (u = the error quaternion's vector part)
    Q = np.zeros((E, 3, 3))
    Q[:, 0, 0] = qw; Q[:, 0, 1] = -qz; Q[:, 0, 2] = qy
    Q[:, 1, 0] = qz; Q[:, 1, 1] = qw; Q[:, 1, 2] = -qx
    Q[:, 2, 0] = -qy; Q[:, 2, 1] = qx; Q[:, 2, 2] = qw
    # S = 2 [ta]x
    S = np.zeros((E, 3, 3))
    a2 = [2.0 * ta[:, k] for k in range(3)]
    S[:, 0, 1] = -a2[2]; S[:, 0, 2] = a2[1]
    S[:, 1, 0] = a2[2]; S[:, 1, 2] = -a2[0]
    S[:, 2, 0] = -a2[1]; S[:, 2, 1] = a2[0]
    for a in range(3):
        for b in range(3):
            Jj[:, a, b] = RD[:, a, b]
            Jj[:, 3 + a, 3 + b] = Q[:, a, b]
            Ji[:, a, b] = -ZR[:, b, a]
            Ji[:, a, 3 + b] = dot3(ZR[:, 0, a], ZR[:, 1, a], ZR[:, 2, a], S[:, 0, b], S[:, 1, b], S[:, 2, b])
            Ji[:, 3 + a, 3 + b] = -dot3(Q[:, a, 0], Q[:, a, 1], Q[:, a, 2], Ra[:, b, 0], Ra[:, b, 1], Ra[:, b, 2])

    def om_times(J):
        W = np.empty((E, 6, 6))
        for a in range(6):
            for b in range(6):
                acc = Om[:, a, 0] * J[:, 0, b]
                for k in range(1, 6):
                    acc = acc + Om[:, a, k] * J[:, k, b]
                W[:, a, b] = acc
        return W

    def jt_times(J, W):
        H = np.empty((E, 6, 6))
        for a in range(6):
            for b in range(6):
                acc = J[:, 0, a] * W[:, 0, b]
                for k in range(1, 6):
                    acc = acc + J[:, k, a] * W[:, k, b]
                H[:, a, b] = w * acc
        return H

    def jt_vec(J):
        bv = np.empty((E, 6))
        for a in range(6):
            acc = J[:, 0, a] * Oe[:, 0]
            for k in range(1, 6):
                acc = acc + J[:, k, a] * Oe[:, k]
            bv[:, a] = -(w * acc)
        return bv

    Wi, Wj = om_times(Ji), om_times(Jj)
    out.update(Ji=Ji, Jj=Jj, Hii=jt_times(Ji, Wi), Hij=jt_times(Ji, Wj), Hjj=jt_times(Jj, Wj), bi=jt_vec(Ji), bj=jt_vec(Jj))
    return out


def chi2(g, R=None, t=None):
    if len(g.ei) == 0:
        return F8(0.0)
    return tree_sum(edge_terms(g, g.R if R is None else R, g.t if t is None else t, jacobians=False)["rho"])


def linearize(g, plan=None, R=None, t=None):
    """errors, weights, chi2, and the system: Hd[nf,6,6], b[nf,6], the off-diagonal blocks B[nb,6,6] at plan.blocks --
    every sum over edges in insertion order."""
    plan = plan or Plan(g)
    R = g.R if R is None else R
    t = g.t if t is None else t
    T = edge_terms(g, R, t)
    Hd = np.zeros((plan.nf, 6, 6)); b = np.zeros((plan.nf, 6))
    for e, (i, j) in enumerate(zip(g.ei, g.ej)):
        fi, fj = plan.free_of[i], plan.free_of[j]
        if fi >= 0:
            Hd[fi] = Hd[fi] + T["Hii"][e]
            b[fi] = b[fi] + T["bi"][e]
        if fj >= 0:
            Hd[fj] = Hd[fj] + T["Hjj"][e]
            b[fj] = b[fj] + T["bj"][e]
    B = np.zeros((len(plan.blocks), 6, 6))
    for k, feeds in enumerate(plan.feeds):
        for e, tr in feeds:
            B[k] = B[k] + (T["Hij"][e].T if tr else T["Hij"][e])
    return dict(e=T["e"], w=T["w"], rho=T["rho"], chi2=tree_sum(T["rho"]), Hd=Hd, b=b, B=B, plan=plan, terms=T)


# ---- PCG --------------------------------------------------------------------------------------------------------------
def cholesky6(A):
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            L[:, j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                s = A[:, i, j].copy()
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                L[:, i, j] = s / L[:, j, j]
    return L


def chol_solve(L, r):
    y = np.empty_like(r)
    with np.errstate(all="ignore"):
        for i in range(6):
            s = r[:, i].copy()
            for k in range(i):
                s = s - L[:, i, k] * y[:, k]
            y[:, i] = s / L[:, i, i]
        z = np.empty_like(r)
        for i in range(5, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 6):
                s = s - L[:, k, i] * z[:, k]
            z[:, i] = s / L[:, i, i]
    return z


def vdot(a, b):
    """sum_f (a_f . b_f): six terms per vertex left to right, then the tree over the vertices."""
    d = a[:, 0] * b[:, 0]
    for k in range(1, 6):
        d = d + a[:, k] * b[:, k]
    return tree_sum(d)


def spmv(plan, Ad, B, p):
    """q = A p: a row takes its diagonal block's six terms, then its off-diagonal blocks in block order, six terms each."""
    q = Ad[:, :, 0] * p[:, 0:1]
    for k in range(1, 6):
        q = q + Ad[:, :, k] * p[:, k:k + 1]
    for n, (r, c) in enumerate(plan.blocks):
        for k in range(6):
            q[r] = q[r] + B[n][:, k] * p[c][k]
        for k in range(6):
            q[c] = q[c] + B[n][k, :] * p[r][k]
    return q


def pcg(plan, Hd, B, b, lam, max_iter=None):
    """(x, iterations) of (H + lam I) x = b."""
    nf = plan.nf
    max_iter = 6 * nf if max_iter is None else max_iter
    Ad = Hd.copy()
    for a in range(6):
        Ad[:, a, a] = Ad[:, a, a] + lam
    L = cholesky6(Ad)
    x = np.zeros((nf, 6))
    r = b.copy()
    z = chol_solve(L, r)
    p = z.copy()
    rz = vdot(r, z)
    it = 0
    with np.errstate(all="ignore"):
        while not (rz <= PCG_TOL) and it < max_iter:
            q = spmv(plan, Ad, B, p)
            alpha = rz / vdot(p, q)
            x = x + alpha * p
            r = r - alpha * q
            z = chol_solve(L, r)
            rz_new = vdot(r, z)
            beta = rz_new / rz
            p = z + beta * p
            rz = rz_new
            it += 1
    return x, it


# ---- Levenberg-Marquardt ----------------------------------------------------------------------------------------------
def new_report():
    return dict(iterations=0, chi2=F8(0.0), its=[])


def optimize(g, iterations, report=None, solver=None):
    """SparseOptimizer::optimize(iterations) on g (estimates updated in place).  solver(plan, Hd, B, b, lam) -> (x, its)
    replaces PCG (tests: a dense solve)."""
    report = new_report() if report is None else report
    solver = solver or pcg
    plan = Plan(g)
    if len(g.ei) == 0 or plan.nf == 0:
        report["chi2"] = chi2(g)
        return 0
    lam = ni = None
    done = 0
    for it in range(iterations):
        lin = linearize(g, plan)
        cur = lin["chi2"]
        if it == 0:
            mx = F8(0.0)
            for a in range(6):
                mx = max(mx, np.abs(lin["Hd"][:, a, a]).max())
            lam = F8(1e-5) * mx
            ni = F8(2.0)
        rec = dict(trials=0, pcg=[], chi2_before=cur, chi2_after=cur, lam=lam)
        rho = F8(0.0)
        qmax = 0
        while True:
            x, its = solver(plan, lin["Hd"], lin["B"], lin["b"], lam)
            d = np.zeros((g.n, 6))
            d[plan.verts] = x
            Rn, tn = apply_update(g.R, g.t, d)
            Rn[g.fixed], tn[g.fixed] = g.R[g.fixed], g.t[g.fixed]
            with np.errstate(all="ignore"):
                trial = chi2(g, Rn, tn)
                sc = x[:, 0] * (lam * x[:, 0] + lin["b"][:, 0])
                for k in range(1, 6):
                    sc = sc + x[:, k] * (lam * x[:, k] + lin["b"][:, k])
                scale = tree_sum(sc) + 1e-3
                rho = (cur - trial) / scale
            rec["trials"] += 1
            rec["pcg"].append(its)
            if rho > 0 and np.isfinite(trial):
                g.R, g.t = Rn, tn
                a = 2.0 * rho - 1.0
                a = 1.0 - (a * a) * a
                a = min(a, F8(2.0) / F8(3.0))
                a = max(F8(1.0) / F8(3.0), a)
                lam = lam * a
                ni = F8(2.0)
                cur = trial
            else:
                lam = lam * ni
                ni = ni * 2.0
            qmax += 1
            if not (rho < 0 and qmax < MAX_TRIALS):
                break
        rec["chi2_after"] = cur
        rec["lam"] = lam
        report["its"].append(rec)
        done += 1
        if qmax == MAX_TRIALS or rho == 0:
            break
    report["iterations"] += done
    report["chi2"] = chi2(g)
    return done


def optimize_graph(g, break_criterion, report=None, solver=None):
    """The outer loop of GraphManager::optimizeGraphImpl (graph_manager.cpp:996-1014); returns chi2."""
    report = new_report() if report is None else report
    c = float(break_criterion)
    if c >= 1.0:
        total = 0
        while True:
            n = optimize(g, int(math.ceil(c / 10.0)), report, solver)
            total += n
            if not (total < c and n > 0):
                break
        return report["chi2"]
    prev = None
    value = F8(np.finfo(F8).max)
    while True:
        prev = value
        n = optimize(g, 5, report, solver)
        value = report["chi2"]
        with np.errstate(all="ignore"):
            go_on = n > 0 and (value / prev < (1.0 - c))
        if not go_on:
            break
    return value


# ---- planted graphs ---------------------------------------------------------------------------------------------------
def rot_axis(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    R = np.eye(3)
    a, b = (axis + 1) % 3, (axis + 2) % 3
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


def pose(rng, sigma_t=1.0, sigma_r=0.5):
    v = rng.normal(size=3) * sigma_r
    ang = np.linalg.norm(v)
    T = np.eye(4)
    if ang > 0:
        k = v / ang
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    T[:3, 3] = rng.normal(size=3) * sigma_t
    return T


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def make_graph(n, edges, seed, fixed=(0,), noise=0.02, init_noise=(0.1, 0.05), info=None, rot_sigma=None):
    """Ground-truth poses, measurements with noise, initial estimates perturbed.  edges: (i, j) pairs."""
    rng = np.random.default_rng(seed)
    truth = [pose(rng) for _ in range(n)]
    g = Graph(n)
    for v in range(n):
        st, sr = init_noise
        if rot_sigma is not None:
            sr = rot_sigma
        g.set_estimate(v, truth[v] @ pose(rng, st, sr) if v not in fixed else truth[v])
    g.fixed[list(fixed)] = True
    for (i, j) in edges:
        Z = inv(truth[i]) @ truth[j] @ pose(rng, noise, noise)
        Om = info(rng) if info else np.eye(6) * 100.0
        g.add_edge(i, j, Z, Om)
    return g


def chain_edges(n, pred=1, loops=()):
    e = [(i - k, i) for i in range(n) for k in range(1, pred + 1) if i - k >= 0]
    return e + list(loops)


def general_info(rng):
    A = rng.normal(size=(6, 6))
    return A @ A.T * 10.0 + np.eye(6) * 5.0


def rejecting_graph(seed):
    return make_graph(12, chain_edges(12, 3, [(0, 11), (2, 9)]), seed, rot_sigma=1.5)


def huber_boundary(up):
    g = Graph(2)
    g.fixed[0] = True
    T = np.eye(4)
    T[0, 3] = np.nextafter(1.0, 2.0) if up else 1.0
    g.set_estimate(1, T)
    g.add_edge(0, 1, np.eye(4), np.eye(6))
    return g


def branch_graph():
    """Error rotations of about 170 degrees about x, y and z (and a small one): every quaternion branch."""
    g = Graph(5)
    g.fixed[0] = True
    for v, (axis, ang) in enumerate([(0, 0.1), (0, 2.97), (1, 2.97), (2, 2.97)], start=1):
        T = np.eye(4)
        T[:3, :3] = rot_axis(axis, ang)
        T[:3, 3] = [0.1 * v, -0.2, 0.3]
        g.set_estimate(v, T)
        g.add_edge(0, v, np.eye(4), np.eye(6) * 2.0)
    return g


def planted_graphs():
    """(name, builder) pairs: the smallest graphs at which each piece can go wrong.  Builders give a fresh Graph."""
    hub = [(0, i) for i in range(1, 66)]
    out = [
        ("one edge", lambda: make_graph(2, [(0, 1)], 1)),
        ("chain of 3, middle fixed", lambda: make_graph(3, [(0, 1), (1, 2)], 2, fixed=(1,))),
        ("edge with id1 > id2", lambda: make_graph(3, [(0, 1), (2, 1), (2, 0)], 3)),
        ("three edges on one pair", lambda: make_graph(3, [(1, 2), (2, 1), (1, 2), (0, 1)], 4)),
        ("hub of degree 65", lambda: make_graph(66, hub + [(i, i + 1) for i in range(1, 65)], 5, fixed=(3,))),
        ("65 vertices, 129 edges", lambda: make_graph(65, chain_edges(65, 2) + [(0, 64), (5, 40)], 6)),
        ("quaternion branches", branch_graph),
        ("general information", lambda: make_graph(6, chain_edges(6, 2, [(0, 5)]), 7, info=general_info)),
        ("huber boundary", lambda: huber_boundary(False)),
        ("huber boundary, next up", lambda: huber_boundary(True)),
        ("no fixed vertex", lambda: make_graph(5, chain_edges(5, 2, [(0, 4)]), 8, fixed=())),
        ("all but one fixed", lambda: make_graph(5, chain_edges(5, 2, [(0, 4)]), 9, fixed=(0, 1, 3, 4))),
        ("rejected trials a", lambda: rejecting_graph(REJECT_SEEDS[0])),
        ("rejected trials b", lambda: rejecting_graph(REJECT_SEEDS[1])),
        ("second pcg chunk", lambda: make_graph(40, chain_edges(40, 1, [(0, 39)]), 10, fixed=(0,), init_noise=(0.5, 0.2))),
    ]
    return out


REJECT_SEEDS = (12, 27)  # chosen on the CPU: the oracle's report has rejected trials (asserted by the tests that use them)
PCG_FIRST_CHUNK = 8       # the library's first read-back chunk of PCG iterations
