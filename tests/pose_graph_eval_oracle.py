"""TEST INFRASTRUCTURE: the literal restatement of the pose graph's last stage (include/rgbdfe.h, "fixation strategies,
pruning and the evaluation rounds") on top of tests/pose_graph_oracle.py, which it imports unchanged: the
pose_relative_to strategies (graph_manager.cpp:444, :889-896, :911-937, :1031-1036), pruneEdgesWithErrorAbove (:1106-1246),
sanityCheck (:1347-1360), the five rounds of OpenNIListener::evaluation (openni_listener.cpp:431-518) and saveTrajectory's
estimate file (graph_mgr_io.cpp:615-677).  Float64 elementwise + - * / sqrt in the contract's order, so the device's results
can be compared byte for byte.  Nodes are 0 .. n - 1 and a node's id is its index (the library's ids may be shifted by a
constant: only differences of ids and their order matter).

An inactive (pruned) edge keeps its slot: rho 0 in its place of the chi2 tree, no part in H, b or the block list.  The lists of
the active edges in insertion order are those of a graph that holds the active edges alone, so the linear algebra is
pose_graph_oracle's on that graph; only the chi2 tree is laid over all slots."""
import math

import numpy as np

import pose_graph_oracle as po

F8 = np.float64
NONE, FIRST, PREVIOUS, LARGEST_LOOP, INAFFECTED = range(5)
STRATEGIES = dict(none=NONE, first=FIRST, previous=PREVIOUS, largest_loop=LARGEST_LOOP, inaffected=INAFFECTED)
KEPT, REMOVED, DISCOUNTED, ZERO_MOTION = range(4)
PRUNE_THRESHOLDS = (5.0, 1.0, 0.25)


class EvalGraph(po.Graph):
    """po.Graph that grows node by node, with an active flag per edge and the strategy's bookkeeping."""

    def __init__(self, n=0):
        super().__init__(n)
        self.active = []
        self.strategy = NONE
        self.earliest = 0

    def add_node(self):
        v = self.n
        self.n += 1
        self.R = np.concatenate([self.R.reshape(-1, 3, 3), np.eye(3)[None]])
        self.t = np.concatenate([self.t.reshape(-1, 3), np.zeros((1, 3))])
        self.fixed = np.append(self.fixed, False)
        if self.strategy != NONE:
            self.earliest = v                                    # :444
        return v

    def add_edge(self, i, j, Z, Om, set_estimate=False):
        super().add_edge(i, j, Z, Om, set_estimate)
        self.active.append(True)
        if self.strategy == INAFFECTED:                          # :889-892
            self.fixed[i] = False
            self.fixed[j] = False
        elif self.strategy == LARGEST_LOOP:                      # :893-896
            self.earliest = min(self.earliest, i, j)

    def edge(self, e):
        Z = np.eye(4)
        Z[:3, :3], Z[:3, 3] = self.ZR[e], self.Zt[e]
        return dict(id1=self.ei[e], id2=self.ej[e], transform=Z, information=self.Om[e].copy(), active=self.active[e])


def from_graph(g):
    """An EvalGraph with the vertices, flags and edges of a po.Graph."""
    out = EvalGraph(g.n)
    out.R, out.t, out.fixed = g.R.copy(), g.t.copy(), g.fixed.copy()
    out.ei, out.ej = list(g.ei), list(g.ej)
    out.ZR, out.Zt, out.Om = [a.copy() for a in g.ZR], [a.copy() for a in g.Zt], [a.copy() for a in g.Om]
    out.active = [True] * len(g.ei)
    return out


def active_view(g):
    """(the graph of g's active edges in insertion order, sharing g's vertices; their slots)."""
    idx = [e for e in range(len(g.ei)) if g.active[e]]
    v = po.Graph(g.n)
    v.R, v.t, v.fixed = g.R, g.t, g.fixed
    v.ei, v.ej = [g.ei[e] for e in idx], [g.ej[e] for e in idx]
    v.ZR, v.Zt, v.Om = [g.ZR[e] for e in idx], [g.Zt[e] for e in idx], [g.Om[e] for e in idx]
    return v, idx


def over_slots(g, idx, values, shape=()):
    out = np.zeros((len(g.ei),) + shape, F8)
    if len(idx):
        out[idx] = values
    return out


def chi2(g, R=None, t=None, view=None):
    if len(g.ei) == 0:
        return F8(0.0)
    v, idx = view or active_view(g)
    R = g.R if R is None else R
    t = g.t if t is None else t
    rho = po.edge_terms(v, R, t, jacobians=False)["rho"] if len(idx) else []
    return po.tree_sum(over_slots(g, idx, rho))


def linearize(g, plan=None, R=None, t=None, view=None):
    """po.linearize over the active edges; e, w, rho per slot (0 at an inactive one), chi2 through the tree over all slots."""
    v, idx = view or active_view(g)
    plan = plan or po.Plan(v)
    lin = po.linearize(v, plan, g.R if R is None else R, g.t if t is None else t)
    lin["rho"] = over_slots(g, idx, lin["rho"])
    lin["chi2"] = po.tree_sum(lin["rho"])
    lin["e"] = over_slots(g, idx, lin["e"], (6,))
    lin["w"] = over_slots(g, idx, lin["w"])
    return lin


def edge_errors(g):
    """chi2 = e'Oe before Huber, err_sq = e.e left to right, the active flag; per slot."""
    v, idx = active_view(g)
    c = sq = []
    if len(idx):
        T = po.edge_terms(v, g.R, g.t, jacobians=False)
        e = T["e"]
        sq = e[:, 0] * e[:, 0]
        for k in range(1, 6):
            sq = sq + e[:, k] * e[:, k]
        c = T["chi2"]
    return dict(chi2=over_slots(g, idx, c), err_sq=over_slots(g, idx, sq), active=np.array(g.active, bool))


# ---- Levenberg-Marquardt with the gate: po.optimize, its sums over edges taken over all slots --------------------------------
def optimize(g, iterations, report=None, solver=None):
    report = po.new_report() if report is None else report
    solver = solver or po.pcg
    view = active_view(g)
    plan = po.Plan(view[0])
    if len(view[1]) == 0 or plan.nf == 0:
        report["chi2"] = chi2(g, view=view)
        return 0
    lam = ni = None
    done = 0
    for it in range(iterations):
        lin = linearize(g, plan, view=view)
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
            Rn, tn = po.apply_update(g.R, g.t, d)
            Rn[g.fixed], tn[g.fixed] = g.R[g.fixed], g.t[g.fixed]
            with np.errstate(all="ignore"):
                trial = chi2(g, Rn, tn, view=view)
                sc = x[:, 0] * (lam * x[:, 0] + lin["b"][:, 0])
                for k in range(1, 6):
                    sc = sc + x[:, k] * (lam * x[:, k] + lin["b"][:, k])
                scale = po.tree_sum(sc) + 1e-3
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
            if not (rho < 0 and qmax < po.MAX_TRIALS):
                break
        rec["chi2_after"] = cur
        rec["lam"] = lam
        report["its"].append(rec)
        done += 1
        if qmax == po.MAX_TRIALS or rho == 0:
            break
    report["iterations"] += done
    report["chi2"] = chi2(g, view=view)
    return done


def apply_fixation(g):
    """fixationOfVertices (:911-937)."""
    if g.strategy == FIRST:
        g.fixed[:] = False
        if g.n:
            g.fixed[0] = True          # the reference indexes graph_[0]: the node of lowest id
    elif g.strategy == PREVIOUS:
        if g.n > 2:
            g.fixed[:] = False
            g.fixed[g.n - 2] = True
    elif g.strategy == LARGEST_LOOP:
        g.fixed[:] = np.arange(g.n) < g.earliest


def release_fixation(g):
    """After the optimisation (:1031-1036)."""
    if g.strategy != NONE:
        g.fixed[:] = g.strategy == INAFFECTED


def optimize_graph(g, break_criterion, report=None, solver=None):
    """rgbdfe_pose_graph_optimize_graph: the strategy's flags, the loop of po.optimize_graph, the flags after; returns chi2."""
    report = po.new_report() if report is None else report
    apply_fixation(g)
    value = F8(0.0)
    if len(g.ei):
        c = float(break_criterion)
        if c >= 1.0:
            total = 0
            while True:
                n = optimize(g, int(math.ceil(c / 10.0)), report, solver)
                total += n
                if not (total < c and n > 0):
                    break
        else:
            cur = F8(np.finfo(F8).max)
            while True:
                prev = cur
                n = optimize(g, 5, report, solver)
                cur = report["chi2"]
                with np.errstate(all="ignore"):
                    go_on = n > 0 and (cur / prev < (1.0 - c))
                if not go_on:
                    break
        value = report["chi2"]
    release_fixation(g)
    return value


# ---- pruning ----------------------------------------------------------------------------------------------------------------------
def prune_edges(g, thresh):
    """pruneEdgesWithErrorAbove as it behaves: (count, a verdict per slot)."""
    thresh = F8(np.float32(thresh))
    E = len(g.ei)
    verdicts = np.zeros(E, np.uint8)
    if E == 0:
        return 0, verdicts
    c = edge_errors(g)["chi2"]
    degree = np.zeros(g.n, np.int64)         # every measured edge ever added counts, inactive ones included
    for i, j in zip(g.ei, g.ej):
        degree[i] += 1
        degree[j] += 1
    was_active = list(g.active)
    count = 0
    for e in range(E):
        if not was_active[e] or not (c[e] > thresh):   # NaN compares false: kept
            continue
        count += 1
        g.ZR[e], g.Zt[e] = np.eye(3), np.zeros(3)
        i, j = g.ei[e], g.ej[e]
        if abs(i - j) != 1:
            if degree[i] > 1 and degree[j] > 1:
                g.active[e] = False
                verdicts[e] = REMOVED
            else:
                g.Om[e] = np.eye(6) * 1e-100
                verdicts[e] = DISCOUNTED
        else:
            g.Om[e] = np.eye(6)
            verdicts[e] = ZERO_MOTION
    return count, verdicts


def sanity_check(g, thresh):
    """sanityCheck: thresh *= thresh in float; returns the number of edges changed."""
    t32 = np.float32(thresh)
    t32 = np.float32(t32 * t32)
    changed = 0
    for e in range(len(g.ei)):
        z = g.Zt[e]
        if g.active[e] and (z[0] * z[0] + z[1] * z[1]) + z[2] * z[2] > F8(t32):
            g.Om[e] = np.eye(6) * 0.000001
            changed += 1
    return changed


# ---- the evaluation rounds -----------------------------------------------------------------------------------------------------
def estimates(g):
    out = np.tile(np.eye(4), (g.n, 1, 1))
    out[:, :3, :3], out[:, :3, 3] = g.R, g.t
    return out


def evaluate(g, optimizer_iterations):
    """(rounds: dict(chi2, iterations, pruned, verdicts) each, estimates[5, n, 4, 4])."""
    rounds, est = [], []
    for r in range(5):
        pruned, verdicts, criterion = 0, None, optimizer_iterations
        if r == 1:
            g.strategy = FIRST
        if r >= 2:
            pruned, verdicts = prune_edges(g, PRUNE_THRESHOLDS[r - 2])
            if pruned == 0:
                criterion = 1.0
        rep = po.new_report()
        optimize_graph(g, criterion, rep)
        rounds.append(dict(chi2=rep["chi2"], iterations=rep["iterations"], pruned=pruned, verdicts=verdicts))
        est.append(estimates(g))
    return rounds, np.array(est)


# ---- the trajectory file -------------------------------------------------------------------------------------------------------
def pose_mul(A, B):
    out = np.eye(4)
    for a in range(3):
        for b in range(3):
            out[a, b] = po.dot3(A[a, 0], A[a, 1], A[a, 2], B[0, b], B[1, b], B[2, b])
        out[a, 3] = po.dot3(A[a, 0], A[a, 1], A[a, 2], B[0, 3], B[1, 3], B[2, 3]) + A[a, 3]
    return out


def rigid_inverse(A):
    out = np.eye(4)
    out[:3, :3] = A[:3, :3].T
    for a in range(3):
        out[a, 3] = -po.dot3(A[0, a], A[1, a], A[2, a], A[0, 3], A[1, 3], A[2, 3])
    return out


def trajectory_text(g, nodes, stamps, base2points=None, init_base_pose=None, frame_id=None, child_frame_id=None):
    """The estimate file of saveTrajectory; also returns the quaternion branch taken per line."""
    b2p = np.eye(4) if base2points is None else np.asarray(base2points, F8).reshape(4, 4)
    init = np.eye(4) if init_base_pose is None else np.asarray(init_base_pose, F8).reshape(4, 4)
    left, inv = pose_mul(init, b2p), rigid_inverse(b2p)
    text = ""
    if frame_id is not None:
        text += "# TF Coordinate Frame ID: %s(data: %s)\n" % (frame_id, child_frame_id or "")
    branches = []
    for v, stamp in zip(nodes, stamps):
        W = pose_mul(pose_mul(left, g.estimate(v)), inv)
        (x, y, z, w), branch = po.quat_from_rot(W[:3, :3])
        branches.append(int(branch))
        text += "%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n" % (stamp, W[0, 3], W[1, 3], W[2, 3], x, y, z, w)
    return text, branches


# ---- planted graphs -----------------------------------------------------------------------------------------------------------
def online_sequence(n=12, pred=3, loop=(2, 9), seed=31):
    """The frames of an online run: per frame the new node's edges [(i, j, Z, Om)], the first to a predecessor placing the
    node (set_estimate); the loop edge arrives with node loop[1]."""
    rng = np.random.default_rng(seed)
    truth = [po.pose(rng) for _ in range(n)]
    frames = []
    for v in range(n):
        edges = []
        for k in range(1, pred + 1):
            if v - k >= 0:
                edges.append((v - k, v, po.inv(truth[v - k]) @ truth[v] @ po.pose(rng, 0.02, 0.02), np.eye(6) * 100.0))
        if v == loop[1]:
            edges.append((loop[0], v, po.inv(truth[loop[0]]) @ truth[v] @ po.pose(rng, 0.02, 0.02), np.eye(6) * 100.0))
        frames.append(edges)
    return frames


def run_online(g, frames, on_frame=None, optimize_with=None):
    """Add the frames to g (an EvalGraph or anything with its add_node / add_edge / optimize_graph interface)."""
    optimize_with = optimize_with or (lambda: optimize_graph(g, 0.01))
    for v, edges in enumerate(frames):
        g.add_node()
        for k, (i, j, Z, Om) in enumerate(edges):
            g.add_edge(i, j, Z, Om, set_estimate=(k == 0))
        if edges:
            optimize_with()
        if on_frame:
            on_frame(v)


RING_N, RING_SEED = 64, 3   # the seed is chosen on the CPU: tests/test_oracle_pose_graph_eval.py asserts what it was chosen for


def ring(seed=RING_SEED, n=RING_N, n_false=4):
    """(graph, truth[n,4,4], the slots of the planted false edges): a ring of n poses, sequential edges and true loop
    edges (i, i + 5) and the closing ones with small noise, and n_false loop edges with a wrong measurement.  Estimates start
    from the odometry chain."""
    rng = np.random.default_rng(seed)
    truth = []
    for v in range(n):
        T = np.eye(4)
        a = 2.0 * math.pi * v / n
        T[:3, :3] = po.rot_axis(2, a)
        T[:3, 3] = [3.0 * math.cos(a), 3.0 * math.sin(a), 0.05 * math.sin(3 * a)]
        truth.append(T)
    g = EvalGraph(0)
    g.strategy = INAFFECTED
    info = np.eye(6) * 400.0
    false_slots = []
    false_at = {int(v): int(rng.integers(0, v - 7)) for v in rng.choice(np.arange(10, n - 1), n_false, replace=False)}
    for v in range(n):
        g.add_node()
        for k, u in enumerate([v - 1, v - 5, v - 2]):
            if u >= 0:
                g.add_edge(u, v, po.inv(truth[u]) @ truth[v] @ po.pose(rng, 0.004, 0.002), info, set_estimate=(k == 0))
        if v in false_at:
            false_slots.append(len(g.ei))
            g.add_edge(false_at[v], v, po.pose(rng, 1.0, 0.6), info)
        if v == n - 1:
            for u in (0, 1, 4):
                g.add_edge(v, u, po.inv(truth[v]) @ truth[u] @ po.pose(rng, 0.004, 0.002), info)
    return g, np.array(truth), false_slots


_RING = {}


def ring_run():
    """The oracle's evaluation of the ring, computed once per process and shared by the tests that need it."""
    if not _RING:
        g, truth, false_slots = ring()
        n_edges = len(g.ei)
        rounds, est = evaluate(g, 0.01)
        _RING.update(g=g, truth=truth, false_slots=false_slots, rounds=rounds, est=est, n_edges=n_edges)
    return _RING


def planted(n, good, bad, seed=11):
    """n vertices at ground-truth poses; `good` edges measure the truth exactly (chi2 of the order of rounding), a `bad`
    edge (i, j, d) measures it with d metres added along x: information 100 I, so chi2 = 100 d^2 to rounding.  Edges go in
    as listed: the good ones, then the bad ones."""
    rng = np.random.default_rng(seed)
    truth = [po.pose(rng) for _ in range(n)]
    g = EvalGraph(n)
    for v in range(n):
        g.set_estimate(v, truth[v])
    g.fixed[0] = True
    for i, j in good:
        g.add_edge(i, j, po.inv(truth[i]) @ truth[j], np.eye(6) * 100.0)
    for i, j, d in bad:
        off = np.eye(4)
        off[0, 3] = d
        g.add_edge(i, j, po.inv(truth[i]) @ truth[j] @ off, np.eye(6) * 100.0)
    return g


CHAIN4 = [(0, 1), (1, 2), (2, 3)]
# name, vertices, good edges, bad edges, then per prune call (threshold, count, the verdicts of the bad edges in order): written
# out by hand from graph_manager.cpp:1106-1246; every good edge is KEPT in every call
VERDICT_CASES = [
    ("removed", 4, CHAIN4, [(0, 3, 1.0)], [(5.0, 1, [REMOVED])]),
    ("discounted through a vertex of degree 1", 5, CHAIN4, [(1, 4, 1.0)], [(5.0, 1, [DISCOUNTED])]),
    ("zero motion, id1 < id2", 4, CHAIN4[:1] + CHAIN4[2:], [(1, 2, 1.0)], [(5.0, 1, [ZERO_MOTION])]),
    ("zero motion, id1 > id2", 4, CHAIN4[:1] + CHAIN4[2:], [(2, 1, 1.0)], [(5.0, 1, [ZERO_MOTION])]),
    ("both edges of a degree-2 vertex", 5, CHAIN4, [(0, 4, 1.0), (2, 4, 1.0)], [(5.0, 2, [REMOVED, REMOVED])]),
    # the vertex 4 has degree 2; after the first call one of its edges is inactive and still counts: the second is REMOVED,
    # not DISCOUNTED, and the first, whose chi2 is still 100, is skipped (KEPT, not counted)
    ("a removed edge counts in the degree; inactive edges are skipped", 5, CHAIN4, [(0, 4, 1.0), (2, 4, 0.15)],
     [(5.0, 1, [REMOVED, KEPT]), (1.0, 1, [KEPT, REMOVED]), (0.25, 0, [KEPT, KEPT])]),
    ("below every threshold", 4, CHAIN4, [(0, 3, 0.01)], [(5.0, 0, [KEPT]), (0.25, 0, [KEPT])]),
]


def verdict_case(name):
    _, n, good, bad, calls = next(c for c in VERDICT_CASES if c[0] == name)
    return planted(n, good, bad), len(good), calls


def threshold_graph(s):
    """Two vertices at the identity, Z = translation (1, 0, 0), O = s I: chi2 = s exactly."""
    g = EvalGraph(2)
    g.fixed[0] = True
    Z = np.eye(4)
    Z[0, 3] = 1.0
    g.add_edge(0, 1, Z, np.eye(6) * s)
    return g


SLOTS_129 = (0, 63, 64, 128)


def slots_graph_129():
    """65 vertices, 129 edges, of which those at slots 0, 63, 64 and 128 (the ends of the tree's first two leaves and the
    one value of its third) are loop edges 3 m off: a prune call at 5 removes exactly these."""
    chain = [e for e in po.chain_edges(65, 2) if e not in ((10, 12), (20, 22))]
    assert len(chain) == 125
    rng = np.random.default_rng(17)
    truth = [po.pose(rng) for _ in range(65)]
    loops = iter([(3, 40), (7, 22), (30, 9), (50, 12)])
    g = EvalGraph(65)
    g.fixed[0] = True
    for v in range(65):
        g.set_estimate(v, truth[v] @ po.pose(rng, 0.01, 0.005) if v else truth[v])
    k = 0
    for slot in range(129):
        if slot in SLOTS_129:
            i, j = next(loops)
            off = np.eye(4)
            off[1, 3] = 3.0
            g.add_edge(i, j, po.inv(truth[i]) @ truth[j] @ off, np.eye(6) * 100.0)
        else:
            i, j = chain[k]
            k += 1
            g.add_edge(i, j, po.inv(truth[i]) @ truth[j] @ po.pose(rng, 0.002, 0.002), np.eye(6) * 100.0)
    return g


SLOTS_4161 = (5, 4101)   # leaves 0 and 64: both go into accumulator 0 of the tree's second level


def slots_graph_4161():
    """The 4161-edge graph of tests/test_gpu_pose_graph.py (5 vertices, 66 leaves) with the edges at slots 5 and 4101 replaced
    by (0, 3) edges 5 m off: a prune call at 500 removes exactly these."""
    rng = np.random.default_rng(21)
    pairs = [(int(a), int(b)) for a, b in (rng.choice(5, 2, replace=False) for _ in range(4161))]
    g = from_graph(po.make_graph(5, pairs, 21))
    for e in SLOTS_4161:
        g.ei[e], g.ej[e] = 0, 3
        g.Zt[e] = g.Zt[e] + np.array([5.0, 0.0, 0.0])
    return g
