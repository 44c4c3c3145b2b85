"""-m gpu: the pose graph's last stage (include/rgbdfe.h, "fixation strategies, pruning and the evaluation rounds";
csrc/pose_graph.hip pg_prune_kernel, csrc/api_pose_graph.hip) through the C ABI against the literal restatement in
tests/pose_graph_eval_oracle.py.  Every comparison is on bytes: per-edge figures, verdicts and patched edges, chi2 /
linearize / optimize over inactive slots, the flags and estimates of an online loop under each strategy, the five evaluation
rounds, the trajectory file.  tests/test_oracle_pose_graph_eval.py holds the oracle against expectations written by hand."""
import ctypes as C
import importlib.util
import os
import struct

import numpy as np
import pytest

import pose_graph_eval_oracle as pe
import pose_graph_oracle as po

pytestmark = pytest.mark.gpu

INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
ID0 = 3   # the library's node id of the oracle's node 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("evaluate_ate", os.path.join(ROOT, "tools", "evaluate_ate.py"))
ate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ate)


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=512, max_pairs_per_batch=64)
    yield f
    f.close()


def library_graph(g):
    """The library's copy of an oracle graph as it stands (every edge still active)."""
    from rgbdslam_v2_amd.candidates import PoseGraph
    assert all(g.active)
    pg = PoseGraph()
    for v in range(g.n):
        pg.add_node(ID0 + v)
        pg.set_estimate(ID0 + v, g.estimate(v))
        pg.set_fixed(ID0 + v, bool(g.fixed[v]))
    for e in range(len(g.ei)):
        ed = g.edge(e)
        pg.add_edge_se3(ID0 + ed["id1"], ID0 + ed["id2"], ed["transform"], ed["information"])
    pg.set_strategy(g.strategy)
    return pg


def bits(v):
    return struct.pack("<d", float(v))


def same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def check_report(got, want):
    assert got["iterations"] == want["iterations"]
    assert bits(got["chi2"]) == bits(want["chi2"]), (got["chi2"], float(want["chi2"]))
    assert len(got["its"]) == len(want["its"])
    for k, (a, b) in enumerate(zip(got["its"], want["its"])):
        assert a["trials"] == b["trials"] and a["pcg"] == [int(v) for v in b["pcg"]], (k, a, b)
        for f in ("chi2_before", "chi2_after", "lam"):
            assert bits(a[f]) == bits(b[f]), (k, f, a[f], float(b[f]))


def check_estimates(pg, g):
    for v in range(g.n):
        assert same(pg.get_estimate(ID0 + v), g.estimate(v)), v


def check_flags(pg, g):
    assert [pg.get_fixed(ID0 + v) for v in range(g.n)] == [bool(f) for f in g.fixed]


def check_edges(pg, g):
    for e in range(len(g.ei)):
        a, b = pg.edge(e), g.edge(e)
        assert (a["id1"], a["id2"], a["active"]) == (ID0 + b["id1"], ID0 + b["id2"], b["active"]), e
        assert same(a["transform"], b["transform"]) and same(a["information"], b["information"]), e


def check_edge_errors(fe, pg, g):
    got, want = pg.edge_errors(fe), pe.edge_errors(g)
    assert same(got["chi2"], want["chi2"]) and same(got["err_sq"], want["err_sq"]) and list(got["active"]) == list(want["active"])


def prune_both(fe, pg, g, thresh):
    got_n, got_v = pg.prune_edges(fe, thresh)
    want_n, want_v = pe.prune_edges(g, thresh)
    assert got_n == want_n and got_v.tobytes() == want_v.tobytes()
    check_edges(pg, g)
    return got_n, got_v


@pytest.mark.parametrize("s", [5.0, 1.0, 0.25])
def test_thresholds(fe, s):
    """chi2 = s exactly: kept at the threshold s, pruned at the next double above it."""
    g = pe.threshold_graph(s)
    pg = library_graph(g)
    assert pg.edge_errors(fe)["chi2"][0] == s and pg.edge_errors(fe)["err_sq"][0] == 1.0
    assert prune_both(fe, pg, g, s)[0] == 0
    pg.close()
    g = pe.threshold_graph(np.nextafter(s, 10.0))
    pg = library_graph(g)
    n, v = prune_both(fe, pg, g, s)
    assert n == 1 and list(v) == [pe.ZERO_MOTION]
    pg.close()


@pytest.mark.parametrize("name", [c[0] for c in pe.VERDICT_CASES])
def test_verdicts(fe, name):
    """Every verdict at a planted edge, the expectation written out by hand in the oracle module's table (and asserted on the
    oracle by tests/test_oracle_pose_graph_eval.py): REMOVED, DISCOUNTED through a vertex of degree 1, ZERO_MOTION in both id
    orders, both edges of a degree-2 vertex in one call, a removed edge still counted in the degree, inactive edges skipped."""
    g, n_good, calls = pe.verdict_case(name)
    pg = library_graph(g)
    check_edge_errors(fe, pg, g)
    for thresh, count, want in calls:
        n, v = prune_both(fe, pg, g, thresh)
        assert n == count and list(v[n_good:]) == want and not v[:n_good].any()
        check_edge_errors(fe, pg, g)
        assert bits(pg.chi2(fe)) == bits(pe.chi2(g))
    rep = po.new_report()
    pe.optimize_graph(g, 3.0, rep)   # a vertex may have lost every active edge
    check_report(pg.optimize_graph(fe, 3.0), rep)
    check_estimates(pg, g)
    pg.close()


def check_linearize(fe, pg, g):
    lin = pe.linearize(g)
    got = pg.linearize(fe)
    plan = lin["plan"]
    assert same(got["e"], lin["e"]) and same(got["w"], lin["w"])
    assert [int(i) for i in got["free_ids"]] == [ID0 + int(v) for v in plan.verts]
    assert [(int(r), int(c)) for r, c in zip(got["rows"], got["cols"])] == [(int(r), int(c)) for r, c in plan.blocks]
    assert same(got["Hd"], lin["Hd"]) and same(got["b"], lin["b"]) and same(got["B"], lin["B"])
    assert bits(got["chi2"]) == bits(lin["chi2"]) and bits(pg.chi2(fe)) == bits(lin["chi2"])


def test_inactive_slots_in_the_sums_129(fe):
    """129 edges, those at slots 0, 63, 64 and 128 removed: chi2, linearize and optimize(3)."""
    g = pe.slots_graph_129()
    pg = library_graph(g)
    assert prune_both(fe, pg, g, 5.0)[0] == 4 and [e for e in range(129) if not g.active[e]] == list(pe.SLOTS_129)
    check_linearize(fe, pg, g)
    want = po.new_report()
    pe.optimize(g, 3, want)
    check_report(pg.optimize(fe, 3), want)
    check_estimates(pg, g)
    pg.close()


def test_inactive_slots_in_two_leaves_of_one_accumulator(fe):
    """4161 edges = 66 leaves; the removed slots 5 and 4101 lie in leaves 0 and 64, which share accumulator 0."""
    g = pe.slots_graph_4161()
    pg = library_graph(g)
    assert prune_both(fe, pg, g, 500.0)[0] == 2 and [e for e in range(4161) if not g.active[e]] == list(pe.SLOTS_4161)
    check_linearize(fe, pg, g)
    want = po.new_report()
    pe.optimize(g, 2, want)
    check_report(pg.optimize(fe, 2), want)
    check_estimates(pg, g)
    pg.close()


class LibraryOnline:
    """The interface pe.run_online drives, on the library."""

    def __init__(self, fe, strategy):
        from rgbdslam_v2_amd.candidates import PoseGraph
        self.fe, self.pg, self.n = fe, PoseGraph(), 0
        self.pg.set_strategy(strategy)

    def add_node(self):
        self.pg.add_node(ID0 + self.n)
        self.n += 1

    def add_edge(self, i, j, Z, Om, set_estimate=False):
        self.pg.add_edge_se3(ID0 + i, ID0 + j, Z, Om, set_estimate=set_estimate)


@pytest.mark.parametrize("strategy", ["first", "previous", "largest_loop", "inaffected", "none"])
def test_strategies_online(fe, strategy):
    """12 nodes, 3 predecessors each and one loop edge, optimize_graph(0.01) after every node: the flags and the estimates
    after every frame.  NONE (node 0 fixed by the caller) must equal the bytes of the block as it was: po.optimize_graph."""
    frames = pe.online_sequence()
    g = pe.EvalGraph(0)
    g.strategy = pe.STRATEGIES[strategy]
    lib = LibraryOnline(fe, strategy)
    reports = []

    def both_optimise():
        if strategy == "none" and not g.fixed[0]:
            g.fixed[0] = True
            lib.pg.set_fixed(ID0, True)
        want = po.new_report()
        pe.optimize_graph(g, 0.01, want)
        check_report(lib.pg.optimize_graph(fe, 0.01), want)
        reports.append(want)

    def after_frame(v):
        check_flags(lib.pg, g)
        check_estimates(lib.pg, g)

    class Both:
        def add_node(self):
            g.add_node(); lib.add_node()

        def add_edge(self, i, j, Z, Om, set_estimate=False):
            g.add_edge(i, j, Z, Om, set_estimate); lib.add_edge(i, j, Z, Om, set_estimate)

    pe.run_online(Both(), frames, on_frame=after_frame, optimize_with=both_optimise)
    assert len(reports) == 11 and sum(r["iterations"] for r in reports) > 11
    if strategy == "none":   # the same frames through the oracle of the block as it was, the graph rebuilt per frame
        h = po.Graph(12)
        h.fixed[0] = True
        for v, edges in enumerate(frames):
            for k, (i, j, Z, Om) in enumerate(edges):
                h.add_edge(i, j, Z, Om, set_estimate=(k == 0))
            if edges:
                sub = po.Graph(v + 1)
                sub.R, sub.t, sub.fixed = h.R[:v + 1].copy(), h.t[:v + 1].copy(), h.fixed[:v + 1].copy()
                sub.ei, sub.ej, sub.ZR, sub.Zt, sub.Om = h.ei, h.ej, h.ZR, h.Zt, h.Om
                po.optimize_graph(sub, 0.01)
                h.R[:v + 1], h.t[:v + 1] = sub.R, sub.t
        for v in range(12):
            assert same(lib.pg.get_estimate(ID0 + v), h.estimate(v)), v
    lib.pg.close()


def ring_library_graph():
    g, truth, false_slots = pe.ring()
    return library_graph(g), g


def test_evaluate_on_the_ring(fe):
    """The five rounds on the ring of 64 nodes with planted false loop edges: out, estimates and edges against the oracle; the
    same rounds issued as single calls give the same bytes."""
    want = pe.ring_run()
    pg, start = ring_library_graph()
    rounds, est = pg.evaluate(fe, 0.01)
    assert est.shape == (5, pe.RING_N, 4, 4) and same(est, want["est"])
    for k, (a, b) in enumerate(zip(rounds, want["rounds"])):
        assert (a["iterations"], a["pruned"]) == (b["iterations"], b["pruned"]) and bits(a["chi2"]) == bits(b["chi2"]), k
        assert a["launches"] > 0 and a["readbacks"] > 0
    check_edges(pg, want["g"])
    check_flags(pg, want["g"])
    assert [e for e in range(want["n_edges"]) if not pg.edge(e)["active"]] == want["false_slots"]
    # as single calls
    single, _ = ring_library_graph()
    reps = [single.optimize_graph(fe, 0.01)]
    single.set_strategy("first")
    reps.append(single.optimize_graph(fe, 0.01))
    for thresh in (5.0, 1.0, 0.25):
        n, _ = single.prune_edges(fe, thresh)
        reps.append(single.optimize_graph(fe, 0.01 if n > 0 else 1.0))
        reps[-1]["pruned"] = n
    for k, (a, b) in enumerate(zip(rounds, reps)):
        assert a["iterations"] == b["iterations"] and bits(a["chi2"]) == bits(b["chi2"]) and a["pruned"] == b.get("pruned", 0), k
    for v in range(pe.RING_N):
        assert same(single.get_estimate(ID0 + v), est[4, v]), v
    for e in range(want["n_edges"]):
        a, b = single.edge(e), pg.edge(e)
        assert a["active"] == b["active"] and same(a["transform"], b["transform"]) and same(a["information"], b["information"])
    pg.close()
    single.close()


def test_argument_errors_change_nothing(fe):
    g, _, _ = pe.verdict_case("removed")
    pg = library_graph(g)
    L, h, ctx = pg._L, pg._g, fe._ctx
    n = C.c_int32(-1)
    verdicts = np.full(8, 9, np.uint8)
    from rgbdslam_v2_amd import _lib
    ev = _lib.PoseGraphEvaluation()
    est = np.full(5 * 4 * 16, 9.0)
    assert L.rgbdfe_pose_graph_set_strategy(h, 5) == INVALID_ARG and L.rgbdfe_pose_graph_set_strategy(h, -1) == INVALID_ARG
    assert L.rgbdfe_pose_graph_prune_edges(ctx, h, 5.0, verdicts.ctypes.data, 3, C.byref(n)) == CAPACITY and n.value == 4
    assert (verdicts == 9).all()
    assert L.rgbdfe_pose_graph_prune_edges(ctx, None, 5.0, verdicts.ctypes.data, 8, C.byref(n)) == INVALID_ARG
    assert L.rgbdfe_pose_graph_prune_edges(None, h, 5.0, verdicts.ctypes.data, 8, C.byref(n)) == INVALID_ARG
    assert L.rgbdfe_pose_graph_edge_errors(ctx, h, None, None, None, 3, C.byref(n)) == CAPACITY and n.value == 4
    assert L.rgbdfe_pose_graph_edge_errors(ctx, None, None, None, None, 8, C.byref(n)) == INVALID_ARG
    assert L.rgbdfe_pose_graph_evaluate(ctx, None, 0.01, None, None, 0) == INVALID_ARG
    assert L.rgbdfe_pose_graph_evaluate(ctx, h, float("nan"), None, None, 0) == INVALID_ARG
    assert L.rgbdfe_pose_graph_evaluate(ctx, h, 0.01, C.byref(ev), est.ctypes.data, 3) == CAPACITY and (est == 9.0).all()
    ids = np.array([ID0], np.int32); ts = np.zeros(1)
    assert L.rgbdfe_pose_graph_write_trajectory(h, b"/nonexistent-directory/estimate.txt", 1, ids.ctypes.data, ts.ctypes.data, None,
                                                None, None, None) == INVALID_ARG
    check_edges(pg, g)
    check_estimates(pg, g)
    check_flags(pg, g)
    check_edge_errors(fe, pg, g)
    pg.close()


@pytest.mark.parametrize("variant", range(4))
def test_write_trajectory(fe, variant, tmp_path):
    """The file's bytes against the oracle's text with and without base2points / init_base_pose / header, on poses that take
    every quaternion branch -- after an optimisation on the device, so the estimates written are the device's."""
    import test_oracle_pose_graph_eval as cpu
    g = cpu.trajectory_graph()
    g.fixed[0] = True
    for v in range(1, 6):
        g.add_edge(v - 1, v, po.inv(g.estimate(v - 1)) @ g.estimate(v) @ po.pose(np.random.default_rng(v), 0.01, 0.01), np.eye(6) * 50.0)
    pg = library_graph(g)
    want_rep = po.new_report()
    pe.optimize_graph(g, 2.0, want_rep)
    check_report(pg.optimize_graph(fe, 2.0), want_rep)
    kw = cpu.trajectory_arguments(cpu.TRAJECTORY_VARIANTS[variant])
    nodes, stamps = [4, 0, 1, 2, 3, 5], [1311868164.363181 + 0.033 * k for k in range(6)]
    want, branches = pe.trajectory_text(g, nodes, stamps, **kw)
    if "base2points" not in kw:
        assert sorted(set(branches)) == [0, 1, 2, 3]
    path = tmp_path / "estimate.txt"
    pg.write_trajectory(path, [ID0 + v for v in nodes], stamps, **kw)
    assert path.read_bytes() == want.encode()
    pg.close()


def test_nodes_to_edges_to_the_evaluation_to_the_ate(fe, tmp_path):
    """synthetic nodes -> match_node_pairs -> add_edge_se3 -> evaluate -> write_trajectory -> evaluate_ate against synth.py's
    ground-truth poses.  Asserts that the pipeline runs and that the ATE equals the one computed from the oracle's estimates."""
    from rgbdslam_v2_amd import synth
    from rgbdslam_v2_amd.candidates import PoseGraph
    n = 6
    seq = synth.make_sequence(n_frames=n, n_kp=500, n_world=2000, seed=7)
    pg, g = PoseGraph(), pe.EvalGraph(0)
    pg.set_strategy("inaffected")
    g.strategy = pe.INAFFECTED
    n_edges = 0
    for f in range(n):
        fe.upload_node(f, seq["desc"][f], seq["xyz1"][f])
        pg.add_node(f)
        g.add_node()
        placed = False
        for rec in (fe.match_node_pairs(f, list(range(max(0, f - 3), f))[::-1]) if f else []):
            if rec["id1"] < 0 or not rec["info_scale"] > 0:
                continue
            Z = np.array(rec["trafo"], np.float64).reshape(4, 4).T
            first = not placed and int(rec["id2"]) == f
            pg.add_edge_se3(int(rec["id1"]), int(rec["id2"]), Z, float(rec["info_scale"]), set_estimate=first)
            g.add_edge(int(rec["id1"]), int(rec["id2"]), Z, np.eye(6) * float(rec["info_scale"]), set_estimate=first)
            placed = placed or first
            n_edges += 1
    assert n_edges >= n - 1
    want_rounds, want_est = pe.evaluate(g, 0.01)
    rounds, est = pg.evaluate(fe, 0.01)
    assert same(est, want_est)
    assert [(r["iterations"], r["pruned"]) for r in rounds] == [(r["iterations"], r["pruned"]) for r in want_rounds]
    stamps = [10.0 + 0.033 * f for f in range(n)]
    pg.write_trajectory(tmp_path / "estimate.txt", list(range(n)), stamps)
    truth = synth_ground_truth(seq, n)
    with open(tmp_path / "ground_truth.txt", "w") as f:
        for s, p in zip(stamps, truth):
            f.write("%.6f %.9f %.9f %.9f 0 0 0 1\n" % (s, p[0], p[1], p[2]))
    got = ate.ate(ate.read_trajectory(tmp_path / "ground_truth.txt"), ate.read_trajectory(tmp_path / "estimate.txt"))
    text, _ = pe.trajectory_text(g, range(n), stamps)
    (tmp_path / "oracle.txt").write_text(text)
    want = ate.ate(ate.read_trajectory(tmp_path / "ground_truth.txt"), ate.read_trajectory(tmp_path / "oracle.txt"))
    print("ATE", got)
    assert got == want and got["pairs"] == n
    pg.close()


def synth_ground_truth(seq, n):
    """The positions of synth.make_sequence's ground-truth poses."""
    P = np.asarray(seq["poses"], np.float64)
    return [P[f].reshape(4, 4)[:3, 3] for f in range(n)]
