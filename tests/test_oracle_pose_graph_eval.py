"""CPU: tests/pose_graph_eval_oracle.py held against expectations written out by hand from the reference
(graph_manager.cpp:444, :889-896, :911-937, :1031-1036 for the flags; :1106-1246 for the prune verdicts; :1347-1360 for
sanityCheck), tools/evaluate_ate.py against planted trajectories, and the library's host-side entry points (strategies,
sanity_check, get_edge, write_trajectory: no device work) against the oracle.  The device is tests/test_gpu_pose_graph_eval.py;
the prune kernel's source on the CPU is tests/test_emu_pose_graph_prune.py."""
import importlib.util
import math
import os

import numpy as np
import pytest

import pose_graph_eval_oracle as pe
import pose_graph_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("evaluate_ate", os.path.join(ROOT, "tools", "evaluate_ate.py"))
ate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ate)

ID0 = 3   # the library's node id of the oracle's node 0: ids are shifted, their differences kept


# ---- the flags of a 6-node online sequence: node v joins v - 1 and v - 2; node 4 also closes a loop to node 1 --------------------
def frame_edges(v):
    return [(u, v) for u in (v - 1, v - 2) if u >= 0] + ([(1, 4)] if v == 4 else [])


F, T = False, True
# per frame 1 .. 5: the flags after the edges went in, after fixationOfVertices, after the optimisation
FLAGS = {
    "none": [([T, F], [T, F], [T, F]), ([T, F, F],) * 3, ([T, F, F, F],) * 3, ([T, F, F, F, F],) * 3, ([T, F, F, F, F, F],) * 3],
    "first": [([F] * n, [T] + [F] * (n - 1), [F] * n) for n in range(2, 7)],
    # graph[size - 2]; with two nodes the flags stay as they are
    "previous": [([F, F], [F, F], [F, F]), ([F] * 3, [F, T, F], [F] * 3), ([F] * 4, [F, F, T, F], [F] * 4),
                 ([F] * 5, [F, F, F, T, F], [F] * 5), ([F] * 6, [F, F, F, F, T, F], [F] * 6)],
    # earliest = the new node's id, then the minimum over its edges' ids: 0, 0, 1, 1 (the loop edge), 3
    "largest_loop": [([F] * 2, [F] * 2, [F] * 2), ([F] * 3, [F] * 3, [F] * 3), ([F] * 4, [T, F, F, F], [F] * 4),
                     ([F] * 5, [T, F, F, F, F], [F] * 5), ([F] * 6, [T, T, T, F, F, F], [F] * 6)],
    # every flag set after an optimisation; an edge clears its two vertices; fixationOfVertices does nothing
    "inaffected": [([F, F], [F, F], [T, T]), ([F, F, F], [F, F, F], [T] * 3), ([T, F, F, F], [T, F, F, F], [T] * 4),
                   ([T, F, F, F, F], [T, F, F, F, F], [T] * 5), ([T, T, T, F, F, F], [T, T, T, F, F, F], [T] * 6)],
}


@pytest.mark.parametrize("strategy", list(FLAGS))
def test_the_flags_of_an_online_sequence(strategy):
    g = pe.EvalGraph(0)
    g.strategy = pe.STRATEGIES[strategy]
    g.add_node()
    if strategy == "none":
        g.fixed[0] = True   # the caller's flag: it must stay
    for v in range(1, 6):
        g.add_node()
        for i, j in frame_edges(v):
            g.add_edge(i, j, np.eye(4), np.eye(6))
        after_edges = list(g.fixed)
        pe.apply_fixation(g)
        during = list(g.fixed)
        pe.release_fixation(g)
        assert (after_edges, during, list(g.fixed)) == FLAGS[strategy][v - 1], v


@pytest.mark.parametrize("strategy", list(FLAGS))
def test_the_librarys_flags_are_the_oracles(strategy):
    """Host code: the flags after add_edge_se3 and after optimize_graph.  Without a measured edge no device is touched, so
    the frames here carry topology only where the device would be needed; the flags in between are the GPU test's."""
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg = PoseGraph()
    pg.set_strategy(strategy)
    g = pe.EvalGraph(0)
    g.strategy = pe.STRATEGIES[strategy]
    for v in range(6):
        g.add_node()
        pg.add_node(ID0 + v)
        if strategy == "none" and v == 0:
            g.fixed[0] = True
            pg.set_fixed(ID0, True)
        for i, j in frame_edges(v):
            g.add_edge(i, j, np.eye(4), np.eye(6))
            pg.add_edge_se3(ID0 + i, ID0 + j, np.eye(4), np.eye(6))
        assert [pg.get_fixed(ID0 + u) for u in range(v + 1)] == list(g.fixed), v
    pg.close()


# ---- prune verdicts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in pe.VERDICT_CASES])
def test_every_prune_verdict_at_a_planted_edge(name):
    g, n_good, calls = pe.verdict_case(name)
    n_bad = len(g.ei) - n_good
    for thresh, count, want in calls:
        before = [g.edge(e) for e in range(len(g.ei))]
        got, verdicts = pe.prune_edges(g, thresh)
        assert got == count and list(verdicts[n_good:]) == want and not verdicts[:n_good].any()
        for e in range(len(g.ei)):
            now, v = g.edge(e), verdicts[e]
            if v == pe.KEPT:
                assert now["active"] == before[e]["active"] and (now["transform"] == before[e]["transform"]).all()
                assert (now["information"] == before[e]["information"]).all()
                continue
            assert (now["transform"] == np.eye(4)).all()
            assert now["active"] == (v != pe.REMOVED)
            want_info = {pe.REMOVED: before[e]["information"], pe.DISCOUNTED: np.eye(6) * 1e-100, pe.ZERO_MOTION: np.eye(6)}[v]
            assert (now["information"] == want_info).all()
    assert n_bad == len(calls[0][2])


def test_verdicts_do_not_depend_on_the_edge_order():
    g, n_good, calls = pe.verdict_case("both edges of a degree-2 vertex")
    h = pe.from_graph(g)
    order = list(range(len(g.ei)))[::-1]
    for name in ("ei", "ej", "ZR", "Zt", "Om"):
        setattr(h, name, [getattr(g, name)[e] for e in order])
    a = pe.prune_edges(g, 5.0)
    b = pe.prune_edges(h, 5.0)
    assert a[0] == b[0] == 2 and list(a[1]) == list(b[1][::-1])


def test_a_pruned_vertex_can_end_up_without_an_active_edge():
    """Both edges of a degree-2 vertex go in one call: the reference's comment ("without making vertices disconnected")
    does not hold, and the optimiser must live with a vertex that no active edge touches."""
    g, _, _ = pe.verdict_case("both edges of a degree-2 vertex")
    pe.prune_edges(g, 5.0)
    assert not any(g.active[e] and 4 in (g.ei[e], g.ej[e]) for e in range(len(g.ei)))
    before = g.estimate(4).copy()
    rep = po.new_report()
    pe.optimize_graph(g, 3.0, rep)
    assert np.isfinite(rep["chi2"]) and (g.estimate(4) == before).all()


@pytest.mark.parametrize("s", [5.0, 1.0, 0.25])
def test_the_threshold_is_strict(s):
    g = pe.threshold_graph(s)
    assert pe.edge_errors(g)["chi2"][0] == s and pe.prune_edges(g, s) == (0, [pe.KEPT])
    up = pe.threshold_graph(np.nextafter(s, 10.0))
    assert pe.prune_edges(up, s)[0] == 1 and up.active == [True] and (up.Om[0] == np.eye(6)).all()   # ids 0, 1: zero motion


def test_a_nan_error_is_kept():
    g = pe.threshold_graph(1.0)
    g.t[1, 0] = np.nan
    with np.errstate(all="ignore"):
        assert pe.prune_edges(g, 0.25)[0] == 0


def test_inactive_slots_contribute_exactly_nothing():
    """chi2, H and b of a graph with removed slots are those of the graph without these edges, except for the tree's shape."""
    g = pe.slots_graph_129()
    assert pe.prune_edges(g, 5.0)[0] == 4 and [e for e in range(129) if not g.active[e]] == list(pe.SLOTS_129)
    lin = pe.linearize(g)
    view, idx = pe.active_view(g)
    ref = po.linearize(view)
    assert len(lin["rho"]) == 129 and not lin["rho"][list(pe.SLOTS_129)].any() and not lin["w"][list(pe.SLOTS_129)].any()
    assert lin["Hd"].tobytes() == ref["Hd"].tobytes() and lin["B"].tobytes() == ref["B"].tobytes()
    assert abs(lin["chi2"] - ref["chi2"]) <= 1e-12 * ref["chi2"]
    g2 = pe.slots_graph_4161()
    assert pe.prune_edges(g2, 500.0)[0] == 2 and [e for e in range(4161) if not g2.active[e]] == list(pe.SLOTS_4161)
    assert {e // po.TILE % po.TILE for e in pe.SLOTS_4161} == {0} and len({e // po.TILE for e in pe.SLOTS_4161}) == 2


def test_the_ungated_path_is_the_old_oracle():
    """With every edge active the gated restatement gives pose_graph_oracle's bytes."""
    name = "general information"
    a, b = dict(po.planted_graphs())[name](), pe.from_graph(dict(po.planted_graphs())[name]())
    ra, rb = po.new_report(), po.new_report()
    po.optimize_graph(a, 0.01, ra)
    pe.optimize_graph(b, 0.01, rb)
    assert a.R.tobytes() == b.R.tobytes() and a.t.tobytes() == b.t.tobytes() and repr(ra) == repr(rb)


# ---- sanityCheck ---------------------------------------------------------------------------------------------------------------
def sanity_graph():
    """Three edges: translations whose squared norm lies between the double square and the FLOAT square of 0.1f, well
    above both, and well below both."""
    t32 = np.float32(0.1)
    float_sq, double_sq = float(np.float32(t32 * t32)), float(t32) * float(t32)
    between = math.sqrt(0.0100000005)
    assert double_sq < between * between < float_sq
    g = pe.EvalGraph(4)
    for k, tx in enumerate([between, 0.2, 0.05]):
        Z = np.eye(4)
        Z[0, 3] = tx
        g.add_edge(k, k + 1, Z, np.eye(6) * 7.0)
    return g


def test_sanity_check_squares_in_float():
    g = sanity_graph()
    assert pe.sanity_check(g, 0.1) == 1
    assert (g.Om[0] == np.eye(6) * 7.0).all() and (g.Om[1] == np.eye(6) * 0.000001).all() and (g.Om[2] == np.eye(6) * 7.0).all()


def library_graph(g, strategy=None):
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg = PoseGraph()
    if strategy is not None:
        pg.set_strategy(strategy)
    for v in range(g.n):
        pg.add_node(ID0 + v)
        pg.set_estimate(ID0 + v, g.estimate(v))
        pg.set_fixed(ID0 + v, bool(g.fixed[v]))
    for e in range(len(g.ei)):
        ed = g.edge(e)
        pg.add_edge_se3(ID0 + ed["id1"], ID0 + ed["id2"], ed["transform"], ed["information"])
    return pg


def same_edges(pg, g):
    for e in range(len(g.ei)):
        a, b = pg.edge(e), g.edge(e)
        assert (a["id1"], a["id2"], a["active"]) == (ID0 + b["id1"], ID0 + b["id2"], b["active"]), e
        assert a["transform"].tobytes() == b["transform"].tobytes() and a["information"].tobytes() == b["information"].tobytes(), e


def test_the_librarys_sanity_check_is_the_oracles():
    g = sanity_graph()
    pg = library_graph(g)
    same_edges(pg, g)
    assert pg.sanity_check(0.1) == pe.sanity_check(g, 0.1) == 1
    same_edges(pg, g)
    assert pg._L.rgbdfe_pose_graph_sanity_check(None, 0.1) == -1 and pg._L.rgbdfe_pose_graph_sanity_check(pg._g, float("nan")) == -1
    assert pg._L.rgbdfe_pose_graph_get_edge(pg._g, 3, None, None, None, None, None) == -1
    assert pg._L.rgbdfe_pose_graph_set_strategy(pg._g, 5) == -1 and pg._L.rgbdfe_pose_graph_set_strategy(None, 1) == -1
    pg.close()


# ---- the trajectory file --------------------------------------------------------------------------------------------------------
def trajectory_graph():
    """Six poses: a small rotation (trace > 0) and rotations of about 170 degrees about x, y and z (the other three
    branches of the conversion), a negative-w candidate and the identity."""
    g = pe.EvalGraph(6)
    for v, (axis, ang) in enumerate([(0, 0.1), (0, 2.97), (1, 2.97), (2, 2.97), (2, -1.2), (0, 0.0)]):
        P = np.eye(4)
        P[:3, :3] = po.rot_axis(axis, ang)
        P[:3, 3] = [0.1 * v - 0.25, -1.5 + v, 1000.123456789 * (v % 2)]
        g.set_estimate(v, P)
    return g


TRAJECTORY_VARIANTS = [dict(), dict(frame_id="/openni_camera", child_frame_id="/openni_rgb_optical_frame"),
                       dict(base2points="b2p"), dict(base2points="b2p", init_base_pose="init", frame_id="world", child_frame_id=None)]


def trajectory_arguments(variant):
    rng = np.random.default_rng(9)
    mats = dict(b2p=po.pose(rng, 0.3, 0.8), init=po.pose(rng, 2.0, 1.0))
    return {k: (mats[v] if v in ("b2p", "init") else v) for k, v in variant.items()}


def test_the_trajectory_takes_every_quaternion_branch():
    g = trajectory_graph()
    text, branches = pe.trajectory_text(g, range(6), [0.5 * v for v in range(6)])
    assert sorted(set(branches)) == [0, 1, 2, 3]
    rows = np.array([[float(x) for x in line.split()] for line in text.splitlines()])
    assert rows.shape == (6, 8) and (rows[:, 7] >= 0).all() and np.allclose(np.linalg.norm(rows[:, 4:], axis=1), 1, atol=2e-6)
    assert text.splitlines()[1].startswith("0.500000 -0.150000 -0.500000 1000.123457 ")


@pytest.mark.parametrize("variant", range(len(TRAJECTORY_VARIANTS)))
def test_the_librarys_trajectory_file_is_the_oracles(variant, tmp_path):
    g = trajectory_graph()
    kw = trajectory_arguments(TRAJECTORY_VARIANTS[variant])
    nodes, stamps = [4, 0, 1, 2, 3, 5], [1311868164.363181 + 0.033 * k for k in range(6)]
    want, _ = pe.trajectory_text(g, nodes, stamps, **kw)
    pg = library_graph(g)
    path = tmp_path / "estimate.txt"
    pg.write_trajectory(path, [ID0 + v for v in nodes], stamps, **kw)
    assert path.read_bytes() == want.encode()
    # errors: nothing is written
    ids = np.array([ID0, ID0 + 9], np.int32); ts = np.zeros(2)
    other = tmp_path / "other.txt"
    L = pg._L
    assert L.rgbdfe_pose_graph_write_trajectory(pg._g, str(other).encode(), 2, ids.ctypes.data, ts.ctypes.data, None, None, None, None) == -4
    assert not other.exists()
    assert L.rgbdfe_pose_graph_write_trajectory(pg._g, str(tmp_path / "no" / "dir.txt").encode(), 1, ids.ctypes.data, ts.ctypes.data,
                                                None, None, None, None) == -1
    assert L.rgbdfe_pose_graph_write_trajectory(None, str(other).encode(), 0, None, None, None, None, None, None) == -1
    pg.close()


# ---- evaluate_ate ---------------------------------------------------------------------------------------------------------------
def write_tum(path, stamps, positions):
    with open(path, "w") as f:
        f.write("# stamp tx ty tz qx qy qz qw\n")
        for s, p in zip(stamps, positions):
            f.write("%.6f %.17g %.17g %.17g 0 0 0 1\n" % (s, p[0], p[1], p[2]))


def test_ate_of_a_rigidly_moved_copy_is_zero(tmp_path):
    rng = np.random.default_rng(4)
    gt = rng.normal(size=(40, 3)) * 2.0
    M = po.pose(rng, 3.0, 1.2)
    moved = gt @ M[:3, :3].T + M[:3, 3]
    stamps = 100.0 + 0.1 * np.arange(40)
    write_tum(tmp_path / "gt.txt", stamps, gt)
    write_tum(tmp_path / "est.txt", stamps + 0.004, moved)
    out = ate.ate(ate.read_trajectory(tmp_path / "gt.txt"), ate.read_trajectory(tmp_path / "est.txt"))
    assert out["pairs"] == 40 and out["rmse"] < 1e-12 and out["max"] < 1e-12


def test_ate_of_planted_offsets_and_the_association_bound(tmp_path):
    """The corners of a cube, each pushed outwards by s * c * corner with c equal at opposite corners: the offsets have no
    mean and no moment and the cross-covariance stays symmetric positive definite, so the best rigid alignment is the
    identity and the errors are the offsets' lengths: RMSE = s sqrt(3) sqrt(mean c^2)."""
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    c = np.array([1, 2, 3, 4, 4, 3, 2, 1], np.float64)   # corner k and its opposite 7 - k
    s = 0.01
    rng = np.random.default_rng(8)
    M = po.pose(rng, 1.0, 0.9)
    est = (corners * (1.0 + s * c[:, None])) @ M[:3, :3].T + M[:3, 3]
    stamps = 5.0 + np.arange(8)
    write_tum(tmp_path / "gt.txt", stamps, corners)
    write_tum(tmp_path / "est.txt", stamps, est)
    out = ate.ate(ate.read_trajectory(tmp_path / "gt.txt"), ate.read_trajectory(tmp_path / "est.txt"))
    lengths = s * c * math.sqrt(3.0)
    assert out["pairs"] == 8 and abs(out["rmse"] - math.sqrt(np.mean(lengths ** 2))) < 1e-12
    assert abs(out["mean"] - lengths.mean()) < 1e-12 and abs(out["median"] - np.median(lengths)) < 1e-12
    assert abs(out["std"] - lengths.std()) < 1e-12 and abs(out["min"] - lengths.min()) < 1e-12 and abs(out["max"] - lengths.max()) < 1e-12
    # a stamp 0.021 s off is not associated, one 0.019 s off is
    off = stamps.copy()
    off[3] += 0.021
    off[5] += 0.019
    write_tum(tmp_path / "est2.txt", off, est)
    pairs = ate.associate(ate.read_trajectory(tmp_path / "gt.txt"), ate.read_trajectory(tmp_path / "est2.txt"))
    assert len(pairs) == 7 and all(abs(a - stamps[3]) > 0.5 for a, _ in pairs) and any(abs(b - off[5]) < 1e-9 for _, b in pairs)


# ---- the evaluation rounds on the ring ---------------------------------------------------------------------------------------------
ring_run = pe.ring_run


def ring_ate(est, truth):
    return ate.statistics(ate.align(est[:, :3, 3].T, truth[:, :3, 3].T)[2])["rmse"]


def test_the_ring_seed_does_what_it_was_chosen_for():
    """In the oracle alone: every planted false edge ends REMOVED, no true edge is touched, and the ATE after round 4 is below
    the ATE after round 1."""
    r = ring_run()
    g = r["g"]
    final = np.zeros(r["n_edges"], np.uint8)
    for rd in r["rounds"][2:]:
        final[rd["verdicts"] != pe.KEPT] = rd["verdicts"][rd["verdicts"] != pe.KEPT]
    assert len(r["false_slots"]) == 4
    assert [e for e in range(r["n_edges"]) if final[e] != pe.KEPT] == r["false_slots"]
    assert all(final[e] == pe.REMOVED and not g.active[e] for e in r["false_slots"])
    assert [rd["pruned"] for rd in r["rounds"]] == [0, 0, 4, 0, 0]   # both arms of the rounds' branch are taken
    a1, a4 = ring_ate(r["est"][1], r["truth"]), ring_ate(r["est"][4], r["truth"])
    print("ATE after round 1: %.4f m, after round 4: %.4f m" % (a1, a4))
    assert a4 < a1
    assert g.strategy == pe.FIRST and not g.fixed.any()
