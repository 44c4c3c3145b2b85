"""Scripted runs of the SLAM step's decision machine (include/rgbdfe.h, "the SLAM step"; csrc/slam_machine.h), written out
by hand: per frame the slot, the row count, the stamp, the comparison results by graph id (an id that is not listed gives
no edge) and the step record the contract demands.  tests/test_slam_machine.py drives rgbdfe_slam_begin / _feed of the
library with them, tests/test_slam_machine_host.py the header's machine in a stand-alone program.

Candidate lists below follow rgbdfe_potential_edge_targets (tests/test_candidates.py pins it): while the graph has no more
vertices than targets are asked for, the list is every predecessor of graph_size - 1 downwards, then (without a matched
predecessor) graph_size - 1 itself; no random draw happens in any script here."""
import ctypes as C
import struct

import numpy as np

from rgbdslam_v2_amd import _lib

FRAME_NS = 33333333   # 1 / 30 s

TOO_FEW, FIRST, OUT_OF_BOUNDS, ADDED, NO_MATCH, REPLACED_FIRST = 1, 2, 3, 4, 5, 6
V_NO_EDGE, V_ACCEPTED, V_NOT_SMALL, V_TOO_SHORT, V_WITHDRAWN, V_OUT_OF_BOUNDS, V_ICP = 0, 1, 2, 3, 4, 5, 16
NONE, STRAT_FIRST, LARGEST_LOOP = 0, 1, 3


def trafo(tx=0.0, deg=0.0, diag0=None):
    """Column-major Matrix4f: rotation by `deg` about z, translation tx along x.  diag0 replaces R00 (an acos argument
    above 1: float32 nextafter(1) gives trace = 3 + 2^-23, (trace - 1) / 2 = 1 + 2^-24, the smallest excess a float
    rotation can produce)."""
    a = np.deg2rad(deg)
    T = np.eye(4, dtype=np.float64)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    T[0, 3] = tx
    T = T.astype(np.float32)
    if diag0 is not None:
        T[0, 0] = diag0
    return np.ascontiguousarray(T.T).reshape(16)


def R(tx=0.03, deg=2.0, n_inl=50, info=1.0, flags=0, diag0=None, edge=True):
    return dict(edge=edge, T=trafo(tx, deg, diag0), n_inl=n_inl, info=float(info), flags=flags)


NO_EDGE = dict(edge=False, T=trafo(), n_inl=0, info=0.0, flags=0)
ABOVE_ONE = float(np.nextafter(np.float32(1), np.float32(2)))


def F(slot, rows=100, k=None, t=None, res=None, **expect):
    """Frame `slot` stamped k / 30 s (or t = (sec, nsec)); expect: fields of the step record."""
    if t is None:
        k = slot if k is None else k
        ns = k * FRAME_NS
        t = (ns // 1000000000, ns % 1000000000)
    return dict(slot=slot, rows=rows, t=t, res=res or {}, expect=expect)


# nodes 1, 2, 3 reach keyframe 0; node 4 reaches node 3 alone, which makes 3 a keyframe
LOOP_FRAMES = [F(0, status=FIRST), F(1, res={0: R()}, status=ADDED, keyframe_added=-1),
               F(2, res={0: R(), 1: R()}, status=ADDED, keyframe_added=-1), F(3, res={0: R(), 2: R()}, status=ADDED, keyframe_added=-1),
               F(4, res={3: R()}, status=ADDED, edge_to_keyframe=0, keyframe_added=3)]
SMALL = dict(predecessor_candidates=2, neighbor_candidates=0, min_sampled_candidates=0)   # one predecessor besides the previous node
GAP = 6   # frames: 0.2 s, the constant-position clause |dt_prev| < 0.1 stays off

CASES = [
    dict(name="first node", frames=[
        F(7, status=FIRST, id=0, found=0, n_candidates=0, keyframe_added=-1, optimize_due=0, best_id1=-1)],
        final=dict(keyframes=[0], slots=[7], valid_tf=[1], fixed=[1], edges=[])),
    dict(name="19 rows", params=dict(keep_all_nodes=1), frames=[
        F(0, rows=19, status=TOO_FEW, id=-1),
        F(1, rows=20, status=FIRST, id=0),
        F(2, rows=19, status=TOO_FEW, id=-1, n_candidates=0)],
        final=dict(keyframes=[0], slots=[1], valid_tf=[1], edges=[])),
    dict(name="default thresholds: no initial comparison", frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED, id=1, found=1, initial_id=-1, candidates=[0], verdicts=[V_ACCEPTED],
          best_id1=0, best_id2=1, best_n_inl=50, predecessor_matched=1, edge_to_keyframe=1, keyframe_added=-1,
          constant_position=0, optimize_due=1, sequential_edges=1, loop_closure_edges=0, motion_tx=float(np.float32(0.03)))],
        final=dict(keyframes=[0], slots=[0, 1], valid_tf=[1, 1], fixed=[1, 0], edges=[(0, 1)])),
    dict(name="initial comparison: motion too small", params=dict(min_translation_meter=0.01, min_rotation_degree=1.0), frames=[
        F(0, status=FIRST),
        F(1, res={0: R(tx=0.0, deg=0.0, n_inl=90)}, status=OUT_OF_BOUNDS, id=-1, found=0, initial_id=0,
          initial_verdict=V_OUT_OF_BOUNDS, n_candidates=0, best_id1=0, best_id2=1, best_n_inl=90, has_broadcast_pose=1,
          broadcast_tx=0.0),
        F(2, res={0: R(tx=0.03, deg=0.5)}, status=ADDED, id=1, initial_id=0, initial_verdict=V_ACCEPTED)],
        final=dict(keyframes=[0], slots=[0, 2], valid_tf=[1, 1], edges=[(0, 1), (0, 1)])),
    dict(name="initial comparison: motion too fast", params=dict(min_translation_meter=0.01, max_translation_meter=1.0), frames=[
        F(0, status=FIRST),
        F(1, res={0: R(tx=0.1)}, status=OUT_OF_BOUNDS, id=-1, initial_verdict=V_OUT_OF_BOUNDS, has_broadcast_pose=1,
          broadcast_tx=float(np.float32(0.1))),          # 3 m/s
        F(2, rows=100, k=1, res={0: R(tx=0.03, deg=0.0)}, status=ADDED, id=1)],   # 0.9 m/s
        final=dict(slots=[0, 2])),
    dict(name="initial comparison accepted: the list without the predecessor; set_estimate only on more inliers",
         params=dict(min_translation_meter=0.01, **SMALL), frames=[
        F(0, status=FIRST),
        F(1, res={0: R(tx=0.03, deg=0.0)}, status=ADDED, id=1, initial_id=0, initial_verdict=V_ACCEPTED, candidates=[],
          verdicts=[]),               # the matched predecessor 0 has no predecessor of its own
        F(2, res={1: R(tx=0.03, deg=0.0, n_inl=50), 0: R(tx=0.07, deg=0.0, n_inl=30)}, status=ADDED, id=2, initial_id=1,
          initial_verdict=V_ACCEPTED, candidates=[0], verdicts=[V_ACCEPTED], best_id1=1, best_n_inl=50,
          motion_tx=float(np.float32(0.03)) + float(np.float32(0.03))),          # X1 * Z(1 -> 2) stays
        F(3, res={2: R(tx=0.03, deg=0.0, n_inl=50), 1: R(tx=0.07, deg=0.0, n_inl=60)}, status=ADDED, id=3, candidates=[1],
          verdicts=[V_ACCEPTED], best_id1=1, best_n_inl=60,
          motion_tx=float(np.float32(0.03)) + float(np.float32(0.07)))],         # overwritten with X1 * Z(1 -> 3)
        final=dict(slots=[0, 1, 2, 3])),
    dict(name="an edge that is not big: with a vertex it is accepted", params=dict(min_translation_meter=0.05, **SMALL), frames=[
        F(0, status=FIRST),
        F(1, res={0: R(tx=0.06)}, status=ADDED),
        F(2, res={1: R(tx=0.06), 0: R(tx=0.001, deg=0.0, n_inl=40)}, status=ADDED, id=2, initial_verdict=V_ACCEPTED,
          candidates=[0], verdicts=[V_ACCEPTED])],
        final=dict(edges=[(0, 1), (1, 2), (0, 2)])),
    dict(name="an edge that is not big: without a vertex it is refused", params=dict(min_translation_meter=0.05, **SMALL), frames=[
        F(0, status=FIRST),
        F(1, res={0: R(tx=0.06)}, status=ADDED),
        F(2, k=1 + GAP, res={0: R(tx=0.001, deg=0.0, n_inl=40)}, status=NO_MATCH, id=-1, found=0, initial_id=1,
          initial_verdict=V_NO_EDGE, candidates=[0, 1], verdicts=[V_TOO_SHORT, V_NO_EDGE], constant_position=0)],
        final=dict(slots=[0, 1], edges=[(0, 1)])),
    dict(name="dt <= 0 skips the test for a small transformation", params=dict(max_translation_meter=1.0), frames=[
        F(0, t=(1, 0), status=FIRST),
        F(1, t=(1, FRAME_NS), res={0: R()}, status=ADDED),
        F(2, t=(1, 0), res={0: R(tx=5.0), 1: R(tx=5.0)}, status=ADDED, candidates=[0, 1], verdicts=[V_ACCEPTED, V_ACCEPTED]),   # dt 0 and < 0
        F(3, t=(0, 999999999), res={0: R(tx=5.0), 2: R(tx=5.0)}, status=ADDED, candidates=[1, 0, 2],
          verdicts=[V_NO_EDGE, V_ACCEPTED, V_ACCEPTED]),
        F(4, t=(2, 0), res={0: R(tx=5.0), 3: R(tx=0.5)}, status=ADDED, candidates=[2, 1, 0, 3],       # 5 m/s and 0.5 m/s
          verdicts=[V_NO_EDGE, V_NO_EDGE, V_NOT_SMALL, V_ACCEPTED])]),
    dict(name="an acos argument above 1 is neither big nor small", frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, res={0: R(tx=0.02, deg=0.0, diag0=ABOVE_ONE), 1: R()}, status=ADDED, candidates=[0, 1],
          verdicts=[V_NOT_SMALL, V_ACCEPTED])]),
    dict(name="an acos argument above 1 in the initial comparison", params=dict(min_rotation_degree=1.0), frames=[
        F(0, status=FIRST),
        F(1, res={0: R(tx=0.0, deg=0.0, diag0=ABOVE_ONE)}, status=OUT_OF_BOUNDS, initial_verdict=V_OUT_OF_BOUNDS)]),
    dict(name="keyframe promotion of id - 1 under first", strategy=STRAT_FIRST, params=SMALL, frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED, edge_to_keyframe=1, keyframe_added=-1),
        F(2, res={1: R()}, status=ADDED, candidates=[0, 1], edge_to_keyframe=0, keyframe_added=1),
        F(3, res={1: R(n_inl=30), 2: R()}, status=ADDED, candidates=[1, 2], edge_to_keyframe=1, keyframe_added=-1),
        F(4, res={3: R()}, status=ADDED, candidates=[2, 3], edge_to_keyframe=0, keyframe_added=3)],
        final=dict(keyframes=[0, 1, 3])),
    dict(name="under largest_loop an edge to an old node lowers earliest and holds the promotion back", strategy=LARGEST_LOOP,
         frames=LOOP_FRAMES + [
        # earliest = min(5, 1) is not above the last keyframe 3: no promotion, though no edge reaches a keyframe ...
        F(5, res={4: R(), 1: R(n_inl=30)}, status=ADDED, candidates=[3, 2, 1, 0, 4], edge_to_keyframe=0, keyframe_added=-1)],
        final=dict(keyframes=[0, 3])),
    dict(name="... which under first happens", strategy=STRAT_FIRST, frames=LOOP_FRAMES + [
        F(5, res={4: R(), 1: R(n_inl=30)}, status=ADDED, candidates=[3, 2, 1, 0, 4], edge_to_keyframe=0, keyframe_added=4)],
        final=dict(keyframes=[0, 3, 4])),
    dict(name="clear_non_keyframes with 2 and with 3 keyframes", strategy=STRAT_FIRST, params=dict(clear_non_keyframes=1), frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, res={0: R()}, status=ADDED, predecessor_matched=0, constant_position=1),
        F(3, res={0: R()}, status=ADDED),
        F(4, res={3: R()}, status=ADDED, keyframe_added=3, cleared_first=-1, cleared_last=-1),    # one keyframe before: nothing to clear
        F(5, res={4: R()}, status=ADDED, keyframe_added=4, cleared_first=1, cleared_last=2),      # between 0 and 3
        F(6, res={5: R()}, status=ADDED, keyframe_added=5, cleared_first=-1, cleared_last=-1)],   # between 3 and 4: none
        final=dict(keyframes=[0, 3, 4, 5], slots=[0, -1, -1, 3, 4, 5, 6], valid_tf=[1, 1, 0, 1, 1, 1, 1])),   # node 3 got an edge from node 4, node 2 none
    dict(name="constant position: no transformation and an odometry frame", params=dict(have_odometry_frame=1), frames=[
        F(0, status=FIRST),
        F(1, k=GAP, status=ADDED, id=1, found=1, candidates=[0], verdicts=[V_NO_EDGE], constant_position=1, best_id1=0,
          best_id2=1, best_n_inl=0, predecessor_matched=0, sequential_edges=1, motion_tx=0.0)],
        final=dict(valid_tf=[1, 0], edges=[(0, 1)], info00=[1.0 / float(np.float32(abs(GAP * FRAME_NS * 1e-9)))])),
    dict(name="constant position: no transformation and keep_all_nodes", params=dict(keep_all_nodes=1), frames=[
        F(0, status=FIRST),
        F(1, k=GAP, status=ADDED, constant_position=1)],
        final=dict(valid_tf=[1, 0])),
    dict(name="constant position: a loop closure alone, the predecessor unmatched and near in time", frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, res={0: R()}, status=ADDED, candidates=[0, 1], verdicts=[V_ACCEPTED, V_NO_EDGE], predecessor_matched=0,
          constant_position=1, best_id1=1, best_id2=2, best_n_inl=0, sequential_edges=3)],
        final=dict(valid_tf=[1, 1, 0], edges=[(0, 1), (0, 2), (1, 2)])),
    dict(name="constant position: the same loop closure 0.2 s later adds none", frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, k=1 + GAP, res={0: R()}, status=ADDED, predecessor_matched=0, constant_position=0, best_id1=0)],
        final=dict(valid_tf=[1, 1, 1], edges=[(0, 1), (0, 2)])),
    dict(name="constant position: dt_prev == 0 is not handed to the optimiser", frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, k=1, status=NO_MATCH, id=-1, found=0, constant_position=2)],
        final=dict(slots=[0, 1], edges=[(0, 1)])),
    dict(name="keep_good_nodes at rows == min_matches", params=dict(keep_good_nodes=1), frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, rows=20, k=1 + GAP, status=NO_MATCH, constant_position=0)]),
    dict(name="keep_good_nodes at rows == min_matches + 1", params=dict(keep_good_nodes=1), frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, rows=21, k=1 + GAP, status=ADDED, constant_position=1)]),
    dict(name="a weak first node is replaced", frames=[
        F(5, rows=25, k=0, status=FIRST),
        F(6, rows=128, k=GAP, status=REPLACED_FIRST, id=0, found=0, released_slot=5, candidates=[0], verdicts=[V_NO_EDGE])],
        final=dict(keyframes=[0], slots=[6], valid_tf=[1], fixed=[1], edges=[])),
    dict(name="a first node that is not weaker stays", frames=[
        F(5, rows=25, k=0, status=FIRST),
        F(6, rows=25, k=GAP, status=NO_MATCH, id=-1, released_slot=-1)],
        final=dict(slots=[5])),
    dict(name="optimizer_skip_step 0", params=dict(optimizer_skip_step=0), frames=[
        F(0, status=FIRST)] + [F(k, res={k - 1: R()}, status=ADDED, optimize_due=0) for k in range(1, 4)]),
    dict(name="optimizer_skip_step 1", params=dict(optimizer_skip_step=1), frames=[
        F(0, status=FIRST)] + [F(k, res={k - 1: R()}, status=ADDED, optimize_due=1) for k in range(1, 4)]),
    dict(name="optimizer_skip_step 3", params=dict(optimizer_skip_step=3), frames=[
        F(0, status=FIRST)] + [F(k, res={k - 1: R()}, status=ADDED, optimize_due=int((k + 1) % 3 == 0)) for k in range(1, 7)]),
    dict(name="create_cloud_every_nth_node 2", params=dict(create_cloud_every_nth_node=2), frames=[
        F(0, status=FIRST, cloud_released=0)] + [F(k, res={k - 1: R()}, status=ADDED, cloud_released=k % 2) for k in range(1, 5)]),
    dict(name="loop closure or sequential at |id1 - id2| == predecessor_candidates and one more",
         params=dict(predecessor_candidates=2), frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED, sequential_edges=1, loop_closure_edges=0),
        F(2, res={1: R()}, status=ADDED, sequential_edges=2, loop_closure_edges=0),
        F(3, res={2: R(), 1: R(n_inl=30), 0: R(n_inl=20)}, status=ADDED, candidates=[1, 0, 2],
          verdicts=[V_ACCEPTED, V_ACCEPTED, V_ACCEPTED], sequential_edges=4, loop_closure_edges=1)]),
    dict(name="an edge the measurement model withdrew, and an ICP edge", frames=[
        F(0, status=FIRST),
        F(1, res={0: R()}, status=ADDED),
        F(2, res={0: R(flags=_lib.SLAM_RESULT_WITHDRAWN), 1: R(flags=_lib.SLAM_RESULT_ICP, n_inl=77, info=123.0)}, status=ADDED,
          candidates=[0, 1], verdicts=[V_WITHDRAWN, V_ACCEPTED | V_ICP], best_id1=-1, best_id2=-1, best_n_inl=0,
          predecessor_matched=1)],   # an ICP edge has no inliers: it never becomes the best result
        final=dict(edges=[(0, 1), (1, 2)], info00=[1.0, 1e-2])),
]


# ---- running a case through the library ------------------------------------------------------------------------------
def params_of(lib, case):
    p = _lib.SlamParams()
    lib.rgbdfe_slam_default_params(C.byref(p))
    for k, v in case.get("params", {}).items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def hex64(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def step_line(st):
    """The canonical text of a step record without its times (tests/emu/slam_machine_main.cpp prints the same)."""
    n = st.n_candidates
    head = [st.status, st.id, st.found, st.initial_id, st.initial_verdict, n] + list(st.candidates[:n]) + list(st.verdicts[:n])
    tail = [st.best_id1, st.best_id2, st.best_n_inl, st.predecessor_matched, st.edge_to_keyframe, st.keyframe_added,
            st.cleared_first, st.cleared_last, st.released_slot, st.constant_position, st.cloud_released,
            st.has_broadcast_pose, st.optimize_due, st.sequential_edges, st.loop_closure_edges]
    return " ".join(str(int(v)) for v in head + tail) + " | " + " ".join(hex64(v) for v in st.motion_estimate) + " | " + \
        " ".join(hex64(v) for v in st.broadcast_pose)


def compact_records(frame, ids):
    rec = np.zeros(len(ids), _lib.COMPACT_DTYPE)
    flags = np.zeros(len(ids), np.uint8)
    for k, i in enumerate(ids):
        r = frame["res"].get(int(i), NO_EDGE)
        rec[k]["id1"], rec[k]["id2"] = (900 + int(i), 999) if r["edge"] else (-1, -1)   # slot names: the machine must not use them
        rec[k]["n_inl"], rec[k]["trafo"], rec[k]["info_scale"] = r["n_inl"], r["T"], r["info"]
        flags[k] = r["flags"]
    return rec, flags


def run_case(lib, case):
    """-> (the step record of every frame, the final state) through rgbdfe_slam_begin / rgbdfe_slam_feed without a context."""
    g = lib.rgbdfe_pose_graph_create()
    assert lib.rgbdfe_pose_graph_set_strategy(g, case.get("strategy", NONE)) == 0
    p = params_of(lib, case)
    s = C.c_void_p()
    assert lib.rgbdfe_slam_create(None, g, C.byref(p), C.byref(s)) == 0
    steps = []
    try:
        for fr in case["frames"]:
            ids = np.zeros(_lib.SLAM_MAX_CANDIDATES, np.int32)
            n, st = C.c_int32(0), _lib.SlamStep()
            rc = lib.rgbdfe_slam_begin(s, fr["slot"], fr["rows"], fr["t"][0], fr["t"][1], ids.ctypes.data, len(ids), C.byref(n),
                                       C.byref(st))
            assert rc == 0, rc
            rounds = 0
            while n.value > 0:
                rec, flags = compact_records(fr, ids[:n.value])
                rc = lib.rgbdfe_slam_feed(s, rec.ctypes.data, flags.ctypes.data, n.value, ids.ctypes.data, len(ids), C.byref(n),
                                          C.byref(st))
                assert rc == 0, rc
                rounds += 1
                assert rounds <= 2
            steps.append(st)
        final = final_state(lib, g, s)
    finally:
        lib.rgbdfe_slam_destroy(s)
        lib.rgbdfe_pose_graph_destroy(g)
    return steps, final


def final_state(lib, g, s):
    n = lib.rgbdfe_slam_node_count(s)
    kf, nk = np.zeros(n + 1, np.int32), C.c_int32(0)
    assert lib.rgbdfe_slam_keyframes(s, kf.ctypes.data, len(kf), C.byref(nk)) == 0
    out = dict(keyframes=[int(v) for v in kf[:nk.value]], slots=[lib.rgbdfe_slam_slot_of(s, i) for i in range(n)],
               valid_tf=[lib.rgbdfe_slam_valid_tf(s, i) for i in range(n)], fixed=[], edges=[], info00=[], estimates=[])
    for i in range(n):
        f, X = C.c_int32(-1), np.zeros(16)
        assert lib.rgbdfe_pose_graph_get_fixed(g, i, C.byref(f)) == 0 and lib.rgbdfe_pose_graph_get_estimate(g, i, X.ctypes.data) == 0
        out["fixed"].append(f.value)
        out["estimates"].append(X)
    e = 0
    while True:
        a, b, info = C.c_int32(), C.c_int32(), np.zeros(36)
        if lib.rgbdfe_pose_graph_get_edge(g, e, C.byref(a), C.byref(b), None, info.ctypes.data, None) != 0:
            break
        out["edges"].append((a.value, b.value))
        out["info00"].append(float(info[0]))
        e += 1
    return out


def check_case(case, steps, final):
    """The step records and the final state against what the case writes out."""
    assert len(steps) == len(case["frames"])
    for k, (fr, st) in enumerate(zip(case["frames"], steps)):
        for name, want in fr["expect"].items():
            where = "%s, frame %d, %s" % (case["name"], k, name)
            if name == "candidates":
                assert list(st.candidates[:st.n_candidates]) == want, where
            elif name == "verdicts":
                assert list(st.verdicts[:st.n_candidates]) == want, where
            elif name == "motion_tx":
                assert st.motion_estimate[12] == want, (where, st.motion_estimate[12])
            elif name == "broadcast_tx":
                assert st.broadcast_pose[12] == want, (where, st.broadcast_pose[12])
            else:
                assert getattr(st, name) == want, (where, getattr(st, name))
    for name, want in case.get("final", {}).items():
        assert final[name] == want, (case["name"], name, final[name])


# ---- the same case as the text the stand-alone program reads ----------------------------------------------------------
def script_text(case):
    """P name value / S strategy / F slot rows sec nsec n_results / R id edge n_inl info(hex) flags T(16 hex) ..."""
    out = ["S %d" % case.get("strategy", NONE)]
    for k, v in case.get("params", {}).items():
        out.append("P %s %s" % (k, hex64(v)))
    for fr in case["frames"]:
        out.append("F %d %d %d %d %d" % (fr["slot"], fr["rows"], fr["t"][0], fr["t"][1], len(fr["res"])))
        for i, r in fr["res"].items():
            out.append("R %d %d %d %s %d %s" % (i, int(r["edge"]), r["n_inl"], hex64(r["info"]), r["flags"],
                                               " ".join("%08x" % v for v in r["T"].view(np.uint32))))
    return "\n".join(out) + "\n"


def final_lines(final):
    return ["K " + " ".join(map(str, final["keyframes"])), "T " + " ".join(map(str, final["slots"])),
            "V " + " ".join(map(str, final["valid_tf"])), "X " + " ".join(map(str, final["fixed"])),
            "E " + " ".join("%d-%d:%s" % (a, b, hex64(i)) for (a, b), i in zip(final["edges"], final["info00"]))] + \
           ["N %d " % k + " ".join(hex64(v) for v in X) for k, X in enumerate(final["estimates"])]
