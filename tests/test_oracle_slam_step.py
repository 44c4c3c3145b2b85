"""CPU: the SLAM step's oracle (tests/slam_step_oracle.py) on the planted sequences of tests/slam_sequence.py with the pairs
through oracle.pyoracle.match_node_pair.  First the conditions the GPU test relies on -- a loop-closure edge, a keyframe
beyond node 0, a rejected candidate, every planted frame meeting its fate, the trajectory inside the convention guard --
then the library's decision machine (rgbdfe_slam_begin / _feed, no device) fed the same records: every step record and
the whole graph, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import slam_sequence as sq
import slam_step_oracle as so
from oracle import pyoracle as po
from rgbdslam_v2_amd import _lib
from rgbdslam_v2_amd.candidates import PoseGraph
from rgbdslam_v2_amd.frontend import Slam

RUNS = sq.RUNS


def cpu_pairs(frames):
    cfg = _lib.RgbdfeConfig()
    _lib.load().rgbdfe_default_config(C.byref(cfg))
    prm = po.default_params(seed=cfg.params.seed, depth_cov=cfg.params.depth_cov)
    cache = {}

    def pairs(new_slot, slots):
        out = []
        for t in slots:
            if (new_slot, t) not in cache:
                q, o = frames[new_slot], frames[t]
                cache[(new_slot, t)] = sq.record_of_pyoracle(po.match_node_pair(q["desc"], q["xyz1"], new_slot, o["desc"], o["xyz1"], t, prm))
            out.append(cache[(new_slot, t)])
        return out
    return pairs


@pytest.fixture(scope="module")
def runs():
    """name -> (frames, the oracle after the run, its step records, the pair function with its cache)"""
    out = {}
    for name, run in RUNS.items():
        frames = run["frames"]()
        pairs = cpu_pairs(frames)
        oracle = so.SlamOracle(pairs, strategy=run["strategy"], optimizer_skip_step=0, **run["params"])
        steps = [oracle.add_node(slot, len(f["desc"]), f["stamp"]) for slot, f in enumerate(frames)]
        out[name] = (frames, oracle, steps, pairs)
    return out


def test_the_planted_frames_meet_their_fates(runs):
    frames, oracle, steps, _ = runs["main, first"]
    status = [s["status"] for s in steps]
    assert status[0] == so.FIRST and status[3] == so.TOO_FEW and status[6] == so.ADDED and steps[6]["constant_position"] == 1
    assert status[10] == so.NO_MATCH and status[-1] == so.ADDED and status.count(so.ADDED) == 13
    assert oracle.loop_closure_edges >= 1                      # the revisit of frame 0 closes a loop
    assert len(oracle.keyframes) >= 2                          # a keyframe beyond node 0
    assert any(v != so.V_ACCEPTED for s in steps for v in s["verdicts"])   # a rejected candidate
    # The revisit against node 0 itself: RANSAC on identical frames gives a rotation whose trace is above 3 by a few ulps,
    # acos' argument is above 1, the angle is NaN and the edge is "not small" -- the reference's unclamped acos at work.
    assert steps[-1]["verdicts"][steps[-1]["candidates"].index(0)] == so.V_NOT_SMALL
    assert steps[-1]["verdicts"].count(so.V_ACCEPTED) >= 3 and steps[-1]["predecessor_matched"] == 1
    assert oracle.valid_tf.count(0) == 1                       # the frame the constant-position edge kept
    _, first, fsteps, _ = runs["main, first, clear_non_keyframes"]
    _, loop, lsteps, _ = runs["main, largest_loop, clear_non_keyframes"]
    assert first.keyframes != loop.keyframes and len(loop.keyframes) >= 3
    for o, st in ((first, fsteps), (loop, lsteps)):
        assert any(s["cleared"] for s in st) and -1 in o.slots and any(s["cloud_released"] for s in st)
        assert any(o.slots[i] < 0 for s in st for i in s["candidates"])   # a later frame is compared with a cleared node


def test_the_repeat_the_jump_and_the_weak_first_node(runs):
    steps = runs["repeat"][2]
    assert [s["status"] for s in steps] == [so.FIRST, so.ADDED, so.OUT_OF_BOUNDS, so.ADDED, so.ADDED]
    assert steps[2]["broadcast_pose"] is not None and steps[3]["initial_verdict"] == so.V_ACCEPTED
    steps = runs["jump"][2]
    assert [s["status"] for s in steps][:3] == [so.FIRST, so.ADDED, so.ADDED]
    assert steps[3]["verdicts"] == [so.V_NOT_SMALL] * 3 and so.V_NOT_SMALL not in steps[1]["verdicts"] + steps[2]["verdicts"]
    assert steps[3]["status"] == so.ADDED and steps[3]["constant_position"] == 1   # kept by the constant-position edge alone
    steps = runs["weak first"][2]
    assert [s["status"] for s in steps] == [so.FIRST, so.REPLACED_FIRST, so.ADDED] and steps[1]["released_slot"] == 0


def test_the_convention_guard_holds_for_the_oracle(runs):
    """The last node's estimate against its synthetic pose relative to node 0: below 0.05 x the path length.  A wrong
    transform direction or multiplication side gives an error of the order of the path itself."""
    frames, oracle, _, _ = runs["main, first"]
    in_graph = [frames[s] for s in oracle.slots]
    want = np.linalg.inv(in_graph[0]["pose"]) @ in_graph[-2]["pose"]   # the last base frame; the revisit sits on node 0
    got = oracle.estimates[len(oracle.slots) - 2]
    assert np.linalg.norm(got[:3, 3] - want[:3, 3]) < 0.05 * sq.path_length(in_graph[:-1])
    assert np.linalg.norm(oracle.estimates[len(oracle.slots) - 1][:3, 3]) < 0.05 * sq.path_length(in_graph[:-1])   # the revisit


@pytest.mark.parametrize("name", list(RUNS))
def test_the_librarys_machine_gives_the_oracles_run(runs, name):
    frames, oracle, steps, pairs = runs[name]
    graph = PoseGraph()
    graph.set_strategy(RUNS[name]["strategy"])
    slam = Slam(None, graph, optimizer_skip_step=0, **RUNS[name]["params"])
    for slot, (f, want) in enumerate(zip(frames, steps)):
        ids, rec = slam.begin(slot, len(f["desc"]), f["stamp"])
        while rec is None:
            live = [i for i in ids if slam.slot_of(i) >= 0]
            by_id = dict(zip(live, pairs(slot, [slam.slot_of(i) for i in live])))
            ids, rec = slam.feed(sq.compact_of_fields([by_id.get(i) for i in ids]))
        sq.same_step(rec, want)
    sq.same_state(slam, graph, oracle)
    slam.close()
