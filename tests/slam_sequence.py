"""The planted sequences of the SLAM-step tests (tests/test_oracle_slam_step.py on the CPU, tests/test_gpu_slam_step.py on
the device) and the comparison of a run against tests/slam_step_oracle.py.

Base: synth.make_sequence(n_frames=12, n_kp=128, n_world=400, motion_scale=4.0, depth_noise=0.0005, pixel_noise=0.1): every
(frame, predecessor) pair gives an edge; consecutive motion is 1.7-4.6 cm and 2.1-2.5 degrees, i.e. 0.5-1.4 m/s at 30 Hz."""
import functools

import numpy as np

from rgbdslam_v2_amd import _lib, synth

FRAME_NS = 33333333
SPARSE = dict(clear_non_keyframes=1, create_cloud_every_nth_node=2, predecessor_candidates=3, neighbor_candidates=1,
              min_sampled_candidates=0)


@functools.lru_cache(maxsize=None)
def base():
    return synth.make_sequence(n_frames=12, n_kp=128, n_world=400, motion_scale=4.0, depth_noise=0.0005, pixel_noise=0.1)


@functools.lru_cache(maxsize=None)
def elsewhere():
    """Frames of another world: nothing in them matches the base sequence."""
    return synth.make_sequence(n_frames=2, n_kp=128, n_world=400, motion_scale=4.0, depth_noise=0.0005, pixel_noise=0.1, seed=77)


def stamp(ticks):
    ns = ticks * FRAME_NS
    return (ns // 1000000000, ns % 1000000000)


def frame(k, ticks, rows=None, source=None, random_desc=False):
    s = source or base()
    desc, xyz = s["desc"][k][:rows].copy(), s["xyz1"][k][:rows].copy()
    if random_desc:
        desc = np.random.default_rng(1000 + k).integers(0, 256, desc.shape, dtype=np.uint8)
    return dict(desc=desc, xyz1=xyz, stamp=stamp(ticks), pose=s["poses"][k] if source is None else None)


def main_sequence():
    """12 frames with a 19-row frame, a frame of random descriptors 1 / 30 s after its predecessor (kept by the constant-
    position edge) and one 0.2 s after (dropped) planted among them, and a revisit of frame 0, 0.2 s after the last frame."""
    fr, t = [], 0
    for k in range(12):
        fr.append(frame(k, t)); t += 1
        if k == 2:
            fr.append(frame(3, t, rows=19)); t += 1
        if k == 4:
            fr.append(frame(5, t, random_desc=True)); t += 1
        if k == 7:
            t += 5
            fr.append(frame(8, t, random_desc=True)); t += 1
    fr.append(frame(0, t + 5))
    return fr


def repeat_sequence():
    """An exact repeat of the previous frame: with min_translation_meter 0.01 and min_rotation_degree 1.0 it is out of bounds."""
    return [frame(0, 0), frame(1, 1), frame(1, 2), frame(2, 3), frame(3, 4)]


def jump_sequence():
    """A frame taken five frames ahead, one tick after its predecessor: several times the speed of the others."""
    return [frame(0, 0), frame(1, 1), frame(2, 2), frame(7, 3), frame(3, 4)]


def weak_first_sequence():
    """A 25-row first frame followed, 0.2 s later, by an unrelated 128-row one."""
    return [frame(0, 0, rows=25), frame(0, 6, source=elsewhere()), frame(1, 7, source=elsewhere())]


# the runs of both tests: the frames, the pose-graph strategy, the SLAM parameters
RUNS = {
    "main, first": dict(frames=main_sequence, strategy="first", params={}),
    # fewer candidates: fewer edges reach a keyframe, more keyframes are declared, and the two strategies part ways
    "main, first, clear_non_keyframes": dict(frames=main_sequence, strategy="first", params=SPARSE),
    "main, largest_loop, clear_non_keyframes": dict(frames=main_sequence, strategy="largest_loop", params=SPARSE),
    "repeat": dict(frames=repeat_sequence, strategy="first", params=dict(min_translation_meter=0.01, min_rotation_degree=1.0)),
    # consecutive frames move at 1.0-1.1 m/s, the frame five ahead at 1.6-2.5 m/s against its three predecessors
    "jump": dict(frames=jump_sequence, strategy="first", params=dict(max_translation_meter=1.4)),
    "weak first": dict(frames=weak_first_sequence, strategy="first", params={}),
}


def record_of_pyoracle(ref):
    """oracle.pyoracle.match_node_pair's dict as the fields of a match record the SLAM oracle reads."""
    mask = np.zeros(_lib.RGBDFE_MASK_WORDS, np.uint64)
    for m in ref["inl_idx"]:
        mask[int(m) // 64] |= np.uint64(1) << np.uint64(int(m) % 64)
    return dict(id1=ref["id1"], id2=ref["id2"], n_inl=ref["n_inl"], trafo=np.asarray(ref["T"], np.float32).T.reshape(16),
                info_scale=ref["info_scale"], inlier_mask=mask, all_q=ref["all_q"], all_t=ref["all_t"])


def compact_of_fields(recs):
    out = np.zeros(len(recs), _lib.COMPACT_DTYPE)
    for k, r in enumerate(recs):
        out[k]["id1"], out[k]["id2"] = (-1, -1) if r is None else (r["id1"], r["id2"])
        if r is not None:
            out[k]["n_inl"], out[k]["trafo"], out[k]["info_scale"], out[k]["inlier_mask"] = r["n_inl"], r["trafo"], r["info_scale"], r["inlier_mask"]
    return out


def same_step(got, want):
    """A SlamStepRecord of the library against the oracle's step, field for field (times aside); matrices byte for byte."""
    for name in ("status", "id", "found", "initial_id", "initial_verdict", "candidates", "verdicts", "best_id1", "best_id2",
                 "best_n_inl", "predecessor_matched", "edge_to_keyframe", "keyframe_added", "released_slot", "constant_position",
                 "cloud_released", "optimize_due", "sequential_edges", "loop_closure_edges", "optimized", "lm_iterations"):
        assert getattr(got, name) == want[name], (name, getattr(got, name), want[name])
    assert np.float64(got.chi2).tobytes() == np.float64(want["chi2"]).tobytes(), (got.chi2, want["chi2"])
    cleared = list(range(got.cleared_first, got.cleared_last + 1)) if got.cleared_first >= 0 else []
    assert cleared == want["cleared"]
    assert got.motion_estimate.tobytes() == np.ascontiguousarray(want["motion_estimate"]).tobytes()
    assert bool(got.has_broadcast_pose) == (want["broadcast_pose"] is not None)
    if want["broadcast_pose"] is not None:
        assert got.broadcast_pose.tobytes() == np.ascontiguousarray(want["broadcast_pose"]).tobytes()


def same_state(slam, graph, oracle, estimates=True):
    """Slot table, keyframes, valid_tf, fixed flags, the edges (ids, measurement, information) and the estimates."""
    assert slam.slots() == oracle.slots and slam.keyframes() == oracle.keyframes and slam.valid_tf() == oracle.valid_tf
    for k, (id1, id2, Z, info) in enumerate(oracle.edges):
        e = graph.edge(k)
        assert (e["id1"], e["id2"]) == (id1, id2)
        assert e["transform"].tobytes() == np.ascontiguousarray(Z).tobytes()
        assert e["information"].tobytes() == (np.eye(6) * info).tobytes()
    with np.testing.assert_raises(Exception):
        graph.edge(len(oracle.edges))
    for i in range(len(oracle.slots)):
        if estimates:
            assert graph.get_estimate(i).tobytes() == np.ascontiguousarray(oracle.estimates[i]).tobytes(), i
            assert int(graph.get_fixed(i)) == oracle.fixed[i]


def path_length(frames_in_graph):
    p = [f["pose"][:3, 3] for f in frames_in_graph]
    return float(sum(np.linalg.norm(b - a) for a, b in zip(p, p[1:])))
