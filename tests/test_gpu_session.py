"""GPU: what leaves a context and goes back in -- rgbdfe_download_nodes against what was uploaded (every comparison on
bytes: no tolerance anywhere), the counters and detector thresholds written back, and a detector that continues on another
context as the first one would have; then session files: restored nodes match as before, tests/test_gpu_slam_step.py's
lockstep with the oracle while the library is cut, saved, torn down and loaded into fresh objects, clouds, the file's
properties and refusals, and the C++ header.  Shapes: 130 keypoints per slot, so a slot's counters end inside a word and the counter
stride is 132; nodes of 0, 1, 63, 64, 65 and 130 rows (one row, one below / at / one above the pack kernel's 64-row tile, a
full slot), whose odd sizes leave the next node's KeyPoint.pt half a 16-byte unit off and its counters on an odd byte."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import icp_oracle as io
import pose_graph_eval_oracle as pe
import session_file as sfile
import slam_sequence as sq
import slam_step_oracle as so
from rgbdslam_v2_amd import _lib, synth
from rgbdslam_v2_amd.candidates import PoseGraph
from rgbdslam_v2_amd.frontend import FrontEnd, RgbdfeError, Slam

pytestmark = pytest.mark.gpu

POISON = 0xA5
INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
# id -> rows, uploaded in this order into a fresh context: the slots follow the order of the uploads, not the ids
ORB_ROWS = {5: 65, 0: 0, 23: 130, 7: 1, 11: 63, 2: 64}
WITH_KEYPOINTS = (5, 23, 11)
ASK = [23, 2, 5, 0, 11, 7]   # neither id order nor upload (= slot) order


def new_fe(max_nodes=24, max_keypoints=130):
    return FrontEnd(device_id=0, max_nodes=max_nodes, max_keypoints=max_keypoints, max_pairs_per_batch=16)


@pytest.fixture(scope="module")
def orb():
    """One context with the ORB nodes, keypoints for some, and counters that one statistics launch over a batch between
    them has left non-zero.  Returns (fe, {id: dict(desc, xyz1, kp_xy, stats)})."""
    import torch
    seq = synth.make_sequence(n_frames=6, n_kp=130, n_world=400, motion_scale=4.0, depth_noise=0.0005, pixel_noise=0.1)
    rng = np.random.default_rng(3)
    fe = new_fe()
    assert not fe.download_nodes_stats()["feature_stats_allocated"]
    nodes = {}
    for k, (i, rows) in enumerate(ORB_ROWS.items()):
        nodes[i] = dict(desc=seq["desc"][k][:rows].copy(), xyz1=seq["xyz1"][k][:rows].copy(), kp_xy=np.zeros((rows, 2), np.float32))
        fe.upload_node(i, nodes[i]["desc"], nodes[i]["xyz1"])
        if i in WITH_KEYPOINTS:
            nodes[i]["kp_xy"] = rng.uniform(0, 640, (rows, 2)).astype(np.float32)
            fe.upload_node_keypoints(i, nodes[i]["kp_xy"])
    # before any call has counted: zeros, and the read-back leaves the counters unallocated (rgbdfe_download_nodes_stats)
    first = fe.download_nodes(ASK)
    assert not first["stats"].any() and not fe.download_nodes_stats()["feature_stats_allocated"]
    q, t = np.array([23, 23, 2, 5], np.int32), np.array([5, 2, 11, 11], np.int32)
    recs = fe.match_pair_list(q, t)
    d = torch.empty(len(q) * recs.dtype.itemsize, dtype=torch.uint8, device="cuda")
    fe.match_pair_list_device(q, t, d.data_ptr())
    fe.synchronize()
    assert fe.update_inlier_features(d.data_ptr(), q, t, [1, 1, 1, 1]) == 1
    for i in nodes:
        nodes[i]["stats"] = fe.node_feature_stats(i)
    assert all(nodes[i]["stats"].any() for i in (23, 5, 2, 11))   # (a condition on the frames) every pair had inliers
    yield fe, nodes
    fe.close()


def packed(nodes, ids, field):
    return b"".join(nodes[i][field].tobytes() for i in ids)


def raw_download(fe, ids, capacity, want=("desc", "xyz1", "kp_xy", "stats"), desc_row=32, tail=9):
    """The C entry point on poisoned arrays with `tail` rows of room behind `capacity`.  Returns (status, arrays, offsets, kinds)."""
    ids = np.array(ids, np.int32)
    width = {"desc": desc_row, "xyz1": 16, "kp_xy": 8, "stats": 1}
    arr = {f: np.full((capacity + tail) * width[f], POISON, np.uint8) for f in want}
    off = np.full(len(ids) + 1, -7, np.int64)
    kinds = np.full(len(ids), -7, np.int32)
    p = lambda f: arr[f].ctypes.data if f in arr else None
    st = fe._L.rgbdfe_download_nodes(fe._ctx, len(ids), ids.ctypes.data, capacity, p("desc"), p("xyz1"), p("kp_xy"), p("stats"),
                                     off.ctypes.data, kinds.ctypes.data)
    return st, arr, off, kinds


def test_download_is_upload(orb):
    fe, nodes = orb
    total = sum(ORB_ROWS[i] for i in ASK)
    st, arr, off, kinds = raw_download(fe, ASK, total)
    assert st == 0
    assert off.tolist() == np.concatenate([[0], np.cumsum([ORB_ROWS[i] for i in ASK])]).tolist()
    assert kinds.tolist() == [_lib.RGBDFE_NODE_HAS_KEYPOINTS if i in WITH_KEYPOINTS else 0 for i in ASK]
    for f, w in (("desc", 32), ("xyz1", 16), ("kp_xy", 8), ("stats", 1)):
        got = arr[f].tobytes()
        assert got[:total * w] == packed(nodes, ASK, f), f
        assert got[total * w:] == bytes([POISON]) * (len(got) - total * w), f + ": written beyond row_offsets[-1]"
    s = fe.download_nodes_stats()
    assert s["launches"] == 1 and s["copies"] == 4   # whatever the number of nodes
    out = fe.download_nodes(ASK)   # the binding: typed arrays
    assert out["desc"].shape == (total, 32) and out["kp_xy"].shape == (total, 2) and out["has_keypoints"].tolist() == [i in WITH_KEYPOINTS for i in ASK]
    for f in ("desc", "xyz1", "kp_xy", "stats"):
        assert out[f].tobytes() == packed(nodes, ASK, f)


@pytest.mark.parametrize("want", [("desc",), ("xyz1",), ("kp_xy",), ("stats",), ("desc", "stats"), ("xyz1", "kp_xy"),
                                  ("desc", "xyz1", "kp_xy"), ()])
def test_any_output_may_be_null(orb, want):
    fe, nodes = orb
    total = sum(ORB_ROWS[i] for i in ASK)
    st, arr, off, kinds = raw_download(fe, ASK, total, want=want)
    assert st == 0 and off[-1] == total
    for f in want:
        assert arr[f].tobytes()[:total * {"desc": 32, "xyz1": 16, "kp_xy": 8, "stats": 1}[f]] == packed(nodes, ASK, f)
    s = fe.download_nodes_stats()
    assert s["copies"] == len(want) and s["launches"] == (1 if want else 0)
    assert fe._L.rgbdfe_download_nodes(fe._ctx, 2, np.array([5, 7], np.int32).ctypes.data, 2 ** 40, None, None, None, None, None, None) == 0


def test_single_nodes_and_lists_without_rows(orb):
    fe, nodes = orb
    for i, rows in ORB_ROWS.items():
        out = fe.download_nodes([i])
        assert out["row_offsets"].tolist() == [0, rows]
        for f in ("desc", "xyz1", "kp_xy", "stats"):
            assert out[f].tobytes() == nodes[i][f].tobytes(), (i, f)
        kind, has = C.c_int32(-1), C.c_int32(-1)
        desc = np.full((rows + 1) * 32, POISON, np.uint8)
        n = fe._L.rgbdfe_download_node(fe._ctx, i, rows, desc.ctypes.data, None, None, None, C.byref(kind), C.byref(has))
        assert n == rows and kind.value == 0 and has.value == int(i in WITH_KEYPOINTS)
        assert desc.tobytes() == nodes[i]["desc"].tobytes() + bytes([POISON]) * 32
    assert fe.download_nodes([])["row_offsets"].tolist() == [0]
    assert fe.download_nodes([0, 0])["row_offsets"].tolist() == [0, 0, 0]
    twice = fe.download_nodes([5, 7, 5])   # a gather: an id may appear twice
    assert twice["stats"].tobytes() == packed(nodes, [5, 7, 5], "stats")


def test_refusals_write_nothing(orb):
    fe, nodes = orb
    total = sum(ORB_ROWS[i] for i in ASK)
    st, arr, off, kinds = raw_download(fe, ASK, total - 1)
    assert st == CAPACITY and off[-1] == total
    assert (off[:-1] == -7).all() and (kinds == -7).all() and all((a == POISON).all() for a in arr.values())
    st, arr, off, kinds = raw_download(fe, [23, 99, 5], 400)
    assert st == UNKNOWN_NODE
    assert (off == -7).all() and (kinds == -7).all() and all((a == POISON).all() for a in arr.values())
    assert fe._L.rgbdfe_download_node(fe._ctx, 99, 10, None, None, None, None, None, None) == UNKNOWN_NODE
    assert fe._L.rgbdfe_download_node(fe._ctx, 23, 129, None, None, None, None, None, None) == CAPACITY


@pytest.mark.parametrize("kind", ["sift", "float"])
def test_float_nodes_and_mixed_lists(kind):
    rng = np.random.default_rng(17)
    fe = new_fe()
    try:
        nodes = {}
        for i, rows in ((9, 65), (1, 1), (4, 64)):
            d = np.abs(rng.standard_normal((rows, 128))).astype(np.float32)
            d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
            nodes[i] = dict(desc=d, xyz1=rng.standard_normal((rows, 4)).astype(np.float32), kp_xy=np.zeros((rows, 2), np.float32),
                            stats=np.zeros(rows, np.uint8))
            (fe.upload_sift_node if kind == "sift" else fe.upload_float_node)(i, d, nodes[i]["xyz1"])
        nodes[4]["kp_xy"] = rng.uniform(0, 640, (64, 2)).astype(np.float32)
        fe.upload_node_keypoints(4, nodes[4]["kp_xy"])
        nodes[9]["stats"] = rng.integers(0, 256, 65, np.uint8)   # written back as a restore would
        fe.set_node_feature_stats(9, nodes[9]["stats"])
        assert fe.node_feature_stats(9).tobytes() == nodes[9]["stats"].tobytes()
        ask = [4, 9, 1]
        st, arr, off, kinds = raw_download(fe, ask, 130, desc_row=512)
        assert st == 0 and off.tolist() == [0, 64, 129, 130]
        k = 1 if kind == "sift" else 2
        assert kinds.tolist() == [k | _lib.RGBDFE_NODE_HAS_KEYPOINTS, k, k]
        for f, w in (("desc", 512), ("xyz1", 16), ("kp_xy", 8), ("stats", 1)):
            got = arr[f].tobytes()
            assert got[:130 * w] == packed(nodes, ask, f), f
            assert got[130 * w:] == bytes([POISON]) * (9 * w), f
        out = fe.download_nodes(ask)
        assert out["desc"].dtype == np.float32 and out["desc"].tobytes() == packed(nodes, ask, "desc")
        fe.upload_node(12, np.zeros((3, 32), np.uint8), np.ones((3, 4), np.float32))
        st, arr, off, kinds = raw_download(fe, [9, 12], 200, desc_row=512)
        assert st == INVALID_ARG and "kinds" in fe._L.rgbdfe_last_error(fe._ctx).decode()
        assert (off == -7).all() and all((a == POISON).all() for a in arr.values())
        with pytest.raises(RgbdfeError):
            fe.set_node_feature_stats(12, np.zeros(4, np.uint8))   # not the node's row count
    finally:
        fe.close()


def test_a_float_node_of_fewer_dimensions_comes_back_padded():
    rng = np.random.default_rng(2)
    fe = new_fe()
    try:
        d = rng.standard_normal((65, 64)).astype(np.float32)
        fe.upload_float_node(3, d, np.ones((65, 4), np.float32))
        out = fe.download_nodes([3], fields=("desc",))
        assert out["desc"][:, :64].tobytes() == d.tobytes() and not out["desc"][:, 64:].any()
    finally:
        fe.close()


# ---- the grid detector's state ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("detector", ["ORB", "FAST"])
def test_a_detector_continues_on_another_context(detector):
    """Four frames through detect_describe on context A; B gets A's thresholds after two and must give A's keypoints,
    descriptors, points and thresholds for frames 3 and 4.  The thresholds have moved by then (asserted): a B that started
    from 20 would not."""
    seq = synth.make_image_sequence(n_frames=4, width=320, height=240, seed=3)
    K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])

    def configured():
        f = new_fe(max_nodes=4, max_keypoints=600)
        f.detector_configure(max_keypoints=300, grid_resolution=3, adjuster_max_iterations=5)
        f.set_detector_type(detector)
        return f

    a, b = configured(), configured()
    try:
        for k in range(2):
            a.detect_describe(seq["gray"][k], seq["mask"][k], seq["depth"][k], *K)
        saved = a.detector_thresholds()
        assert len(saved) == 9 and (saved != 20.0).any()
        with pytest.raises(RgbdfeError):
            b.detector_set_thresholds(saved[:4])   # not the configured grid
        with pytest.raises(RgbdfeError):
            b.detector_set_thresholds(np.where(np.arange(9) == 3, np.nan, saved))
        assert (b.detector_thresholds() == 20.0).all()   # a refusal changes nothing
        b.detector_set_thresholds(saved)
        assert b.detector_thresholds().tobytes() == saved.tobytes()
        for k in (2, 3):
            ra = a.detect_describe(seq["gray"][k], seq["mask"][k], seq["depth"][k], *K)
            rb = b.detect_describe(seq["gray"][k], seq["mask"][k], seq["depth"][k], *K)
            assert len(ra[0]) > 0
            for x, y in zip(ra, rb):
                assert x.tobytes() == y.tobytes(), k
            assert a.detector_thresholds().tobytes() == b.detector_thresholds().tobytes()
    finally:
        a.close(); b.close()


# ---- session files ----------------------------------------------------------------------------------------------------
class Session:
    """A context, a graph and a Slam that can be saved, torn down and brought back from the file into fresh objects."""

    def __init__(self, params, strategy=None, **fe_args):
        self.params, self.fe_args = params, fe_args
        self.open()
        if strategy is not None:
            self.graph.set_strategy(strategy)

    def open(self):
        self.fe = new_fe(**self.fe_args) if not self.fe_args.get("raw") else FrontEnd(**{k: v for k, v in self.fe_args.items() if k != "raw"})
        self.graph = PoseGraph()
        self.slam = Slam(self.fe, self.graph, **self.params)

    def close(self):
        self.slam.close(); self.graph.close(); self.fe.close()

    def through_a_file(self, path, clouds=False):
        self.fe.save_session(path, self.slam, self.graph, clouds=clouds)
        self.close()
        self.open()   # (the strategy comes with the file)
        self.fe.load_session(path, self.slam, self.graph)


def lockstep_with_cuts(tmp_path, frames, strategy, params, cut_after, before_step=None, icp=None, emm=None, clouds=False, **fe_args):
    """tests/test_gpu_slam_step.py's lockstep with the library cut where cut_after(slot, record) says so: the oracle runs
    uninterrupted, the library goes through a file into fresh objects.  After every step and after every cut: the step record
    with chi2 and the LM iterations, the graph, the slot table and the counters of every resident node, byte for byte.
    Returns (oracle, its steps, the library's records, the slots after which it was cut, the session)."""
    ses = Session(params, strategy, **fe_args)
    oracle = so.SlamOracle(lambda new, slots: ses.fe.match_node_pairs(new, slots), strategy=strategy, icp=icp and (lambda n, s: icp(ses, n, s)),
                           emm=emm and (lambda n, s, r: emm(ses, n, s, r)), **params)
    want, got, cuts = [], [], []

    def same_everything(where):
        sq.same_state(ses.slam, ses.graph, oracle)
        for i, s in enumerate(oracle.slots):
            if s >= 0:
                assert ses.fe.node_feature_stats(s).tobytes() == oracle.stats[i].tobytes(), (where, i)

    try:
        for slot, f in enumerate(frames):
            ses.fe.upload_node(slot, f["desc"], f["xyz1"])
            if before_step:
                before_step(ses, slot)
            want.append(oracle.add_node(slot, len(f["desc"]), f["stamp"]))
            got.append(ses.slam.add_node(slot, f["stamp"]))
            sq.same_step(got[-1], want[-1])
            same_everything(slot)
            if cut_after(slot, got[-1]):
                ses.through_a_file(str(tmp_path / ("cut%02d.session" % slot)), clouds=clouds)
                cuts.append(slot)
                same_everything(("cut", slot))
    except BaseException:
        ses.close()
        raise
    return oracle, want, got, cuts, ses


@pytest.mark.parametrize("name", ["main, first, clear_non_keyframes", "main, largest_loop, clear_non_keyframes"])
def test_resume_under_the_oracle(tmp_path, name):
    run = sq.RUNS[name]
    frames = run["frames"]()
    seen_clear = []

    def cut_after(slot, rec):
        first_clear = rec.cleared_first >= 0 and not seen_clear
        if first_clear:
            seen_clear.append(slot)
        return slot == 1 or first_clear or slot == len(frames) - 2

    oracle, want, got, cuts, ses = lockstep_with_cuts(tmp_path, frames, run["strategy"], dict(run["params"], optimizer_skip_step=1), cut_after)
    try:
        assert len(cuts) >= 3 and cuts[0] == 1 and cuts[-1] == len(frames) - 2
        # (conditions on the run) a cut lies behind a step that cleared non-keyframes: released slots and -1 entries travel ...
        assert seen_clear and seen_clear[0] in cuts and -1 in oracle.slots
        # ... and every cut lies before an optimisation that moves an estimate
        for c in cuts:
            assert any(g.optimized and g.lm_iterations > 0 for g in got[c + 1:]), c
        assert any(o.any() for o in oracle.stats.values())
    finally:
        ses.close()


def test_restored_nodes_match_as_before(tmp_path, orb):
    """The nodes of the read-back fixture through a file into a context with more slots: the pair records of before the save,
    and the same downloads (features, keypoints and counters)."""
    fe, nodes = orb
    q, t = np.array([23, 23, 2, 5, 11, 7], np.int32), np.array([5, 2, 11, 11, 23, 0], np.int32)
    before = fe.match_pair_list(q, t)
    path = str(tmp_path / "nodes.session")
    fe.save_session(path)
    big = new_fe(max_nodes=40)
    try:
        big.load_session(path)
        assert big.match_pair_list(q, t).tobytes() == before.tobytes() and (before["n_inl"] > 0).any()
        a, b = fe.download_nodes(ASK), big.download_nodes(ASK)
        for f in ("desc", "xyz1", "kp_xy", "stats", "row_offsets", "kinds", "has_keypoints"):
            assert a[f].tobytes() == b[f].tobytes(), f
        assert b["stats"].any() and b["kp_xy"].any()
        again = str(tmp_path / "again.session")
        big.save_session(again)
        assert open(again, "rb").read() == open(path, "rb").read()   # save(load(f)) == f, slots and max_nodes notwithstanding
    finally:
        big.close()


# ---- clouds: tests/test_gpu_slam_step.py's six frames with the ICP fallback and the measurement model inside the step ---------
EMM_SKIP_STEP, OBSERVABILITY_THRESHOLD, MIN_DEPTH = 8, 0.6, 0.1
CLOUD_FE = dict(raw=True, device_id=0, max_nodes=16, max_keypoints=512, max_pairs_per_batch=64)
CLOUD_PARAMS = dict(min_matches=5, use_icp=1, observability_threshold=OBSERVABILITY_THRESHOLD, emm__skip_step=EMM_SKIP_STEP, optimizer_skip_step=1)


def cloud_frames():
    seq = synth.make_sequence(n_frames=6, n_kp=300, n_world=1200, seed=7)
    other = synth.make_sequence(n_frames=1, n_kp=300, n_world=1200, seed=99)
    rows = [300, 300, 5, 300, 5, 300]
    frames = []
    for k in range(6):
        src, j = (other, 0) if k == 0 else (seq, k)
        frames.append(dict(desc=src["desc"][j][:rows[k]].copy(), xyz1=src["xyz1"][j][:rows[k]].copy(), stamp=sq.stamp(k)))
    poses = [seq["poses"][k].copy() for k in range(6)]
    poses[1] = poses[1] @ io.rigid([0, 0, 0], [0, 0, -0.6])
    return frames, [io.corner_depth(64, 48, p)[0] for p in poses], io.corner_depth(64, 48)[1]


def icp_of(ses, new, slots):
    T, rep = ses.fe.icp_align_nodes(slots, [new] * len(slots))
    return [(bool(r["converged"]), t) for r, t in zip(rep, T)]


def emm_of(ses, new, slots, recs):
    r = np.zeros(len(recs), _lib.RESULT_DTYPE)
    for k, rec in enumerate(recs):
        r[k]["id1"], r[k]["id2"], r[k]["trafo"] = rec["id1"], rec["id2"], rec["trafo"]
    return [bool(m) for m in ses.fe.pairwise_observation_likelihood(r, OBSERVABILITY_THRESHOLD, EMM_SKIP_STEP)[1]]


def test_clouds_travel_with_the_flag(tmp_path):
    frames, depth, K = cloud_frames()
    cloud = lambda ses, slot: ses.fe.upload_node_cloud(slot, depth[slot], *K, min_depth=MIN_DEPTH, cloud_skip=1)
    kept = {}

    def cut_after(slot, rec):
        return slot == 3

    def before_step(ses, slot):
        if slot == 4:   # right behind the cut: the restored clouds against the ones an upload builds
            for s in range(4):
                kept[s] = (ses.fe.node_cloud(s).tobytes(), ses.fe.node_cloud_info(s))
        cloud(ses, slot)

    oracle, want, got, cuts, ses = lockstep_with_cuts(tmp_path, frames, "first", CLOUD_PARAMS, cut_after, before_step=before_step, icp=icp_of,
                                                      emm=emm_of, clouds=True, **CLOUD_FE)
    try:
        assert cuts == [3] and oracle.slots == list(range(6)) and want[5]["candidates"] == [3, 2, 1, 0, 4]
        # the last frame's verdicts need the restored clouds of nodes 3 and 1 (measurement model) -- node 4's is its own upload
        assert want[5]["verdicts"] == [so.V_ACCEPTED, so.V_NO_EDGE, so.V_WITHDRAWN, so.V_NO_EDGE, so.V_ACCEPTED | so.V_ICP]
        fresh = FrontEnd(**{k: v for k, v in CLOUD_FE.items() if k != "raw"})
        try:
            for s in range(4):
                fresh.upload_node_cloud(s, depth[s], *K, min_depth=MIN_DEPTH, cloud_skip=1)
                assert kept[s][0] == fresh.node_cloud(s).tobytes(), s
                assert kept[s][1] == fresh.node_cloud_info(s) and kept[s][1]["rows"] == 48 and kept[s][1]["cloud_skip"] == 1
        finally:
            fresh.close()
    finally:
        ses.close()


def test_without_the_flag_no_cloud_travels(tmp_path):
    """The load succeeds; a step that needs an older node's cloud reports RGBDFE_ERR_UNKNOWN_NODE, as for a node without one."""
    frames, depth, K = cloud_frames()
    ses = Session(CLOUD_PARAMS, "first", **CLOUD_FE)
    try:
        for slot in range(4):
            ses.fe.upload_node(slot, frames[slot]["desc"], frames[slot]["xyz1"])
            ses.fe.upload_node_cloud(slot, depth[slot], *K, min_depth=MIN_DEPTH, cloud_skip=1)
            ses.slam.add_node(slot, frames[slot]["stamp"])
        slots_before = ses.slam.slots()
        ses.through_a_file(str(tmp_path / "no_clouds.session"), clouds=False)
        assert ses.slam.slots() == slots_before
        with pytest.raises(RgbdfeError):
            ses.fe.node_cloud(3)
        ses.fe.upload_node(4, frames[4]["desc"], frames[4]["xyz1"])
        ses.fe.upload_node_cloud(4, depth[4], *K, min_depth=MIN_DEPTH, cloud_skip=1)
        with pytest.raises(RgbdfeError) as e:   # five rows: no RANSAC edge to the adjacent node 3, so ICP is asked -- for a cloud that is gone
            ses.slam.add_node(4, frames[4]["stamp"])
        assert "unknown node" in str(e.value)
    finally:
        ses.close()


@pytest.mark.parametrize("detector", ["ORB", "FAST"])
def test_a_detector_continues_from_a_file(tmp_path, detector):
    seq = synth.make_image_sequence(n_frames=4, width=320, height=240, seed=3)
    K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
    a, b = new_fe(max_nodes=4, max_keypoints=600), new_fe(max_nodes=4, max_keypoints=600)
    try:
        a.detector_configure(max_keypoints=300, grid_resolution=3, adjuster_max_iterations=5)
        a.set_detector_type(detector)
        a.set_feature_min_depth(True)
        for k in range(2):
            a.detect_describe(seq["gray"][k], seq["mask"][k], seq["depth"][k], *K)
        path = str(tmp_path / "detector.session")
        a.save_session(path)
        b.load_session(path)   # an unconfigured context: type, configuration and thresholds come from the file
        assert b.detector_thresholds().tobytes() == a.detector_thresholds().tobytes() and (a.detector_thresholds() != 20.0).any()
        for k in (2, 3):
            ra = a.detect_describe(seq["gray"][k], seq["mask"][k], seq["depth"][k], *K)
            rb = b.detect_describe(seq["gray"][k], seq["mask"][k], seq["depth"][k], *K)
            assert len(ra[0]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb)), k
            assert a.detector_thresholds().tobytes() == b.detector_thresholds().tobytes()
    finally:
        a.close(); b.close()


# ---- file properties ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """A run with clouds on half of its nodes, cut short and saved twice.  Returns (path, bytes, the live session)."""
    d = tmp_path_factory.mktemp("saved")
    frames = sq.main_sequence()[:6]
    depth, K = io.corner_depth(64, 48)[:2]
    ses = Session(dict(sq.SPARSE, optimizer_skip_step=1), "largest_loop")
    for slot, f in enumerate(frames):
        ses.fe.upload_node(slot, f["desc"], f["xyz1"])
        if slot % 2 == 0:
            ses.fe.upload_node_cloud(slot, depth, *K, min_depth=MIN_DEPTH, cloud_skip=2)
        ses.slam.add_node(slot, f["stamp"])
    ses.fe.upload_node_keypoints(5, np.arange(2 * ses.fe.node_count(5), dtype=np.float32).reshape(-1, 2))
    path = str(d / "run.session")
    ses.fe.save_session(path, ses.slam, ses.graph, clouds=True)
    data = open(path, "rb").read()
    yield path, data, ses
    ses.close()


def state_bytes(tmp_path, fe, slam=None, graph=None):
    """Everything a load could change, as the bytes a save of it gives."""
    p = str(tmp_path / "state.session")
    fe.save_session(p, slam, graph, clouds=True)
    return open(p, "rb").read()


def test_saving_twice_and_saving_what_was_loaded(tmp_path, saved):
    path, data, ses = saved
    assert state_bytes(tmp_path, ses.fe, ses.slam, ses.graph) == data
    assert not os.path.exists(path + ".tmp")
    other = Session(ses.params, max_nodes=30)
    try:
        other.fe.load_session(path, other.slam, other.graph)
        assert state_bytes(tmp_path, other.fe, other.slam, other.graph) == data
    finally:
        other.close()


def test_a_reader_written_from_the_header_finds_what_the_getters_report(saved):
    path, data, ses = saved
    f = sfile.read(data)
    fe = ses.fe
    assert [t for t, _, _ in f["table"]] == sfile.ORDER and f["flags"] == sfile.CLOUDS
    assert f["max_keypoints"] == 130 and f["abi"] == _lib.load().rgbdfe_abi_version() and f["kinds"] == 1
    assert f["dete"]["thresholds"].tobytes() == fe.detector_thresholds().tobytes() and f["dete"]["grid"] == 3 and f["dete"]["type"] == 0
    resident = [s for s in range(24) if fe.node_count(s) >= 0]
    assert sorted(f["nodes"]) == resident and len(resident) >= 3
    for i in resident:
        one = fe.download_nodes([i])
        n = f["nodes"][i]
        assert (n["kind"], n["rows"], n["has_kp"]) == (0, fe.node_count(i), int(i == 5))
        for key in ("desc", "xyz1", "kp_xy", "stats"):
            assert n[key] == one[key].tobytes(), (i, key)
        assert n["stats"] == fe.node_feature_stats(i).tobytes()
    assert any(any(n["stats"]) for n in f["nodes"].values())
    with_cloud = [s for s in resident if s % 2 == 0]
    assert sorted(f["clouds"]) == [s for s in with_cloud if _has_cloud(fe, s)] and f["clouds"]
    for i, c in f["clouds"].items():
        info = fe.node_cloud_info(i)
        assert {k: c[k] for k in info} == info and c["points"] == fe.node_cloud(i).tobytes()
    assert f["graph"] == ses.graph.serialize() and f["slam"] == ses.slam.serialize()
    # the two strings, read from their description: the graph's nodes, edges and keyframes; the machine's slot table
    g = f["graph"]
    strategy, earliest, n_nodes, n_edges, n_kf = struct.unpack_from("<iiIII", g, 24)
    assert g[:8] == b"RGBDFEPG" and zlib.crc32(g[16:]) == struct.unpack_from("<I", g, 12)[0]
    assert strategy == _lib.POSE_RELATIVE_TO["largest_loop"] and n_nodes == ses.slam.node_count() == len(ses.graph.node_ids())
    for k in range(n_nodes):
        i, v, matchable, fixed = struct.unpack_from("<iiBB", g, 56 + 112 * k)
        X = ses.graph.get_estimate(i)
        assert g[56 + 112 * k + 16:56 + 112 * (k + 1)] == X[:3, :3].tobytes() + X[:3, 3].tobytes() and bool(fixed) == ses.graph.get_fixed(i)
    at = 56 + 112 * n_nodes
    for k in range(n_edges):
        e = ses.graph.edge(k)
        i, j, active = struct.unpack_from("<iiB", g, at + 400 * k)
        assert (i, j, bool(active)) == (e["id1"], e["id2"], e["active"]) and g[at + 400 * k + 112:at + 400 * (k + 1)] == e["information"].tobytes()
    assert list(struct.unpack_from("<%di" % n_kf, g, at + 400 * n_edges)) == ses.slam.keyframes()
    s = f["slam"]
    n = struct.unpack_from("<I", s, 24 + 232)[0]
    assert s[:8] == b"RGBDFESM" and n == ses.slam.node_count()
    assert list(struct.unpack_from("<%di" % n, s, 24 + 232 + 40)) == ses.slam.slots()


def _has_cloud(fe, node_id):
    try:
        fe.node_cloud_info(node_id)
        return True
    except RgbdfeError:
        return False


def test_a_load_that_is_refused_changes_nothing(tmp_path, saved):
    path, data, ses = saved
    flags, table = sfile.chunk_table(data)
    bad = {}
    for tag, off, n in table[:-1]:
        b = bytearray(data)
        b[off + n // 2] ^= 0x10
        bad["CRC mismatch in chunk " + tag.decode()] = bytes(b)
    bad["shorter than"] = data[:20]
    bad["length field"] = data[:len(data) - 24]
    b = bytearray(data); struct.pack_into("<I", b, 8, 2); bad["unknown version"] = bytes(b)
    b = bytearray(data); struct.pack_into("<Q", b, 16, len(data) - 8); bad["length field#"] = bytes(b)
    target = Session(ses.params, max_nodes=30)
    try:
        target.fe.upload_node(50, np.zeros((3, 32), np.uint8), np.ones((3, 4), np.float32))   # something of its own, no id of the file
        before = state_bytes(tmp_path, target.fe, target.slam, target.graph)
        for cause, blob in bad.items():
            p = tmp_path / "bad.session"
            p.write_bytes(blob)
            st = target.fe._L.rgbdfe_session_load(target.fe._ctx, target.slam._s, target.graph._g, str(p).encode())
            assert st == INVALID_ARG and cause.split("#")[0] in target.fe._L.rgbdfe_last_error(target.fe._ctx).decode(), cause
            assert state_bytes(tmp_path, target.fe, target.slam, target.graph) == before, cause
        # the id rule: an id of the file that is already resident; a graph that is not empty; a slam with other parameters
        resident_id = sorted(sfile.read(data)["nodes"])[-1]
        target.fe.upload_node(resident_id, np.zeros((3, 32), np.uint8), np.ones((3, 4), np.float32))
        before = state_bytes(tmp_path, target.fe, target.slam, target.graph)
        load = lambda slam, graph: target.fe._L.rgbdfe_session_load(target.fe._ctx, slam._s if slam else None, graph._g if graph else None, path.encode())
        message = lambda: target.fe._L.rgbdfe_last_error(target.fe._ctx).decode()
        assert load(target.slam, target.graph) == INVALID_ARG and "already resident" in message()
        assert state_bytes(tmp_path, target.fe, target.slam, target.graph) == before
        target.fe.release_node(resident_id)
        other_graph = PoseGraph()
        other_graph.add_node(0)
        other = Slam(target.fe, other_graph, **target.params)
        assert load(other, other_graph) == INVALID_ARG and "not empty" in message()
        differing = Slam(target.fe, target.graph, **dict(target.params, min_matches=33))
        assert load(differing, target.graph) == INVALID_ARG and "min_matches" in message()
        before = state_bytes(tmp_path, target.fe, target.slam, target.graph)
        other.close(); differing.close(); other_graph.close()
        # capacity: rows above max_keypoints; more nodes than free slots
        for args in (dict(max_keypoints=64), dict(max_nodes=2)):
            small = new_fe(**args)
            try:
                g = PoseGraph()
                s = Slam(small, g, **target.params)
                st = small._L.rgbdfe_session_load(small._ctx, s._s, g._g, path.encode())
                assert st == CAPACITY and small._L.rgbdfe_last_error(small._ctx).decode() != "", args
                assert g.node_count() == 0 and len(g.node_ids()) == 0 and s.node_count() == 0 and all(small.node_count(i) < 0 for i in range(24))
                s.close(); g.close()
            finally:
                small.close()
        # and the good file still goes in
        assert load(target.slam, target.graph) == 0
    finally:
        target.close()


def test_saving_into_a_directory_that_does_not_exist(tmp_path, saved):
    path, data, ses = saved
    p = str(tmp_path / "no_such_directory" / "run.session")
    st = ses.fe._L.rgbdfe_session_save(ses.fe._ctx, ses.slam._s, ses.graph._g, 1, p.encode())
    assert st == INVALID_ARG and "cannot open" in ses.fe._L.rgbdfe_last_error(ses.fe._ctx).decode()
    assert not os.path.exists(p) and not os.path.exists(p + ".tmp") and os.listdir(tmp_path) == []


def test_a_pruned_graph_keeps_its_inactive_slots(saved):
    """Pruning runs on the device: an edge it removed stays in its slot, inactive, through a string."""
    path, data, ses = saved
    og, n_good, calls = pe.verdict_case("removed")
    g = PoseGraph()
    g.set_strategy("first")
    for v in range(og.n):
        g.add_node(v)
        X = np.eye(4)
        X[:3, :3], X[:3, 3] = og.R[v], og.t[v]
        g.set_estimate(v, X)
    g.set_fixed(0, True)
    for e in range(len(og.ei)):
        g.add_edge_se3(og.ei[e], og.ej[e], og.edge(e)["transform"], og.Om[e])
    pruned, verdicts = g.prune_edges(ses.fe, calls[0][0])
    assert pruned == 1 and verdicts[-1] == pe.REMOVED
    h = PoseGraph()
    h.deserialize(g.serialize())
    assert [h.edge(e)["active"] for e in range(len(og.ei))] == [True] * n_good + [False] and h.serialize() == g.serialize()
    assert h.chi2(ses.fe) == g.chi2(ses.fe)
    g.close(); h.close()


# ---- the C++ header ----------------------------------------------------------------------------------------------------
def test_the_headers_session_is_the_bindings(tmp_path):
    """include/rgbdfe.hpp's saveSession / loadSession / downloadNodes (tests/cpp/session_resume.cpp, plain g++, a child process)
    on the main sequence cut after 7 frames, against the binding doing the same: the files are equal byte for byte, and so
    are the steps after the cut, the keyframes, the slot table and the read-back of the resident nodes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "session_resume")
    lib = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "session_resume.cpp"),
                           "-o", exe, "-L" + lib, "-lrgbdfe", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    frames, cut, p = sq.main_sequence(), 7, sq.SPARSE
    with open(tmp_path / "frames.bin", "wb") as f:
        f.write(struct.pack("<i", len(frames)))
        for fr in frames:
            f.write(struct.pack("<iqi", len(fr["desc"]), fr["stamp"][0], fr["stamp"][1]) + fr["desc"].tobytes() + fr["xyz1"].tobytes())
    r = subprocess.run([exe, str(tmp_path / "frames.bin"), str(_lib.POSE_RELATIVE_TO["largest_loop"]), "1", str(p["clear_non_keyframes"]),
                        str(p["predecessor_candidates"]), str(p["neighbor_candidates"]), str(p["min_sampled_candidates"]), str(cut),
                        str(tmp_path / "cpp.session")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    # the header's slamParams() start from the defaults: create_cloud_every_nth_node stays 1 there
    params = dict({k: v for k, v in p.items() if k != "create_cloud_every_nth_node"}, optimizer_skip_step=1)
    ses = Session(params, "largest_loop")
    try:
        want = []
        for slot, fr in enumerate(frames):
            if slot == cut:
                ses.through_a_file(str(tmp_path / "py.session"))
            ses.fe.upload_node(slot, fr["desc"], fr["xyz1"])
            g = ses.slam.add_node(slot, fr["stamp"])
            want.append("%d %d %d %d %d %d %016x" % (g.status, g.id, g.keyframe_added, g.cleared_first, g.optimized, g.lm_iterations,
                                                     struct.unpack("<Q", struct.pack("<d", g.chi2))[0]))
        resident = [s for s in range(24) if ses.fe.node_count(s) >= 0]
        rows = ses.fe.download_nodes(resident)
        want += ["K " + " ".join(map(str, ses.slam.keyframes())), "T " + " ".join(map(str, ses.slam.slots())),
                 "D %d %d %d" % (len(resident), rows["row_offsets"][-1], int(rows["desc"].sum(dtype=np.uint64)) + int(rows["stats"].sum(dtype=np.uint64)))]
        assert open(tmp_path / "cpp.session", "rb").read() == open(tmp_path / "py.session", "rb").read()
        assert [l.rstrip() for l in r.stdout.splitlines()] == want
        assert -1 in ses.slam.slots() and rows["stats"].any()
    finally:
        ses.close()
