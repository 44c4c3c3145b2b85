"""GPU: rgbdfe_slam_add_node on the planted sequences of tests/slam_sequence.py against tests/slam_step_oracle.py, whose
pairs are the device's own pair op (tests/test_gpu_pairs.py holds that against the CPU oracle): after every frame the step
record (times aside), the graph's edges, flags and estimates, the keyframes, valid_tf, the slot table and the
feature_matching_stats_ of every resident node, byte for byte.  The conditions on the sequences (a loop closure, keyframes,
rejected candidates, cleared nodes ...) are checked on the CPU by tests/test_oracle_slam_step.py.  Then the same call against
rgbdfe_slam_begin / _feed driven by hand, the same comparison with the optimiser on under both strategies (the oracle optimises
through tests/pose_graph_eval_oracle.py), the convention guard, the ICP fallback and the measurement model inside the step on
nodes with clouds, and one run from images to a map."""
import numpy as np
import pytest

import icp_oracle as io
import slam_sequence as sq
import slam_step_oracle as so
from rgbdslam_v2_amd import _lib, synth
from rgbdslam_v2_amd.candidates import PoseGraph
from rgbdslam_v2_amd.frontend import FrontEnd, GraphManager, Node, Slam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(device_id=0, max_nodes=24, max_keypoints=130, max_pairs_per_batch=16)   # (130: a slot's counters end inside a word)
    yield f
    f.close()


def release_all(fe, slots):
    for s in slots:
        if fe.node_count(s) >= 0:
            fe.release_node(s)


def lockstep(fe, name=None, frames=None, strategy=None, params=None, before_step=None, icp=None, emm=None, **more):
    """A run (by its name in sq.RUNS, or given): every frame is uploaded into the slot of its index, the oracle steps first
    (its pairs need the nodes a step may release), then the library; after every step the step record with chi2 and the
    Levenberg-Marquardt iterations, the graph's edges, estimates and fixed flags, keyframes, valid_tf, the slot table and the
    counters of every resident node, byte for byte.  Returns (frames, oracle, its steps, the library's records, slam, graph)."""
    if name is not None:
        run = sq.RUNS[name]
        frames, strategy, params = run["frames"](), run["strategy"], run["params"]
    params = dict(params, **more)
    oracle = so.SlamOracle(lambda new, slots: fe.match_node_pairs(new, slots), strategy=strategy, icp=icp, emm=emm, **params)
    graph = PoseGraph()
    graph.set_strategy(strategy)
    slam = Slam(fe, graph, **params)
    want, got = [], []
    for slot, f in enumerate(frames):
        fe.upload_node(slot, f["desc"], f["xyz1"])
        assert not fe.node_feature_stats(slot).any()
        if before_step:
            before_step(slot)
        want.append(oracle.add_node(slot, len(f["desc"]), f["stamp"]))
        got.append(slam.add_node(slot, f["stamp"]))
        sq.same_step(got[-1], want[-1])
        sq.same_state(slam, graph, oracle)
        for i, s in enumerate(oracle.slots):
            if s >= 0:
                assert fe.node_feature_stats(s).tobytes() == oracle.stats[i].tobytes(), (slot, i)
        accepted_inliers = any(v == so.V_ACCEPTED for v in want[-1]["verdicts"] + [want[-1]["initial_verdict"]])
        assert got[-1].stats_launches == int(accepted_inliers)   # one launch per step, none without an accepted RANSAC pair
    return frames, oracle, want, got, slam, graph


@pytest.mark.parametrize("name", list(sq.RUNS))
def test_add_node_gives_the_oracles_run(fe, name):
    frames, oracle, want, got, slam, graph = lockstep(fe, name, optimizer_skip_step=0)
    assert any(o.any() for o in oracle.stats.values()) or name == "weak first"
    if "clear" in name:   # a cleared node's slot is free again, its cloudless features gone
        assert all(fe.node_count(s) < 0 for s, f in enumerate(frames) if s not in oracle.slots and want[s]["status"] == so.ADDED)
    slam.close()
    release_all(fe, range(len(frames)))


def test_add_node_is_begin_and_feed_by_hand(fe):
    frames = sq.main_sequence()
    graph, hand_graph = PoseGraph(), PoseGraph()
    for g in (graph, hand_graph):
        g.set_strategy("largest_loop")
    slam, hand = Slam(fe, graph, optimizer_skip_step=0, **sq.SPARSE), Slam(None, hand_graph, optimizer_skip_step=0, **sq.SPARSE)
    for slot, f in enumerate(frames):
        fe.upload_node(slot, f["desc"], f["xyz1"])
        ids, rec = hand.begin(slot, len(f["desc"]), f["stamp"])
        while rec is None:
            live = [i for i in ids if hand.slot_of(i) >= 0]
            by_id = dict(zip(live, fe.match_node_pairs(slot, [hand.slot_of(i) for i in live]))) if live else {}
            ids, rec = hand.feed(sq.compact_of_fields([by_id.get(i) for i in ids]))
        got = slam.add_node(slot, f["stamp"])
        for name, _ in rec.raw._fields_:
            if name not in ("seconds", "stats_launches"):
                a, b = getattr(got.raw, name), getattr(rec.raw, name)
                assert (a == b) if isinstance(a, (int, float)) else (bytes(a) == bytes(b)), (slot, name)
    assert slam.slots() == hand.slots() and slam.keyframes() == hand.keyframes() and slam.valid_tf() == hand.valid_tf()
    for i in range(slam.node_count()):
        assert graph.get_estimate(i).tobytes() == hand_graph.get_estimate(i).tobytes()
    slam.close(); hand.close()
    release_all(fe, range(len(frames)))


@pytest.mark.parametrize("skip", [1, 3])
@pytest.mark.parametrize("name", ["main, first", "main, first, clear_non_keyframes", "main, largest_loop, clear_non_keyframes"])
def test_with_the_optimiser_on_every_step_is_still_the_oracles(fe, name, skip):
    """The oracle optimises through tests/pose_graph_eval_oracle.py whenever a step is due: estimates, fixed flags, chi2 and the
    iteration count after every step, byte for byte (lockstep), under first and under largest_loop -- whose fixation reads
    the earliest_loop_closure_node the step writes.  And the convention guard: the last base frame's estimate against its
    synthetic pose relative to node 0, and the revisit of frame 0 against the origin, below 0.05 x the path length."""
    frames, oracle, want, got, slam, graph = lockstep(fe, name, optimizer_skip_step=skip)
    due = [w["optimize_due"] for w in want if w["status"] == so.ADDED]
    assert due == [int((k + 2) % skip == 0) for k in range(len(due))] and all(g.optimized == w["optimize_due"] for g, w in zip(got, want))
    assert any(g.optimized and g.lm_iterations > 0 for g in got)
    if "largest_loop" in name:   # (a condition on the run) some optimisation had fixed vertices behind the earliest loop closure
        assert len(oracle.keyframes) >= 3
    if name == "main, first":
        in_graph = [frames[s] for s in oracle.slots]
        truth = np.linalg.inv(in_graph[0]["pose"]) @ in_graph[-2]["pose"]
        bound = 0.05 * sq.path_length(in_graph[:-1])
        assert np.linalg.norm(graph.get_estimate(len(in_graph) - 2)[:3, 3] - truth[:3, 3]) < bound
        assert np.linalg.norm(graph.get_estimate(len(in_graph) - 1)[:3, 3]) < bound   # the revisit of frame 0
    slam.close()
    release_all(fe, range(len(frames)))


# ---- matchNodePair's chain behind the pair op: the ICP fallback and the measurement model on nodes with 64 x 48 clouds ---------
EMM_SKIP_STEP, OBSERVABILITY_THRESHOLD, MIN_DEPTH = 8, 0.6, 0.1


def cloud_frames():
    """Six frames with room-corner clouds seen from their poses (tests/test_gpu_cpp_mapping.py plants the same): node 0 has
    unrelated features, nodes 2 and 4 five rows (no RANSAC transformation against them), node 1's cloud is the room from
    0.6 m further back (the measurement model contradicts its edges)."""
    seq = synth.make_sequence(n_frames=6, n_kp=300, n_world=1200, seed=7)
    other = synth.make_sequence(n_frames=1, n_kp=300, n_world=1200, seed=99)
    rows = [300, 300, 5, 300, 5, 300]
    frames = []
    for k in range(6):
        src = other if k == 0 else seq
        j = 0 if k == 0 else k
        frames.append(dict(desc=src["desc"][j][:rows[k]].copy(), xyz1=src["xyz1"][j][:rows[k]].copy(), stamp=sq.stamp(k)))
    poses = [seq["poses"][k].copy() for k in range(6)]
    poses[1] = poses[1] @ io.rigid([0, 0, 0], [0, 0, -0.6])
    depth = [io.corner_depth(64, 48, p)[0] for p in poses]
    return frames, depth, io.corner_depth(64, 48)[1]


@pytest.mark.parametrize("use_icp,threshold", [(1, -0.6), (0, OBSERVABILITY_THRESHOLD), (1, OBSERVABILITY_THRESHOLD)],
                         ids=["icp", "measurement model", "both"])
def test_the_icp_fallback_and_the_measurement_model_inside_the_step(use_icp, threshold):
    """add_node with use_icp and / or observability_threshold > 0 against the oracle, whose ICP and measurement model are the
    binding's own entry points (tests/test_gpu_icp.py and tests/test_gpu_emm.py hold those against their oracles).  The last
    frame is compared with node 3 (a RANSAC edge the model keeps), 2 (five rows, not adjacent: nothing), 1 (a RANSAC edge
    the model withdraws), 0 (unrelated) and 4 (five rows, adjacent: served by ICP) -- tests/test_gpu_cpp_mapping.py::test_pairs
    establishes those outcomes for the same nodes."""
    frames, depth, K = cloud_frames()
    fe = FrontEnd(device_id=0, max_nodes=16, max_keypoints=512, max_pairs_per_batch=64)
    try:
        def icp(new, slots):
            T, rep = fe.icp_align_nodes(slots, [new] * len(slots))   # the OLDER cloud onto the new node's
            return [(bool(r["converged"]), t) for r, t in zip(rep, T)]

        def emm(new, slots, recs):
            r = np.zeros(len(recs), _lib.RESULT_DTYPE)
            for k, rec in enumerate(recs):
                r[k]["id1"], r[k]["id2"], r[k]["trafo"] = rec["id1"], rec["id2"], rec["trafo"]
            return [bool(m) for m in fe.pairwise_observation_likelihood(r, threshold, EMM_SKIP_STEP)[1]]

        cloud = lambda slot: fe.upload_node_cloud(slot, depth[slot], *K, min_depth=MIN_DEPTH, cloud_skip=1)
        _, oracle, want, got, slam, graph = lockstep(fe, frames=frames, strategy="first", before_step=cloud, icp=icp, emm=emm,
                                                     params=dict(min_matches=5, use_icp=use_icp, observability_threshold=threshold,
                                                                 emm__skip_step=EMM_SKIP_STEP, optimizer_skip_step=1))
        assert oracle.slots == list(range(6)) and want[5]["candidates"] == [3, 2, 1, 0, 4]
        icp_verdict = (so.V_ACCEPTED | so.V_ICP) if use_icp else so.V_NO_EDGE
        withdrawn = so.V_WITHDRAWN if threshold > 0 else so.V_ACCEPTED
        assert want[5]["verdicts"] == [so.V_ACCEPTED, so.V_NO_EDGE, withdrawn, so.V_NO_EDGE, icp_verdict], want[5]["verdicts"]
        if use_icp:   # an ICP edge carries 1e-2 I, never becomes the best result and touches no counter
            e = [graph.edge(k) for k in range(len(oracle.edges)) if oracle.edges[k][:2] == (4, 5)]
            assert len(e) == 1 and e[0]["information"].tobytes() == (np.eye(6) * 1e-2).tobytes() and want[5]["best_id1"] in (1, 3)
        print("verdicts per step:", [g.verdict_names for g in got])
        slam.close()
    finally:
        fe.close()


def test_update_inlier_features_on_a_batch_left_in_device_memory(fe):
    """The kernel through its own entry point: records of a pair batch in a device buffer, accept bytes from the host."""
    import torch
    base = sq.base()
    for k in range(4):
        fe.upload_node(k, base["desc"][k], base["xyz1"][k])
    q, t = np.array([3, 3, 3, 2], np.int32), np.array([0, 1, 2, 1], np.int32)
    recs = fe.match_pair_list(q, t)
    d = torch.empty(len(q) * recs.dtype.itemsize, dtype=torch.uint8, device="cuda")
    fe.match_pair_list_device(q, t, d.data_ptr())
    fe.synchronize()
    want = {k: np.zeros(128, np.uint8) for k in range(4)}
    for rounds, accept in enumerate([[1, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]]):
        assert fe.update_inlier_features(d.data_ptr(), q, t, accept) == int(any(accept))
        for r, a in zip(recs, accept):
            for m in (range(320) if a and r["id1"] >= 0 else []):
                if (int(r["inlier_mask"][m // 64]) >> (m % 64)) & 1:
                    want[int(r["id2"])][r["all_q"][m]] += 1
                    want[int(r["id1"])][r["all_t"][m]] += 1
        for k in range(4):
            assert fe.node_feature_stats(k).tobytes() == want[k].tobytes(), (rounds, k)
    assert want[3].max() >= 2 and (recs["n_inl"] > 0).all()   # (conditions on the frames) rows hit by several pairs
    fe.upload_node(3, base["desc"][3], base["xyz1"][3])   # a node uploaded into the slot starts from zero
    assert not fe.node_feature_stats(3).any() and fe.node_feature_stats(1).any()
    release_all(fe, range(4))


def test_from_images_to_a_map():
    """make_image_sequence -> sensor_detect_describe_batch_nodes (features and clouds into the slots) -> addNode -> the
    estimates of the nodes with a valid transform -> assemble_map: the cloud assembled from the oracle's poses."""
    seq = synth.make_image_sequence(n_frames=4, width=320, height=240, seed=3)
    fe = FrontEnd(device_id=0, max_nodes=8, max_keypoints=600, max_pairs_per_batch=16)
    try:
        fe.detector_configure(max_keypoints=600)
        K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
        feats = fe.sensor_detect_describe_batch_nodes(list(seq["gray"]), list(seq["depth"]), *K, node_ids=np.arange(4), cloud_skip=8)
        gm = GraphManager(fe, PoseGraph())
        gm.set_pose_relative_to("first")
        oracle = so.SlamOracle(lambda new, slots: fe.match_node_pairs(new, slots), strategy="first", optimizer_skip_step=0)
        gm.slam(optimizer_skip_step=0)
        for k in range(4):
            node = Node.__new__(Node)   # the features are resident already: no upload
            node.frontend, node.id_ = fe, k
            want = oracle.add_node(k, len(feats[k][1]), sq.stamp(k))
            rec = gm.firstNode(node, sq.stamp(k)) if k == 0 else gm.addNode(node, sq.stamp(k))
            sq.same_step(rec, want)
            print("frame %d: %s, %d rows, verdicts %s" % (k, rec.status_name, len(feats[k][1]), rec.verdict_names))
        slam = gm.slam()
        sq.same_state(slam, gm.pose_graph, oracle)
        ids = [i for i in range(slam.node_count()) if slam.valid_tf()[i]]
        assert len(ids) >= 2   # (a condition on the images: frames after the first find their predecessor)
        slots = [slam.slot_of(i) for i in ids]
        cloud = fe.assemble_map(slots, gm.pose_graph.transforms(ids))
        want_cloud = fe.assemble_map(slots, np.stack([oracle.estimates[i] for i in ids]).astype(np.float32))
        assert len(cloud) > 0 and cloud.tobytes() == want_cloud.tobytes()
        slam.close()
    finally:
        fe.close()
