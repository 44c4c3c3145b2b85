"""-m gpu: the g2o refinement after RANSAC (params.g2o_iterations = "g2o_transformation_refinement"; node.cpp:1222-1268,
transformation_estimation.cpp:37-170) -- g2o_refine_kernel vs the oracle's restatement.  The kernel follows the oracle
operation by operation (same partial-sum order), so poses, inlier sets and errors are compared bit for bit, and within the
1e-4 pose tolerance of north_star."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rgbdslam_v2_amd import synth
from rgbdslam_v2_amd.frontend import inlier_indices

pytestmark = pytest.mark.gpu
K = (521.0, 521.0, 319.5, 239.5)  # transformation_estimation.cpp:56


def keypoints_of(xyz1, rng, noise=0.2):
    u = K[0] * xyz1[:, 0] / xyz1[:, 2] + K[2]
    v = K[1] * xyz1[:, 1] / xyz1[:, 2] + K[3]
    return (np.stack([u, v], 1) + rng.normal(0, noise, (len(xyz1), 2))).astype(np.float32)


@pytest.mark.parametrize("iters,mode", [(1, 0), (3, 1 << 20), (8, 1 << 20)])
def test_pairs_with_g2o_refinement_match_oracle(iters, mode):
    from rgbdslam_v2_amd.frontend import FrontEnd
    seq = synth.make_sequence(n_frames=10, n_kp=600, n_world=2000, seed=55, depth_noise=0.004)
    rng = np.random.default_rng(9)
    kps = [keypoints_of(seq["xyz1"][f], rng) for f in range(10)]
    seq["desc"][9] = rng.integers(0, 256, seq["desc"][9].shape, dtype=np.uint8)   # an unrelated node: no edge, no refinement
    fe = FrontEnd(device_id=0, max_nodes=12, max_keypoints=640, max_pairs_per_batch=64, g2o_iterations=iters)
    fe.set_latency_mode(mode, 0)
    for f in range(10):
        fe.upload_node(f, seq["desc"][f], seq["xyz1"][f])
        fe.upload_node_keypoints(f, kps[f])
    pq = np.array([1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 5], np.int32)
    pt = np.array([0, 1, 2, 0, 4, 3, 6, 7, 0, 8, 1], np.int32)
    out = fe.match_pair_list(pq, pt)
    plain = FrontEnd(device_id=0, max_nodes=12, max_keypoints=640, max_pairs_per_batch=64)
    plain.set_latency_mode(mode, 0)
    for f in range(10):
        plain.upload_node(f, seq["desc"][f], seq["xyz1"][f])
    base = plain.match_pair_list(pq, pt)
    plain.close()
    prm = po.default_params(seed=fe.params.seed, depth_cov=fe.params.depth_cov)
    changed = 0
    for rec, b, q, t in zip(out, base, pq, pt):
        ref = po.match_node_pair_g2o(seq["desc"][q], seq["xyz1"][q], kps[q], int(q), seq["desc"][t], seq["xyz1"][t], kps[t],
                                     int(t), iters, prm)
        assert rec["n_all"] == ref["n_all"] and rec["n_inl"] == ref["n_inl"], (q, t)
        assert (rec["id1"], rec["id2"]) == (ref["id1"], ref["id2"])
        assert np.array_equal(inlier_indices(rec), ref["inl_idx"])
        T = np.array(rec["trafo"], np.float32).reshape(4, 4).T
        assert np.abs(T - ref["T"]).max() <= 1e-4, (q, t, np.abs(T - ref["T"]).max())
        assert np.array_equal(T, ref["T"]) and rec["rmse"] == np.float32(ref["rmse"])
        assert rec["valid_iterations"] == ref["valid_iterations"]
        assert rec["info_scale"] == ref["info_scale"]
        changed += int(rec["valid_iterations"] != b["valid_iterations"])
        if rec["valid_iterations"] == b["valid_iterations"]:      # refinement not adopted: the RANSAC result stands
            assert rec.tobytes() == b.tobytes()
    assert changed >= 1, changed       # the refinement is adopted for some pairs (it must not lose inliers, :1252)
    assert out[9]["id1"] == -1
    fe.close()


def test_g2o_needs_keypoints():
    from rgbdslam_v2_amd._lib import RgbdfeError
    from rgbdslam_v2_amd.frontend import FrontEnd
    seq = synth.make_sequence(n_frames=3, n_kp=200, n_world=600, seed=1)
    fe = FrontEnd(device_id=0, max_nodes=4, max_keypoints=256, max_pairs_per_batch=8, g2o_iterations=2)
    for f in range(3):
        fe.upload_node(f, seq["desc"][f], seq["xyz1"][f])
    with pytest.raises(RgbdfeError, match="keypoints"):
        fe.match_pair_list([1], [0])
    with pytest.raises(RgbdfeError):
        fe.upload_node_keypoints(0, np.zeros((5, 2), np.float32))     # wrong count
    # keypoints belong to one upload of one node -- a re-upload, or a new node in a recycled slot, must not be
    # refined against the slot's previous KeyPoint.pt
    rng = np.random.default_rng(3)
    kps = [keypoints_of(seq["xyz1"][f], rng) for f in range(3)]
    for f in range(3):
        fe.upload_node_keypoints(f, kps[f])
    ok = fe.match_pair_list([1, 2], [0, 1])
    fe.upload_node(1, seq["desc"][1], seq["xyz1"][1])                  # re-upload in place: keypoints gone
    with pytest.raises(RgbdfeError, match="keypoints"):
        fe.match_pair_list([1], [0])
    fe.upload_node_keypoints(1, kps[1])
    assert fe.match_pair_list([1, 2], [0, 1]).tobytes() == ok.tobytes()
    fe.release_node(2)
    fe.upload_node(7, seq["desc"][2], seq["xyz1"][2])                  # a new node takes the recycled slot
    with pytest.raises(RgbdfeError, match="keypoints"):
        fe.match_pair_list([7], [1])
    fe.upload_node_keypoints(7, kps[2])
    fe.match_pair_list([7], [1])                                       # (another node id = another RANSAC stream)
    fe.release_node(7)
    fe.upload_node(2, seq["desc"][2], seq["xyz1"][2])                  # node 2 again, into the slot node 7 just left
    with pytest.raises(RgbdfeError, match="keypoints"):
        fe.match_pair_list([2], [1])
    fe.upload_node_keypoints(2, kps[2])
    assert fe.match_pair_list([1, 2], [0, 1]).tobytes() == ok.tobytes()
    fe.set_params(g2o_iterations=0)
    assert fe.match_pair_list([1], [0])["n_all"][0] > 0
    fe.close()


# ---- the planted cases of tests/g2o_cases.py, the fuzz, the float matchers, the submission paths ----------------------
import g2o_cases as gc  # noqa: E402

SCHEDULES = [((0, 0), "one_wave_per_pair"), ((1 << 20, 0), "record_replay")]
LEFT_ALONE = (po.G2O_NOT_RUN, po.G2O_REJECTED, po.G2O_ENTERED_NOT_ADOPTED)


@pytest.fixture(scope="module")
def fe_small():
    """The smallest context that holds every planted case: 8 nodes of up to 400 rows (capacity 448, a whole number of 64-row tiles), up to 24 pairs."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=8, max_keypoints=448, max_pairs_per_batch=24)
    yield f
    f.close()


def _upload(fe, nodes):
    for k, (d, x, kp) in enumerate(nodes):
        fe.upload_node(k, d, x)
        fe.upload_node_keypoints(k, kp)


def _run_case(fe, c):
    """The case's pairs on both schedules and with the refinement off: (records per schedule, RANSAC-only records)."""
    pq = np.array([p[0] for p in c["pairs"]], np.int32)
    pt = np.array([p[1] for p in c["pairs"]], np.int32)
    try:
        _upload(fe, c["nodes"])
        outs = []
        for mode, _ in SCHEDULES:
            fe.set_latency_mode(*mode)
            fe.set_params(g2o_iterations=c["iters"], **c["params"])
            outs.append(fe.match_pair_list(pq, pt))
        fe.set_params(g2o_iterations=0)
        plain = fe.match_pair_list(pq, pt)
        return outs, plain
    finally:
        fe.set_params(g2o_iterations=0, **gc.DEFAULTS)
        for k in range(len(c["nodes"])):
            fe.release_node(k)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_planted_cases_match_oracle(fe_small, name):
    """Every pair of every planted case (tests/g2o_cases.py; what each is for: DESIGN.md, "Two-view refinement: branches and
    the cases that reach them") against the oracle's full record, bit for bit, on both schedules; a pair whose refinement
    is not adopted -- a NaN pose included -- keeps the RANSAC record byte for byte."""
    c = gc.get(name)
    refs = gc.oracle_records(name)
    outs, plain = _run_case(fe_small, c)
    for out, (_, schedule) in zip(outs, SCHEDULES):
        for rec, base, ref, pair in zip(out, plain, refs, c["pairs"]):
            try:
                gc.check_record(rec, ref)
            except AssertionError as e:
                raise AssertionError("%s %s pair %s: %s" % (name, schedule, pair, e)) from e
            if ref["trace"]["outcome"] in LEFT_ALONE:
                assert rec.tobytes() == base.tobytes(), (name, schedule, pair)
            else:
                assert rec["valid_iterations"] == base["valid_iterations"] + 1
    assert outs[0].tobytes() == outs[1].tobytes()


def test_randomised_nodes_and_parameters_with_refinement():
    """test_randomised_nodes_and_parameters_match_oracle's fuzz with the refinement on (gc.fuzz_trials: node sizes from 0 to
    400, NaN / zero depths, unrelated and duplicated descriptors, keypoints 0 / 0.2 / 2 pixels off, 1 / 3 / 8 steps, random
    matching and RANSAC parameters): every pair equals the oracle bit for bit on both schedules, and the phased plan forced
    onto the batch gives the same bytes."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    fe = FrontEnd(device_id=0, max_nodes=8, max_keypoints=448, max_pairs_per_batch=24)
    try:
        refined = 0
        for trial, c in enumerate(gc.fuzz_trials()):
            refs = gc.records_of(c)
            pq = np.array([p[0] for p in c["pairs"]], np.int32)
            pt = np.array([p[1] for p in c["pairs"]], np.int32)
            _upload(fe, c["nodes"])
            fe.set_params(g2o_iterations=c["iters"], **c["params"])
            outs = []
            for mode in ((0, 0), (1 << 20, 0), (1 << 30, -5)):
                fe.set_latency_mode(*mode)
                outs.append(fe.match_pair_list(pq, pt))
            for out in outs[:2]:
                for rec, ref, pair in zip(out, refs, c["pairs"]):
                    try:
                        gc.check_record(rec, ref)
                    except AssertionError as e:
                        raise AssertionError("trial %d pair %s %s: %s" % (trial, pair, c["params"], e)) from e
            assert outs[2].tobytes() == outs[0].tobytes() == outs[1].tobytes(), trial
            refined += sum(r["trace"]["n_calls"] for r in refs)
            for k in range(len(c["nodes"])):
                fe.release_node(k)
        assert refined >= 10
    finally:
        fe.close()


@pytest.mark.parametrize("matcher", ["sift", "flann"])
def test_refinement_behind_the_float_matchers(matcher):
    """launch_g2o_refine after launch_select_ransac_sift / ..._sift_latency (api_batches.hip: the float matchers' branch): the
    PairPrep that the refinement reads is written by the list path's prep.  Resident SIFT nodes and FLANN float nodes with
    keypoints, 3 steps, records and distance lists against the oracle's float pair followed by its refinement block."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    c = gc.float_case()
    refs = gc.float_records(matcher, c)
    outcomes = [r["trace"]["outcome"] for r in refs]
    assert any(o >= po.G2O_ADOPTED for o in outcomes) and any(o in (po.G2O_REJECTED, po.G2O_ENTERED_NOT_ADOPTED) for o in outcomes)
    assert outcomes[-2:] == [po.G2O_NOT_RUN] * 2                                   # the unrelated frame
    pq = np.array([p[0] for p in c["pairs"]], np.int32)
    pt = np.array([p[1] for p in c["pairs"]], np.int32)
    fe = FrontEnd(device_id=0, max_nodes=8, max_keypoints=320, max_pairs_per_batch=16, g2o_iterations=c["iters"])
    try:
        for k, (d, x, kp) in enumerate(c["nodes"]):
            (fe.upload_sift_node if matcher == "sift" else fe.upload_float_node)(k, d, x)
            fe.upload_node_keypoints(k, kp)
        run = fe.match_sift_pair_list if matcher == "sift" else fe.match_flann_pair_list
        results = []
        for mode, schedule in SCHEDULES:
            fe.set_latency_mode(*mode)
            out, dist = run(pq, pt)
            for rec, dd, ref, pair in zip(out, dist, refs, c["pairs"]):
                try:
                    gc.check_record(rec, ref, hd=False)
                    assert np.array_equal(dd[: ref["n_all"]], ref["all_dist"])
                except AssertionError as e:
                    raise AssertionError("%s %s pair %s: %s" % (matcher, schedule, pair, e)) from e
            results.append(out.tobytes() + dist.tobytes())
        assert results[0] == results[1]
        fe.set_params(g2o_iterations=0)
        plain, _ = run(pq, pt)
        for rec, base, o in zip(out, plain, outcomes):
            assert (rec.tobytes() == base.tobytes()) == (o in LEFT_ALONE)
    finally:
        fe.close()


def test_refinement_through_tickets_and_with_graph_capture(monkeypatch):
    """With the refinement on, two submit_pair_list batches in flight give the bytes of the synchronous call; and a context
    created with RGBDFE_GRAPHS=1 gives them again while capturing nothing: `graphable` requires g2o_iterations == 0, so the
    chain goes out as plain launches."""
    import torch
    from rgbdslam_v2_amd.frontend import FrontEnd, RESULT_DTYPE
    c = gc.get("adopt_mix_a")
    refs = gc.oracle_records("adopt_mix_a")
    pq = np.array([p[0] for p in c["pairs"]], np.int32)
    pt = np.array([p[1] for p in c["pairs"]], np.int32)

    def run(graphs):
        monkeypatch.setenv("RGBDFE_GRAPHS", "1" if graphs else "0")
        fe = FrontEnd(device_id=0, max_nodes=8, max_keypoints=320, max_pairs_per_batch=24, g2o_iterations=c["iters"])
        try:
            assert fe.graph_stats()["enabled"] == (1 if graphs else 0)
            _upload(fe, c["nodes"])
            sync = fe.match_pair_list(pq, pt)
            bufs = [torch.zeros(len(pq) * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2)]
            tickets = [fe.submit_pair_list(pq, pt, b.data_ptr()) for b in bufs]
            outs = []
            for tk, b in zip(tickets, bufs):
                fe.wait_ticket(tk, None)
                outs.append(b.cpu().numpy().tobytes())
            again = fe.match_pair_list(pq, pt)
            return sync, outs, again, fe.graph_stats()
        finally:
            fe.close()

    sync, outs, again, st = run(False)
    for rec, ref in zip(sync, refs):
        gc.check_record(rec, ref)
    assert outs[0] == outs[1] == sync.tobytes() == again.tobytes()
    g_sync, g_outs, g_again, g_st = run(True)
    assert g_sync.tobytes() == sync.tobytes() and g_outs[0] == g_outs[1] == sync.tobytes() == g_again.tobytes()
    assert g_st["enabled"] == 1 and g_st["launches"] == 0 and g_st["captures"] == 0, g_st
    assert sum(r["trace"]["outcome"] >= po.G2O_ADOPTED for r in refs) >= 5
