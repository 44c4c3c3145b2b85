"""-m gpu: ORB detect / describe kernels + the grid-adaptive detector vs oracle/orb_oracle.c.
Keypoint coordinates, octaves, FAST/NMS decisions and descriptor bytes are integer work: exact.
Harris responses and angles are float, computed in the same operation order: asserted within 1e-6
relative AND bit-equal.  (The oracle itself restates OpenCV 3.3 from the published algorithm:
"parity unpinned" against a real OpenCV build.)"""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from oracle import pyorb
from rgbdslam_v2_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=4, max_keypoints=1024, max_pairs_per_batch=8)
    yield f
    f.close()


@pytest.fixture(scope="module")
def frames():
    return synth.make_image_sequence(n_frames=4, seed=3)


def assert_kps_equal(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "octave", "size"):
        assert np.array_equal(a[f], b[f]), f
    assert np.allclose(a["response"], b["response"], rtol=1e-6, atol=0)
    assert np.allclose(a["angle"], b["angle"], rtol=1e-6, atol=0)
    assert np.array_equal(a["response"], b["response"]) and np.array_equal(a["angle"], b["angle"])


@pytest.mark.parametrize("thr", [5, 20, 60])
@pytest.mark.parametrize("mask_kind", ["none", "binary", "depth"])
def test_orb_detect_matches_oracle(fe, frames, thr, mask_kind):
    g = frames["gray"][0]
    mask = None
    if mask_kind == "binary":
        mask = np.where(frames["mask"][0] > 0, 255, 0).astype(np.uint8)
    elif mask_kind == "depth":
        mask = frames["mask"][0]  # depth*100: levels >= 1 are wiped by threshold(254) (orb.cpp)
    kp = fe.orb_detect(g, mask, thr)
    ref = pyorb.detect(g, mask, thr)
    assert_kps_equal(kp, ref)
    assert len(kp) > (100 if thr < 60 else 10)
    if mask_kind == "depth":
        assert np.all(kp["octave"] == 0)


@pytest.mark.parametrize("kind,thr", [("noise", 1), ("noise", 40), ("binary", 0), ("binary", 254), ("ramp", 2), ("flat", 0),
                                      ("checker", 10)])
def test_orb_detect_on_adversarial_images(fe, kind, thr):
    """The fused FAST + NMS kernel and the LDS-patch measure kernel on images a camera never delivers: pure noise (a corner on
    almost every pixel: tens of thousands of scored corners, the second read-back of a crowded pass), saturated 0 / 255
    patterns (differences of +-255, thresholds at both ends of the range), ramps (long monotone arcs, score ties for the strict
    3x3 maximum), a flat image (nothing), a checkerboard (corners exactly on the 64 x 16 tile seams of several levels)."""
    rng = np.random.default_rng(9)
    h, w = 240, 330                                       # not a multiple of the tile sizes
    if kind == "noise":
        g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "binary":
        g = (rng.integers(0, 2, (h, w), dtype=np.uint8) * 255)
    elif kind == "ramp":
        g = ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 2) % 256).astype(np.uint8)
    elif kind == "flat":
        g = np.full((h, w), 77, np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        g = np.where(((xx // 16) + (yy // 16)) % 2 == 0, 40, 200).astype(np.uint8)
    mask = np.where(rng.random((h, w)) < 0.9, 255, 0).astype(np.uint8) if kind in ("noise", "checker") else None
    kp = fe.orb_detect(np.ascontiguousarray(g), mask, thr, capacity=200000)
    ref = pyorb.detect(np.ascontiguousarray(g), mask, thr, cap=200000)
    assert_kps_equal(kp, ref)
    if kind == "flat":
        assert len(kp) == 0
    if kind == "noise" and thr == 1:
        assert len(kp) > 2000


@pytest.mark.parametrize("shape", [(480, 640), (231, 309), (64, 80)])
def test_orb_detect_other_sizes(fe, frames, shape):
    g = np.ascontiguousarray(frames["gray"][1][: shape[0], : shape[1]])
    kp = fe.orb_detect(g, None, 15)
    assert_kps_equal(kp, pyorb.detect(g, None, 15))


def test_orb_compute_matches_oracle(fe, frames):
    g = frames["gray"][2]
    kp = pyorb.detect(g, None, 20)
    sel = kp[np.random.default_rng(0).permutation(len(kp))[:1500]]  # unsorted by level on purpose
    k1, d1 = fe.orb_compute(g, sel)
    k2, d2 = pyorb.compute(g, sel)
    assert_kps_equal(k1, k2)
    assert np.array_equal(d1, d2)
    assert np.all(np.diff(k1["octave"]) >= 0)          # regrouped by level
    assert len(k1) < len(sel)                            # border (31 px) keypoints dropped
    assert 60 < np.unpackbits(d1, axis=1).sum(1).mean() < 196


def test_detect_describe_sequence_matches_oracle(fe, frames):
    """The whole Node::Node feature path over consecutive frames: the per-cell thresholds persist."""
    fe.detector_configure(max_keypoints=1000)
    st = pyorb.grid_state(1000)
    for f in range(4):
        g, d = frames["gray"][f], frames["depth"][f]
        m = np.where(frames["mask"][f] > 0, 255, 0).astype(np.uint8) if f % 2 == 0 else frames["mask"][f]
        kp, desc, xyz = fe.detect_describe(g, m, d, frames["fx"], frames["fy"], frames["cx"], frames["cy"])
        rk, rdesc = pyorb.node_features(st, g, m, d, 1000)
        assert_kps_equal(kp, rk)
        assert np.array_equal(desc, rdesc)
        kept, rxyz = po.project_to_3d(np.stack([rk["x"], rk["y"]], 1), d, frames["fx"], frames["fy"],
                                      frames["cx"], frames["cy"], 1.0, 1000)
        assert len(kept) == len(rk) and np.array_equal(xyz, rxyz)
        assert np.array_equal(fe.detector_thresholds(), np.array(st.thresh[:9]))
        assert 300 < len(kp) <= 1000
    # texture-poor frame: the adjuster lowers thresholds and re-detects (up to 5 passes per cell)
    flat = np.full((480, 640), 128, np.uint8)
    flat[200:280, 300:340] = 140
    depth = np.full((480, 640), 2.0, np.float32)
    mask = np.full((480, 640), 255, np.uint8)
    kp, desc, xyz = fe.detect_describe(flat, mask, depth, 525, 525, 319.5, 239.5)
    rk, rdesc = pyorb.node_features(st, flat, mask, depth, 1000)
    assert_kps_equal(kp, rk) and np.array_equal(desc, rdesc)
    assert np.array_equal(fe.detector_thresholds(), np.array(st.thresh[:9]))
    assert fe.detector_thresholds().min() < 10


def test_detected_frames_match_and_register(fe, frames):
    """End to end on images: detect+describe two frames, upload as nodes, match + RANSAC; the plane is
    seen from a translating / rotating camera, so an edge with many inliers must come out."""
    from rgbdslam_v2_amd.frontend import inlier_indices
    fe.detector_configure(max_keypoints=1000)
    nodes = []
    for f in range(2):
        m = np.where(frames["mask"][f] > 0, 255, 0).astype(np.uint8)
        kp, desc, xyz = fe.detect_describe(frames["gray"][f], m, frames["depth"][f], frames["fx"], frames["fy"],
                                           frames["cx"], frames["cy"])
        fe.upload_node(200 + f, desc, xyz)
        nodes.append((kp, desc, xyz))
    rec = fe.match_pair_list([201], [200])[0]
    ref = po.match_node_pair(nodes[1][1], nodes[1][2], 201, nodes[0][1], nodes[0][2], 200,
                             po.default_params(seed=fe.params.seed, depth_cov=fe.params.depth_cov))
    assert rec["n_all"] == ref["n_all"] and rec["n_inl"] == ref["n_inl"]
    assert np.array_equal(inlier_indices(rec), ref["inl_idx"])
    assert rec["id1"] == 200 and rec["n_inl"] >= 40
    fe.release_node(200)
    fe.release_node(201)


# ---- the sizes of the other BASELINE configs (detection was only tested at 640x480 / 1000 keypoints) -----
@pytest.mark.parametrize("w,h,n_kp", [(640, 480, 600),      # configs[0]: ORB 600 (parameter_server.cpp:83 default)
                                      (640, 480, 1500),     # configs[2]: ORB 1500
                                      (1280, 960, 4000)])   # configs[4]: 1280x960, ORB 4000
def test_detect_describe_at_config_sizes(w, h, n_kp):
    """Node::Node's feature path (node.cpp:139-210) with adjustedGridWrapper's min = N, max = 1.5 N wiring
    (features.cpp:42-60) at the keypoint budgets / image size of configs[0], [2] and [4]; thresholds persist over
    the frames, a dark frame drives the x0.7 re-detection loop (feature_adjuster.cpp:185-224, 286-317)."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    fr = synth.make_image_sequence(n_frames=3, seed=11, width=w, height=h)
    fe = FrontEnd(device_id=0, max_nodes=4, max_keypoints=((n_kp + 63) // 64) * 64, max_pairs_per_batch=8)
    fe.detector_configure(max_keypoints=n_kp)
    st = pyorb.grid_state(n_kp)
    counts = []
    for f in range(3):
        g, d = fr["gray"][f], fr["depth"][f]
        m = np.where(fr["mask"][f] > 0, 255, 0).astype(np.uint8)
        kp, desc, xyz = fe.detect_describe(g, m, d, fr["fx"], fr["fy"], fr["cx"], fr["cy"])
        rk, rdesc = pyorb.node_features(st, g, m, d, n_kp)
        assert_kps_equal(kp, rk)
        assert np.array_equal(desc, rdesc)
        kept, rxyz = po.project_to_3d(np.stack([rk["x"], rk["y"]], 1), d, fr["fx"], fr["fy"], fr["cx"], fr["cy"], 1.0,
                                      n_kp)
        assert len(kept) == len(rk) and np.array_equal(xyz, rxyz)
        assert np.array_equal(fe.detector_thresholds(), np.array(st.thresh[:9]))
        assert len(kp) <= n_kp
        counts.append(len(kp))
    assert max(counts) > n_kp // 3
    # low-contrast frame: every cell falls short of its minimum and re-detects with thresholds x0.7, up to 5 times
    dark = (fr["gray"][0].astype(np.float32) * 0.3 + 80).astype(np.uint8)
    m = np.full((h, w), 255, np.uint8)
    before = fe.detector_thresholds()
    kp, desc, xyz = fe.detect_describe(dark, m, fr["depth"][0], fr["fx"], fr["fy"], fr["cx"], fr["cy"])
    rk, rdesc = pyorb.node_features(st, dark, m, fr["depth"][0], n_kp)
    assert_kps_equal(kp, rk)
    assert np.array_equal(desc, rdesc)
    assert np.array_equal(fe.detector_thresholds(), np.array(st.thresh[:9]))
    assert fe.detector_thresholds().max() < before.max()   # the adjuster's x0.7 re-detection passes ran
    fe.close()


def test_orb_detect_full_resolution_levels():
    """cv::ORB::detect on a 1280x960 image: 8 pyramid levels, every level's FAST / NMS / Harris / angle."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    fr = synth.make_image_sequence(n_frames=1, seed=12, width=1280, height=960)
    fe = FrontEnd(device_id=0, max_nodes=2, max_keypoints=4096, max_pairs_per_batch=8)
    g = fr["gray"][0]
    for thr in (12, 40):
        kp = fe.orb_detect(g, None, thr)
        ref = pyorb.detect(g, None, thr)
        assert_kps_equal(kp, ref)
        assert len(np.unique(kp["octave"])) == 8
    sel = ref[np.random.default_rng(1).permutation(len(ref))[:4000]]
    k1, d1 = fe.orb_compute(g, sel)
    k2, d2 = pyorb.compute(g, sel)
    assert_kps_equal(k1, k2)
    assert np.array_equal(d1, d2)
    fe.close()


def test_detect_describe_batch_equals_frame_by_frame(frames):
    """rgbdfe_detect_describe_batch: frame k+1's upload and pyramid overlap frame k's detection (second image set, second
    stream); the detector state carries over as in single calls -- identical keypoints, descriptors, points, thresholds.
    The run includes a dark frame (several adjuster iterations), a frame without a mask, and a batch of one."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    K = (frames["fx"], frames["fy"], frames["cx"], frames["cy"])
    grays = [frames["gray"][f] for f in range(4)]
    grays.insert(2, (frames["gray"][0].astype(np.float32) * 0.3 + 80).astype(np.uint8))
    depths = [frames["depth"][f] for f in (0, 1, 0, 2, 3)]
    masks = [np.where(frames["mask"][f] > 0, 255, 0).astype(np.uint8) for f in (0, 1, 0, 2, 3)]
    masks[3] = None
    outs = []
    # (a run longer than two super-frames of 7: the super-frame pipeline's double buffering, a partial last super-frame)
    long_idx = [i % 5 for i in range(17)]
    for mode in ("single", "batch", "batch_then_single", "single_long", "batch_long"):
        fe = FrontEnd(device_id=0, max_nodes=2, max_keypoints=1024, max_pairs_per_batch=8)
        fe.detector_configure(max_keypoints=1000)
        if mode == "single":
            res = [fe.detect_describe(g, m, d, *K) for g, m, d in zip(grays, masks, depths)]
        elif mode == "single_long":
            res = [fe.detect_describe(grays[i], masks[i], depths[i], *K) for i in long_idx]
        elif mode == "batch_long":
            res = fe.detect_describe_batch([grays[i] for i in long_idx], [masks[i] for i in long_idx],
                                           [depths[i] for i in long_idx], *K)
        elif mode == "batch":
            res = fe.detect_describe_batch(grays, masks, depths, *K)
        else:
            res = fe.detect_describe_batch(grays[:1], masks[:1], depths[:1], *K)
            res += fe.detect_describe_batch(grays[1:4], masks[1:4], depths[1:4], *K)
            res.append(fe.detect_describe(grays[4], masks[4], depths[4], *K))
        outs.append((res, fe.detector_thresholds().copy()))
        assert fe.detect_describe_batch([], [], [], *K) == []
        fe.close()
    assert min(len(r[0]) for r in outs[0][0]) > 100
    for got, want in ((outs[1], outs[0]), (outs[2], outs[0]), (outs[4], outs[3])):
        (res, thr), (ref, ref_thr) = got, want
        assert len(res) == len(ref) and np.array_equal(thr, ref_thr)
        for (k1, d1, x1), (k2, d2, x2) in zip(res, ref):
            assert_kps_equal(k1, k2)
            assert np.array_equal(d1, d2) and np.array_equal(x1, x2)


def test_detect_describe_batch_min_depth_equals_single_calls_and_oracle():
    """use_feature_min_depth sends a batch through the frame pipeline (frame k + 1 detected while frame k is described), whose
    removeDepthless then runs on the neighbourhood depths (the `zmin` compaction) before the max_keypoints cut: the batch, six
    single calls and the oracle (orb_node_features + projectTo3D, both in min-depth mode) agree bit for bit, thresholds
    included.  The depth has holes, so that on every frame removeDepthless drops keypoints and the cut still has work."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    n, mk = 6, 150
    fr = synth.make_image_sequence(n_frames=n, seed=5, width=320, height=240)
    K = (fr["fx"], fr["fy"], fr["cx"], fr["cy"])
    rng = np.random.default_rng(5)
    grays = [fr["gray"][f] for f in range(n)]
    masks = [np.full(g.shape, 255, np.uint8) for g in grays]
    depths = []
    for f in range(n):
        d = fr["depth"][f].copy()
        d[rng.random(d.shape) < 0.2] = np.nan
        d[60:140, 100:220] = np.nan
        depths.append(d)
    outs = []
    for mode in ("single", "batch"):
        fe = FrontEnd(device_id=0, max_nodes=2, max_keypoints=256, max_pairs_per_batch=8)
        fe.detector_configure(max_keypoints=mk, grid_resolution=3)
        fe.set_feature_min_depth(True)
        if mode == "single":
            res = [fe.detect_describe(g, m, d, *K) for g, m, d in zip(grays, masks, depths)]
        else:
            res = fe.detect_describe_batch(grays, masks, depths, *K)
        outs.append((res, fe.detector_thresholds().copy()))
        fe.close()
    pyorb.set_use_feature_min_depth(True)
    try:
        st = pyorb.grid_state(mk, 3)
        for f in range(n):
            g, m, d = grays[f], masks[f], depths[f]
            agg = pyorb.grid_detect(type(st).from_buffer_copy(st), g, m)   # the detector's aggregate, on a copy of its state
            left = po.remove_depthless_min_depth(np.stack([agg["x"], agg["y"]], 1), agg["size"], d)
            print("frame %d: aggregate %d, after the min-depth removeDepthless %d" % (f, len(agg), len(left)))
            assert mk < len(left) < len(agg)       # the zmin compaction and the cut both run
            rk, rdesc = pyorb.node_features(st, g, m, d, mk)
            okept, oxyz = po.project_to_3d_min_depth(np.stack([rk["x"], rk["y"]], 1), rk["size"], d, *K, 1.0, mk)
            assert len(okept) == len(rk) <= mk
            for res, _ in outs:
                kp, desc, xyz = res[f]
                assert_kps_equal(kp, rk)
                assert np.array_equal(desc, rdesc) and np.array_equal(xyz, oxyz)
        for _, thr in outs:
            assert np.array_equal(thr, np.array(st.thresh[:9]))
    finally:
        pyorb.set_use_feature_min_depth(False)


@pytest.mark.parametrize("grid,n_frames,shape,depth", [(3, 37, (480, 640), "3"), (3, 30, (480, 640), "2"), (2, 23, (240, 320), "3"),
                                                       (4, 11, (240, 320), "3"), (1, 16, (120, 160), "3")])
def test_detect_describe_batch_long_runs_and_grids(grid, n_frames, shape, depth):
    """The super-frame pipeline in its steady state -- more super-frames than image sets / pass slots / staging buffers, so
    every ring wraps around (37 frames = 6 super-frames of 7 with three in flight) --, with both pipeline depths, other
    grid resolutions (a super-frame holds floor(64 / grid^2) frames: 7, 7, 4, 7) and image sizes, a dark stretch that makes
    the adjuster iterate and thresholds fall below the floors of passes already in flight (re-passes), and a frame without
    a mask: the outputs and the thresholds left behind are those of single calls."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    h, w = shape
    seq = synth.make_image_sequence(n_frames=min(n_frames, 12), seed=31 + grid, width=w, height=h)
    idx = synth.forth_and_back(n_frames, len(seq["gray"]))
    grays = [seq["gray"][i] for i in idx]
    depths = [seq["depth"][i] for i in idx]
    masks = [np.where(seq["mask"][i] > 0, 255, 0).astype(np.uint8) for i in idx]
    for f in range(n_frames // 3, n_frames // 3 + 5):          # a dark, low-contrast stretch
        grays[f] = (grays[f].astype(np.float32) * 0.25 + 70).astype(np.uint8)
    masks[n_frames // 2] = None
    K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
    outs = []
    old = os.environ.get("RGBDFE_SUPER_DEPTH")
    os.environ["RGBDFE_SUPER_DEPTH"] = depth
    try:
        for mode in ("single", "batch"):
            fe = FrontEnd(device_id=0, max_nodes=2, max_keypoints=512, max_pairs_per_batch=8)
            fe.detector_configure(max_keypoints=400, grid_resolution=grid, adjuster_max_iterations=5)
            if mode == "single":
                res = [fe.detect_describe(g, m, d, *K) for g, m, d in zip(grays, masks, depths)]
            else:
                res = fe.detect_describe_batch(grays, masks, depths, *K)
            outs.append((res, fe.detector_thresholds().copy()))
            fe.close()
    finally:
        if old is None:
            os.environ.pop("RGBDFE_SUPER_DEPTH", None)
        else:
            os.environ["RGBDFE_SUPER_DEPTH"] = old
    (res, thr), (ref, ref_thr) = outs[1], outs[0]
    assert len(res) == len(ref) == n_frames and np.array_equal(thr, ref_thr)
    assert sum(len(r[0]) for r in ref) > 20 * n_frames
    for (k1, d1, x1), (k2, d2, x2) in zip(res, ref):
        assert_kps_equal(k1, k2)
        assert np.array_equal(d1, d2) and np.array_equal(x1, x2)


@pytest.mark.parametrize("devs,grid", [(None, 3), (None, 6), ([0, 0], 3)], ids=["super_frames", "frame_pipeline", "two_device_handle"])
def test_detect_describe_batch_nodes(devs, grid):
    """rgbdfe_detect_describe_batch_nodes: the frames' features become resident nodes inside the call (device-to-device from
    the description's buffers on the super-frame path; from the host outputs on the frame-by-frame path -- grid 6 -- and on a
    multi-device handle) -- pair results are those of upload_node + match on the returned features; an empty frame gives an
    empty node, a negative id none, an existing id is rewritten."""
    from rgbdslam_v2_amd.frontend import FrontEnd, RgbdfeError
    n = 16
    seq = synth.make_image_sequence(n_frames=8, seed=41)
    idx = synth.forth_and_back(n, 8)
    grays = [seq["gray"][i] for i in idx]
    depths = [seq["depth"][i].copy() for i in idx]
    masks = [np.where(seq["mask"][i] > 0, 255, 0).astype(np.uint8) for i in idx]
    depths[5][:] = np.nan                                   # no depth anywhere: no features, an empty node
    K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
    ids = np.arange(100, 100 + n, dtype=np.int32)
    ids[9] = -1                                             # no node for frame 9
    pq = np.array([100 + f for f in range(1, n) for c in (1, 2, 3) if f - c >= 0 and f != 9 and f - c != 9], np.int32)
    pt = np.array([100 + f - c for f in range(1, n) for c in (1, 2, 3) if f - c >= 0 and f != 9 and f - c != 9], np.int32)
    a = FrontEnd(device_id=0, max_nodes=n + 2, max_keypoints=1024, max_pairs_per_batch=64, device_ids=devs)
    a.detector_configure(max_keypoints=600, grid_resolution=grid)
    feats = a.detect_describe_batch(grays, masks, depths, *K)
    for f in range(n):
        if ids[f] >= 0:
            a.upload_node(int(ids[f]), feats[f][1], feats[f][2])
    ref = a.match_pair_list(pq, pt)
    b = FrontEnd(device_id=0, max_nodes=n + 2, max_keypoints=1024, max_pairs_per_batch=64, device_ids=devs)
    b.detector_configure(max_keypoints=600, grid_resolution=grid)
    b.upload_node(103, feats[0][1][:50], feats[0][2][:50])  # id 103 exists already: rewritten by the call
    got = b.detect_describe_batch(grays, masks, depths, *K, node_ids=ids)
    for (k1, d1, x1), (k2, d2, x2) in zip(got, feats):
        assert_kps_equal(k1, k2)
        assert np.array_equal(d1, d2) and np.array_equal(x1, x2)
    assert len(got[5][0]) == 0 and (ref["id1"] >= 0).sum() > 10
    assert b.match_pair_list(pq, pt).tobytes() == ref.tobytes()
    with pytest.raises(RgbdfeError):
        b.match_pair_list([100], [109])                     # frame 9 got no node
    with pytest.raises(RgbdfeError):
        b.detect_describe_batch(grays[:2], masks[:2], depths[:2], *K, node_ids=[7, 7])
    a.close(); b.close()


def test_detect_describe_batch_nodes_out_of_slots_leaves_a_usable_context():
    """More frames with node ids than free node slots: the call is refused with RGBDFE_ERR_CAPACITY before anything is
    detected (all-or-nothing, like rgbdfe_upload_nodes: ADVICE r3); no node was made, no slot is lost -- a later batch that
    needs every slot of the context succeeds."""
    from rgbdslam_v2_amd.frontend import FrontEnd, RgbdfeError
    seq = synth.make_image_sequence(n_frames=8, seed=43)
    idx = synth.forth_and_back(16, 8)
    grays = [seq["gray"][i] for i in idx]
    depths = [seq["depth"][i] for i in idx]
    masks = [np.where(seq["mask"][i] > 0, 255, 0).astype(np.uint8) for i in idx]
    K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
    fe = FrontEnd(device_id=0, max_nodes=10, max_keypoints=1024, max_pairs_per_batch=16)
    fe.detector_configure(max_keypoints=600)
    with pytest.raises(RgbdfeError):
        fe.detect_describe_batch(grays, masks, depths, *K, node_ids=np.arange(16, dtype=np.int32))
    made = [i for i in range(16) if fe.node_count(i) >= 0]      # rgbdfe_node_count: rows of a resident node, < 0 otherwise
    assert made == []
    out = fe.detect_describe_batch(grays[:10], masks[:10], depths[:10], *K, node_ids=np.arange(10, dtype=np.int32))   # all 10 slots
    assert all(fe.node_count(i) == len(out[i][0]) for i in range(10)) and min(len(o[0]) for o in out) > 100
    r = fe.match_pair_list([1, 2, 3], [0, 1, 2])
    assert (r["id1"] >= 0).sum() >= 2
    fe.close()


def test_detect_describe_with_page_locked_images(frames):
    """rgbdfe_host_register: page-locked caller images are copied to the device directly (no staging copy); the outputs
    are those of the pageable path, and the buffers can be unregistered and reused afterwards."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    K = (frames["fx"], frames["fy"], frames["cx"], frames["cy"])
    outs = []
    for pinned in (False, True):
        fe = FrontEnd(device_id=0, max_nodes=2, max_keypoints=1024, max_pairs_per_batch=8)
        fe.detector_configure(max_keypoints=1000)
        res = []
        for f in range(3):
            gray = np.ascontiguousarray(frames["gray"][f]).copy()
            mask = np.where(frames["mask"][f] > 0, 255, 0).astype(np.uint8)
            if pinned:
                fe.host_register(gray)
                fe.host_register(mask)
            res.append(fe.detect_describe(gray, mask if f != 1 else None, frames["depth"][f], *K))
            if pinned:
                fe.host_unregister(gray)
                fe.host_unregister(mask)
                with pytest.raises(Exception):
                    fe.host_unregister(gray)   # not registered any more
        outs.append(res)
        fe.close()
    for (k1, d1, x1), (k2, d2, x2) in zip(*outs):
        assert_kps_equal(k1, k2)
        assert np.array_equal(d1, d2) and np.array_equal(x1, x2)
