"""-m gpu: the sensor entry points (include/rgbdfe.h, "sensor frames") on the device.

The contract: rgbdfe_ingest_frame equals the numpy restatement of the listener's and Node::Node's image preparation
(tests/ingest_oracle.py) bit for bit, and every sensor call gives, bit for bit, what the corresponding existing call gives
when it is fed those three planes -- keypoints, descriptors, xyz1, counts, the per-cell thresholds afterwards, the nodes, the
clouds.  The detector is stateful: the comparison always runs on a SECOND context that is fed the prepared planes.

Colour test frames are composed from the luminance photographs under tests/golden (frame k = channels 640_{k}, 640_{k+1},
640_{k+2}, cyclically), depth = plane_depth(shape, 2.0, k) with binary_mask(shape, k) holes."""
import ctypes as C

import numpy as np
import pytest

import ingest_oracle as io
from rgbdslam_v2_amd import _lib
from test_gpu_orb_photos import binary_mask, intrinsics, plane_depth
from test_oracle_ingest import GEOMETRIES, assert_planes_equal, synth_depth, synth_visual
from test_oracle_orb_photos import load_photos

pytestmark = pytest.mark.gpu

SHAPE = (480, 640)
K = intrinsics(SHAPE)
DEPTH_KINDS = ("32FC1", "16UC1", "16UC1_half")


def _fe(**kw):
    from rgbdslam_v2_amd.frontend import FrontEnd
    args = dict(device_id=0, max_nodes=48, max_keypoints=1024, max_pairs_per_batch=256)
    args.update(kw)
    return FrontEnd(**args)


@pytest.fixture(scope="module")
def photos():
    return load_photos()


@pytest.fixture(scope="module")
def pair():
    a, b = _fe(), _fe()
    yield a, b
    a.close()
    b.close()


def restart(fe, detector, min_depth, max_keypoints=1000):
    fe.detector_configure(max_keypoints=max_keypoints, grid_resolution=3)
    fe.set_detector_type(detector)
    fe.set_feature_min_depth(min_depth)


def sensor_frame(photos, k, visual_enc, depth_kind):
    """(visual, depth, encoding argument) of test frame k."""
    rgb = io.colour_frame(photos, k % 5)
    if visual_enc == "mono8":
        visual, enc = np.ascontiguousarray(rgb[..., 0]), None
    elif visual_enc == "bgr8":
        visual, enc = np.ascontiguousarray(rgb[..., ::-1]), "bgr8"   # the same scene as a bgr8 camera would deliver it
    else:
        visual, enc = rgb, "rgb8"
    if depth_kind == "16UC1_half":
        depth = io.depth_frame((SHAPE[0] // 2, SHAPE[1] // 2), k, "16UC1", plane_depth, binary_mask)
    else:
        depth = io.depth_frame(SHAPE, k, depth_kind, plane_depth, binary_mask)
    return visual, depth, enc


def assert_features_equal(got, want):
    (k1, d1, x1), (k2, d2, x2) = got, want
    assert len(k1) == len(k2)
    assert k1.tobytes() == k2.tobytes()
    assert np.array_equal(d1, d2)
    assert x1.tobytes() == x2.tobytes()


# ---- rgbdfe_ingest_frame = the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_enc", ["32FC1", "16UC1"])
@pytest.mark.parametrize("visual_enc", ["mono8", "rgb8", "bgr8"])
@pytest.mark.parametrize("geom", GEOMETRIES[:4] + [((960, 1280), (480, 640), 0, 0)],
                         ids=lambda g: "%dx%d_d%dx%d_pad%d" % (g[0][1], g[0][0], g[1][1], g[1][0], g[2]))
def test_ingest_frame_equals_the_restatement(pair, geom, visual_enc, depth_enc):
    (rows, cols), (drows, dcols), pad, _ = geom
    v = synth_visual(rows, cols, 1 if visual_enc == "mono8" else 3, 11 * rows + cols, pad)
    d = synth_depth(drows, dcols, depth_enc, 7 * drows + dcols)
    got = pair[0].ingest_frame(v, d, None if visual_enc == "mono8" else visual_enc)
    assert_planes_equal(got, io.prepared_planes(v, d))


def test_ingest_frame_on_the_photo_frames_and_null_outputs(pair, photos):
    fe = pair[0]
    for kind in DEPTH_KINDS:
        v, d, enc = sensor_frame(photos, 1, "rgb8", kind)
        want = io.prepared_planes(v, d)
        assert_planes_equal(fe.ingest_frame(v, d, enc), want)
        g, m, dm = fe.ingest_frame(v, d, enc, mono8=False, depth_m=False)
        assert m is None and dm is None and np.array_equal(g, want[0])
        g, m, dm = fe.ingest_frame(v, d, enc, gray=False, depth_m=False)
        assert g is None and dm is None and np.array_equal(m, want[1])
        g, m, dm = fe.ingest_frame(v, d, enc, gray=False, mono8=False)
        assert g is None and m is None and dm.tobytes() == np.ascontiguousarray(want[2]).tobytes()
    assert fe.ingest_frame(v, d, enc, gray=False, mono8=False, depth_m=False) == (None, None, None)


def test_depth_to_mono8_has_not_moved(pair):
    """rgbdfe_depth_to_mono8 shares its expressions with the ingest kernel through csrc/depth_convert.h."""
    from oracle import pyoracle as po
    fe = pair[0]
    d32 = synth_depth(480, 640, "32FC1", 3)
    assert np.array_equal(fe.depth_to_mono8(d32), po.depth_to_mono8(d32))
    d16 = synth_depth(480, 640, "16UC1", 4)
    m, dm = fe.depth_to_mono8(d16)
    rm, rdm = po.depth_to_mono8(d16)
    assert np.array_equal(m, rm) and dm.tobytes() == rdm.tobytes()


# ---- rgbdfe_sensor_detect_describe = rgbdfe_detect_describe on the prepared planes ---------------------------------------------
@pytest.mark.parametrize("visual_enc", ["rgb8", "bgr8", "mono8"])
@pytest.mark.parametrize("depth_kind", DEPTH_KINDS)
@pytest.mark.parametrize("min_depth", [False, True], ids=["", "min_depth"])
@pytest.mark.parametrize("detector", ["ORB", "FAST"])
def test_sensor_detect_describe_sequence(pair, photos, detector, min_depth, depth_kind, visual_enc):
    a, b = pair
    restart(a, detector, min_depth)
    restart(b, detector, min_depth)
    for k in range(5):
        v, d, enc = sensor_frame(photos, k, visual_enc, depth_kind)
        got = a.sensor_detect_describe(v, d, *K, visual_encoding=enc)
        gray, mono8, dm = io.prepared_planes(v, d)
        want = b.detect_describe(gray, mono8, dm, *K)
        print("%s min_depth=%d %s %s frame %d: %d features" % (detector, min_depth, depth_kind, visual_enc, k, len(got[0])))
        assert_features_equal(got, want)
        assert np.array_equal(a.detector_thresholds(), b.detector_thresholds())
        if detector == "ORB" and not min_depth and visual_enc == "rgb8":
            assert len(got[0]) >= 900   # (the oracle keeps 939 .. 982 of 1000 on these frames)
        assert len(got[0]) > 0


def test_rgb8_and_bgr8_of_one_scene_give_different_features(pair, photos):
    """No channel swap for bgr8: the same scene delivered as bgr8 has another gray image, hence other keypoints."""
    a, _ = pair
    restart(a, "ORB", False)
    v, d, enc = sensor_frame(photos, 0, "rgb8", "32FC1")
    k_rgb = a.sensor_detect_describe(v, d, *K, visual_encoding=enc)[0]
    restart(a, "ORB", False)
    v, d, enc = sensor_frame(photos, 0, "bgr8", "32FC1")
    k_bgr = a.sensor_detect_describe(v, d, *K, visual_encoding=enc)[0]
    assert k_rgb.tobytes() != k_bgr.tobytes()


# ---- rgbdfe_sensor_detect_describe_batch_nodes = rgbdfe_detect_describe_batch_nodes on the prepared planes ----------------------
N_RUN = 30   # more than two super-frames of 14


def run_frames(photos, visual_enc, depth_kind):
    vis, dep, enc = [], [], None
    for k in range(N_RUN):
        v, d, enc = sensor_frame(photos, k, visual_enc, depth_kind)
        if k == 9 and d.dtype == np.float32:
            d = np.full_like(d, np.nan)                    # no depth anywhere: an empty node
        if k == 17:
            v = np.full_like(v, 128)                       # a flat gray frame: no corners, an empty node
        vis.append(v)
        dep.append(d)
    return vis, dep, enc


def predecessor_pairs(n):
    """Every node against its three predecessors, and against the frame five back (the same photographs, another depth)."""
    pq = np.array([f for f in range(n) for c in (1, 2, 3, 5) if f - c >= 0], np.int32)
    pt = np.array([f - c for f in range(n) for c in (1, 2, 3, 5) if f - c >= 0], np.int32)
    return pq, pt


@pytest.mark.parametrize("visual_enc,depth_kind", [("rgb8", "32FC1"), ("rgb8", "16UC1"), ("bgr8", "16UC1_half"), ("mono8", "32FC1")])
@pytest.mark.parametrize("min_depth", [False, True], ids=["", "min_depth"])
@pytest.mark.parametrize("detector", ["ORB", "FAST"])
def test_sensor_batch_nodes_equal_the_batch_on_prepared_planes(pair, photos, detector, min_depth, visual_enc, depth_kind):
    a, b = pair
    restart(a, detector, min_depth)
    restart(b, detector, min_depth)
    vis, dep, enc = run_frames(photos, visual_enc, depth_kind)
    planes = [io.prepared_planes(v, d) for v, d in zip(vis, dep)]
    ids = np.arange(N_RUN, dtype=np.int32)
    got = a.sensor_detect_describe_batch_nodes(vis, dep, *K, node_ids=ids, visual_encoding=enc)
    want = b.detect_describe_batch([p[0] for p in planes], [p[1] for p in planes], [p[2] for p in planes], *K, node_ids=ids)
    counts = [len(g[0]) for g in got]
    print("%s min_depth=%d %s %s: counts %s" % (detector, min_depth, visual_enc, depth_kind, counts))
    for g, w in zip(got, want):
        assert_features_equal(g, w)
    assert np.array_equal(a.detector_thresholds(), b.detector_thresholds())
    assert counts[17] == 0 and (depth_kind != "32FC1" or counts[9] == 0)
    assert sum(c > 0 for c in counts) >= N_RUN - 2
    for f in range(N_RUN):
        assert a.node_count(f) == b.node_count(f) == counts[f]
    pq, pt = predecessor_pairs(N_RUN)
    ra, rb = a.match_pair_list(pq, pt), b.match_pair_list(pq, pt)
    assert ra.tobytes() == rb.tobytes()
    print("pairs with matches: %d, with inliers: %d of %d" % ((ra["n_all"] > 0).sum(), (ra["n_inl"] > 0).sum(), len(ra)))
    assert (ra["n_all"] > 0).any()
    # the plain batch form (node_ids NULL) gives the same host outputs
    restart(a, detector, min_depth)
    plain = a.sensor_detect_describe_batch_nodes(vis, dep, *K, visual_encoding=enc)
    for g, w in zip(plain, want):
        assert_features_equal(g, w)


def test_sensor_batch_nodes_fast_without_host_outputs_still_writes_the_nodes(pair, photos):
    a, b = pair
    restart(a, "FAST", False)
    restart(b, "FAST", False)
    vis, dep, enc = run_frames(photos, "rgb8", "16UC1")
    planes = [io.prepared_planes(v, d) for v, d in zip(vis, dep)]
    ids = np.arange(N_RUN, dtype=np.int32)
    cnt = a.sensor_detect_describe_batch_nodes(vis, dep, *K, node_ids=ids, visual_encoding=enc, host_outputs=False)
    ref = b.detect_describe_batch([p[0] for p in planes], [p[1] for p in planes], [p[2] for p in planes], *K, node_ids=ids,
                                  host_outputs=False)
    assert np.array_equal(cnt, ref) and cnt.max() > 0
    pq, pt = predecessor_pairs(N_RUN)
    assert a.match_pair_list(pq, pt).tobytes() == b.match_pair_list(pq, pt).tobytes()


def test_sensor_batch_nodes_on_a_two_device_handle(pair, photos):
    _, b = pair
    restart(b, "ORB", False)
    n = 16
    vis, dep, enc = run_frames(photos, "rgb8", "16UC1")
    vis, dep = vis[:n], dep[:n]
    planes = [io.prepared_planes(v, d) for v, d in zip(vis, dep)]
    ids = np.arange(n, dtype=np.int32)
    b.detect_describe_batch([p[0] for p in planes], [p[1] for p in planes], [p[2] for p in planes], *K, node_ids=ids)
    pq, pt = predecessor_pairs(n)
    two = _fe(device_ids=[0, 0])
    try:
        restart(two, "ORB", False)
        two.sensor_detect_describe_batch_nodes(vis, dep, *K, node_ids=ids, visual_encoding=enc)
        assert two.match_pair_list(pq, pt).tobytes() == b.match_pair_list(pq, pt).tobytes()
    finally:
        two.close()


# ---- clouds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding_bgr", [False, True])
@pytest.mark.parametrize("visual_enc,depth_kind", [("rgb8", "32FC1"), ("rgb8", "16UC1_half"), ("mono8", "16UC1")])
def test_sensor_clouds_equal_upload_node_cloud_on_the_prepared_depth(pair, photos, visual_enc, depth_kind, encoding_bgr):
    a, b = pair
    restart(a, "ORB", False)
    restart(b, "ORB", False)
    n = 11
    vis, dep = [], []
    for k in range(n):
        v, d, enc = sensor_frame(photos, k, visual_enc, depth_kind)
        if d.dtype == np.uint16:   # frames at different distances, so that the edges below see inliers, outliers and occlusion
            d = (d.astype(np.float64) * (1.0 + 0.004 * k)).astype(np.uint16) * (d > 0)
            d = d.astype(np.uint16)
        else:
            d = (d * np.float32(1.0 + 0.004 * k)).astype(np.float32)
        vis.append(v)
        dep.append(d)
    ids = np.arange(n, dtype=np.int32)
    a.sensor_detect_describe_batch_nodes(vis, dep, *K, node_ids=ids, visual_encoding=enc, cloud_skip=2,
                                         cloud_encoding_bgr=encoding_bgr, cloud_min_depth=0.1)
    for k in range(n):
        _, _, dm = io.prepared_planes(vis[k], dep[k])
        b.upload_node_cloud(k, dm, *K, rgb=vis[k], encoding_bgr=encoding_bgr, min_depth=0.1, cloud_skip=2)
    new_ids = np.arange(1, n, dtype=np.int32)
    old_ids = new_ids - 1
    T = np.tile(np.eye(4, dtype=np.float32), (n - 1, 1, 1))
    T[:, 0, 3] = 0.01
    ca, cb = a.observation_likelihood(new_ids, old_ids, T), b.observation_likelihood(new_ids, old_ids, T)
    print(ca.tolist())
    assert np.array_equal(ca, cb)
    assert ca[:, 3].min() > 0 and ca[:, 0].max() > 0
    for k in range(n):
        a.release_node_cloud(k)
        b.release_node_cloud(k)


# ---- validation: INVALID_ARG before any state changes -----------------------------------------------------------------------------
def _raw_batch(fe, frames, node_ids=None, cloud=None, cap=1000):
    n = len(frames)
    arr = (_lib.RgbdfeSensorFrame * max(n, 1))(*frames)
    kp = np.zeros((max(n, 1), cap), _lib.KEYPOINT_DTYPE)
    desc = np.zeros((max(n, 1), cap, 32), np.uint8)
    xyz = np.zeros((max(n, 1), cap, 4), np.float32)
    cnt = np.zeros(max(n, 1), np.int32)
    ids = None if node_ids is None else np.ascontiguousarray(node_ids, np.int32)
    return fe._L.rgbdfe_sensor_detect_describe_batch_nodes(
        fe._ctx, n, arr, *K, 1.0, cap, kp.ctypes.data, desc.ctypes.data, xyz.ctypes.data, cnt.ctypes.data,
        None if ids is None else ids.ctypes.data, None if cloud is None else C.byref(cloud))


def test_validation_refuses_before_any_state_changes(pair, photos):
    from rgbdslam_v2_amd.frontend import FrontEnd
    a, _ = pair
    INVALID = -1
    assert a._L.rgbdfe_status_string(INVALID) is not None
    restart(a, "ORB", False)
    v, d, enc = sensor_frame(photos, 0, "rgb8", "32FC1")
    a.sensor_detect_describe(v, d, *K, visual_encoding=enc)          # moves the thresholds off their start values
    thr0 = a.detector_thresholds().copy()
    ids = [40, 41]
    for i in ids:
        assert a.node_count(i) < 0
    keep = []

    def frame(v=v, d=d, enc=enc, **override):
        fr, k = FrontEnd._sensor_frame(v, d, enc)
        keep.append(k)
        for name, value in override.items():
            setattr(fr, name, value)
        return fr

    v_small = np.ascontiguousarray(v[:240, :320])
    d_half = np.ascontiguousarray(d[::2, ::2])
    d_u16 = io.depth_frame(SHAPE, 0, "16UC1", plane_depth, binary_mask)
    v_bgr = np.ascontiguousarray(v[..., ::-1])
    cloud_ok = _lib.RgbdfeSensorCloud(2, 0, 0.1)
    cases = {
        "null visual": ([frame(), frame(visual=None)], ids, None),
        "null depth": ([frame(depth=None), frame()], ids, None),
        "unknown visual encoding": ([frame(), frame(visual_encoding=3)], ids, None),
        "unknown depth encoding": ([frame(depth_encoding=2), frame()], ids, None),
        "visual step smaller than a row": ([frame(visual_step=3 * 640 - 1), frame()], ids, None),
        "depth step smaller than a row": ([frame(), frame(depth_step=4 * 640 - 4)], ids, None),
        "zero rows": ([frame(visual_rows=0), frame()], ids, None),
        "negative depth cols": ([frame(), frame(depth_cols=-640)], ids, None),
        "frames differ in visual size": ([frame(), frame(v=v_small)], ids, None),
        "frames differ in depth size": ([frame(), frame(d=d_half)], ids, None),
        "frames differ in depth encoding": ([frame(), frame(d=d_u16)], ids, None),
        "frames differ in visual encoding": ([frame(), frame(v=v_bgr, enc="bgr8")], ids, None),
        "cloud_skip does not divide the size": ([frame(), frame()], ids, _lib.RgbdfeSensorCloud(7, 0, 0.1)),
        "cloud_skip zero": ([frame(), frame()], ids, _lib.RgbdfeSensorCloud(0, 0, 0.1)),
        "cloud without node_ids": ([frame(), frame()], None, cloud_ok),
    }
    for name, (frames, node_ids, cloud) in cases.items():
        rc = _raw_batch(a, frames, node_ids, cloud)
        assert rc == INVALID, (name, rc)
        assert np.array_equal(a.detector_thresholds(), thr0), name
        for i in ids:
            assert a.node_count(i) < 0, name
    # NULL frame pointers and the single-frame calls
    L = a._L
    n = C.c_int32(0)
    buf = np.zeros(1000 * 32, np.uint8)
    assert L.rgbdfe_sensor_detect_describe_batch_nodes(a._ctx, 2, None, *K, 1.0, 1000, buf.ctypes.data, buf.ctypes.data,
                                                       buf.ctypes.data, buf.ctypes.data, None, None) == INVALID
    assert L.rgbdfe_sensor_detect_describe(a._ctx, None, *K, 1.0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, C.byref(n)) == INVALID
    bad = frame(visual_encoding=7)
    assert L.rgbdfe_sensor_detect_describe(a._ctx, C.byref(bad), *K, 1.0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                           C.byref(n)) == INVALID
    assert L.rgbdfe_ingest_frame(a._ctx, None, buf.ctypes.data, None, None) == INVALID
    assert L.rgbdfe_ingest_frame(a._ctx, C.byref(bad), buf.ctypes.data, None, None) == INVALID
    assert np.array_equal(a.detector_thresholds(), thr0)
    # and the valid two-frame run still works afterwards
    assert _raw_batch(a, [frame(), frame()], ids, cloud_ok) == 0
    assert a.node_count(40) > 0 and a.node_count(41) > 0
    for i in ids:
        a.release_node_cloud(i)
        a.release_node(i)
