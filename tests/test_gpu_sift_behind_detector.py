"""-m gpu: SIFTGPU descriptors behind the ORB and FAST grid detectors -- rgbdfe_detect, rgbdfe_detect_sift_describe and
rgbdfe_detect_sift_describe_batch_nodes against the oracle composition (tests/sift_behind_detector_oracle.py) and against the
library's own single calls composed by hand, bit for bit."""
import numpy as np
import pytest

import sift_behind_detector_oracle as sbo
from oracle import pyoracle as po
from rgbdslam_v2_amd import _lib
from test_gpu_orb_photos import binary_mask, intrinsics, plane_depth
from test_oracle_orb_photos import load_photos

pytestmark = pytest.mark.gpu

KINDS = ("ORB", "FAST")
NAMES = ["640_1", "640_2", "640_3", "640_4", "640_5"]
DESC_RTOL, DESC_RTOL_ALL, TIGHT_FRACTION = 1e-3, 5e-2, 0.995   # tests/test_gpu_sift_extract.py


@pytest.fixture(scope="module")
def photos():
    return load_photos()


def _fe(**kw):
    from rgbdslam_v2_amd.frontend import FrontEnd
    args = dict(device_id=0, max_nodes=64, max_keypoints=1000, max_pairs_per_batch=256)
    args.update(kw)
    return FrontEnd(**args)


def _setup(fe, kind, mk=500, grid=3, min_depth=False):
    fe.detector_configure(mk, grid, 5)
    fe.set_detector_type(kind)
    fe.set_feature_min_depth(min_depth)


def _depth(shape, seed, holes=True):
    d = plane_depth(shape, 2.0, seed)
    if holes:
        d[binary_mask(shape, seed) == 0] = np.nan
    return d


def _frames(photos, n):
    grays = [photos[NAMES[(i * 3) % len(NAMES)]] for i in range(n)]
    depths = [_depth(g.shape, i) for i, g in enumerate(grays)]
    return grays, depths


def assert_kps_equal(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(a[f], b[f]), f


def _check_descriptors(desc, ref):
    assert desc.shape == ref.shape
    if len(desc) == 0:
        return
    rel = np.linalg.norm(desc - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-12)
    assert rel.max() <= DESC_RTOL_ALL and (rel <= DESC_RTOL).mean() >= TIGHT_FRACTION, (rel.max(), (rel <= DESC_RTOL).mean())


def _composed(fe, g, m, d, K, mk, min_depth, root):
    """rgbdfe_detect -> rgbdfe_project_to_3d -> rgbdfe_sift_describe -> rgbdfe_sift_node_features (or rgbdfe_sift_detect
    when projectTo3D keeps nothing)."""
    agg = fe.detect(g, m)
    xy = np.stack([agg["x"], agg["y"]], 1)
    if len(agg) == 0:
        kept = np.zeros(0, np.int64)
    elif min_depth:
        kept, _ = fe.project_to_3d_min_depth(xy, agg["size"], d, *K, 1.0, mk)
    else:
        kept, _ = fe.project_to_3d(xy, d, *K, 1.0, mk)
    if len(kept) == 0:
        kl, desc = fe.sift_detect(g, None, mk)
    else:
        kl, desc = fe.sift_describe(g, agg[np.asarray(kept)])
    if len(kl) == 0:
        z = np.zeros((0, 128), np.float32)
        return kl, np.zeros((0, 4), np.float32), z, z
    k2, xyz, raw, feat = fe.sift_node_features(np.stack([kl["x"], kl["y"]], 1), desc, d, *K, 1.0, mk, root,
                                               kp_size=kl["size"] if min_depth else None)
    return kl[np.asarray(k2)], xyz, raw, feat


# ---- rgbdfe_detect ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [2, 3, 6])
@pytest.mark.parametrize("kind", KINDS)
def test_detect_matches_oracle_aggregate(photos, kind, grid):
    fe, fe2 = _fe(), _fe()
    try:
        _setup(fe, kind, 600, grid)
        _setup(fe2, kind, 600, grid)
        det = sbo.Detector(kind, 600, grid)
        grays, depths = _frames(photos, 5)
        for i, (g, d) in enumerate(zip(grays, depths)):
            m = binary_mask(g.shape, i) if i % 2 else np.full(g.shape, 255, np.uint8)   # Node::Node's detection_mask
            kp = fe.detect(g, m)
            assert_kps_equal(kp, det.detect(g, m))
            assert np.array_equal(fe.detector_thresholds(), det.thresholds())
            fe2.detect_describe(g, m, d, *intrinsics(g.shape))
        assert np.array_equal(fe.detector_thresholds(), fe2.detector_thresholds())
    finally:
        fe.close()
        fe2.close()


# ---- rgbdfe_detect_sift_describe -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("root", [0, 1])
@pytest.mark.parametrize("min_depth", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_single_frame_equals_composition_and_oracle(photos, kind, min_depth, root):
    mk = 500
    fe, fe2 = _fe(), _fe()
    try:
        _setup(fe, kind, mk, 3, min_depth)
        _setup(fe2, kind, mk, 3, min_depth)
        det = sbo.Detector(kind, mk, 3)
        grays, depths = _frames(photos, 3)
        for i, (g, d) in enumerate(zip(grays, depths)):
            K = intrinsics(g.shape)
            m = np.full(g.shape, 255, np.uint8)
            kp, xyz, raw, feat = fe.detect_sift_describe(g, m, d, *K, use_root_sift=root)
            ck, cx, cr, cf = _composed(fe2, g, m, d, K, mk, min_depth, root)
            assert_kps_equal(kp, ck)
            assert np.array_equal(xyz, cx) and np.array_equal(raw, cr) and np.array_equal(feat, cf)
            assert 0 < len(kp) <= mk
            det_agg = det.detect(g, m)
            have_ref = po.ref_siftgpu_lib() is not None
            describe = po.ref_sift_describe if have_ref else (lambda gr, keys: np.zeros((len(keys), 128), np.float32))
            ok, ox, oraw, ofeat, _, quirk = sbo.frame(_Replay(det_agg), g, m, d, K, mk, min_depth, bool(root),
                                                      describe=describe)
            assert not quirk
            assert_kps_equal(kp, ok)
            assert np.array_equal(xyz, ox)
            assert np.array_equal(fe.detector_thresholds(), det.thresholds())
            if have_ref:
                _check_descriptors(raw, oraw)
    finally:
        fe.close()
        fe2.close()


class _Replay:
    """A detector that hands back a given aggregate (the oracle's own, computed once per frame above)."""

    def __init__(self, agg):
        self.agg = agg

    def detect(self, img, mask):
        return self.agg


@pytest.mark.parametrize("kind", KINDS)
def test_frame_without_depth_gets_siftgpu_detection(photos, kind):
    """The empty-list rule: projectTo3D keeps nothing, so SiftGPU detects on its own -- rgbdfe_sift_detect ->
    rgbdfe_sift_node_features, bit for bit."""
    mk = 400
    fe, fe2 = _fe(), _fe()
    try:
        _setup(fe, kind, mk)
        _setup(fe2, kind, mk)
        g = photos["640_2"]
        K = intrinsics(g.shape)
        # all-NaN depth: SiftGPU's own keypoints, none of which has depth either
        dn = np.full(g.shape, np.nan, np.float32)
        kp, xyz, raw, feat = fe.detect_sift_describe(g, None, dn, *K)
        assert len(kp) == 0 and len(fe2.detect(g, None)) > 0
        skp, sdesc = fe2.sift_detect(g, None, mk)
        assert len(skp) > 0
        assert len(fe2.sift_node_features(np.stack([skp["x"], skp["y"]], 1), sdesc, dn, *K, 1.0, mk, True)[0]) == 0
        # depth everywhere but under the detector's corners: the features of SiftGPU's own detection survive
        agg = fe2.detect(g, None)
        dq = plane_depth(g.shape, 2.0, 4)
        r = np.minimum(np.floor(agg["y"].astype(np.float64) + 0.5).astype(int), g.shape[0] - 1)
        c = np.minimum(np.floor(agg["x"].astype(np.float64) + 0.5).astype(int), g.shape[1] - 1)
        dq[r, c] = np.nan
        kp, xyz, raw, feat = fe.detect_sift_describe(g, None, dq, *K)
        skp, sdesc = fe2.sift_detect(g, None, mk)
        k3, x3, r3, f3 = fe2.sift_node_features(np.stack([skp["x"], skp["y"]], 1), sdesc, dq, *K, 1.0, mk, True)
        assert len(kp) == len(k3) > 0
        assert_kps_equal(kp, skp[np.asarray(k3)])
        assert np.array_equal(xyz, x3) and np.array_equal(raw, r3) and np.array_equal(feat, f3)
        assert np.array_equal(fe.detector_thresholds(), fe2.detector_thresholds())
    finally:
        fe.close()
        fe2.close()


# ---- rgbdfe_detect_sift_describe_batch_nodes -------------------------------------------------------------------------------
def _pairs(n, ids):
    q, t = [], []
    for f in range(1, n):
        for c in (1, 2, 3):
            if f - c >= 0 and ids[f] >= 0 and ids[f - c] >= 0:
                q.append(ids[f]); t.append(ids[f - c])
    return np.array(q, np.int32), np.array(t, np.int32)


def _batch_frames(photos, n):
    grays, depths = _frames(photos, n)
    masks = [binary_mask(g.shape, i) if i % 3 == 1 else None for i, g in enumerate(grays)]
    if n > 4:
        depths[4] = np.full(grays[4].shape, np.nan, np.float32)      # the empty-list rule inside a chunk
    if n > 6:
        grays[6] = np.full(grays[6].shape, 128, np.uint8)            # no corners at all
    return grays, masks, depths


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17, 37])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_equals_single_calls(photos, kind, n):
    mk = 300
    grays, masks, depths = _batch_frames(photos, n)
    K = intrinsics(grays[0].shape)
    ids = np.arange(10, 10 + n, dtype=np.int32)
    if n > 9:
        ids[9] = -1
    fe, fe2 = _fe(max_keypoints=mk), _fe(max_keypoints=mk)
    try:
        for f in (fe, fe2):
            _setup(f, kind, mk, 3)
        out = fe.detect_sift_describe_batch_nodes(grays, masks, depths, *K, ids)
        for f in range(n):
            kp, xyz, raw, feat = fe2.detect_sift_describe(grays[f], masks[f], depths[f], *K)
            assert_kps_equal(out[f][0], kp)
            assert np.array_equal(out[f][1], xyz) and np.array_equal(out[f][2], feat)
            if ids[f] >= 0:
                fe2.upload_float_node(int(ids[f]), feat, xyz)
                assert fe.node_count(int(ids[f])) == len(kp)
        assert np.array_equal(fe.detector_thresholds(), fe2.detector_thresholds())
        q, t = _pairs(n, ids)
        if len(q):
            r1, d1 = fe.match_flann_pair_list(q, t)
            r2, d2 = fe2.match_flann_pair_list(q, t)
            assert r1.tobytes() == r2.tobytes() and np.array_equal(d1, d2)
    finally:
        fe.close()
        fe2.close()


@pytest.mark.parametrize("kind", KINDS)
def test_batch_null_outputs_rewrite_capacity_and_two_devices(photos, kind):
    mk = 300
    grays, masks, depths = _batch_frames(photos, 9)
    K = intrinsics(grays[0].shape)
    ids = np.arange(0, 9, dtype=np.int32)
    fe, fe2 = _fe(max_keypoints=mk, max_nodes=12), _fe(max_keypoints=mk, max_nodes=12, device_ids=[0, 0])
    try:
        for f in (fe, fe2):
            _setup(f, kind, mk, 3)
        cnt = fe.detect_sift_describe_batch_nodes(grays, masks, depths, *K, ids, return_features=False)
        out = fe2.detect_sift_describe_batch_nodes(grays, masks, depths, *K, ids)
        assert np.array_equal(cnt, [len(o[0]) for o in out])
        assert cnt[4] == 0 and cnt[6] == 0 and cnt.sum() > 0
        q, t = _pairs(9, ids)
        r1, d1 = fe.match_flann_pair_list(q, t)
        r2, d2 = fe2.match_flann_pair_list(q, t)
        assert r1.tobytes() == r2.tobytes() and np.array_equal(d1, d2)
        # rewriting existing ids in place (frames in reverse order) -- and the handle keeps working
        cnt2 = fe.detect_sift_describe_batch_nodes(grays[::-1], masks[::-1], depths[::-1], *K, ids, return_features=False)
        out2 = fe2.detect_sift_describe_batch_nodes(grays[::-1], masks[::-1], depths[::-1], *K, ids)
        assert np.array_equal(cnt2, [len(o[0]) for o in out2])
        for f in range(9):
            assert fe.node_count(int(ids[f])) == cnt2[f]
        r1, d1 = fe.match_flann_pair_list(q, t)
        r2, d2 = fe2.match_flann_pair_list(q, t)
        assert r1.tobytes() == r2.tobytes() and np.array_equal(d1, d2)
        # capacity: 3 free slots, 4 fresh ids -> refused before any work, nothing registered
        th = fe.detector_thresholds()
        with pytest.raises(Exception):
            fe.detect_sift_describe_batch_nodes(grays[:4], None, depths[:4], *K, np.arange(100, 104, dtype=np.int32))
        assert all(fe.node_count(i) < 0 for i in range(100, 104))
        assert np.array_equal(fe.detector_thresholds(), th)
        fe.detect_sift_describe_batch_nodes(grays[:3], None, depths[:3], *K, np.arange(100, 103, dtype=np.int32))
        assert all(fe.node_count(i) >= 0 for i in range(100, 103))
    finally:
        fe.close()
        fe2.close()


def test_error_cases(photos):
    import ctypes as C
    from rgbdslam_v2_amd.frontend import RgbdfeError
    fe = _fe(max_keypoints=300)
    try:
        _setup(fe, "ORB", 300, 3)
        g = photos["640_1"]
        d = _depth(g.shape, 0)
        K = intrinsics(g.shape)
        th = fe.detector_thresholds()
        with pytest.raises(RgbdfeError):
            fe.detect(g, None, capacity=449)              # max_total = 450
        assert np.array_equal(fe.detector_thresholds(), th)
        assert len(fe.detect(g, None, capacity=450)) <= 450
        L, ctx = fe._L, fe._ctx
        kp = np.zeros(300, _lib.KEYPOINT_DTYPE)
        xyz = np.zeros((300, 4), np.float32)
        raw = np.zeros((300, 128), np.float32)
        n = C.c_int32(0)
        assert L.rgbdfe_detect(ctx, None, None, 480, 640, kp.ctypes.data, 450, C.byref(n)) == -1
        assert L.rgbdfe_detect(ctx, g.ctypes.data, None, 480, 640, None, 450, C.byref(n)) == -1
        assert L.rgbdfe_detect_sift_describe(ctx, g.ctypes.data, None, None, 480, 640, *K, 1.0, 1, kp.ctypes.data,
                                             xyz.ctypes.data, raw.ctypes.data, None, C.byref(n)) == -1
        assert L.rgbdfe_detect_sift_describe(ctx, g.ctypes.data, None, d.ctypes.data, 480, 640, *K, 1.0, 1, kp.ctypes.data,
                                             None, raw.ctypes.data, None, C.byref(n)) == -1
        pg = (C.c_void_p * 1)(g.ctypes.data)
        pd = (C.c_void_p * 1)(d.ctypes.data)
        th = fe.detector_thresholds()
        ids = np.array([5], np.int32)
        cnt = np.zeros(1, np.int32)
        assert L.rgbdfe_detect_sift_describe_batch_nodes(ctx, 1, C.cast(pg, C.c_void_p), None, C.cast(pd, C.c_void_p), 480, 640,
                                                         *K, 1.0, 1, ids.ctypes.data, 299, None, None, None,
                                                         cnt.ctypes.data) == -1      # out_stride < max_keypoints
        assert L.rgbdfe_detect_sift_describe_batch_nodes(ctx, 1, C.cast(pg, C.c_void_p), None, C.cast(pd, C.c_void_p), 480, 640,
                                                         *K, 1.0, 1, None, 300, None, None, None, cnt.ctypes.data) == -1
        dup = np.array([5, 5], np.int32)
        pg2 = (C.c_void_p * 2)(g.ctypes.data, g.ctypes.data)
        pd2 = (C.c_void_p * 2)(d.ctypes.data, d.ctypes.data)
        cnt2 = np.zeros(2, np.int32)
        assert L.rgbdfe_detect_sift_describe_batch_nodes(ctx, 2, C.cast(pg2, C.c_void_p), None, C.cast(pd2, C.c_void_p), 480,
                                                         640, *K, 1.0, 1, dup.ctypes.data, 300, None, None, None,
                                                         cnt2.ctypes.data) == -1
        assert fe.node_count(5) < 0
        assert np.array_equal(fe.detector_thresholds(), th)   # refused before any detection
    finally:
        fe.close()
