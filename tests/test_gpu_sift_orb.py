"""-m gpu: ORB descriptors behind SiftGPU's detection -- rgbdfe_sift_detect_orb_describe and
rgbdfe_sift_detect_orb_describe_batch_nodes against the library's own single calls chained by hand and against the oracle
composition (tests/sift_orb_oracle.py) fed the GPU's own SIFT keypoints, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import sift_orb_oracle as soo
from oracle import pyoracle as po
from rgbdslam_v2_amd import _lib
from test_gpu_orb_photos import binary_mask, intrinsics, plane_depth
from test_oracle_orb_photos import load_photos

pytestmark = pytest.mark.gpu

NAMES = ["640_1", "640_2", "640_3", "640_4", "640_5"]


@pytest.fixture(scope="module")
def photos():
    return load_photos()


def _fe(**kw):
    from rgbdslam_v2_amd.frontend import FrontEnd
    args = dict(device_id=0, max_nodes=64, max_keypoints=1000, max_pairs_per_batch=256)
    args.update(kw)
    return FrontEnd(**args)


def _depth(shape, seed, holes=True):
    d = plane_depth(shape, 2.0, seed)
    if holes:
        d[binary_mask(shape, seed) == 0] = np.nan
        d[:, -25:] = np.nan   # a NaN border
    return d


def _frames(photos, n):
    grays = [photos[NAMES[(i * 3) % len(NAMES)]] for i in range(n)]
    depths = [_depth(g.shape, i) for i, g in enumerate(grays)]
    if n > 4:
        depths[4] = np.full(grays[4].shape, np.nan, np.float32)   # no depth anywhere
    if n > 6:
        grays[6] = np.full(grays[6].shape, 128, np.uint8)         # no SIFT feature at all
    return grays, depths


def assert_kps_equal(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(a[f], b[f]), f


def _chained(fe, g, d, K, mk, min_depth):
    """rgbdfe_sift_detect -> removeDepthless and the cut on the host -> rgbdfe_orb_compute -> rgbdfe_project_to_3d."""
    kp, _ = fe.sift_detect(g, None, mk)
    kp = soo.remove_depthless(kp, d, min_depth)[:mk]
    if len(kp) == 0:
        return kp, np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.float32)
    kp, desc = fe.orb_compute(g, kp)
    if len(kp) == 0:
        return kp, desc, np.zeros((0, 4), np.float32)
    xy = np.stack([kp["x"], kp["y"]], 1)
    if min_depth:
        kept, xyz = fe.project_to_3d_min_depth(xy, kp["size"], d, *K, 1.0, mk)
    else:
        kept, xyz = fe.project_to_3d(xy, d, *K, 1.0, mk)
    kept = np.asarray(kept, np.int64)
    return kp[kept], desc[kept], xyz


# ---- (a), (b): one frame -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_depth", [False, True])
@pytest.mark.parametrize("mk", [1000, 300])
def test_single_frame_equals_chain_and_oracle(photos, mk, min_depth):
    fe = _fe()
    try:
        fe.set_feature_min_depth(min_depth)
        for i, name in enumerate(NAMES):
            g = photos[name]
            d = _depth(g.shape, i)
            K = intrinsics(g.shape)
            kp, desc, xyz = fe.sift_detect_orb_describe(g, d, *K, max_keypoints=mk)
            ck, cd, cx = _chained(fe, g, d, K, mk, min_depth)
            assert 0 < len(kp) <= mk
            assert_kps_equal(kp, ck)
            assert np.array_equal(desc, cd) and np.array_equal(xyz, cx)
            # (b) the oracle fed the GPU's own SIFT keypoints (orientations are only within tolerance of the reference's)
            skp, _ = fe.sift_detect(g, None, mk)
            ok, od, ox = soo.frame_from_keypoints(g, skp, d, K, mk, min_depth)
            assert_kps_equal(kp, ok)
            assert np.array_equal(desc, od) and np.array_equal(xyz, ox)
    finally:
        fe.close()


def test_cut_before_border_on_the_device(photos):
    """max_keypoints cuts SiftGPU's list before the border filter: fewer rows than max_keypoints although more interior
    keypoints with depth exist."""
    fe = _fe()
    try:
        g = photos["640_2"]
        d = plane_depth(g.shape, 2.0, 1)
        K = intrinsics(g.shape)
        skp, _ = fe.sift_detect(g, None, 1000)
        h, w = g.shape
        near = (skp["x"] < 31) | (skp["x"] >= w - 31) | (skp["y"] < 31) | (skp["y"] >= h - 31)
        first = int(np.nonzero(near)[0][0])
        mk = min(first + 1 + (len(skp) - first - 1) // 2, 1000)
        kp, desc, xyz = fe.sift_detect_orb_describe(g, d, *K, max_keypoints=mk)
        skp2, _ = fe.sift_detect(g, None, mk)
        n_border = int(((skp2["x"][:mk] < 31) | (skp2["x"][:mk] >= w - 31) | (skp2["y"][:mk] < 31) |
                        (skp2["y"][:mk] >= h - 31)).sum())
        assert n_border > 0 and len(kp) == min(mk, len(skp2)) - n_border
    finally:
        fe.close()


# ---- (c), (d): the batch ------------------------------------------------------------------------------------------------
def _pairs(n, ids):
    q, t = [], []
    for f in range(1, n):
        for c in (1, 2, 3):
            if f - c >= 0 and ids[f] >= 0 and ids[f - c] >= 0:
                q.append(ids[f]); t.append(ids[f - c])
    return np.array(q, np.int32), np.array(t, np.int32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
def test_batch_equals_single_calls(photos, n):
    mk = 500
    grays, depths = _frames(photos, n)
    K = intrinsics(grays[0].shape)
    ids = np.arange(10, 10 + n, dtype=np.int32)
    if n > 9:
        ids[9] = -1
    fe, fe2, fe3 = _fe(max_keypoints=mk), _fe(max_keypoints=mk), _fe(max_keypoints=mk)
    try:
        out = fe.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=mk)
        cnt = fe3.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=mk, return_features=False)
        assert np.array_equal(cnt, [len(o[0]) for o in out])
        feats = []
        for f in range(n):
            kp, desc, xyz = fe2.sift_detect_orb_describe(grays[f], depths[f], *K, max_keypoints=mk)
            assert_kps_equal(out[f][0], kp)
            assert np.array_equal(out[f][1], desc) and np.array_equal(out[f][2], xyz)
            feats.append((desc, xyz))
            if ids[f] >= 0:
                fe2.upload_node(int(ids[f]), desc, xyz)
                assert fe.node_count(int(ids[f])) == len(kp) == fe3.node_count(int(ids[f]))
        if n > 4:
            assert cnt[4] == 0
        if n > 6:
            assert cnt[6] == 0
        q, t = _pairs(n, ids)
        if len(q):
            r1 = fe.match_pair_list(q, t)
            r2 = fe2.match_pair_list(q, t)
            r3 = fe3.match_pair_list(q, t)
            assert r1.tobytes() == r2.tobytes() == r3.tobytes()
            if n == 9:   # (d) and the oracle's pair op on the same features
                prm = po.default_params(seed=fe.params.seed, depth_cov=fe.params.depth_cov)
                for rec, a, b in zip(r1, q, t):
                    fa, fb = int(a) - 10, int(b) - 10
                    ref = po.match_node_pair(feats[fa][0], feats[fa][1], int(a), feats[fb][0], feats[fb][1], int(b), prm)
                    m = ref["n_all"]
                    assert rec["n_all"] == m and rec["n_inl"] == ref["n_inl"]
                    assert np.array_equal(rec["all_q"][:m], ref["all_q"]) and np.array_equal(rec["all_t"][:m], ref["all_t"])
    finally:
        fe.close()
        fe2.close()
        fe3.close()


def test_nodes_match_the_oracle_features(photos):
    """(d): nodes of the batch give the MatchingResults of pyoracle.match_node_pair on the oracle's own features."""
    mk = 600
    grays, depths = _frames(photos, 4)
    K = intrinsics(grays[0].shape)
    ids = np.arange(4, dtype=np.int32)
    fe = _fe(max_keypoints=mk)
    try:
        fe.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=mk, return_features=False)
        feats = []
        for g, d in zip(grays, depths):
            skp, _ = fe.sift_detect(g, None, mk)
            _, od, ox = soo.frame_from_keypoints(g, skp, d, K, mk)
            feats.append((od, ox))
        q = np.array([1, 2, 3, 3], np.int32)
        t = np.array([0, 1, 2, 0], np.int32)
        out = fe.match_pair_list(q, t)
        prm = po.default_params(seed=fe.params.seed, depth_cov=fe.params.depth_cov)
        for rec, a, b in zip(out, q, t):
            ref = po.match_node_pair(feats[a][0], feats[a][1], int(a), feats[b][0], feats[b][1], int(b), prm)
            m = ref["n_all"]
            assert rec["n_all"] == m and rec["n_inl"] == ref["n_inl"] and m > 0
            assert np.array_equal(rec["all_q"][:m], ref["all_q"]) and np.array_equal(rec["all_t"][:m], ref["all_t"])
            assert np.array_equal(rec["all_hd"][:m], ref["all_hd"])
    finally:
        fe.close()


# ---- (e), (f): modes, node-table rules, errors, two devices ------------------------------------------------------------
def test_min_depth_batch(photos):
    mk = 400
    grays, depths = _frames(photos, 9)
    K = intrinsics(grays[0].shape)
    ids = np.arange(9, dtype=np.int32)
    fe, fe2 = _fe(max_keypoints=mk), _fe(max_keypoints=mk)
    try:
        for f in (fe, fe2):
            f.set_feature_min_depth(True)
        out = fe.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=mk)
        for f in range(9):
            kp, desc, xyz = _chained(fe2, grays[f], depths[f], K, mk, True)
            assert_kps_equal(out[f][0], kp)
            assert np.array_equal(out[f][1], desc) and np.array_equal(out[f][2], xyz)
    finally:
        fe.close()
        fe2.close()


def test_node_ids_rewrite_capacity_and_errors(photos):
    mk = 300
    grays, depths = _frames(photos, 9)
    K = intrinsics(grays[0].shape)
    fe = _fe(max_keypoints=mk, max_nodes=12)
    try:
        # an existing float node of another kind is rewritten in place as an ORB node
        fe.upload_float_node(3, np.ones((5, 128), np.float32), np.ones((5, 4), np.float32))
        ids = np.array([0, 1, 2, 3, -1, 5, 6, -7, 8], np.int32)
        cnt = fe.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=mk, return_features=False)
        out = fe.sift_detect_orb_describe_batch_nodes(grays, depths, *K, np.full(9, -1, np.int32), max_keypoints=mk)
        assert np.array_equal(cnt, [len(o[0]) for o in out])
        for f, i in enumerate(ids):
            if i >= 0:
                assert fe.node_count(int(i)) == cnt[f]
        assert fe.node_count(4) < 0 and fe.node_count(7) < 0
        assert cnt[4] == 0 and cnt[6] == 0 and fe.node_count(6) == 0   # empty frames become empty nodes
        r = fe.match_pair_list(np.array([3, 2], np.int32), np.array([1, 3], np.int32))
        assert r[0]["n_all"] > 0
        # capacity: 5 free slots, 6 fresh ids -> refused before any work, nothing registered
        with pytest.raises(Exception):
            fe.sift_detect_orb_describe_batch_nodes(grays[:6], depths[:6], *K, np.arange(100, 106, dtype=np.int32),
                                                    max_keypoints=mk, return_features=False)
        assert all(fe.node_count(i) < 0 for i in range(100, 106))
        L, ctx = fe._L, fe._ctx
        g, d = grays[0], depths[0]
        pg = (C.c_void_p * 1)(g.ctypes.data)
        pd = (C.c_void_p * 1)(d.ctypes.data)
        one = np.array([50], np.int32)
        c1 = np.zeros(1, np.int32)
        kp = np.zeros(mk, _lib.KEYPOINT_DTYPE)
        desc = np.zeros((mk, 32), np.uint8)
        xyz = np.zeros((mk, 4), np.float32)
        n = C.c_int32(0)

        def batch(ids_, stride, maxk, kp_=None, desc_=None, xyz_=None):
            return L.rgbdfe_sift_detect_orb_describe_batch_nodes(ctx, len(ids_), C.cast(pg if len(ids_) == 1 else pg2, C.c_void_p),
                                                                 C.cast(pd if len(ids_) == 1 else pd2, C.c_void_p), 480, 640, *K,
                                                                 1.0, maxk, ids_.ctypes.data, stride, kp_, desc_, xyz_,
                                                                 (c1 if len(ids_) == 1 else c2).ctypes.data)
        pg2 = (C.c_void_p * 2)(g.ctypes.data, g.ctypes.data)
        pd2 = (C.c_void_p * 2)(d.ctypes.data, d.ctypes.data)
        c2 = np.zeros(2, np.int32)
        assert batch(one, mk - 1, mk, None, desc.ctypes.data, None) == -5            # out_stride < max_keypoints, an output
        assert batch(np.array([50, 50], np.int32), mk, mk) == -1                    # an id twice
        assert batch(one, 0, 0) == -1 and batch(one, 0, 1001) == -1                # max_keypoints outside [1, 1000]
        assert fe.node_count(50) < 0
        assert batch(one, 0, mk) == 0 and fe.node_count(50) == c1[0] > 0           # NULL outputs, stride 0
        assert L.rgbdfe_sift_detect_orb_describe(ctx, g.ctypes.data, d.ctypes.data, 480, 640, *K, 1.0, 0, kp.ctypes.data,
                                                 desc.ctypes.data, xyz.ctypes.data, C.byref(n)) == -1
        assert L.rgbdfe_sift_detect_orb_describe(ctx, g.ctypes.data, None, 480, 640, *K, 1.0, mk, kp.ctypes.data,
                                                 desc.ctypes.data, xyz.ctypes.data, C.byref(n)) == -1
        # an empty frame through the single call
        k0, d0, x0 = fe.sift_detect_orb_describe(np.full((480, 640), 128, np.uint8), d, *K, max_keypoints=mk)
        assert len(k0) == 0 and d0.shape == (0, 32) and x0.shape == (0, 4)
    finally:
        fe.close()


def test_two_devices_listed_twice(photos):
    mk = 400
    grays, depths = _frames(photos, 9)
    K = intrinsics(grays[0].shape)
    ids = np.arange(20, 29, dtype=np.int32)
    fe, fe2 = _fe(max_keypoints=mk), _fe(max_keypoints=mk, device_ids=[0, 0])
    try:
        out = fe.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=mk)
        out2 = fe2.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=mk)
        cnt2 = fe2.sift_detect_orb_describe_batch_nodes(grays[::-1], depths[::-1], *K, ids[::-1].copy(), max_keypoints=mk,
                                                        return_features=False)
        cnt = fe.sift_detect_orb_describe_batch_nodes(grays[::-1], depths[::-1], *K, ids[::-1].copy(), max_keypoints=mk,
                                                      return_features=False)
        assert np.array_equal(cnt, cnt2)
        for a, b in zip(out, out2):
            assert_kps_equal(a[0], b[0])
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        q, t = _pairs(9, ids)
        assert fe.match_pair_list(q, t).tobytes() == fe2.match_pair_list(q, t).tobytes()
    finally:
        fe.close()
        fe2.close()
