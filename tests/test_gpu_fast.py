"""-m gpu: feature_detector_type "FAST" (rgbdfe_set_detector_type, rgbdfe_fast_detect) against tests/fast_oracle.py --
photographs and their photometric variants, every comparison exact: positions, order, responses, descriptor bytes, xyz1 bits
and the per-cell thresholds after every frame."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fast_oracle as fo
from oracle import pyoracle as po
from test_gpu_orb_photos import binary_mask, depth_mask, frame_image, intrinsics, plane_depth
from test_oracle_orb_photos import load_photos

pytestmark = pytest.mark.gpu

KINDS = ("orig", "dark", "sat", "inv")
_POOL = ThreadPoolExecutor(max_workers=min(16, po.usable_cpus()))
_CACHE = {}


def _oracle(key, fn, *args, **kw):
    if key not in _CACHE:
        fo._lib()
        _CACHE[key] = _POOL.submit(fn, *args, **kw)
    return _CACHE[key]


@pytest.fixture(scope="module")
def photos():
    P = load_photos()
    P["1600_c1283"] = np.ascontiguousarray(P["1600"][57:1014, 411:1694])     # 1283x957: odd, off every tile seam
    return P


def _fe(**kw):
    from rgbdslam_v2_amd.frontend import FrontEnd
    args = dict(device_id=0, max_nodes=160, max_keypoints=4096, max_pairs_per_batch=512)
    args.update(kw)
    return FrontEnd(**args)


@pytest.fixture(scope="module")
def fe():
    f = _fe()
    yield f
    f.close()


def assert_kps_equal(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(a[f], b[f]), f


# ---- rgbdfe_fast_detect: one image, one threshold ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["640_1", "640_3", "800_2", "800_4", "1600_c1283"])
def test_fast_detect_matches_oracle(fe, photos, name, kind):
    g = frame_image(photos, name, kind)
    masks = {"none": None, "binary": binary_mask(g.shape, 3), "depth": depth_mask(g.shape, 4)}
    for t in (2, 5, 20, 60, 254):
        for mk, m in masks.items():
            ref = _oracle(("fd", name, kind, t, mk), fo.fast_detect, g, m, t).result()
            assert_kps_equal(fe.fast_detect(g, m, t, capacity=len(ref) + 16), ref)


def test_fast_detect_tiny_images_and_clamped_thresholds(fe, photos):
    g = photos["640_3"]
    for h, w in ((6, 5), (7, 7), (9, 12), (40, 3)):
        sub = np.ascontiguousarray(g[100:100 + h, 200:200 + w])
        for t in (-3, 0, 1, 2, 9, 300):
            assert_kps_equal(fe.fast_detect(sub, None, t), fo.fast_detect(sub, None, t))
    for t, same in ((-7, 0), (999, 255)):   # cv::FAST clamps its threshold to [0, 255]
        assert_kps_equal(fe.fast_detect(g, None, t), fo.fast_detect(g, None, same))


def test_fast_detect_capacity(fe, photos):
    from rgbdslam_v2_amd.frontend import RgbdfeError
    g = photos["800_2"]
    ref = fo.fast_detect(g, None, 5)
    with pytest.raises(RgbdfeError, match="capacity"):
        fe.fast_detect(g, None, 5, capacity=len(ref) - 1)                       # one row short
    assert_kps_equal(fe.fast_detect(g, None, 5, capacity=len(ref)), ref)        # exactly enough rows
    assert_kps_equal(fe.fast_detect(g, None, 20), fo.fast_detect(g, None, 20))


# ---- Node::Node under FAST ----------------------------------------------------------------------------------------------
SEQ = [("640_1", "orig"), ("640_2", "orig"), ("640_4", "sat"), ("640_5", "inv"), ("640_1", "dark"), ("640_3", "orig"),
       ("640_4", "orig"), ("640_2", "dark"), ("640_5", "dark"), ("640_3", "inv"), ("640_1", "sat"), ("640_3", "sat")]


def _frames(photos, seq=SEQ):
    grays = [frame_image(photos, n, k) for n, k in seq]
    shape = grays[0].shape
    masks = [binary_mask(shape, f) if f % 3 != 2 else np.full(shape, 255, np.uint8) for f in range(len(seq))]
    depths = [plane_depth(shape, 2.0 + 0.1 * (f % 4), f) for f in range(len(seq))]
    for f in range(1, len(seq), 4):
        depths[f][(np.arange(shape[0]) % 7 == 0)] = np.nan       # rows without depth: removeDepthless drops keypoints
    for f in (6, 7):   # two faint frames in a row: the adjuster walks the cells' thresholds down to the floor of 2
        if f < len(seq) - 1:
            grays[f] = (grays[f].astype(np.float32) * 0.04 + 100).astype(np.uint8)
    return grays, masks, depths, intrinsics(shape)


def _single_calls(fe, grays, masks, depths, K):
    out = []
    for g, m, d in zip(grays, masks, depths):
        kp, desc, xyz = fe.detect_describe(g, m, d, *K)
        out.append((kp, desc, xyz, fe.detector_thresholds()))
    return out


def _check(res, ref):
    assert len(res) == len(ref)
    for f, ((kp, desc, xyz, thr), (rk, rdesc, rxyz, rthr)) in enumerate(zip(res, ref)):
        assert_kps_equal(kp, rk)
        assert np.array_equal(desc, rdesc), f
        assert np.array_equal(xyz.view(np.uint32), rxyz.view(np.uint32)), f
        assert np.array_equal(thr, rthr), f


@pytest.mark.parametrize("budget,grid", [(600, 3), (600, 2), (1000, 6), (1000, 3), (4000, 2), (4000, 6)])
def test_detect_describe_sequence_matches_oracle(fe, photos, budget, grid):
    grays, masks, depths, K = _frames(photos)
    ref = _oracle(("seq", budget, grid), fo.run_sequence, grays, masks, depths, K, budget, grid)
    fe.detector_configure(max_keypoints=budget, grid_resolution=grid)
    fe.set_detector_type("FAST")
    assert np.array_equal(fe.detector_thresholds(), np.full(grid * grid, 20.0))
    res = _single_calls(fe, grays, masks, depths, K)
    _check(res, ref.result())
    assert min(len(r[0]) for f, r in enumerate(res) if f not in (6, 7)) > 50
    assert any(r[3].min() == 2.0 for r in res)              # the faint frames walk some cell down to the floor


def test_detect_describe_min_depth_and_cloud(fe, photos):
    grays, masks, depths, K = _frames(photos, SEQ[:8])
    ref = fo.run_sequence(grays, masks, depths, K, 1000, 3, min_depth=True)
    fe.detector_configure(max_keypoints=1000)
    fe.set_detector_type("FAST")
    fe.set_feature_min_depth(True)
    _check(_single_calls(fe, grays, masks, depths, K), ref)
    fe.set_feature_min_depth(False)
    # the point-cloud constructor's path (node.cpp:252-369): grid detect -> projectTo3D(cloud) -> compute
    grid = fo.Grid(1000, 3)
    grid.thresh = list(fe.detector_thresholds())
    rng = np.random.default_rng(2)
    for g, m, d in zip(grays[:4], masks[:4], depths[:4]):
        rows, cols = g.shape
        u, v = np.meshgrid(np.arange(cols, dtype=np.float32), np.arange(rows, dtype=np.float32))
        cloud = np.zeros((rows, cols, 4), np.float32)
        cloud[..., 2] = d
        cloud[..., 0] = (u - K[2]) * d / K[0]
        cloud[..., 1] = (v - K[3]) * d / K[1]
        cloud[..., 2][rng.random((rows, cols)) < 0.03] = np.nan
        kp, desc, xyz = fe.detect_describe_cloud(g, m, cloud, 2.25)   # (frames at 2.3 m: beyond the maximum depth)
        det = grid.detect(g, m, fo.fast_detect)
        kept, pxyz = po.project_to_3d_cloud(np.stack([det["x"], det["y"]], 1), cloud, 2.25, 1000)
        k3 = det[kept]
        inside = (k3["x"] >= 31) & (k3["x"] < cols - 31) & (k3["y"] >= 31) & (k3["y"] < rows - 31)
        rk, rdesc = fo.orb_compute(g, k3)
        assert_kps_equal(kp, rk)
        assert np.array_equal(desc, rdesc) and np.array_equal(xyz, pxyz[inside])
        assert np.array_equal(fe.detector_thresholds(), np.array(grid.thresh))
        assert len(kp) > 50 or float(np.nanmedian(d)) > 2.25


# ---- batches and nodes ----------------------------------------------------------------------------------------------------
def _run_frames(photos, n):
    names = [("640_1", "orig"), ("640_2", "orig"), ("640_3", "sat"), ("640_4", "inv"), ("640_5", "dark"), ("640_3", "orig"),
             ("640_2", "inv")]
    grays = [frame_image(photos, *names[(f * 3) % len(names)]) for f in range(n)]
    shape = grays[0].shape
    masks = [binary_mask(shape, f % 5) if f % 4 else None for f in range(n)]
    depths = [plane_depth(shape, 2.0 + 0.05 * (f % 6), f % 9) for f in range(n)]
    if n > 3:
        depths[3] = np.full(shape, np.nan, np.float32)     # no depth anywhere: no features, an empty node
    return grays, masks, depths, intrinsics(shape)


@pytest.mark.parametrize("n", [1, 7, 64, 65, 130])
def test_batch_and_batch_nodes_equal_single_calls(fe, photos, n):
    """Single calls -> upload_node, then the batch, then the batch into the same node ids (rewritten in place), on one
    context: set_detector_type("FAST") restarts the detector before every run."""
    grays, masks, depths, K = _run_frames(photos, n)
    a = b = fe
    a.detector_configure(max_keypoints=1000)
    a.set_detector_type("FAST")
    single = _single_calls(a, grays, masks, depths, K)
    for f in range(n):
        a.upload_node(f, single[f][1], single[f][2])
    pq = np.array([f for f in range(1, n) for c in (1, 7) if f - c >= 0], np.int32)    # (f, f - 7): the same photograph
    pt = np.array([f - c for f in range(1, n) for c in (1, 7) if f - c >= 0], np.int32)
    ref_pairs = a.match_pair_list(pq, pt) if len(pq) else None
    b.set_detector_type("FAST")
    got = b.detect_describe_batch(grays, masks, depths, *K)
    thr = b.detector_thresholds()
    _check([g + (thr,) for g in got[-1:]], [single[-1]])
    for (k1, d1, x1), (k2, d2, x2, _) in zip(got, single):
        assert_kps_equal(k1, k2)
        assert np.array_equal(d1, d2) and np.array_equal(x1, x2)
    b.set_detector_type("FAST")                          # thresholds back to 20: the nodes call sees the same frames afresh
    ids = np.arange(n, dtype=np.int32)
    cnt = b.detect_describe_batch(grays, masks, depths, *K, node_ids=ids, host_outputs=False)
    assert np.array_equal(cnt, [len(s[0]) for s in single])
    assert all(b.node_count(f) == len(single[f][0]) for f in range(n))
    if ref_pairs is not None:
        assert b.match_pair_list(pq, pt).tobytes() == ref_pairs.tobytes()
        assert n <= 7 or (ref_pairs["id1"] >= 0).sum() > 0
    b.set_detector_type("FAST")
    got2 = b.detect_describe_batch(grays, masks, depths, *K, node_ids=ids)   # host outputs and nodes; ids exist: rewritten
    for (k1, d1, x1), (k2, d2, x2, _) in zip(got2, single):
        assert_kps_equal(k1, k2)
        assert np.array_equal(d1, d2) and np.array_equal(x1, x2)
    if ref_pairs is not None:
        assert b.match_pair_list(pq, pt).tobytes() == ref_pairs.tobytes()


def test_batch_nodes_on_a_two_device_handle(fe, photos):
    n = 9
    grays, masks, depths, K = _run_frames(photos, n)
    fe.detector_configure(max_keypoints=600)
    fe.set_detector_type("FAST")
    single = _single_calls(fe, grays, masks, depths, K)
    pq = np.arange(1, n, dtype=np.int32)
    pt = np.arange(0, n - 1, dtype=np.int32)
    two = _fe(max_nodes=n + 2, device_ids=[0, 0])
    refs = []
    for b in (fe, two):
        b.detector_configure(max_keypoints=600)
        b.set_detector_type("FAST")
        cnt = b.detect_describe_batch(grays, masks, depths, *K, node_ids=np.arange(n, dtype=np.int32), host_outputs=False)
        assert np.array_equal(cnt, [len(s[0]) for s in single])
        refs.append(b.match_pair_list(pq, pt).tobytes())
    two.close()
    assert refs[0] == refs[1]


def test_switching_detector_types(fe, photos):
    from rgbdslam_v2_amd.frontend import RgbdfeError
    grays, masks, depths, K = _frames(photos, SEQ[:4])
    fresh = _fe(max_nodes=2, max_keypoints=1024, max_pairs_per_batch=4)
    fresh.detector_configure(max_keypoints=1000)
    ref = _single_calls(fresh, grays, masks, depths, K)
    fresh.close()
    fe.detector_configure(max_keypoints=1000)
    fe.set_detector_type("ORB")
    _check(_single_calls(fe, grays[:2], masks[:2], depths[:2], K), ref[:2])
    fe.set_detector_type("FAST")
    assert np.array_equal(fe.detector_thresholds(), np.full(9, 20.0))
    fast = _single_calls(fe, grays, masks, depths, K)
    assert all(np.all(r[0]["size"] == 7) and np.all(r[0]["angle"] == -1) for r in fast)
    fe.set_detector_type("ORB")
    assert np.array_equal(fe.detector_thresholds(), np.full(9, 20.0))
    _check(_single_calls(fe, grays, masks, depths, K), ref)
    with pytest.raises(ValueError):
        fe.set_detector_type("SURF")
    with pytest.raises(RgbdfeError):
        fe._check(fe._L.rgbdfe_set_detector_type(fe._ctx, 7))
