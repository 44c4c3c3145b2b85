"""CPU: the oracle of SIFTGPU descriptors behind the ORB / FAST grid detector (tests/sift_behind_detector_oracle.py) on the
photograph fixtures -- its aggregate is the grid detector's output before removeDepthless, step 2 keeps the first
max_keypoints keypoints with depth in aggregate order, and step 3's double -> float conversions round-trip as the wrapper's."""
import numpy as np
import pytest

import fast_oracle as fo
import sift_behind_detector_oracle as sbo
from oracle import pyorb
from test_gpu_orb_photos import binary_mask, intrinsics, plane_depth
from test_oracle_orb_photos import load_photos

NAMES = ["640_1", "640_2", "640_3", "800_1"]


@pytest.fixture(scope="module")
def photos():
    return load_photos()


def _depth(shape, seed):
    d = plane_depth(shape, 2.0, seed)
    d[binary_mask(shape, seed) == 0] = np.nan
    return d


@pytest.mark.parametrize("kind", ["ORB", "FAST"])
def test_aggregate_is_the_detector_before_remove_depthless(photos, kind):
    """Node::Node's ORB-extractor branch is this aggregate followed by removeDepthless, retainBest and compute: the same
    detector run through the pinned ORB-extractor composition gives the same keypoints and the same thresholds."""
    mk = 600
    a, b = sbo.Detector(kind, mk, 3), sbo.Detector(kind, mk, 3)
    for i, name in enumerate(NAMES[:3]):
        g = photos[name]
        d = _depth(g.shape, i)
        m = np.full(g.shape, 255, np.uint8)
        agg = a.detect(g, m)
        assert len(agg) <= a.max_total
        if kind == "FAST":
            kp, desc = fo.node_features(b.g, g, m, d, mk)
            kp2 = fo.remove_depthless(agg, d)
            if len(kp2) > mk:
                order = sorted(range(len(kp2)), key=lambda k: (-float(kp2["response"][k]), k))[:mk]
                kp2 = kp2[np.sort(np.array(order, np.int64))].copy()
            kp2, desc2 = fo.orb_compute(g, kp2)
        else:
            kp, desc = pyorb.node_features(b.st, g, m, d, mk)
            kp2 = fo.remove_depthless(agg, d)
            if len(kp2) > mk:
                order = sorted(range(len(kp2)), key=lambda k: (-float(kp2["response"][k]), k))[:mk]
                kp2 = kp2[np.sort(np.array(order, np.int64))].copy()
            kp2, desc2 = pyorb.compute(g, kp2)
        assert len(kp) == len(kp2)
        for f in ("x", "y", "size", "angle", "response", "octave"):
            assert np.array_equal(kp[f], kp2[f]), f
        assert np.array_equal(desc, desc2)
        assert np.array_equal(a.thresholds(), b.thresholds())


@pytest.mark.parametrize("min_depth", [False, True])
@pytest.mark.parametrize("kind", ["ORB", "FAST"])
def test_step2_keeps_the_first_k_with_depth(photos, kind, min_depth):
    det = sbo.Detector(kind, 300, 2)
    for i, name in enumerate(NAMES):
        g = photos[name]
        d = _depth(g.shape, 10 + i)
        K = intrinsics(g.shape)
        agg = det.detect(g, None)
        kept = sbo.project_kept(agg, d, K, 300, min_depth)
        rows, cols = d.shape
        if min_depth:
            from oracle import pyoracle as po
            ok = np.zeros(len(agg), bool)
            ok[po.remove_depthless_min_depth(np.stack([agg["x"], agg["y"]], 1), agg["size"], d)] = True
        else:
            r = np.minimum(np.floor(agg["y"].astype(np.float64) + 0.5).astype(np.int64), rows - 1)
            c = np.minimum(np.floor(agg["x"].astype(np.float64) + 0.5).astype(np.int64), cols - 1)
            ok = ~np.isnan(d[r, c])
        want = np.nonzero(ok)[0][:300]
        assert np.array_equal(kept, want)
        assert np.all(np.diff(kept) > 0)


def test_wrapper_conversions_round_trip(photos):
    det = sbo.Detector("ORB", 600, 3)
    agg = det.detect(photos["640_2"], None)
    keys, kl = sbo.wrapper_keys(agg)
    assert keys.dtype == np.float32
    # the rebuilt keypoints go through the same conversions to the same keys: a fixed point after one trip
    keys2, kl2 = sbo.wrapper_keys(kl)
    assert np.array_equal(keys, keys2) and np.array_equal(kl["size"], kl2["size"]) and np.array_equal(kl["angle"], kl2["angle"])
    # and the trip moves a field by at most a few float ulps
    assert np.all(np.abs(kl["size"] - agg["size"]) <= 4 * np.spacing(agg["size"]))
    assert np.all(np.abs(kl["angle"] - agg["angle"]) <= 4 * np.spacing(np.maximum(np.abs(agg["angle"]), 1.0).astype(np.float32)))
    assert np.array_equal(kl["x"], agg["x"]) and np.array_equal(kl["y"], agg["y"])
    assert np.all(kl["response"] == 0) and np.all(kl["octave"] == 0)
    fk = sbo.Detector("FAST", 600, 3).detect(photos["640_2"], None)
    _, fl = sbo.wrapper_keys(fk)
    assert np.all(fl["size"] == np.float32(7)) and np.all(np.abs(fl["angle"] + 1) <= 4 * np.spacing(np.float32(1)))
