"""CPU: the oracle of ORB descriptors behind SiftGPU's detection (tests/sift_orb_oracle.py) on the SIFT fixtures with
synthetic depth -- holes, NaN borders, a frame without depth, the cut before the border filter and the min-depth variant."""
import numpy as np
import pytest

import sift_orb_oracle as soo
from oracle import pyorb
from oracle import pyoracle as po
from test_gpu_orb_photos import binary_mask, intrinsics, plane_depth


def _depth(shape, seed, border=0):
    d = plane_depth(shape, 2.0, seed)
    d[binary_mask(shape, seed) == 0] = np.nan
    if border:
        d[:border, :] = np.nan
        d[-border:, :] = np.nan
        d[:, -border:] = np.nan
    return d


@pytest.fixture(scope="module", params=["c", "d"])
def fixture(request):
    return soo.sift_keys(request.param)


def test_wrapper_conversions_round_trip(fixture):
    _, keys, _ = fixture
    kp = soo.wrapper_keypoints(keys)
    assert np.array_equal(kp["x"], keys[:, 0]) and np.array_equal(kp["y"], keys[:, 1])
    assert np.all(kp["response"] == 0) and np.all(kp["octave"] == 0)
    # the double arithmetic stored as float: within one float ulp of the float expressions, 12 * s exact for these scales
    assert np.allclose(kp["size"], 12.0 * keys[:, 2], rtol=1e-6, atol=0)
    assert np.allclose(kp["angle"], keys[:, 3] * np.float32(180.0 / 3.1415927), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("min_depth", [False, True])
@pytest.mark.parametrize("border", [0, 40])
def test_composition_is_the_pinned_steps(fixture, min_depth, border):
    """The oracle's rows are, in SiftGPU's order, the first max_keypoints keypoints with depth, minus those within 31 pixels
    of the border; their descriptors are pyorb.compute's and their points projectTo3D's."""
    img, keys, maxf = fixture
    d = _depth(img.shape, 3, border)
    K = intrinsics(img.shape)
    mk = min(maxf, len(keys)) * 2 // 3
    kp, desc, xyz = soo.frame(img, keys, d, K, mk, min_depth)
    allk = soo.wrapper_keypoints(keys)
    if min_depth:
        kept1 = po.remove_depthless_min_depth(np.stack([allk["x"], allk["y"]], 1), allk["size"], d)
    else:
        r = np.minimum(np.floor(allk["y"].astype(np.float64) + 0.5).astype(int), img.shape[0] - 1)
        c = np.minimum(np.floor(allk["x"].astype(np.float64) + 0.5).astype(int), img.shape[1] - 1)
        kept1 = np.nonzero(~np.isnan(d[r, c]))[0]
    cut = np.asarray(kept1, np.int64)[:mk]
    h, w = img.shape
    inner = cut[(allk["x"][cut] >= 31) & (allk["x"][cut] < w - 31) & (allk["y"][cut] >= 31) & (allk["y"][cut] < h - 31)]
    assert 0 < len(kp) == len(inner) <= mk
    for f in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(kp[f], allk[f][inner]), f
    k2, d2 = pyorb.compute(img, allk[inner])
    assert np.array_equal(desc, d2) and len(k2) == len(kp)
    xy = np.stack([kp["x"], kp["y"]], 1)
    _, x2 = (po.project_to_3d_min_depth(xy, kp["size"], d, *K, 1.0, mk) if min_depth else po.project_to_3d(xy, d, *K, 1.0, mk))
    assert np.array_equal(xyz, x2) and not np.isnan(xyz).any()
    if border and not min_depth:   # (the neighbourhood minimum reaches past a NaN band)
        assert np.all((kp["y"] < h - border) & (kp["x"] < w - border) & (kp["y"] >= border - 0.5))


def test_cut_comes_before_the_border_filter(fixture):
    """With max_keypoints below the number of keypoints with depth, border keypoints inside the first max_keypoints are cut
    away after the cut: fewer than max_keypoints rows, although border-first would have filled them."""
    img, keys, maxf = fixture
    d = plane_depth(img.shape, 2.0, 5)
    K = intrinsics(img.shape)
    allk = soo.wrapper_keypoints(keys)
    h, w = img.shape
    near = (allk["x"] < 31) | (allk["x"] >= w - 31) | (allk["y"] < 31) | (allk["y"] >= h - 31)
    assert near.any()
    mk = int(np.nonzero(near)[0][0]) + 1 + (len(keys) - int(np.nonzero(near)[0][0]) - 1) // 2
    assert mk < len(keys)
    kp, desc, xyz = soo.frame(img, keys, d, K, mk)
    n_border = int(near[:mk].sum())
    assert n_border > 0 and len(kp) == mk - n_border < mk
    # border first, then the cut, would have kept max_keypoints rows
    assert int((~near).sum()) >= mk


def test_frame_without_depth(fixture):
    img, keys, maxf = fixture
    K = intrinsics(img.shape)
    kp, desc, xyz = soo.frame(img, keys, np.full(img.shape, np.nan, np.float32), K, maxf)
    assert len(kp) == 0 and desc.shape == (0, 32) and xyz.shape == (0, 4)
    # depth everywhere but under the keypoints: the rounded lookup drops them all, the neighbourhood minimum keeps them
    d = plane_depth(img.shape, 2.0, 6)
    allk = soo.wrapper_keypoints(keys)
    r = np.minimum(np.floor(allk["y"].astype(np.float64) + 0.5).astype(int), img.shape[0] - 1)
    c = np.minimum(np.floor(allk["x"].astype(np.float64) + 0.5).astype(int), img.shape[1] - 1)
    d[r, c] = np.nan
    assert len(soo.frame(img, keys, d, K, maxf)[0]) == 0
    kp, desc, xyz = soo.frame(img, keys, d, K, maxf, min_depth=True)
    assert len(kp) > 0
    zmin = [po.min_depth_in_neighborhood(d, float(k["x"]), float(k["y"]), float(k["size"])) for k in kp[:20]]
    assert np.array_equal(xyz[:20, 2], np.array(zmin, np.float32))
