"""CPU: the FAST detector's oracle (tests/fast_oracle.py).

1. The helper's grid + adjuster + Node::Node composition, with cv::ORB's detect (pyorb.detect) plugged in as the cell detector,
   reproduces the pinned C restatement (pyorb.grid_detect / pyorb.node_features) frame after frame -- keypoints, descriptors
   and thresholds -- over a sequence that drives tooFew, tooMany and the empty-mask break.
2. The property the GPU design rests on: FAST's keypoints at any threshold t >= 2 are exactly its keypoints at threshold 2
   whose response is >= t (order and scores included), with and without a mask."""
import numpy as np
import pytest

from oracle import pyorb
import fast_oracle as fo
from test_oracle_orb_photos import load_photos, variant

KINDS = ("orig", "dark", "sat", "inv")


@pytest.fixture(scope="module")
def photos():
    return load_photos()


def _orb_cell(sub, sub_mask, t):
    return pyorb.detect(sub, sub_mask, t)


def _kp_equal(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(a[f], b[f]), f


def _mask_with_empty_cell(shape):
    m = np.full(shape, 255, np.uint8)
    h, w = shape
    m[: h // 2, : w // 2] = 0    # the top-left cell of a 3 x 3 grid sees no depth at all
    return m


def _sequence(photos):
    """(gray, mask, depth) frames: textured photographs (tooMany), low-contrast ones (tooFew, re-detection down to the
    floor), a flat frame (zero keypoints everywhere) and a mask with an empty cell (the hasNonZero break)."""
    flat = np.full((480, 640), 128, np.uint8)
    seq = [("640_1", "orig", "full"), ("640_3", "orig", "empty"), ("640_2", "dark", "full"), ("flat", "", "full"),
           ("640_4", "sat", "empty"), ("640_5", "dark", "none"), ("flat", "", "none"), ("640_1", "inv", "full")]
    rng = np.random.default_rng(5)
    out = []
    for name, kind, mk in seq:
        g = flat if name == "flat" else variant(photos[name], kind)
        m = None if mk == "none" else (np.full(g.shape, 255, np.uint8) if mk == "full" else _mask_with_empty_cell(g.shape))
        d = (2.0 + rng.normal(0, 0.01, g.shape)).astype(np.float32)
        d[rng.random(g.shape) < 0.05] = np.nan
        out.append((g, m, d))
    return out


@pytest.mark.parametrize("grid,budget", [(3, 600), (2, 1000)])
def test_grid_composition_reproduces_the_orb_restatement(photos, grid, budget):
    seq = _sequence(photos)
    mine = fo.Grid(budget, grid)
    ref = pyorb.grid_state(budget, grid)
    seen_up = seen_down = seen_break = False
    for g, m, _ in seq:
        before = list(mine.thresh)
        a = mine.detect(g, m, _orb_cell)
        b = pyorb.grid_detect(ref, g, m)
        _kp_equal(a, b)
        assert mine.thresh == list(ref.thresh[: grid * grid])
        for c, (t0, t1) in enumerate(zip(before, mine.thresh)):
            seen_up |= t1 > t0
            seen_down |= t1 < t0
            seen_break |= t1 == max(t0 * 0.7, 2.0) and t0 > 2 and mine.max_iters > 1   # one x0.7 step, then the break
    assert seen_up and seen_down and seen_break


def test_node_composition_reproduces_orb_node_features(photos):
    seq = _sequence(photos)
    for grid, budget in ((3, 600), (6, 1500)):
        mine = fo.Grid(budget, grid)
        ref = pyorb.grid_state(budget, grid)
        for g, m, d in seq:
            mm = np.full(g.shape, 255, np.uint8) if m is None else m
            ka, da = fo.node_features(mine, g, mm, d, budget, cell_detect=_orb_cell)
            kb, db = pyorb.node_features(ref, g, mm, d, budget)
            _kp_equal(ka, kb)
            assert np.array_equal(da, db)
            assert mine.thresh == list(ref.thresh[: grid * grid])


THRESHOLDS = (2, 3, 5, 9, 14, 20, 40, 60, 120, 254)


@pytest.mark.parametrize("kind", KINDS)
def test_fast_keypoints_at_t_are_the_floor_two_keypoints_scoring_at_least_t(photos, kind):
    rng = np.random.default_rng(11)
    for name in sorted(photos):
        g = variant(photos[name], kind)
        mask = np.where(rng.random((g.shape[0] // 16 + 1, g.shape[1] // 16 + 1)) < 0.3, 0, 255).astype(np.uint8)
        mask = np.ascontiguousarray(np.repeat(np.repeat(mask, 16, 0), 16, 1)[: g.shape[0], : g.shape[1]])
        for m in (None, mask):
            base = fo.fast_detect(g, m, 2)
            assert len(base) > 0
            for t in THRESHOLDS:
                at_t = fo.fast_detect(g, m, t)
                _kp_equal(at_t, base[base["response"] >= t])
