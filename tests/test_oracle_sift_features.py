"""CPU: tests/sift_feature_reference.py -- the float64 restatement of SIFT orientation assignment and the descriptor --
against the reference's own pipeline compiled on the CUDA emulation (oracle/_ref/libref_siftgpu.so), on the planted images
and keypoint lists tests/test_gpu_sift_features.py then runs through the HIP kernels.

Three things are established here, none of them on the code under test:
  * the restatement IS the reference's computation: every stable candidate gets the same number of orientations in the
    same order with codes within 2, descriptors agree to a few 1e-6;
  * the planted inputs hold the cases they are planted for (censuses), and at most 5 % of an image's candidates are
    unstable, i.e. could be decided either way by a correct float32 implementation;
  * the compiled float32 reference's largest deviation from the restatement -- the figure the GPU tolerance is 8 x of
    (sift_feature_reference.REF_DEVIATION)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
import sift_feature_reference as sf

pytestmark = pytest.mark.skipif(po.ref_siftgpu_lib() is None, reason="oracle/_ref/libref_siftgpu.so not built")
UNSTABLE_CAP = 0.05
SMALL_CELL = 1.0     # pixels: below it the reference's own rounding of a cell's centre governs (see the last test)


@functools.lru_cache(maxsize=None)
def frame(name):
    """The reference's detection of a planted image and the restatement of every candidate."""
    img = sf.IMAGES[name]()
    keys, desc, _ = po.ref_sift_detect(img, 0)
    geo = po.ref_sift_geometry()
    on = geo["octave_num"]
    planes = {(o, l): po.ref_sift_level(o, l, 0) for o in range(on) for l in range(geo["levels"])}
    cands = {(o, j): po.ref_sift_candidates(o, j) for o in range(on) for j in range(geo["dog_levels"])}
    records, levels = sf.restate_orientations(lambda o, l: planes[(o, l)], lambda o, j: cands[(o, j)], on)
    owned = sf.walk_features(records, keys[:, :2], geo["octave_min"])
    return dict(img=img, keys=keys, desc=desc, geo=geo, planes=planes, records=records, levels=levels, owned=owned)


relative_deviation = sf.relative_deviation


@pytest.mark.parametrize("name", sf.DETECT_IMAGES)
def test_orientations_of_stable_candidates_equal_the_reference(name):
    fr = frame(name)
    assert len(fr["records"]) >= 20
    worst = 0
    for r, mine in zip(fr["records"], fr["owned"]):
        o = r["ori"]
        if not o["stable"]:
            continue
        assert len(mine) == o["n_orient"], (r["octave"], r["level"], r["rec"], o["codes"])
        for f, code in zip(mine, o["codes"]):
            got, off = sf.key_orientation_code(fr["keys"][f, 3])
            assert off < 0.05
            d = sf.circular_code_distance(got, code)
            worst = max(worst, d)
            assert d <= 2, (r["octave"], r["level"], r["rec"], got, code)
    print(name, "largest code distance", worst)


@pytest.mark.parametrize("name", sf.DETECT_IMAGES)
def test_unstable_candidates_are_rare(name):
    """A condition on the planted image, not a measurement: an image that exceeds the cap is to be replaced."""
    rec = frame(name)["records"]
    unstable = [r for r in rec if not r["ori"]["stable"]]
    print(name, len(unstable), "of", len(rec), [r["ori"]["reasons"] for r in unstable])
    assert len(unstable) <= UNSTABLE_CAP * len(rec)


def test_census_of_the_planted_detection_cases():
    rec = [r for name in sf.DETECT_IMAGES for r in frame(name)["records"]]
    clipped = [r for r in rec if any(r["ori"]["cut"])]
    assert len(clipped) >= 20 and len({r["octave"] for r in clipped}) >= 3
    assert np.array([r["ori"]["cut"] for r in clipped]).any(axis=0).all()          # left, right, top, bottom
    generic = frame("generic")["records"]                                           # ... and on one image alone
    cut = [r for r in generic if any(r["ori"]["cut"])]
    assert len(cut) >= 20 and len({r["octave"] for r in cut}) >= 3 and np.array([r["ori"]["cut"] for r in cut]).any(axis=0).all()
    assert sum(r["ori"]["n_orient"] == 2 for r in frame("corners")["records"]) >= 10
    assert sum(r["ori"]["n_orient"] == 2 for r in rec) >= 50
    first = [b for r in rec for b in r["ori"]["best"]]
    assert first.count(0) >= 3 and first.count(DIR_LAST) >= 3                       # the circular neighbours
    facing = [float(sf.code_direction(c)) for r in rec for c in r["ori"]["codes"][:r["ori"]["n_orient"]]]
    quadrant = np.floor(np.array(facing) / (np.pi / 2)).astype(int)
    assert all((quadrant == q).sum() >= 5 for q in range(4)) and (np.array(facing) > np.pi).sum() >= 5


DIR_LAST = sf.DIR_BINS - 1


@functools.lru_cache(maxsize=None)
def described(name):
    """Every planted keypoint list of an image through the reference's describe mode and through the restatement."""
    img = sf.IMAGES[name]()
    po.ref_sift_detect(img, 10)                       # (builds the pyramid whose planes are read below)
    geo = po.ref_sift_geometry()
    on = geo["octave_num"]
    levels, out = {}, {}
    lists = sf.describe_lists(img.shape[0], img.shape[1], on, heavy=(name == "blocks17"))
    planes = {(o, j): po.ref_sift_level(o, j + 1, 0) for o in range(on) for j in range(geo["dog_levels"])}
    for lname, kp in lists.items():
        keys = np.array([sf.keypoint_to_key(*row) for row in kp], np.float32)
        ref = po.ref_sift_describe(img, keys)
        got, edge = sf.assign_levels(keys, on, geo["octave_min"])
        rows = []
        for k, g in enumerate(got):
            o, j, feat = g
            if (o, j) not in levels:
                levels[(o, j)] = sf.Level(planes[(o, j)])
            lv = levels[(o, j)]
            rows.append(dict(octave=o, level=j, feat=feat, shape=(lv.h, lv.w), window=sf.descriptor_window((lv.h, lv.w), feat),
                             desc=sf.descriptor(lv, feat), cell=abs(float(feat[2])) * sf.CELL_SCALES))
        out[lname] = dict(kp=kp, keys=keys, ref=ref, rows=rows, edge=edge)
    return out, on


@pytest.mark.parametrize("name", sf.DESCRIBE_IMAGES + ("strip",))
def test_census_of_the_planted_keypoint_lists(name):
    lists, on = described(name)
    bands = {(o, j) for o in range(on) for j in range(sf.DOG_LEVELS)}
    assert {(r["octave"], r["level"]) for r in lists["all_bands"]["rows"]} == bands             # every segment in use
    used = {(r["octave"], r["level"]) for r in lists["sparse_bands"]["rows"]}
    assert 3 <= len(used) < len(bands) / 2                                                      # empty bands in between
    order = [(r["octave"], r["level"]) for r in lists["all_bands"]["rows"]]
    assert order != sorted(order)                                                               # the list interleaves bands
    assert all(v["edge"] > 1e-3 for v in lists.values())                                        # no scale on a band edge
    sl = lists["slivers"]["rows"]
    empty = [r for r in sl if r["window"][2] * r["window"][3] == 0]
    one = [r for r in sl if r["window"][2] * r["window"][3] > 0 and min(r["window"][2:]) == 1]
    assert len(empty) >= 5 and len(one) >= 5
    ex = lists["extremes"]["rows"]
    assert any(r["cell"] < 1.0 for r in ex) and sum((r["octave"], r["level"]) == (0, 0) for r in ex) >= 3
    top = [r for r in ex if (r["octave"], r["level"]) == (on - 1, sf.DOG_LEVELS - 1)]
    assert len(top) >= 3 and any(r["window"] == (1, 1, r["shape"][1] - 2, r["shape"][0] - 2) for r in top)   # the whole plane
    ang = lists["angles"]["keys"][:, 3]
    assert (ang == 0).any() and ((ang > 0) & (ang < 1e-30)).any() and (ang == sf.PI32).any()
    assert (ang == np.nextafter(sf.PI32, sf.F(0))).any() and (ang == np.nextafter(sf.PI32, sf.F(4))).any()
    assert (ang >= sf.F(6.2831855)).any() and ((ang > 6.28) & (ang < sf.F(6.2831855))).any()


@pytest.mark.parametrize("name", sf.DESCRIBE_IMAGES + ("strip",))
def test_descriptors_of_given_keypoints_equal_the_reference(name):
    """Rows in the caller's order, zero rows exactly where the restatement's window is empty, every other row within the
    recorded deviation (cells of a pixel and more; see test_reference_deviation_is_the_recorded_one for the rest)."""
    lists, _ = described(name)
    for lname, v in lists.items():
        for k, r in enumerate(v["rows"]):
            if r["window"][2] * r["window"][3] == 0:
                assert not v["ref"][k].any() and not r["desc"].any(), (lname, k)
            elif r["cell"] >= SMALL_CELL:
                assert relative_deviation(v["ref"][k], r["desc"]) <= sf.REF_DEVIATION, (lname, k, v["kp"][k])


def test_no_sum_reaches_the_fixed_point_bound():
    """The descriptor kernel sizes its fixed-point grid by (cell + 2)^2 as a bound of any bin's sum.  The largest sum the
    planted inputs produce, the 0 / 255 pattern at the largest cells included, as a fraction of it."""
    worst = 0.0
    for name in sf.DESCRIBE_IMAGES + ("strip",):
        for v in described(name)[0].values():
            worst = max([worst] + [r["desc"].max() / sf.sum_bound(r["feat"]) for r in v["rows"]])
    print("largest bin sum / bound", worst)
    assert 0.01 < worst < 0.25


def test_reference_deviation_is_the_recorded_one():
    """The compiled float32 reference against the restatement, per mode: the measurement the GPU tolerance is derived
    from (8 x REF_DEVIATION).  Detection mode: descriptors at the reference's own reported position, scale and
    orientation.  Describe mode: every planted list, cells of at least one pixel.
    Smaller cells are the reference's own weak spot: it rounds a CELL CENTRE (feature + cell x offset) to float32 and
    measures pixels from there, an error of an ulp of the coordinate that the division by the cell size magnifies --
    4.3e-5 at a 0.6-pixel cell and 1.9e-4 at a 0.15-pixel cell 239 pixels from the origin (at cells of 5 pixels and up the
    same term is the few 1e-6 recorded); bounded here by 32 ulp of the coordinate over the cell."""
    detect = 0.0
    for name in sf.DETECT_IMAGES:
        fr = frame(name)
        for r, mine in zip(fr["records"], fr["owned"]):
            oss = sf.octave_scale(r["octave"], fr["geo"]["octave_min"])
            for f in mine:
                x, y, s, o = fr["keys"][f]
                feat = (sf.F(sf.F(sf.F(x - sf.F(0.5)) / oss) + sf.F(0.5)), sf.F(sf.F(sf.F(y - sf.F(0.5)) / oss) + sf.F(0.5)),
                        sf.F(s / oss), sf.code_direction(sf.key_orientation_code(o)[0]))
                want = sf.descriptor(fr["levels"][(r["octave"], r["level"])], feat)
                detect = max(detect, relative_deviation(fr["desc"][f], want))
    describe, small = 0.0, 0.0
    for name in sf.DESCRIBE_IMAGES + ("strip",):
        for v in described(name)[0].values():
            for k, r in enumerate(v["rows"]):
                if r["window"][2] * r["window"][3] == 0:
                    continue
                dev = relative_deviation(v["ref"][k], r["desc"])
                if r["cell"] >= SMALL_CELL:
                    describe = max(describe, dev)
                else:
                    small = max(small, dev)
                    assert dev <= 32 * 2.0 ** -24 * max(abs(float(r["feat"][0])), abs(float(r["feat"][1])), 1.0) / r["cell"]
    print("reference deviation: detection %.3g, describe %.3g, cells under %.1f px %.3g" % (detect, describe, SMALL_CELL, small))
    measured = max(detect, describe)
    assert 0.7 * sf.REF_DEVIATION <= measured <= sf.REF_DEVIATION, (detect, describe)
    assert 1e-5 <= sf.DESC_TOL <= 1e-4 and sf.DESC_TOL == 8 * sf.REF_DEVIATION
