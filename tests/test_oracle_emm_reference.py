"""CPU: tests/emm_reference.py -- the plain restatement of observationLikelihood (math.erf for every sample) equals the
oracle on every planted scene, the censuses hold (the planted samples decide the counts), and division_boundary, the
constant the kernel compares against instead of dividing, is the exact pre-image of the reference's division."""
import math

import numpy as np
import pytest

from oracle import pyoracle as po

import emm_reference as er


@pytest.fixture(scope="module")
def results():
    return {}


def _run(scene, results):
    if scene["name"] not in results:
        results[scene["name"]] = er.run_scene(scene, po.create_point_cloud)
    return results[scene["name"]]


@pytest.mark.parametrize("scene", er.all_scenes(), ids=lambda s: s["name"])
def test_reference_equals_oracle(scene, results):
    res, clouds = _run(scene, results)
    classes = np.zeros(3, np.int64)
    for (skip_step, jobs), (counts, _) in zip(scene["calls"], res):
        for (n, o, T), c in zip(jobs, counts):
            ref = po.observation_likelihood(clouds[n], clouds[o], T, *scene["K"], cloud_skip=scene["cloud_skip"],
                                            skip_step=skip_step, depth_cov=scene["depth_cov"])
            assert list(c) == list(ref), (scene["name"], skip_step, n, o)
            classes += c[:3].astype(np.int64)
    if scene["expect"] is not None:                 # what the builder planted is what the reference counts
        for want, (counts, _) in zip(scene["expect"], res):
            assert np.array_equal(np.array(want, np.uint32), counts)
    print(scene["name"], "jobs", sum(len(j) for _, j in scene["calls"]), "good/bad/occluded", classes.tolist())


@pytest.mark.parametrize("scene", [s for s in er.all_scenes() if s["name"].startswith("boundary")], ids=lambda s: s["name"])
def test_census_boundary(scene, results):
    flips = er.census_boundary(scene, _run(scene, results)[0])
    print(scene["name"], "d_lo, d_hi ~", scene["d"], "index of the first float of the upper class per window", flips)


def test_census_one_hot_and_edges():
    s = er.one_hot()
    e = np.array(s["expect"][0])
    assert [int((e[:27, k] == 1).sum()) for k in range(3)] == [9, 9, 9] and not e[27:49, :3].any()
    assert (e[49:, 0] == 1).sum() == 4 and (e[49:, 2] == 1).sum() == 3
    for ch, cw in er.EDGE_RASTERS:
        s = er.raster_edge(ch, cw)
        e = np.array(s["expect"][0])
        assert sorted(set(s["kept_sizes"])) == [4, 6, 9] and (ch % 2, cw % 2) in ((0, 1), (1, 0))
        assert (e[:, 1] == 1).sum() > 50 and (e[:, 2] == 1).sum() > 50 and not e[:, 0].any()
        print(s["name"], "jobs", len(e), "bad", int(e[:, 1].sum()), "occluded", int(e[:, 2].sum()))


def test_census_sizes(results):
    totals, classes = set(), np.zeros(3, np.int64)
    for scene in er.all_scenes():
        if not scene["name"].startswith("sizes"):
            continue
        res, _ = _run(scene, results)
        for (counts, _), total in zip(res, scene["totals"]):
            assert np.all(counts[:, 3] == total)                   # `all` = nsx * nsy
            totals.add(total)
            classes += counts[:, :3].sum(0).astype(np.int64)
    assert {1, 255, 256, 272, 1023, 1024, 1025} <= totals and np.all(classes > 100)
    print("sizes: totals", sorted(totals), "good/bad/occluded", classes.tolist())


def test_division_boundary_is_the_preimage_of_the_division():
    """d / denom < q  <=>  d < division_boundary(q, denom), for the 200 doubles either side of the boundary."""
    for cloud_skip in (1, 2):
        for depth_cov in (1e-4, 2.5e-5):
            denom = er.emm_denominator(cloud_skip, depth_cov)
            for q in po.emm_erf_boundaries():
                b = er.division_boundary(q, denom)
                assert b / denom >= q and math.nextafter(b, -math.inf) / denom < q
                d = b
                for _ in range(200):
                    d = math.nextafter(d, -math.inf)
                for _ in range(401):
                    assert (d / denom < q) == (d < b)
                    d = math.nextafter(d, math.inf)
                # and through erf itself: the class the reference computes flips exactly at b
                p = lambda d: 0.5 * (1 + math.erf(d / denom))
                target = 0.001 if q < 0 else 0.999
                assert p(b) >= target and p(math.nextafter(b, -math.inf)) < target
    print("d_lo, d_hi at depth_cov 1e-4:", [er.division_boundary(q, er.emm_denominator(s, 1e-4))
                                          for s in (1, 2) for q in po.emm_erf_boundaries()])
