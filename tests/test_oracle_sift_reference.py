"""CPU: tests/sift_match_reference.py -- the plain exact SIFT matcher and the planted second-best inputs.

The reference must return the oracle's (queryIdx, trainIdx) lists on every input family the GPU tests use, and the planted
inputs must be able to detect a lost second-best dot product: that is asserted from the census of the exact dot matrix
alone, never from a matcher's answer."""
import numpy as np
import pytest

from oracle import pyoracle as po

import sift_match_reference as sr


def _same(d1, d2):
    rq, rt = sr.match(d1, d2)
    oq, ot, _ = po.sift_match(d1, d2)
    assert np.array_equal(rq, oq) and np.array_equal(rt, ot), (d1.shape, d2.shape, len(rq), len(oq))
    return rq, rt


def test_quantise_angle_accept():
    f = np.array([0.0, 0.2, 0.4985, 0.6, 255 / 512.0, 0.00097], np.float32)
    assert sr.quantise(f).tolist() == [0, 102, 255, 51, 255, 0]           # 0.6 * 512 = 307 wraps to 51
    u = np.arange(256)
    assert np.array_equal(sr.quantise((u / 512.0).astype(np.float32)), u)  # planted inputs quantise back exactly
    assert sr.angle(1 << 18) == 0 and sr.angle(8323200) == 0 and sr.angle(0) == np.float32(np.arccos(0.0))
    assert not sr.accept(200000, 200000) and not sr.accept(1 << 18, 1 << 18)   # a tied best is never accepted
    assert sr.accept(1 << 18, 200000) and not sr.accept(250000, 249000) and not sr.accept(100000, 0)


@pytest.mark.parametrize("n1,n2", sr.PLANTED_SIZES)
def test_planted_case_census(n1, n2):
    """What a planted case can detect, from the exact dot matrix: second-critical rows and columns (>= 12 each, >= 6 at
    (64, 96)), >= 2 critical planted pairs in every placement class that exists at the size, every plain planted match in
    the reference's list; and the reference equals the oracle on the case and on the case with its nodes exchanged."""
    d1, d2, planted = sr.planted_case(n1, n2, 1000 * n1 + n2)
    assert d1.shape == (n1, 128) and d2.shape == (n2, 128)
    for d in (d1, d2):
        assert np.array_equal(sr.quantise(d).astype(np.float32) / 512.0, d)
    m = min(n1, n2) // 8
    assert len(planted["row"]) == len(planted["col"]) == len(planted["plain"]) == m
    c = sr.census(d1, d2, planted)
    print("planted (%d, %d): %d per side, critical rows %d, critical columns %d, row classes %s, column classes %s"
          % (n1, n2, m, len(c["rows"]), len(c["cols"]), c["row_classes"], c["col_classes"]))
    least = 6 if (n1, n2) == (64, 96) else 12
    assert len(c["rows"]) >= least and len(c["cols"]) >= least
    assert set(c["row_classes"]) == set(sr.row_classes_at(n2)) and set(c["col_classes"]) == set(sr.col_classes_at(n1))
    assert min(c["row_classes"].values()) >= 2, c["row_classes"]
    assert min(c["col_classes"].values()) >= 2, c["col_classes"]
    rq, rt = _same(d1, d2)
    got = set(zip(rq.tolist(), rt.tolist()))
    assert all((i, j) in got for i, j in planted["plain"])
    # the critical rows and columns are rejected, and each of them would be a match without its second
    assert not set(rq.tolist()) & set(c["rows"].tolist()) and not set(rt.tolist()) & set(c["cols"].tolist())
    _same(d2, d1)
    # exchanged nodes: the census swaps with them
    cs = sr.census(d2, d1)
    assert np.array_equal(cs["rows"], c["cols"]) and np.array_equal(cs["cols"], c["rows"])


def test_placement_classes_exist_where_the_kernels_have_them():
    assert "tile_lt" not in sr.row_classes_at(96) and "ragged_gt" in sr.row_classes_at(96)
    assert "ragged_lt" not in sr.row_classes_at(1024) and "tile_gt" in sr.row_classes_at(1024)
    assert sr.col_classes_at(64) == ["group", "wave", "ragged"] and sr.col_classes_at(1024) == ["group", "wave", "block", "blocks"]
    assert sr.row_classes(5, 0, 96) == ["group_lt", "ragged_lt", "first"]
    assert sr.row_classes(33, 1, 300) == ["lane_lt"] and sr.row_classes(10, 299, 300) == ["tile_gt", "ragged_gt", "last"]
    assert sr.col_classes(3, 40, 700) == ["wave"] and sr.col_classes(3, 600, 700) == ["blocks", "ragged"]
    assert sr.col_classes(3, 200, 700) == ["block"] and sr.col_classes(31, 0, 64) == ["group", "ragged"]


@pytest.mark.parametrize("n1,n2", sr.VS_ORACLE_SIZES)
def test_reference_vs_oracle_random_recipe(n1, n2):
    d1, d2, _, _, k = sr.vs_oracle_case(n1, n2)
    rq, _ = _same(d1, d2)
    if min(n1, n2) > 100:
        assert len(rq) > k // 2


def test_reference_vs_oracle_key_paths_block_shapes_extremes():
    """Non-unit norms (x 1.6), the block just under 2^19 with its duplicates, the wrapping 0.6 value, duplicated rows at
    every block shape, saturated and all-zero rows."""
    total = 0
    for c in sr.key_path_cases() + sr.block_shape_cases() + sr.extreme_cases():
        rq, rt = _same(c["d1"], c["d2"])
        assert len(rq) > c["least"], c["name"]
        total += len(rq)
        if c["name"] == "saturated":
            assert (77, 133) in set(zip(rq.tolist(), rt.tolist()))
            D = sr.dot_matrix(c["d1"], c["d2"])
            assert D.max() == D[77, 133] == 8323200
        if c["name"].startswith("zero_rows"):
            z1, z2 = np.flatnonzero(~c["d1"].any(1)), np.flatnonzero(~c["d2"].any(1))
            assert len(z1) >= len(c["d1"]) // 10 and {0, len(c["d1"]) - 1} <= set(z1.tolist())
            assert (z2 >= len(c["d2"]) // 128 * 128).any()
            assert not set(rq.tolist()) & set(z1.tolist()) and not set(rt.tolist()) & set(z2.tolist())
    assert total > 5000


def test_reference_vs_oracle_tie_rules():
    """test_sift_tie_rules' duplicates: the reference has no tie rule, a tied best is simply never accepted."""
    rng = np.random.default_rng(5)
    base = sr.rand_sift(rng, 40)
    d2 = base[rng.integers(0, 40, 500)]
    d1 = base[rng.integers(0, 40, 300)]
    _same(d1, d2)
    _same(d1, d2 + rng.normal(0, 1e-4, d2.shape).astype(np.float32))


def test_reference_vs_oracle_mixed_batch_nodes():
    nodes, pq, pt = sr.mixed_batch_nodes()
    assert [len(d) for d, _ in nodes] == list(sr.MIXED_SIZES)
    fast = [sr.fast_key_node(d) for d, _ in nodes]
    assert fast == [True, True, False, False, False, True, True, True]
    for q, t in ((0, 1), (2, 3), (3, 0), (4, 5), (5, 1), (6, 0), (0, 6), (7, 0), (0, 7)):
        _same(nodes[q][0], nodes[t][0])


def test_reference_vs_oracle_row_cap():
    """Nodes above 4096 rows are cut to their first 4096 (sift_gpu_wrapper.cpp:231); train indices >= 4064 occur, the
    columns whose sequence number inside a lane is 127."""
    noisy, base, _, _ = sr.cap_nodes()
    for n1, n2 in sr.CAP_SIZES[1:]:
        rq, rt = _same(noisy[:n1], base[:n2])
        assert len(rq) > 500 and rq.max() < sr.CAP and rt.max() < sr.CAP
        if n2 > sr.CAP:
            assert (rt >= 4064).any() and rq.max() >= 4064
