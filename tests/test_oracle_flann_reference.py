"""CPU: tests/flann_reference.py -- the plain numpy restatement of the FLANN branch equals the oracle
(oracle/rgbd_oracle.c::orc_flann_match) on every planted family, and every family's census holds: the inputs decide
the strict double ratio comparison, the tie rule, 0/0, the train-unique claim, the cap and the summation order."""
import numpy as np
import pytest

from oracle import pyoracle as po

import flann_reference as fr


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and \
        np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@pytest.mark.parametrize("fam", fr.all_families(), ids=lambda f: f["name"])
def test_reference_equals_oracle(fam):
    for ratio in fam["ratios"]:
        ref = fr.match(fam["q"], fam["t"], ratio)
        assert _same(ref, po.flann_match(fam["q"], fam["t"], ratio)), ratio
        assert len(set(ref[1].tolist())) == len(ref[1])     # the header's claim: a train row is used once


def test_reference_equals_oracle_on_the_ragged_pairs():
    nodes = fr.ragged_nodes()
    for nq, nt in fr.RAGGED_PAIRS:
        ref = fr.match(nodes[nq], nodes[nt], 0.95)
        assert _same(ref, po.flann_match(nodes[nq], nodes[nt], 0.95)), (nq, nt)
        assert len(ref[0]) > 0 or nq == 0 or nt < 2
        if nq == 0 or nt < 2:
            assert len(ref[0]) == 0


def test_census_exact_ratio():
    c = fr.census_exact_ratio(fr.exact_ratio())
    print("exact_ratio: ratio -> (queries, matches at it, matches just above it)", c)


def test_census_ties_and_nan():
    print("ties_and_nan:", fr.census_ties_and_nan(fr.ties_and_nan()))


@pytest.mark.parametrize("reverse", [False, True])
def test_census_claims(reverse):
    c = fr.census_claims(fr.claims(reverse=reverse))
    print("claims%s: row -> claimer, losing queries" % ("_reversed" if reverse else ""), c)


def test_census_cap():
    print("cap:", fr.census_cap(fr.cap()))


def test_census_winner_by_rounding():
    print("winner_by_rounding:", fr.census_winner_by_rounding(fr.winner_by_rounding()))


def test_dims_pad_with_zeros():
    """A row zero padded to 128 floats has the same distances: the padding adds +0.0 terms."""
    for fam in fr.dims():
        dim = fam["q"].shape[1]
        qp = np.zeros((len(fam["q"]), 128), np.float32); qp[:, :dim] = fam["q"]
        tp = np.zeros((len(fam["t"]), 128), np.float32); tp[:, :dim] = fam["t"]
        assert np.array_equal(fr.l2sq_flann(qp, tp).view(np.uint32), fr.l2sq_flann(fam["q"], fam["t"]).view(np.uint32))
        assert len(fr.match(fam["q"], fam["t"], 0.6)[0]) >= 10
