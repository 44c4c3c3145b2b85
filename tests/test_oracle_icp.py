"""CPU: tests/icp_oracle.py (the literal statement of the ICP fallback's contract) held against independent arithmetic in
float64: scipy's cKDTree (numpy brute force if scipy is absent) for the nearest neighbours and numpy.linalg.svd for the
increment, at every iteration of every planted case.  The planted inputs have nearest-neighbour gaps far above float
rounding, so the correspondence sets must agree everywhere; the increments and the composed transforms agree to the bound
derived below.  Also here: filterCloud's float recurrence and the states the cases were planted for."""
import numpy as np
import pytest

import icp_oracle as io

try:
    from scipy.spatial import cKDTree
except Exception:  # pragma: no cover
    cKDTree = None

CASES = io.planted_cases()

# The largest difference between the oracle's float increments / composed transforms and the float64 ones, measured over all
# planted cases (every iteration whose Kabsch problem is well posed), is 7.60e-6: the transform of the case that runs to 50
# iterations, each of whose increments carries what a float Jacobi SVD of a 3 x 3 covariance and float products leave (a few
# float epsilons of 1.19e-7 per entry, times coordinates of up to 2.6 m in the translation).  A single increment differs by
# at most 1.7e-6.  The bound is four times the measured figure.
MEASURED, BOUND = 7.60e-6, 4 * 7.60e-6


def nearest64(P, T):
    """Float64 nearest neighbours of the finite rows of P among the finite rows of T: (j, squared distance), j = -1 without."""
    P, T = P[:, :3].astype(np.float64), T[:, :3].astype(np.float64)
    okT = np.flatnonzero(np.isfinite(T).all(axis=1))
    okP = np.isfinite(P).all(axis=1)
    j = np.full(len(P), -1, np.int64)
    if len(okT) == 0 or not okP.any():
        return j, np.full(len(P), np.inf)
    if cKDTree is not None:
        _, k = cKDTree(T[okT]).query(P[okP])
    else:
        k = np.array([np.argmin(((T[okT] - p) ** 2).sum(axis=1)) for p in P[okP]])
    j[okP] = okT[k]
    d = P - T[np.maximum(j, 0)]
    return j, np.where(j >= 0, (d * d).sum(axis=1), np.inf)


def kabsch64(P, Tj):
    """The least-squares rigid map of P onto Tj (Umeyama without scale), float64; also how well posed it is."""
    mP, mT = P.mean(axis=0), Tj.mean(axis=0)
    H = (Tj - mT).T @ (P - mP) / len(P)
    U, s, Vt = np.linalg.svd(H)
    d = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    posed = (s[1] + d * s[2]) / s[0] if s[0] > 0 else 0.0
    full_rank = s[0] > 0 and s[2] / s[0] > 1e-6   # below that the sign of det(U) det(V') is the SVD's choice, R is not
    return R, mT - R @ mP, posed, (d < 0) if full_rank else None


def walk(name):
    """Every iteration of the oracle's run against the float64 pieces; returns the figures of the case."""
    case = CASES[name]
    ref = io.reference(name, trace=True)
    maxdist2 = case["params"]["max_correspondence_distance"] ** 2
    G = np.eye(4) if case["G"] is None else np.asarray(case["G"], np.float64)
    F64 = G.copy()
    worst, compared, all_posed = 0.0, 0, True
    for tr in ref["trace"]:
        P, T = tr["P"], tr["T"]
        j64, e64 = nearest64(P, T)
        j = tr["nn_j"].astype(np.int64)
        differ = np.flatnonzero(j != j64)
        for i in differ:   # only a duplicated target row may answer with another index: the oracle's is the first of them
            assert j[i] >= 0 and j64[i] >= 0 and T[j[i], :3].tobytes() == T[j64[i], :3].tobytes() and j[i] < j64[i], (name, tr["k"], i)
        kept64 = (j >= 0) & (e64 <= maxdist2)
        assert np.array_equal(kept64, tr["kept"]), (name, tr["k"])
        assert int(kept64.sum()) == tr["c"]
        assert abs(e64[kept64].mean() - tr["mse"]) <= 1e-6 * tr["mse"] + 1e-15
        R64, t64, posed, reflected64 = kabsch64(P[kept64, :3].astype(np.float64), T[j[kept64], :3].astype(np.float64))
        inc = np.eye(4)
        if posed > 1e-3:
            assert reflected64 is None or reflected64 == tr["reflected"], (name, tr["k"])
            worst = max(worst, np.abs(R64 - tr["R"]).max(), np.abs(t64 - tr["t"]).max())
            compared += 1
            inc[:3, :3], inc[:3, 3] = R64, t64
        else:   # no unique answer to compare with: go on from the oracle's own increment
            all_posed = False
            inc[:3, :3], inc[:3, 3] = tr["R"], tr["t"]
        F64 = inc @ F64
    if ref["converged"] and all_posed:
        worst = max(worst, np.abs(F64 - ref["T"]).max())
    return worst, compared, len(ref["trace"])


@pytest.fixture(scope="module")
def figures():
    return {name: walk(name) for name in sorted(CASES)}


def test_the_correspondences_agree_everywhere_and_the_transforms_within_the_bound(figures):
    worst = max(v[0] for v in figures.values())
    print("largest difference to float64 over %d cases, %d iterations: %.3e (bound %.3e)" %
          (len(figures), sum(v[1] for v in figures.values()), worst, BOUND))
    for name, (w, compared, iterations) in figures.items():
        assert w <= BOUND, (name, w)
    # the well-posedness filter leaves out next to nothing: every iteration of every case but those whose kept pairs share
    # one target row or lie on a line
    skipped = {name: it - c for name, (w, c, it) in figures.items() if it != c}
    assert set(skipped) <= {"sizes 257 x 1"}, skipped


def test_the_bound_is_four_times_the_measured_difference(figures):
    worst = max(v[0] for v in figures.values())
    # the documented figure is the measured one, to the two digits it is given with and a little more: another LAPACK build
    # moves the last digits of the float64 side, not the size of the difference
    assert MEASURED / 1.25 <= worst <= MEASURED * 1.25, worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_planted_case_ends_as_planted(name):
    ref = io.reference(name)
    assert (ref["state"], ref["iterations"]) == CASES[name]["expect"]
    assert ref["converged"] == (0 if ref["state"] == io.NO_CORRESPONDENCES else 1)


def test_the_float_recurrence_sample_counts():
    assert len(io.sample_positions(3072, 100)) == 101   # exact arithmetic: 100
    assert len(io.sample_positions(2999, 7)) == 8       # exact arithmetic: 7
    assert len(io.sample_positions(3072, 3072)) == 3072 and len(io.sample_positions(3072, 10000)) == 3072
    assert len(io.sample_positions(0, 10)) == 0 and list(io.sample_positions(1, 10)) == [0]
    pos = io.sample_positions(3072, 100)
    assert pos[0] == 0 and pos[-1] < 3072 and np.all(np.diff(pos) > 0)


def test_filter_cloud_keeps_the_rows_and_skips_nan_z():
    cloud = io.room_corner(holes=500, seed=9)
    cloud[7, 0] = np.inf   # z alone decides
    idx, rows = io.filter_cloud(cloud, 300)
    assert not np.isnan(cloud[idx, 2]).any() and rows.tobytes() == cloud[idx].tobytes()
    valid = np.flatnonzero(~np.isnan(cloud[:, 2]))
    assert np.array_equal(idx, valid[io.sample_positions(len(valid), 300)])


def test_source_equal_target_stays_at_the_identity():
    ref = io.reference("source = target, 48 x 36")
    assert (ref["state"], ref["iterations"]) == (io.TRANSFORM, 1)
    # one float increment from exact pairs: measured 4.8e-7 (four float epsilons); four times that is allowed
    assert np.abs(ref["T"] - np.eye(4)).max() <= 4 * 4.8e-7 and ref["mse"] == 0.0


def test_a_small_rigid_move_is_recovered():
    M = io.rigid(np.array([0, 0.6, 0.8]) * 0.003, np.array([0, 0.6, 0.8]) * 0.01)
    ref = io.reference("3 mrad, 1 cm")
    assert (ref["state"], ref["iterations"]) == (io.TRANSFORM, 2)
    # two float increments: measured 4.5e-7 against the planted move; four times that is allowed
    assert np.abs(ref["T"] - M).max() <= 4 * 4.5e-7


def test_the_quirk_of_the_reference_defaults():
    """setEuclideanFitnessEpsilon(1): the relative test passes at k = 2, far from the answer."""
    ref = io.reference("defaults, 10 mrad, 3 cm")
    M = io.rigid([0.006, 0.0064, 0.0048], [0.018, 0.0192, 0.0144])
    assert (ref["state"], ref["iterations"]) == (io.REL_MSE, 2) and np.abs(ref["T"] - M).max() > 1e-3
    full = io.align_clouds(CASES["defaults, 10 mrad, 3 cm"]["source"], CASES["defaults, 10 mrad, 3 cm"]["target"],
                           euclidean_fitness_epsilon=1e-6)
    assert full["iterations"] > 2 and np.abs(full["T"] - M).max() < np.abs(ref["T"] - M).max()


def test_the_special_pairs():
    thr = io.reference("d2 at the threshold and one float above", trace=True)
    f = np.float32(0.0625)
    assert thr["nn_d2"][0] == f and thr["nn_d2"][1] == np.nextafter(f, np.float32(1))
    assert list(thr["trace"][0]["kept"]) == [True, False, True, True, True]
    dup = io.reference("duplicated target rows")
    assert dup["nn_j"].max() < 3072 <= dup["n_target"] // 2 + 0
    assert io.reference("reflection")["reflected"]
    assert io.reference("exactly 3 correspondences")["c"] == 3 and io.reference("only 2 correspondences")["c"] == 2
    nf = io.reference("non-finite rows", trace=True)
    assert list(np.flatnonzero(nf["trace"][0]["nn_j"] < 0)) == [5, 70, 300, 301]
    assert not np.isin([9, 10, 11], nf["trace"][0]["nn_j"]).any()
