"""Planted inputs for the two-view refinement after RANSAC (g2o_refine_kernel / orc_g2o_refine, orc_g2o_block) -- a helper,
no tests in it.  tests/test_oracle_g2o.py holds the oracle to independent arithmetic on these cases and asserts, from the
oracle's trace, that every case takes the path it names; tests/test_gpu_g2o.py holds the kernel to the oracle on them.

Construction of a direct pair: the newer node (query, id 1) holds points seen through K = (521, 521, 319.5, 239.5); the
earlier node (train, id 0) holds the same points under a known rigid motion plus depth noise, in another row order;
its descriptors are the query's rows with a few flipped bits; rows that belong to no common point (random descriptors,
random places) pad both nodes.  KeyPoint.pt is the projection of a node's own 3-D points plus `kp_noise` pixels -- the
lever that pulls the refinement (which fits u, v, depth) away from RANSAC's optimum (which fits x, y, z).

What every case is for is in CASES below and, per branch of the code, in DESIGN.md ("Two-view refinement: branches and the
cases that reach them").  Every case was found on the CPU with the traced oracle (po.match_node_pair_g2o(..., trace=True));
test_the_planted_cases_cover_what_they_name asserts the paths.  What differs from the plan the cases were written to:

  * A NaN or infinite keypoint does NOT stop the solver at its first step: measurements enter the right-hand side only, so
    the first reduced system factors and the pivot test fails one step later, on a NaN estimate (stop_nan_keypoint,
    stop_inf_keypoint: pivot_failed_at == 1).  Stops at the first step come from selections of one or two matches
    (rank_deficient_1, _2) and from coordinates of 1e-15 (scale_1e-15).  A stop at a later step from finite inputs:
    stop_later_mirrored (step 5).
  * u -> 640 - u on one node does not reach |dq| > 1 in three steps (mirrored_u); keypoints shifted by 3000 pixels, one
    keypoint 1e4 pixels away, or both coordinates mirrored do (ww_negative_shifted, ww_negative_far_keypoint,
    stop_later_mirrored).
  * Fewer than three inliers score 1e9 (computeInliersAndError, node.cpp:1012), so a selection of one or two matches needs
    max_dist_for_inliers above that (1e10 here: the ABI only asks for a positive value).
  * The NaN-depth initialisation (:118) is unreachable through the pair op (errorFunction2 gives DBL_MAX for a NaN depth,
    so such a match is never an inlier and never selected); test_the_fuzz_runs_refinements_and_selects_no_nan_depth
    asserts that over the fuzz inputs instead.
"""
import functools

import numpy as np

from oracle import pyoracle as po
from rgbdslam_v2_amd import synth

K = (521.0, 521.0, 319.5, 239.5)  # transformation_estimation.cpp:56
POSE_TOL = 1e-4
DEFAULTS = dict(max_matches=300, min_matches=20, ransac_iterations=200, max_dist_for_inliers=3.0, depth_cov=1e-4,
                seed=20260923)


def rot(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def keypoints_of(xyz1, rng, noise):
    """KeyPoint.pt: the projection of the node's own points through K, plus `noise` pixels."""
    with np.errstate(all="ignore"):
        u = K[0] * xyz1[:, 0].astype(np.float64) / xyz1[:, 2] + K[2]
        v = K[1] * xyz1[:, 1].astype(np.float64) / xyz1[:, 2] + K[3]
    kp = np.stack([u, v], 1)
    if noise:
        kp = kp + rng.normal(0, noise, kp.shape)
    return np.nan_to_num(kp, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)   # (a NaN / zero depth has no projection: any finite pixel)


def _back_project(u, v, z):
    return np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z, np.ones_like(z)], 1).astype(np.float32)


def direct_pair(seed, n_true, R=None, t=(0.05, -0.02, 0.03), n_pad=0, n_wrong=0, z=(1.0, 3.0), depth_noise=0.002,
                kp_noise=0.2, flips=6):
    """Two nodes [train (id 0), query (id 1)] as (desc, xyz1, kp): n_true common points, n_wrong rows whose descriptors
    correspond but whose train point is somewhere else, n_pad unrelated rows per node."""
    rng = np.random.default_rng(seed)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    n = n_true + n_wrong
    u, v = rng.uniform(20, 620, n), rng.uniform(20, 460, n)
    zq = rng.uniform(z[0], z[1], n)
    xq = _back_project(u, v, zq)
    Xt = xq[:, :3].astype(np.float64) @ R.T + t
    Xt[:, 2] += rng.normal(0, 1, n) * depth_noise * Xt[:, 2] ** 2
    Xt[n_true:] = np.stack([rng.uniform(-1, 1, n_wrong), rng.uniform(-1, 1, n_wrong), rng.uniform(z[0], z[1], n_wrong)], 1)
    xt = np.concatenate([Xt, np.ones((n, 1))], 1).astype(np.float32)
    dq = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    bits = np.zeros((n, 256), bool)
    for r in range(n):
        bits[r, rng.choice(256, flips, replace=False)] = True
    dt = dq ^ np.packbits(bits, axis=1, bitorder="little")

    def pad(d, x):
        pd = rng.integers(0, 256, (n_pad, 32), dtype=np.uint8)
        px = _back_project(rng.uniform(20, 620, n_pad), rng.uniform(20, 460, n_pad), rng.uniform(z[0], z[1], n_pad))
        d, x = np.concatenate([d, pd]), np.concatenate([x, px])
        perm = rng.permutation(len(d))
        return d[perm], x[perm]
    dq, xq = pad(dq, xq)
    dt, xt = pad(dt, xt)
    # bruteForceSearchORB never looks at the last train row (features.cpp:163-182, restated by the oracle and the kernel):
    # an unrelated row takes that place, so that every common point can be matched
    dt = np.concatenate([dt, rng.integers(0, 256, (1, 32), dtype=np.uint8)])
    xt = np.concatenate([xt, _back_project(rng.uniform(20, 620, 1), rng.uniform(20, 460, 1), rng.uniform(z[0], z[1], 1))])
    return [(dt, xt, keypoints_of(xt, rng, kp_noise)), (dq, xq, keypoints_of(xq, rng, kp_noise))]


def sequence_nodes(seed, n_frames, n_kp, kp_noise, depth_noise=0.004, n_world=None, rows=None, **kw):
    seq = synth.make_sequence(n_frames=n_frames, n_kp=n_kp, n_world=n_world or 3 * n_kp + 200, seed=seed,
                              depth_noise=depth_noise, **kw)
    rng = np.random.default_rng(seed + 1000)
    nodes = []
    for f in range(n_frames):
        m = n_kp if rows is None else rows[f]
        x = seq["xyz1"][f][:m]
        nodes.append((seq["desc"][f][:m], x, keypoints_of(x, rng, kp_noise)))
    return nodes


def case(nodes, pairs, iters=3, **params):
    return dict(nodes=nodes, pairs=list(pairs), iters=iters, params={**DEFAULTS, **params})


def _ransac_inlier_rows(c, which=0):
    """(query rows, train rows) of the RANSAC inliers of the case's first pair, strongest match first."""
    q, t = c["pairs"][0]
    r = po.match_node_pair(c["nodes"][q][0], c["nodes"][q][1], q, c["nodes"][t][0], c["nodes"][t][1], t,
                           po.default_params(**c["params"]))
    assert r["n_inl"] > 0
    return r["all_q"][r["inl_idx"]], r["all_t"][r["inl_idx"]]


def _with_keypoint(c, node, row, value):
    d, x, kp = c["nodes"][node]
    kp = kp.copy()
    kp[row] = value
    c["nodes"][node] = (d, x, kp)
    return c


# ---- the cases -------------------------------------------------------------------------------------------------------
def quat_x180():
    return case(direct_pair(11, 120, rot([1, 0, 0], 180), (0.02, 0.03, 4.0), n_pad=30), [(1, 0)])


def quat_y180():
    return case(direct_pair(12, 120, rot([0, 1, 0], 180), (0.03, -0.02, 4.0), n_pad=30), [(1, 0)])


def quat_z180():
    return case(direct_pair(13, 120, rot([0, 0, 1], 180), (0.02, 0.03, 0.05), n_pad=30), [(1, 0)])


def quat_skew170():
    return case(direct_pair(14, 120, rot([1.0, 0.3, 0.2], 170), (0.1, 0.5, 4.0), n_pad=30), [(1, 0)])


def _stop_keypoint(seed, node, value, iters=3):
    c = case(direct_pair(seed, 100, rot([0, 1, 0], 5), n_pad=20), [(1, 0)], iters=iters)
    return _with_keypoint(c, node, _ransac_inlier_rows(c)[1 - node][3], value)


def stop_nan_keypoint():
    return _stop_keypoint(21, 1, (np.nan, 100.0))


def stop_inf_keypoint():
    return _stop_keypoint(22, 0, (200.0, np.inf))


def nan_keypoint_one_iteration():
    # a single step: no pivot is tested after the NaN entered the estimate; the NaN pose itself is re-scored (no inliers)
    return _stop_keypoint(21, 1, (np.nan, 100.0), iters=1)


def _moved_keypoints(f, iters):
    c = case(direct_pair(41, 100, rot([0, 1, 0], 5), n_pad=20), [(1, 0)], iters=iters)
    d, x, kp = c["nodes"][0]
    c["nodes"][0] = (d, x, f(kp).astype(np.float32))
    return c


def stop_later_mirrored():
    """u -> 640 - u, v -> 480 - v on the earlier node: finite keypoints that contradict the 3-D points; the steps go astray
    (|dq| > 1 twice) until, at the sixth, the normal equations have a non-positive pivot."""
    return _moved_keypoints(lambda kp: np.stack([640 - kp[:, 0], 480 - kp[:, 1]], 1), 8)


def ww_negative_shifted():
    # every keypoint of the earlier node 3000 pixels off: |dq| > 1 in all three steps, every pivot positive
    return _moved_keypoints(lambda kp: kp + 3000, 3)


def ww_negative_far_keypoint():
    # ONE keypoint 10^4 pixels off among 36 selected matches: |dq| > 1 in one step of three
    c = case(direct_pair(23, 40, rot([0, 1, 0], 5), n_pad=10), [(1, 0)])
    return _with_keypoint(c, 0, _ransac_inlier_rows(c)[1][0], (1.0e4, -1.0e4))


def mirrored_u():
    # the issue's u -> 640 - u: does not reach |dq| > 1 in three steps (the trace says so); kept as a rejected refinement
    return _moved_keypoints(lambda kp: np.stack([640 - kp[:, 0], kp[:, 1]], 1), 3)


def _tiny(n, **kw):
    # no motion, no RANSAC loop below 4 matches: the identity hypothesis (:1192) leaves n inliers and the refinement runs on
    # them.  Fewer than 3 inliers score 1e9 (:1012), which only a max_dist_for_inliers above that lets through (:1206).
    return case(direct_pair(30 + n, n, None, (0.0, 0.0, 0.0), depth_noise=0.0005, kp_noise=0.3), [(1, 0)], min_matches=0, **kw)


def rank_deficient_3():
    return _tiny(3)


def rank_deficient_2():
    return _tiny(2, max_dist_for_inliers=1e10)


def rank_deficient_1():
    return _tiny(1, max_dist_for_inliers=1e10)


def nsel_band(n_true, n_pad, seed=None, **kw):
    return case(direct_pair(seed or 50 + n_true, n_true, rot([0.2, 1, 0.1], 6), n_pad=n_pad), [(1, 0)], **kw)


def nsel_le_8():
    return nsel_band(7, 2, min_matches=4)


def nsel_9_63():
    return nsel_band(40, 10)


def nsel_65_128():
    return nsel_band(100, 20)


def nsel_129_256():
    return nsel_band(200, 40)


def nsel_257_320():
    return nsel_band(340, 59, seed=392, max_matches=320)     # (the earlier node: 340 + 59 + 1 = 400 rows)


def thr_edge(n_true, n_wrong, seed=61):
    # n_all = 24 > min_matches = 20: thr = floor(0.75 * 24) = 18, the clipped value
    return case(direct_pair(seed, n_true, rot([0, 1, 0], 4), n_wrong=n_wrong, depth_noise=0.0005), [(1, 0)])


def thr_exact():
    return thr_edge(18, 6)


def thr_plus_one():
    return thr_edge(19, 5)


def depth_cov_case(dc):
    return case(direct_pair(71, 120, rot([0.1, 1, 0], 5), n_pad=30), [(1, 0)], depth_cov=dc)


def scaled_case(scale, depth_cov, max_dist):
    """test_numeric_range_fallbacks' (scale, depth_cov, max_dist_for_inliers) triples with the refinement on."""
    nodes = sequence_nodes(31, 4, 300, 0.2, depth_noise=0.01, n_world=900)
    rng = np.random.default_rng(5)
    out = []
    for d, x, _ in nodes:
        xs = x.copy()
        xs[:, :3] = (x[:, :3].astype(np.float64) * scale).astype(np.float32)
        out.append((d, xs, keypoints_of(x, rng, 0.2)))
    pq, pt = synth.candidate_pairs(4, per_frame=3, seed=31)
    c = case(out, zip(pq.tolist(), pt.tolist()), depth_cov=depth_cov, max_dist_for_inliers=max_dist)
    c["scale"] = scale
    return c


def iterations_case(iters):
    return case(direct_pair(81, 60, rot([0.3, 1, 0.2], 8), n_pad=15, kp_noise=0.5), [(1, 0)], iters=iters)


def adopt_mix(kp_noise, max_dist, depth_noise, seed):
    nodes = sequence_nodes(seed, 8, 300, kp_noise, depth_noise=depth_noise)
    pairs = [(q, t) for q in range(1, 8) for t in range(max(0, q - 3), q)]
    return case(nodes, pairs, max_dist_for_inliers=max_dist)


CASES = {
    "quat_x180": quat_x180, "quat_y180": quat_y180, "quat_z180": quat_z180, "quat_skew170": quat_skew170,
    "stop_nan_keypoint": stop_nan_keypoint, "stop_inf_keypoint": stop_inf_keypoint,
    "nan_keypoint_one_iteration": nan_keypoint_one_iteration, "stop_later_mirrored": stop_later_mirrored,
    "rank_deficient_3": rank_deficient_3, "rank_deficient_2": rank_deficient_2, "rank_deficient_1": rank_deficient_1,
    "ww_negative_shifted": ww_negative_shifted, "ww_negative_far_keypoint": ww_negative_far_keypoint, "mirrored_u": mirrored_u,
    "nsel_le_8": nsel_le_8, "nsel_9_63": nsel_9_63, "nsel_65_128": nsel_65_128, "nsel_129_256": nsel_129_256,
    "nsel_257_320": nsel_257_320,
    "thr_exact": thr_exact, "thr_plus_one": thr_plus_one,
    "depth_cov_1e-8": lambda: depth_cov_case(1e-8), "depth_cov_1e-4": lambda: depth_cov_case(1e-4),
    "depth_cov_1": lambda: depth_cov_case(1.0),
    "scale_1e-7": lambda: scaled_case(1e-7, 1e-4, 3.0), "scale_1e8": lambda: scaled_case(1e8, 1e18, 1e6),
    "scale_1e-15": lambda: scaled_case(1e-15, 1e-70, 3.0),
    "iterations_1": lambda: iterations_case(1), "iterations_2": lambda: iterations_case(2),
    "iterations_8": lambda: iterations_case(8), "iterations_50": lambda: iterations_case(50),
    "adopt_mix_a": lambda: adopt_mix(0.2, 3.0, 0.004, 55), "adopt_mix_b": lambda: adopt_mix(2.0, 3.0, 0.004, 56),
    "adopt_mix_c": lambda: adopt_mix(1.0, 2.0, 0.002, 57),
}


FUZZ_SEED = 2   # chosen with the traced oracle: refinements run in four of the six trials and end in all four outcomes


@functools.lru_cache(maxsize=None)
def fuzz_trials(seed=FUZZ_SEED):
    """test_randomised_nodes_and_parameters_match_oracle's fuzz with the refinement on: 6 trials of 8 nodes and 24 pairs, in
    the shape of a case (nodes, pairs, iters, params)."""
    rng = np.random.default_rng(seed)
    trials = []
    for trial in range(6):
        F = 8
        # (the sizes at which a refinement can run at all are drawn more often: uniformly, 19 pairs in 20 do nothing)
        sizes = [int(rng.choice([0, 1, 3, 5, 21, 64, 300, 400], p=[.05, .05, .05, .05, .1, .2, .25, .25])) for _ in range(F)]
        seq = synth.make_sequence(n_frames=F, n_kp=400, n_world=1100, seed=300 + trial,
                                  nan_fraction=float(rng.choice([0.0, 0.05, 0.3])), depth_noise=(0.002, 0.01, 0.03)[trial % 3])
        kp_noise = float(rng.choice([0.0, 0.2, 2.0]))
        nodes = []
        for f in range(F):
            d, x = seq["desc"][f][: sizes[f]].copy(), seq["xyz1"][f][: sizes[f]].copy()
            if sizes[f] > 10 and rng.random() < 0.3:
                x[rng.random(sizes[f]) < 0.1, 2] = 0.0          # zero depths
            if sizes[f] > 10 and rng.random() < 0.2:
                d[:] = rng.integers(0, 256, d.shape, dtype=np.uint8)  # unrelated descriptors
            if sizes[f] > 10 and rng.random() < 0.2:
                d[1::2] = d[0::2][: len(d[1::2])]                 # duplicated rows: ties in hd and in the train index
            nodes.append((d, x, keypoints_of(x, rng, kp_noise)))
        kw = dict(max_matches=int(rng.choice([1, 4, 5, 63, 64, 65, 200, 300, 320])),
                  min_matches=int(rng.choice([0, 1, 4, 20, 50])),
                  ransac_iterations=int(rng.choice([0, 1, 7, 8, 50, 200, 300])),
                  max_dist_for_inliers=float(rng.choice([0.5, 2.0, 3.0])),
                  depth_cov=float(rng.choice([1e-4, 2.5e-5, 1e-3])), seed=int(rng.integers(0, 2**31)))
        pairs = list(zip(rng.integers(0, F, 24).tolist(), rng.integers(0, F, 24).tolist()))
        trials.append(dict(nodes=nodes, pairs=pairs, iters=int(rng.choice([1, 3, 8])), params=kw))
    return trials


@functools.lru_cache(maxsize=None)
def float_case():
    """Six related frames of 300 rows and an unrelated one as 128-d float descriptors (for SIFT and for FLANN nodes), with
    keypoints 1.5 pixels off: a case whose "nodes" are (desc128, xyz1, kp)."""
    nodes = sequence_nodes(91, 7, 300, 1.5, depth_noise=0.004)
    rng = np.random.default_rng(92)
    bits = [d for d, _, _ in nodes]
    bits[6] = rng.integers(0, 256, bits[6].shape, dtype=np.uint8)
    nodes = [(synth.sift_descriptors_like(b, seed=91), x, kp) for b, (_, x, kp) in zip(bits, nodes)]
    pairs = [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (2, 0), (3, 1), (5, 3), (4, 1), (5, 2), (6, 5), (3, 6)]
    return case(nodes, pairs)


def float_records(matcher, c):
    prm = po.default_params(**c["params"])
    out = []
    for q, t in c["pairs"]:
        (dq, xq, kq), (dt, xt, kt) = c["nodes"][q], c["nodes"][t]
        out.append(po.match_float_node_pair_g2o(matcher, dq, xq, kq, q, dt, xt, kt, t, c["iters"], 0.95, prm))
    return out


def records_of(c):
    prm = po.default_params(**c["params"])
    out = []
    for q, t in c["pairs"]:
        (dq, xq, kq), (dt, xt, kt) = c["nodes"][q], c["nodes"][t]
        out.append(po.match_node_pair_g2o(dq, xq, kq, q, dt, xt, kt, t, c["iters"], prm, trace=True))
    return out


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle_records(name):
    """The oracle's record and trace of every pair of the case (computed once; do not modify)."""
    return records_of(get(name))


def check_record(rec, ref, hd=True):
    """test_gpu_pairs.check_against_oracle with exact=True: a device record against the oracle's, lists and bits (two NaNs
    compare equal by bytes)."""
    from rgbdslam_v2_amd.frontend import inlier_indices
    n = ref["n_all"]
    assert rec["n_all"] == n
    assert np.array_equal(rec["all_q"][:n], ref["all_q"])
    assert np.array_equal(rec["all_t"][:n], ref["all_t"])
    if hd:
        assert np.array_equal(rec["all_hd"][:n], ref["all_hd"])
    assert (rec["id1"], rec["id2"]) == (ref["id1"], ref["id2"])
    assert rec["real_iterations"] == ref["real_iterations"]
    assert rec["valid_iterations"] == ref["valid_iterations"]
    assert rec["n_inl"] == ref["n_inl"]
    assert np.array_equal(inlier_indices(rec), ref["inl_idx"])
    T = np.array(rec["trafo"], np.float32).reshape(4, 4).T
    if np.isfinite(ref["T"]).all():
        assert np.abs(T - ref["T"]).max() <= POSE_TOL
    assert T.tobytes() == ref["T"].tobytes(), "pose bits differ from the oracle"
    assert np.float32(rec["rmse"]).tobytes() == np.float32(ref["rmse"]).tobytes()
    assert np.float64(rec["info_scale"]).tobytes() == np.float64(ref["info_scale"]).tobytes()
