#!/usr/bin/env python3
"""Absolute trajectory error between two TUM-format trajectory files (lines of `stamp tx ty tz qx qy qz qw`; `#` starts a
comment), numpy only: what the RGB-D benchmark's evaluate_ate / associate tools compute, written for this project.

  1. association: every pair of stamps (first file, second file + offset) closer than max_difference (0.02 s; the bound is
     strict) is a candidate; candidates are taken in ascending difference, each stamp used once;
  2. alignment: the rigid motion (no scale) that maps the second file's positions onto the first's in the least-squares
     sense (Horn's closed form through the SVD of the cross-covariance, the reflection case corrected);
  3. the error of a pair is the distance between the first position and the aligned second one: RMSE, mean, median,
     standard deviation, minimum and maximum over the pairs.

Usage: tools/evaluate_ate.py GROUND_TRUTH ESTIMATE [--offset S] [--max_difference S]      (prints one JSON line)
The file written by rgbdfe_pose_graph_write_trajectory is an ESTIMATE."""
import argparse
import json

import numpy as np


def read_trajectory(path):
    """{stamp: [tx, ty, tz]} of a TUM-format file (fields separated by blanks, tabs or commas)."""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line[0] == "#":
                continue
            v = line.replace(",", " ").split()
            if len(v) >= 4:
                out[float(v[0])] = [float(x) for x in v[1:4]]
    return out


def associate(first, second, offset=0.0, max_difference=0.02):
    """Pairs (t1, t2) of stamps of `first` and `second` with |t1 - (t2 + offset)| < max_difference, closest first, each
    stamp in one pair at the most; returned in ascending t1."""
    t1 = np.array(sorted(first), np.float64)
    t2 = np.array(sorted(second), np.float64)
    if len(t1) == 0 or len(t2) == 0:
        return []
    diff = np.abs(t1[:, None] - (t2[None, :] + offset))
    ii, jj = np.nonzero(diff < max_difference)
    order = np.lexsort((t2[jj], t1[ii], diff[ii, jj]))
    used1, used2, pairs = set(), set(), []
    for k in order:
        i, j = int(ii[k]), int(jj[k])
        if i in used1 or j in used2:
            continue
        used1.add(i)
        used2.add(j)
        pairs.append((float(t1[i]), float(t2[j])))
    return sorted(pairs)


def align(model, data):
    """(R, t, errors): the rotation and translation that minimise sum |data_k - (R model_k + t)|^2 over the columns of the
    3 x n arrays, and the n distances that remain."""
    model = np.asarray(model, np.float64)
    data = np.asarray(data, np.float64)
    mc = model.mean(axis=1, keepdims=True)
    dc = data.mean(axis=1, keepdims=True)
    W = (model - mc) @ (data - dc).T
    U, _, Vt = np.linalg.svd(W.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    t = dc - R @ mc
    err = np.sqrt(np.sum((R @ model + t - data) ** 2, axis=0))
    return R, t, err


def statistics(err):
    err = np.asarray(err, np.float64)
    return dict(pairs=int(len(err)), rmse=float(np.sqrt(np.dot(err, err) / len(err))), mean=float(np.mean(err)),
                median=float(np.median(err)), std=float(np.std(err)), min=float(np.min(err)), max=float(np.max(err)))


def ate(first, second, offset=0.0, max_difference=0.02):
    """The statistics for two {stamp: position} trajectories (first: ground truth, second: estimate)."""
    pairs = associate(first, second, offset, max_difference)
    if len(pairs) < 2:
        raise ValueError("fewer than two stamps could be associated: check the files and --offset")
    gt = np.array([first[a] for a, _ in pairs], np.float64).T
    est = np.array([second[b] for _, b in pairs], np.float64).T
    return statistics(align(est, gt)[2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ground_truth")
    ap.add_argument("estimate")
    ap.add_argument("--offset", type=float, default=0.0, help="seconds added to the estimate's stamps")
    ap.add_argument("--max_difference", type=float, default=0.02, help="largest stamp difference of a pair, seconds")
    a = ap.parse_args()
    print(json.dumps(ate(read_trajectory(a.ground_truth), read_trajectory(a.estimate), a.offset, a.max_difference)))


if __name__ == "__main__":
    main()
