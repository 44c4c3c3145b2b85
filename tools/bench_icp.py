#!/usr/bin/env python3
"""Times the ICP fallback (rgbdfe_icp_align_nodes) on one GPU: batches of 1, 20 and 200 jobs over resident
640 x 480 node clouds (a room corner seen along a smooth trajectory, adjacent frames paired as Node::matchNodePair pairs
them: source = the older cloud), desired_size 10000, once with the reference's defaults (which stop at k = 2) and once with
the full loop (euclidean_fitness_epsilon 1e-6).  Per configuration: the median host time of a call over --reps calls after a
warm-up, ms per job, the iterations, launches and read-backs, and -- from a second pass with rgbdfe_set_profiling, never
mixed into the timed one -- the device time of the nearest-neighbour kernel and its share of the call.  --oracle adds the
time of the numpy oracle (tests/icp_oracle.py, one host thread: the literal restatement, not an optimised CPU ICP) for one
job and checks its bytes.  Prints one JSON line; --out writes it to a file as well.  There is no CPU fallback: without a
device the FrontEnd fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import icp_oracle as io  # noqa: E402
from rgbdslam_v2_amd import _lib  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402

COLS, ROWS = 640, 480


PERIOD = 20


def pose(i):
    """Frame i of the trajectory (it repeats after PERIOD frames): up to two centimetres and two milliradians between
    neighbours."""
    a = 3.0 * np.sin(2 * np.pi * i / PERIOD)
    b = 2.0 * np.cos(2 * np.pi * i / PERIOD)
    return io.rigid([0.01 * a, -0.008 * b, 0.005 * a], [0.02 * a, 0.01 * b, -0.015 * a])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 20, 200])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--desired-size", type=int, default=10000)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()

    n_nodes = max(args.jobs) + 1
    fe = FrontEnd(device_id=0, max_nodes=16, max_keypoints=512, max_pairs_per_batch=64)
    frames = [io.corner_depth(COLS, ROWS, pose(i)) for i in range(min(PERIOD, n_nodes))]
    for i in range(n_nodes):   # every node has a cloud of its own on the device; the rasters repeat with the trajectory
        depth, (fx, fy, cx, cy) = frames[i % PERIOD]
        fe.upload_node_cloud(i, depth, fx, fy, cx, cy, cloud_skip=1)
    result = dict(tool="bench_icp", cloud=[COLS, ROWS], desired_size=args.desired_size, reps=args.reps, configs=[])
    for label, kw in (("reference defaults", {}), ("full loop", dict(euclidean_fitness_epsilon=1e-6))):
        prm = fe.icp_params(desired_size=args.desired_size, **kw)
        for n in args.jobs:
            src, tgt = np.arange(0, n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)
            fe.icp_align_nodes(src, tgt, None, prm)   # warm-up: code objects, the call's buffers
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                T, rep = fe.icp_align_nodes(src, tgt, None, prm)   # returns after the last read-back
                times.append((time.perf_counter() - t0) * 1e3)
            fe.set_profiling(True)
            fe.reset_kernel_time()
            t0 = time.perf_counter()
            fe.icp_align_nodes(src, tgt, None, prm)
            profiled_ms = (time.perf_counter() - t0) * 1e3
            nn_ms, nn_launches, _ = fe.kernel_time(_lib.KERNEL_ICP_NN)
            fe.set_profiling(False)
            med = float(np.median(times))
            states = {}
            for r in rep:
                states[io.STATE_NAMES[int(r["state"])]] = states.get(io.STATE_NAMES[int(r["state"])], 0) + 1
            result["configs"].append(dict(
                params=label, jobs=n, ms_per_call=dict(median=med, min=min(times), max=max(times)), ms_per_job=med / n,
                iterations=dict(min=int(rep["iterations"].min()), max=int(rep["iterations"].max())), states=states,
                samples=[int(rep["n_source"].max()), int(rep["n_target"].max())], launches=int(rep[0]["launches"]),
                readbacks=int(rep[0]["readbacks"]), nn_kernel_ms=nn_ms, nn_kernel_launches=int(nn_launches),
                nn_kernel_share_of_the_profiled_call=nn_ms / profiled_ms, profiled_call_ms=profiled_ms,
                # distance evaluations of the launches that did work (an upper bound: a finished job's blocks return at once)
                nn_pair_evaluations_per_s=(float(rep["iterations"].astype(np.float64).sum()) * float(rep["n_source"].max()) *
                                           float(rep["n_target"].max()) / (nn_ms * 1e-3)) if nn_ms > 0 else None))
    if args.oracle:
        a, b = fe.node_cloud(0).reshape(-1, 4), fe.node_cloud(1).reshape(-1, 4)
        t0 = time.perf_counter()
        ref = io.align_clouds(a, b, None, desired_size=args.desired_size)
        result["oracle_ms_one_job_reference_defaults"] = (time.perf_counter() - t0) * 1e3
        T, rep = fe.icp_align_nodes([0], [1], None, fe.icp_params(desired_size=args.desired_size))
        result["oracle_agrees_bytewise"] = bool(T[0].tobytes() == ref["T"].tobytes() and int(rep[0]["iterations"]) == ref["iterations"])
    fe.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
