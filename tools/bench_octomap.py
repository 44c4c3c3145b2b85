"""Measurement of the occupancy map (rgbdfe_octomap_insert_nodes; csrc/octomap.hip, csrc/api_octomap.hip).

Workload: that of tools/bench_map_assembly.py -- NODES (200) nodes of 640x480 depth as resident clouds at
cloud_creation_skip_step 1 and 2, a random rigid transform per node -- inserted in one call, as they are and after
rgbdfe_reduce_node_cloud at voxelfilter_size 0.02 m, at octomap_resolution 0.05 and 0.1, with maximum_depth 3.5 m and off.
Per configuration a sizing run first (the table grows until the map fits; its final capacity is kept), then REPS timed
runs of reset + one insert_nodes call, all in one process (host clock around the call, which ends in a stream synchronise);
the median is reported with the minimum and maximum.

Reported per configuration: seconds per call and per cloud, rays/s and cell visits/s (the visits of a sample cloud counted by
the lockstep oracle, scaled by rays), leaves, table load, kernel launches of the call, and what the kernels issue by
construction: atomics = one atomicMax per visit plus one compare-and-swap per new cell; bytes = 32 per point (the ray and the
colour-key pass) + 12 per visit (key word, mark) + 4 cap + 12 per touched cell (the apply pass) + points (16 + 20 passes)
(the colour sort and gather).  Probes beyond the first are not in these figures.
The scalar oracle of this project (tests/octomap_oracle.py) is timed on ORACLE_RAYS rows of the first cloud on the same
host and scaled by rays; its leaves on that sample are checked against the device byte for byte.  This is the oracle, not
the octomap library: the library is not on this machine and has not been timed.

Prints one JSON line; --out FILE also writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import octomap_oracle as oo  # noqa: E402
from bench_map_assembly import median_time  # noqa: E402
from rgbdslam_v2_amd import synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-rays", type=int, default=3072)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_octomap needs the GPU: no device, no figure")
    base = synth.make_depth_sequence(n_frames=8, nan_fraction=0.10)
    K = (base["fx"], base["fy"], base["cx"], base["cy"])
    depth = (base["depth"] * np.float32(1.5)).astype(np.float32)
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    N = a.nodes
    Ts = []
    for k in range(N):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = q.astype(np.float32)
        T[:3, 3] = rng.uniform(-5, 5, 3).astype(np.float32)
        Ts.append(T)
    Ts = np.stack(Ts)
    ids = np.arange(N, dtype=np.int32)
    fe = FrontEnd(max_nodes=4, max_keypoints=64, max_pairs_per_batch=8)
    res = {"nodes": N, "frame": "640x480", "reps": a.reps, "nan_fraction": 0.10, "configs": []}
    for skip in (1, 2):
        for leaf in (None, 0.02):
            for k in range(N):
                fe.upload_node_cloud(k, depth[k % 8], *K, rgb=rgb[k % 8], min_depth=0.1, cloud_skip=skip)
                if leaf:
                    fe.reduce_node_cloud(k, leaf)
            first = fe.node_cloud(0).reshape(-1, 4)
            rays = sum(fe.node_cloud(k).size // 4 for k in range(min(N, 8))) * (N // min(N, 8))
            sample = first[:: max(1, len(first) // a.oracle_rays)][: a.oracle_rays]
            for resolution in (0.05, 0.1):
                for mr in (3.5, -1.0):
                    m = fe.octomap(1 << 22, resolution=resolution)
                    m.insert_nodes(ids, Ts, mr)  # the sizing run
                    cap, leaves, launches = m.capacity, len(m), m.last_launches

                    def call():
                        m.reset()
                        m.insert_nodes(ids, Ts, mr, grow=False)
                    t, t_min, t_max = median_time(call, a.reps)
                    # the visits of the first cloud, and the oracle's time on a sample of it
                    lock = oo.LockstepMap(resolution=resolution)
                    lock.insert(first, Ts[0].T.reshape(16), mr)
                    visits = lock.visits / max(1, len(first)) * rays
                    t0 = time.perf_counter()
                    lit = oo.LiteralMap(resolution=resolution)
                    lit.insert(sample, Ts[0].T.reshape(16), mr)
                    t_or = time.perf_counter() - t0
                    with fe.octomap(2 * len(lit) + 64, resolution=resolution) as chk:
                        chk.insert_cloud(sample, Ts[0], mr)
                        assert chk.leaves().tobytes() == lit.leaves().tobytes()
                    m.close()
                    passes = (launches // N - 7) // 3
                    touched = len(lock)
                    res["configs"].append({
                        "cloud_skip": skip, "voxelfilter_size": leaf, "resolution": resolution, "max_range": mr, "rays": int(rays),
                        "cell_visits_scaled_from_cloud_0": int(visits), "leaves": leaves, "capacity_cells": cap,
                        "table_load": round(leaves / cap, 4), "kernel_launches": launches, "sort_passes": passes,
                        "s_per_call": round(t, 5), "s_per_call_min": round(t_min, 5), "s_per_call_max": round(t_max, 5),
                        "ms_per_cloud": round(t / N * 1e3, 4), "rays_per_s": round(rays / t, 1),
                        "cell_visits_per_s": round(visits / t, 1),
                        "atomics_by_construction": int(visits + leaves),
                        "bytes_by_construction": int(32 * rays + 12 * visits + N * (4 * cap + 12 * touched) + rays * (16 + 20 * passes)),
                        "scalar_oracle_of_this_project": {"rays_timed": int(len(sample)), "s_timed": round(t_or, 3),
                                                          "s_scaled_to_all_rays": round(t_or * rays / max(1, len(sample)), 1),
                                                          "equal_to_device_on_the_sample": True},
                    })
                    print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
    for k in range(N):
        fe.release_node_cloud(k)
    fe.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
