"""Measurement of the voxel filter (rgbdfe_voxel_filter_device; csrc/voxel_filter.hip).

Workload: the assembled map of tools/bench_map_assembly.py -- 200 nodes of 640x480 depth as resident clouds at
cloud_creation_skip_step 1 and 2, a random rigid transform per node, maximum_depth +inf, compact mode -- filtered on the
device at voxelfilter_size 0.01, 0.02 and 0.05 m.  Per configuration, medians of REPS repetitions after a warm-up, all in
one process (host clock around the call, which ends in a stream synchronise):

* the device entry point: seconds per call, input points/s, the cells it returns, the sort passes and kernel launches of the
  call (from the grid, as api_voxel.hip derives them), and the bytes its kernels read and write by construction:
  32 n (two point passes) + n_valid (8 + 20 passes + 8 + 20) + 20 cells;
* a hipMemcpy device-to-device of the input bytes in the same run, the yardstick;
* the project's vectorised numpy oracle (tests/voxel_filter_oracle.py) on the first ORACLE_POINTS rows of the map, checked
  against the device on those rows byte for byte, and scaled to all points.  This is the oracle, not PCL: PCL's filter has
  not been timed.

Prints one JSON line; --out FILE also writes it there."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import voxel_filter_oracle as vo  # noqa: E402
from bench_map_assembly import median_time  # noqa: E402
from rgbdslam_v2_amd import _lib, synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402


def grid_of(d_map, leaf):
    """(valid points, cells of the grid) as the library derives them from the bounding box."""
    import torch
    ok = torch.isfinite(d_map[:, :3]).all(dim=1)
    xyz = d_map[ok, :3]
    lo, hi = xyz.min(dim=0).values.cpu().numpy(), xyz.max(dim=0).values.cpu().numpy()
    _, inv = vo.leaf_ok(leaf)
    div = [int(np.floor(hi[a] * inv)) - int(np.floor(lo[a] * inv)) + 1 for a in range(3)]
    return int(ok.sum().item()), div[0] * div[1] * div[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-points", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit("at least 7 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel_filter needs the GPU: no device, no figure")
    hip = ctypes.CDLL(_lib.LIB_PATH)  # the HIP runtime the library itself is linked against
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def hip_copy(dst, src, nbytes):
        if hip.hipMemcpy(dst, src, nbytes, 3) != 0 or hip.hipDeviceSynchronize() != 0:
            raise RuntimeError("hipMemcpy failed")

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
        for k in range(N):
            fe.upload_node_cloud(k, depth[k % 8], *K, rgb=rgb[k % 8], min_depth=0.1, cloud_skip=skip)
        points = N * (depth.shape[1] // skip) * (depth.shape[2] // skip)
        d_map = torch.empty((points, 4), dtype=torch.float32, device="cuda:0")
        d_out = torch.empty((points, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        n_map = fe.assemble_map_device(ids, Ts, d_map)
        d_in = d_map[:n_map]
        t_d2d, _, _ = median_time(lambda: hip_copy(d_out.data_ptr(), d_in.data_ptr(), 16 * n_map), a.reps)
        for leaf in (0.01, 0.02, 0.05):
            cells, flags = fe.voxel_filter_device(d_in, leaf, d_out, return_flags=True)
            t, t_min, t_max = median_time(lambda: fe.voxel_filter_device(d_in, leaf, d_out), a.reps)
            n_valid, grid_cells = grid_of(d_in, leaf)
            passes = 0 if flags else vo.sort_passes(grid_cells)
            launches = 2 if flags else 2 + 1 + 3 * passes + 3 + 1
            nbytes = 32 * n_map + n_valid * (8 + 20 * passes + 8 + 20) + 20 * cells
            no = min(a.oracle_points, n_map)
            sample = d_in[:no].cpu().numpy()
            t0 = time.perf_counter()
            want, want_flags, _ = vo.voxel_filter(sample, leaf)
            t_or = time.perf_counter() - t0
            got = fe.voxel_filter(sample, leaf)
            assert want_flags == 0 and got.tobytes() == want.tobytes()
            res["configs"].append({
                "cloud_skip": skip, "voxelfilter_size": leaf, "points": int(n_map), "valid_points": n_valid, "cells_out": int(cells),
                "leaf_too_small": bool(flags), "grid_cells": int(grid_cells), "sort_passes": passes, "kernel_launches": launches,
                "bytes_by_construction": int(nbytes),
                "device_entry": {"ms": round(t * 1e3, 4), "ms_min": round(t_min * 1e3, 4), "ms_max": round(t_max * 1e3, 4),
                                 "points_per_s": round(n_map / t, 1), "bytes_by_construction_per_s": round(nbytes / t, 1)},
                "hipMemcpy_d2d_input_bytes": {"ms": round(t_d2d * 1e3, 4), "bytes": int(16 * n_map),
                                              "device_entry_over_copy": round(t / t_d2d, 2)},
                "numpy_oracle_of_this_project": {"points_timed": int(no), "s_timed": round(t_or, 3),
                                                 "s_scaled_to_all_points": round(t_or * n_map / no, 2),
                                                 "equal_to_device_on_the_sample": True},
            })
            print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
        del d_map, d_out, d_in
        torch.cuda.empty_cache()
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
