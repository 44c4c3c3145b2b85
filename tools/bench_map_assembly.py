"""Measurement of map assembly (rgbdfe_assemble_map / rgbdfe_assemble_map_device; csrc/map_assembly.hip).

Workload: 200 nodes of 640x480 depth (the wavy wall of synth.make_depth_sequence pushed back to ~3 m, 10 % NaN holes) as
resident clouds at cloud_creation_skip_step 1 and 2, a random rigid transform per node, maximum_depth +inf and 3.5, compact
and raster mode.  Per configuration, medians of REPS repetitions after a warm-up, all in one process:

* the device entry point: seconds per call (host clock around the call, which ends in a stream synchronise), points/s, the
  algorithmic bytes (16 B read per point + 16 B written per kept point) per second and their share of the HBM figure
  DESIGN.md section 5 uses (8 TB/s) -- and beside it a hipMemcpy device-to-device that moves the same number of bytes
  (half of them read, half written), the yardstick of the same run;
* the host entry point: seconds per call into a pageable buffer that is reused -- beside it a plain hipMemcpy
  device-to-host of the output bytes into the same buffer, and the numpy oracle (tests/map_assembly_oracle.py) on the same
  host, timed on ORACLE_NODES nodes and scaled to all.

Prints one JSON line; --out FILE also writes it there."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_assembly_oracle as mo  # noqa: E402
from rgbdslam_v2_amd import _lib, synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402

HBM_PEAK = 8.0e12


def median_time(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--oracle-nodes", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit("at least 7 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_assembly needs the GPU: no device, no figure")
    hip = ctypes.CDLL(_lib.LIB_PATH)  # the HIP runtime the library itself is linked against
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    D2H, D2D = 2, 3

    def hip_copy(dst, src, nbytes, kind):
        if hip.hipMemcpy(dst, src, nbytes, kind) != 0 or hip.hipDeviceSynchronize() != 0:
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
    res = {"nodes": N, "frame": "640x480", "reps": a.reps, "nan_fraction": 0.10, "hbm_peak_bytes_per_s": HBM_PEAK, "configs": []}
    for skip in (1, 2):
        for k in range(N):
            fe.upload_node_cloud(k, depth[k % 8], *K, rgb=rgb[k % 8], min_depth=0.1, cloud_skip=skip)
        host_clouds = [fe.node_cloud(k) for k in range(8)]
        points = N * host_clouds[0].shape[0] * host_clouds[0].shape[1]
        d_out = torch.empty((points, 4), dtype=torch.float32, device="cuda:0")
        d_src = torch.empty((points, 4), dtype=torch.float32, device="cuda:0")   # the yardstick copy's source
        h_out = np.zeros((points, 4), np.float32)                                # pageable, touched once
        for md in (float("inf"), 3.5):
            for raster in (False, True):
                kept = fe.assemble_map_device(ids, Ts, d_out, md, raster)
                alg_bytes = 16 * points + 16 * kept
                t_dev, t_dev_min, t_dev_max = median_time(lambda: fe.assemble_map_device(ids, Ts, d_out, md, raster), a.reps)
                half = alg_bytes // 2
                t_d2d, _, _ = median_time(lambda: hip_copy(d_out.data_ptr(), d_src.data_ptr(), half, D2D), a.reps)
                t_host, t_host_min, t_host_max = median_time(
                    lambda: fe.assemble_map(ids, Ts, md, raster, out=h_out), a.reps, warmup=1)
                t_d2h, _, _ = median_time(lambda: hip_copy(h_out.ctypes.data, d_out.data_ptr(), 16 * kept, D2H), a.reps, warmup=1)
                # the bytes of the two entry points are the same (the yardstick copies have written over both buffers)
                assert fe.assemble_map_device(ids, Ts, d_out, md, raster) == kept
                got = fe.assemble_map(ids, Ts, md, raster, out=h_out)
                assert len(got) == kept and got.tobytes() == d_out[:kept].cpu().numpy().tobytes()
                no = min(a.oracle_nodes, N)
                oc = [host_clouds[k % 8] for k in range(no)]
                t0 = time.perf_counter()
                want = mo.assemble(oc, Ts[:no], md, raster)[0]
                t_or = time.perf_counter() - t0
                assert mo.mismatch(got[:len(want)], want) is None
                res["configs"].append({
                    "cloud_skip": skip, "maximum_depth": "inf" if md == float("inf") else md, "mode": "raster" if raster else "compact",
                    "points": points, "kept": int(kept), "algorithmic_bytes": int(alg_bytes),
                    "device_entry": {"ms": round(t_dev * 1e3, 4), "ms_min": round(t_dev_min * 1e3, 4), "ms_max": round(t_dev_max * 1e3, 4),
                                     "points_per_s": round(points / t_dev, 1), "algorithmic_bytes_per_s": round(alg_bytes / t_dev, 1),
                                     "frac_of_hbm_peak": round(alg_bytes / t_dev / HBM_PEAK, 4)},
                    "hipMemcpy_d2d_same_bytes": {"ms": round(t_d2d * 1e3, 4), "bytes_moved_per_s": round(2 * half / t_d2d, 1),
                                                 "device_entry_over_copy": round(t_dev / t_d2d, 3)},
                    "host_entry": {"ms": round(t_host * 1e3, 3), "ms_min": round(t_host_min * 1e3, 3), "ms_max": round(t_host_max * 1e3, 3)},
                    "hipMemcpy_d2h_output_bytes": {"ms": round(t_d2h * 1e3, 3), "bytes": int(16 * kept)},
                    "numpy_oracle": {"nodes_timed": no, "s_timed": round(t_or, 3), "s_scaled_to_all_nodes": round(t_or * N / no, 2)},
                })
                print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
        del d_out, d_src, h_out
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
