"""Measurement of display geometry (rgbdfe_display_geometry / rgbdfe_display_geometry_device; csrc/display_geometry.hip).

Workload: the map-assembly workload of tools/bench_map_assembly.py -- 200 nodes of 640x480 depth (the wavy wall of
synth.make_depth_sequence pushed back to ~3 m, 10 % NaN holes) as resident clouds at cloud_creation_skip_step 2 (320 x 240
points), a random rigid transform per node -- with two boxes pushed 0.8 m back in every frame, so that the holes and the
boxes' rims break the strips.  Per form (POINTS, TRIANGLES, TRIANGLE_STRIP at steps 1 and 2), medians of REPS repetitions
after a warm-up, all in one process:

* the device entry point: seconds per call (host clock around the call, which ends in a stream synchronise) and per cloud, the
  output bytes (16 per vertex + 16 per strip record) -- and beside it a hipMemcpy device-to-device of the same output bytes,
  the yardstick of the same run; kernel launches and read-backs of a call (by construction: a count and a write launch per
  kind of node listed, one scan, one read of the sizes);
* the host entry point: seconds per call into pageable buffers that are reused;
* the numpy oracle (tests/display_oracle.py, the vectorised forms) on the same host, timed on ORACLE_NODES nodes and scaled.

Prints one JSON line; --out FILE also writes it there.  The line is stamped with `git rev-parse --short HEAD` of the tree, or
BENCH_COMMIT where the tree travels without its history."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import display_oracle as do  # noqa: E402
from rgbdslam_v2_amd import _lib, synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402

FORMS = [("POINTS", do.POINTS, 1), ("TRIANGLES", do.TRIANGLES, 1), ("TRIANGLE_STRIP", do.TRIANGLE_STRIP, 1),
         ("TRIANGLE_STRIP", do.TRIANGLE_STRIP, 2)]


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
    ap.add_argument("--oracle-nodes", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit("at least 7 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_display_geometry needs the GPU: no device, no figure")
    hip = ctypes.CDLL(_lib.LIB_PATH)  # the HIP runtime the library itself is linked against
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    D2D = 3

    def hip_copy(dst, src, nbytes):
        if hip.hipMemcpy(dst, src, nbytes, D2D) != 0 or hip.hipDeviceSynchronize() != 0:
            raise RuntimeError("hipMemcpy failed")

    base = synth.make_depth_sequence(n_frames=8, nan_fraction=0.10)
    K = (base["fx"], base["fy"], base["cx"], base["cy"])
    depth = (base["depth"] * np.float32(1.5)).astype(np.float32)
    depth[:, 100:220, 80:240] += np.float32(0.8)
    depth[:, 260:400, 380:560] += np.float32(0.8)
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
    for k in range(N):
        fe.upload_node_cloud(k, depth[k % 8], *K, rgb=rgb[k % 8], min_depth=0.1, cloud_skip=2)
    host_clouds = [fe.node_cloud(k) for k in range(8)]
    rows, cols = host_clouds[0].shape[:2]
    res = {"nodes": N, "cloud": "%dx%d" % (cols, rows), "reps": a.reps, "nan_fraction": 0.10,
           "squared_meshing_threshold": 0.0009, "maximum_depth": "inf", "transforms": True, "configs": []}
    for name, form, step in FORMS:
        prm = do.default_params(display_type=form, visualization_skip_step=step)
        first = fe.display_geometry(ids[:8], Ts[:8], **prm)  # for the buffers' sizes: the clouds cycle over 8 frames
        nv_cap = int(first["node_offsets"][-1]) * (N // 8 + 1) + 16
        ns_cap = int(first["node_strip_offsets"][-1]) * (N // 8 + 1) + 16
        d_v = torch.empty((nv_cap, 4), dtype=torch.float32, device="cuda:0")
        d_s = torch.empty((ns_cap, 2), dtype=torch.int64, device="cuda:0")

        def dev():
            return fe.display_geometry_device(ids, d_v, d_s, Ts, **prm)
        r = dev()
        nv, ns = r["n_vertices"], r["n_strips"]
        out_bytes = 16 * nv + 16 * ns
        kinds = len(set(int(t) == do.TRIANGLE_STRIP for t in r["node_types"]))
        t_dev, t_dev_min, t_dev_max = median_time(dev, a.reps)
        d_src = torch.empty((out_bytes // 16 + 1, 4), dtype=torch.float32, device="cuda:0")
        d_dst = torch.empty((out_bytes // 16 + 1, 4), dtype=torch.float32, device="cuda:0")
        t_d2d, _, _ = median_time(lambda: hip_copy(d_dst.data_ptr(), d_src.data_ptr(), out_bytes), a.reps)
        t_host, t_host_min, t_host_max = median_time(lambda: fe.display_geometry(ids, Ts, **prm), a.reps, warmup=1)
        got = fe.display_geometry(ids, Ts, **prm)
        assert dev()["n_vertices"] == nv == len(got["vertices"]) and ns == len(got["strips"])
        assert got["vertices"].tobytes() == d_v[:nv].cpu().numpy().tobytes()
        assert got["strips"].tobytes() == d_s[:ns].cpu().numpy().tobytes()
        no = min(a.oracle_nodes, N)
        oc = [host_clouds[k % 8] for k in range(no)]
        t0 = time.perf_counter()
        want = do.display(oc, prm, Ts[:no])
        t_or = time.perf_counter() - t0
        assert do.same_vertices(got["vertices"][:len(want["vertices"])], want["vertices"])
        assert np.array_equal(got["strips"][:len(want["strips"])], want["strips"])
        res["configs"].append({
            "form": name, "visualization_skip_step": step, "points": N * rows * cols, "vertices": int(nv), "strips": int(ns),
            "output_bytes": int(out_bytes), "launches": 2 * kinds + 1, "readbacks": 1,
            "device_entry": {"ms": round(t_dev * 1e3, 4), "ms_min": round(t_dev_min * 1e3, 4), "ms_max": round(t_dev_max * 1e3, 4),
                             "us_per_cloud": round(t_dev * 1e6 / N, 3), "output_bytes_per_s": round(out_bytes / t_dev, 1)},
            "hipMemcpy_d2d_output_bytes": {"ms": round(t_d2d * 1e3, 4), "device_entry_over_copy": round(t_dev / t_d2d, 3)},
            "host_entry": {"ms": round(t_host * 1e3, 3), "ms_min": round(t_host_min * 1e3, 3), "ms_max": round(t_host_max * 1e3, 3),
                           "us_per_cloud": round(t_host * 1e6 / N, 2)},
            "numpy_oracle": {"nodes_timed": no, "s_timed": round(t_or, 3), "s_scaled_to_all_nodes": round(t_or * N / no, 2)},
        })
        print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
        del d_v, d_s, d_src, d_dst
        torch.cuda.empty_cache()
    for k in range(N):
        fe.release_node_cloud(k)
    fe.close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res["commit"] = commit or os.environ.get("BENCH_COMMIT") or None
    res["note"] = ("one call of tools/bench_display_geometry.py on one MI355X; times are medians of `reps` calls after warm-up, "
                   "host clock around calls that end in a stream synchronise")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
