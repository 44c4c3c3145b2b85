"""Measurement of the map files (rgbdfe_save_map; csrc/api_map_files.hip, csrc/map_files.hip).

Workload: the 200-cloud 640x480 scene of tools/bench_map_assembly.py (cloud_creation_skip_step 1, maximum_depth +inf, 10 %
NaN holes), written to --dir (default /dev/shm) as PCD and as PLY, compact and raster.  Per configuration two ways to the same
file, timed in the same process, alternating, RUNS times each after one warm-up of both:

* streamed   FrontEnd.save_map: the map group by group through two device buffers and two page-locked slots;
* today      what a user had before: FrontEnd.assemble_map into a host array that is reused, then ndarray.tofile of the
             file's bytes (PCD: header + the rows; PLY: header + the rows packed by numpy + the camera record; the numpy
             packing is timed on its own as well).

The two files are compared byte for byte.  Beside the times: the device and page-locked scratch the streamed export reports,
and what today's path holds (the assembled map once on the device, in the call's staging, and once on the host).  With
--copy-yardstick the tool also times a device-to-device hipMemcpy of the bytes one launch of cloud_pack_ply_kernel writes
for a full group (15 bytes x chunk_points): the figure the kernel's time in a kernel trace is held against.

Prints one JSON line; --out FILE also writes it there."""
import argparse
import ctypes
import hashlib
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
import cloud_file_oracle as co  # noqa: E402
from rgbdslam_v2_amd import _lib, synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402


def sha1(path):
    h = hashlib.sha1()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def spread(ts):
    return {"median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk-points", type=int, default=0)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--formats", default="pcd,ply")
    ap.add_argument("--copy-yardstick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_files needs the GPU: no device, no figure")
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
    for k in range(N):
        fe.upload_node_cloud(k, depth[k % 8], *K, rgb=rgb[k % 8], min_depth=0.1, cloud_skip=1)
    points = N * depth.shape[1] * depth.shape[2]
    h_out = np.zeros((points, 4), np.float32)   # today's host array: pageable, touched once, reused
    res = {"tool": "bench_map_files", "nodes": N, "frame": "640x480", "runs": a.runs, "dir": a.dir, "points": points,
           "chunk_points": a.chunk_points or 1 << 20, "configs": []}
    f_new, f_old = os.path.join(a.dir, "rgbdfe_bench_streamed"), os.path.join(a.dir, "rgbdfe_bench_today")
    try:
        for fmt in a.formats.split(","):
            for raster in (False, True):
                t_new, t_old, t_pack, st = [], [], [], None

                def streamed():
                    return fe.save_map(f_new + "." + fmt, ids, Ts, float("inf"), raster, chunk_points=a.chunk_points)

                def today():
                    rows = fe.assemble_map(ids, Ts, float("inf"), raster, out=h_out)
                    with open(f_old + "." + fmt, "wb") as f:
                        if fmt == "pcd":
                            f.write(co.pcd_header(len(rows), 1))
                            rows.tofile(f)
                            return 0.0
                        t0 = time.perf_counter()
                        packed = np.frombuffer(co.pack_ply(rows), np.uint8)
                        dt = time.perf_counter() - t0
                        f.write((co.PLY_HEADER % len(rows)).encode("ascii"))
                        packed.tofile(f)
                        f.write(co.ply_camera(len(rows), 1))
                        return dt
                streamed(), today()   # the warm-up of both
                for _ in range(a.runs):
                    t0 = time.perf_counter()
                    st = streamed()
                    t_new.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    t_pack.append(today())
                    t_old.append(time.perf_counter() - t0)
                same = sha1(f_new + "." + fmt) == sha1(f_old + "." + fmt)
                kept = st["points"]
                cfg = {"format": fmt, "mode": "raster" if raster else "compact", "kept": kept, "file_bytes": st["bytes_written"],
                       "files_identical": same, "groups": st["groups"],
                       "streamed": dict(spread(t_new), device_scratch_bytes=st["device_scratch_bytes"], pinned_bytes=st["pinned_bytes"],
                                        table_bytes=st["table_bytes"]),
                       "today": dict(spread(t_old), device_staging_bytes=16 * kept, host_array_bytes=16 * kept, pinned_bytes=0,
                                     numpy_pack_median_s=round(statistics.median(t_pack), 4))}
                cfg["streamed_over_today"] = round(cfg["streamed"]["median_s"] / cfg["today"]["median_s"], 3)
                cfg["scratch_fraction_of_today"] = round((st["device_scratch_bytes"] + st["pinned_bytes"] + st["table_bytes"]) / (32.0 * kept), 4)
                res["configs"].append(cfg)
                print(json.dumps(cfg), file=sys.stderr, flush=True)
                assert same, "the two paths wrote different files"
        if a.copy_yardstick:
            hip = ctypes.CDLL(_lib.LIB_PATH)  # the HIP runtime the library itself is linked against
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            nbytes = 15 * res["chunk_points"]
            src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
            dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
            ts = []
            for i in range(12):
                t0 = time.perf_counter()
                if hip.hipMemcpy(dst.data_ptr(), src.data_ptr(), nbytes, 3) != 0 or hip.hipDeviceSynchronize() != 0:
                    raise RuntimeError("hipMemcpy failed")
                if i >= 2:
                    ts.append(time.perf_counter() - t0)
            res["hipMemcpy_d2d_of_one_launchs_output"] = {"bytes": nbytes, "median_us": round(1e6 * statistics.median(ts), 2),
                                                          "min_us": round(1e6 * min(ts), 2)}
    finally:
        for p in (f_new, f_old):
            for fmt in ("pcd", "ply"):
                if os.path.exists(p + "." + fmt):
                    os.remove(p + "." + fmt)
    for k in range(N):
        fe.release_node_cloud(k)
    fe.close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True,
                                    text=True).stdout.strip()) if commit else False
    except OSError:
        commit, dirty = "", False
    commit = commit or os.environ.get("BENCH_COMMIT") or None
    dirty = dirty or os.environ.get("BENCH_TREE_DIRTY", "") not in ("", "0")
    res["commit"] = ("uncommitted changes on top of %s" % commit) if (commit and dirty) else commit
    res["device"] = torch.cuda.get_device_name(0)
    res["note"] = ("one call of tools/bench_map_files.py on one device; host clock around every call, each of which ends with the file "
                   "closed; the two paths alternate within one process")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
