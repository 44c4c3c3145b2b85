"""Measurement of the occupancy map's read side (rgbdfe_octomap_search, rgbdfe_octomap_cast_rays,
rgbdfe_octomap_view_cloud_device; csrc/octomap_query.hip, csrc/api_octomap.hip).

Map: that of tools/bench_octomap.py -- NODES (200) nodes of 640x480 depth as resident clouds (cloud_creation_skip_step 1)
with a random rigid transform each, inserted in one call with maximum_depth 3.5 m -- at the resolutions of --resolutions;
the leaves are then re-housed at a table load of at most 0.5, as the wrappers do.  After a warm-up, REPS (7) timed calls,
the median with minimum and maximum:

  search       the centres of all leaves plus as many points 1000 cells away (misses): host clock around the call, which
               stages the points, runs one kernel and copies the results back
  view         640x480 from POSES (16) of the insertion poses with the insertion intrinsics, ignore_unknown = 1 and
               max_range = the insertion's: view_cloud_device into a torch tensor on a torch stream, device events on that
               stream around the call: the kernel, no copy
  cast_rays    the same rays as host arrays: host clock around the call (two uploads, one kernel, the records back); the
               records' step counts are the walk iterations of the view, whose status plane must equal theirs
  yardstick    the view's cloud (the hit rays' end cells, NaN rows elsewhere) inserted from the same pose into a copy of the
               map: octo_ray_kernel walks the same cells and adds a compare-and-swap and an atomicMax per cell.  Host clock
               around insert_cloud, which also uploads the cloud and runs the apply and colour passes: an upper bound for
               the ray kernel.  Kernel against kernel: --kernel-trace.

Reported: points/s; rays/s, walk iterations/s and ns per iteration of the view (device events) and of cast_rays (host
clock); the yardstick's iterations (the hit rays' steps) and ns per iteration (host clock, upper bound).  The scalar oracle
of this project (tests/octomap_query_oracle.py) is timed on ORACLE_RAYS rays spread over the poses on the same host and scaled
by walk iterations; its records on that sample are checked against the device byte for byte.  This is the oracle, not the octomap
library: the library is not on this machine and has not been timed.
--kernel-trace FILE --profiled-record FILE: the per-dispatch kernel trace CSV of a profiler run of this tool (rocprofv3
--kernel-trace --stats, a run of its own at one resolution, usually of fewer nodes and poses) and the line that run printed;
the times of octo_view_kernel, octo_cast_kernel, octo_search_kernel and of the yardstick's octo_ray_kernel dispatches are
copied into the record with their ns per walk iteration: kernel against kernel.

Prints one JSON line; --out FILE also writes it there."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import octomap_query_oracle as qo  # noqa: E402
from bench_map_assembly import median_time  # noqa: E402
from rgbdslam_v2_amd import synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402

F = np.float32


def profiled_kernels(trace_csv, record_json):
    """Kernel times of a profiled run of this tool (one resolution): trace_csv is its per-dispatch kernel trace, record_json
    the line it printed.  Every pose dispatches octo_view_kernel 1 + reps times, so the mean over all its dispatches times
    the poses is the time of one pass over the poses; the yardstick's octo_ray_kernel dispatches are the last poses * (1 +
    reps) of that kernel (the ones before them built the map)."""
    rec = json.load(open(record_json))
    cfg, n_poses, reps = rec["configs"][0], len(rec["poses"]), rec["reps"]
    rows = list(csv.DictReader(open(trace_csv)))
    col = lambda part: [k for k in rows[0] if part in k.lower()][0]
    name, t0, t1 = col("kernel_name"), col("start_timestamp"), col("end_timestamp")
    rows.sort(key=lambda r: int(r[t0]))
    ns = lambda kernel: [int(r[t1]) - int(r[t0]) for r in rows if kernel in r[name]]
    view, ray, cast, search = ns("octo_view_kernel"), ns("octo_ray_kernel")[-n_poses * (1 + reps):], ns("octo_cast_kernel"), ns("octo_search_kernel")
    it, hit_it = cfg["walk_iterations"], cfg["yardstick_insert_of_the_hit_rays"]["walk_iterations"]
    view_pass, ray_pass = statistics.mean(view) * n_poses, statistics.mean(ray) * n_poses
    return {"nodes": rec["nodes"], "poses": n_poses, "reps": reps, "resolution": cfg["resolution"], "leaves": cfg["leaves"],
            "walk_iterations": it, "walk_iterations_of_the_hit_rays": hit_it,
            "octo_view_kernel": {"dispatches": len(view), "mean_ns": round(statistics.mean(view), 1),
                                 "ns_per_iteration": round(view_pass / it, 4)},
            "octo_cast_kernel_mean_ns": round(statistics.mean(cast), 1) if cast else None,
            "octo_search_kernel": {"dispatches": len(search), "mean_ns": round(statistics.mean(search), 1),
                                   "points_per_s": round(cfg["search"]["points"] / statistics.mean(search) * 1e9, 1)},
            "octo_ray_kernel_of_the_yardstick": {"dispatches": len(ray), "mean_ns": round(statistics.mean(ray), 1),
                                                 "ns_per_iteration": round(ray_pass / max(1, hit_it), 4)}}


def pixel_rays(T, fx, fy, cx, cy, rows, cols):
    """Origins and directions of a view's pixels, by the contract's arithmetic (float, one rounding per operation)."""
    R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    u, v = np.meshgrid(np.arange(cols, dtype=np.float32), np.arange(rows, dtype=np.float32))
    x, y = (u - F(cx)) / F(fx), (v - F(cy)) / F(fy)
    D = np.stack([(R[a, 0] * x + R[a, 1] * y) + R[a, 2] for a in range(3)], axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(t, D.shape)), np.ascontiguousarray(D)


def spread(ts):
    return {"s": round(statistics.median(ts), 6), "s_min": round(min(ts), 6), "s_max": round(max(ts), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--resolutions", type=float, nargs="+", default=[0.1])
    ap.add_argument("--max-range", type=float, default=3.5)
    ap.add_argument("--oracle-rays", type=int, default=512)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--profiled-record", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_octomap_query needs the GPU: no device, no figure")
    base = synth.make_depth_sequence(n_frames=8, nan_fraction=0.10)
    K = (base["fx"], base["fy"], base["cx"], base["cy"])
    depth = (base["depth"] * np.float32(1.5)).astype(np.float32)
    rows, cols = depth.shape[1:]
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
    poses = [int(p) for p in np.linspace(0, N - 1, min(a.poses, N)).round()]
    stream = torch.cuda.Stream(device="cuda:0")
    res = {"nodes": N, "frame": "%dx%d" % (cols, rows), "reps": a.reps, "poses": poses, "max_range": a.max_range,
           "ignore_unknown": 1, "configs": []}
    for resolution in a.resolutions:
        m = fe.octomap(1 << 22, resolution=resolution)
        t0 = time.perf_counter()
        m.insert_nodes(ids, Ts, a.max_range)
        t_build = time.perf_counter() - t0
        if 2 * len(m) > m.capacity:
            m.reserve(2 * len(m))
        leaves = m.leaves()
        cfg = {"resolution": resolution, "leaves": len(leaves), "capacity_cells": m.capacity,
               "table_load": round(len(leaves) / m.capacity, 4), "insert_s_once": round(t_build, 3)}

        # search: every leaf's centre, and as many misses
        c = ((leaves["key"].astype(np.float64) - 32768.0 + 0.5) * resolution).astype(np.float32)
        far = c + np.asarray([0.0, 0.0, 1000 * resolution], np.float32)
        P = np.ascontiguousarray(np.concatenate([c, far]))
        found, _ = m.search(P, grow=False)
        assert (found[:len(c)] == 1).all() and (found[len(c):] == 0).all()
        t, t_min, t_max = median_time(lambda: m.search(P, grow=False), a.reps)
        cfg["search"] = {"points": len(P), "s": round(t, 6), "s_min": round(t_min, 6), "s_max": round(t_max, 6),
                         "points_per_s": round(len(P) / t, 1), "clock": "host, around the call (uploads, kernel, read-back)"}

        # views, the same rays through cast_rays, and the insertion of the same rays
        out = torch.empty((rows, cols, 4), dtype=torch.float32, device="cuda:0")
        status = torch.empty((rows, cols), dtype=torch.uint8, device="cuda:0")
        twin = fe.octomap(m.capacity, resolution=resolution)   # the yardstick inserts into a copy
        twin.set_leaves(leaves)
        tv, tc, ti = [], [], []
        iters = hit_iters = hits = 0
        statuses = np.zeros(8, np.int64)
        for p in poses:
            T = Ts[p]
            view = lambda st=status: m.view_cloud_device(out, T, *K, True, a.max_range, None, status=st, stream=stream.cuda_stream,
                                                         grow=False)
            view()
            ts = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                view()
                e1.record(stream)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3)
            tv.append(statistics.median(ts))
            O, D = pixel_rays(T, *K, rows, cols)
            rec = m.cast_rays(O, D, True, a.max_range, grow=False)
            assert (rec["status"] == status.cpu().numpy().reshape(-1)).all()
            tc.append(median_time(lambda: m.cast_rays(O, D, True, a.max_range, grow=False), a.reps, warmup=1)[0])
            hit = rec["status"] == qo.HIT
            iters += int(rec["steps"].sum())
            hit_iters += int(rec["steps"][hit].sum())
            hits += int(hit.sum())
            statuses += np.bincount(rec["status"], minlength=8)[:8]
            cloud = out.cpu().numpy().reshape(-1, 4)
            ti.append(median_time(lambda: twin.insert_cloud(cloud, T, -1.0), a.reps, warmup=1)[0])
        rays = rows * cols * len(poses)
        t_view, t_cast, t_ins = sum(tv), sum(tc), sum(ti)
        cfg["rays"] = rays
        cfg["walk_iterations"] = iters
        cfg["statuses"] = {str(i): int(n) for i, n in enumerate(statuses) if n}
        cfg["view_cloud_device"] = dict(spread(tv), s_all_poses=round(t_view, 6), rays_per_s=round(rays / t_view, 1),
                                        iterations_per_s=round(iters / t_view, 1), ns_per_iteration=round(t_view / iters * 1e9, 4),
                                        clock="device events on the call's stream; s: the median pose")
        cfg["cast_rays"] = dict(spread(tc), s_all_poses=round(t_cast, 6), rays_per_s=round(rays / t_cast, 1),
                                iterations_per_s=round(iters / t_cast, 1), ns_per_iteration=round(t_cast / iters * 1e9, 4),
                                clock="host, around the call (two uploads, kernel, records back)")
        cfg["yardstick_insert_of_the_hit_rays"] = dict(
            spread(ti), s_all_poses=round(t_ins, 6), rays=hits, walk_iterations=hit_iters,
            ns_per_iteration=round(t_ins / max(1, hit_iters) * 1e9, 4),
            clock="host, around insert_cloud (upload, ray, apply, colour passes): an upper bound for octo_ray_kernel")
        twin.close()

        # the oracle of this project on a sample of every pose's rays, scaled by walk iterations
        if a.oracle_rays > 0 and len(leaves) <= 3000000:
            per = max(1, a.oracle_rays // len(poses))
            O, D = [], []
            for p in poses:
                o, d = pixel_rays(Ts[p], *K, rows, cols)
                pick = np.linspace(0, len(o) - 1, per).round().astype(np.int64)
                O.append(o[pick]), D.append(d[pick])
            O, D = np.concatenate(O), np.concatenate(D)
            orc = qo.QueryOracle(leaves, resolution=resolution)
            t0 = time.perf_counter()
            ref = orc.cast_rays(O, D, True, a.max_range)
            t_or = time.perf_counter() - t0
            got = m.cast_rays(O, D, True, a.max_range, grow=False)
            assert got.tobytes() == ref.tobytes()
            it = int(ref["steps"].sum())
            cfg["scalar_oracle_of_this_project"] = {"rays_timed": len(O), "walk_iterations_timed": it, "s_timed": round(t_or, 3),
                                                    "s_scaled_to_all_iterations": round(t_or * iters / max(1, it), 1),
                                                    "equal_to_device_on_the_sample": True}
        else:
            cfg["scalar_oracle_of_this_project"] = "not measured"
        m.close()
        res["configs"].append(cfg)
        print(json.dumps(cfg), file=sys.stderr, flush=True)
    for k in range(N):
        fe.release_node_cloud(k)
    fe.close()
    res["kernels_in_the_profiled_run"] = (profiled_kernels(a.kernel_trace, a.profiled_record)
                                          if a.kernel_trace and a.profiled_record else "not measured")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
