"""Measurement of rendering (rgbdfe_render_nodes / rgbdfe_render_nodes_device; csrc/render.hip).

Workload: the scene of tools/bench_display_geometry.py, built the same way -- 200 nodes of 640x480 depth (the wavy wall of
synth.make_depth_sequence pushed back to ~3 m, 10 % NaN holes, two boxes pushed 0.8 m back) as resident clouds at
cloud_creation_skip_step 2 (320 x 240 points), a random rigid transform per node -- rendered at 640 x 480 as POINTS, TRIANGLES
and TRIANGLE_STRIP, through the sensor's intrinsics from the last node's pose and from a zoomed-out pose (the last pose pulled
12 m back along its own axis, so most of the scene is in view and most primitives are small).  Per configuration, medians of
REPS repetitions after a warm-up, all in one process:

* the device entry point (images stay on the device) and the host entry point (four images into reused pageable buffers):
  ms per call, host clock around calls that end in a stream synchronise;
* kernel launches and read-backs of a call (by construction: the sizes pass of display geometry, then per group of nodes the
  display-geometry write and three render kernels, one clear; a read of the sizes per display-geometry call);
* fragments offered to the depth test and fragments that lowered a pixel on arrival, from one more call with the counting
  kernels on (rgbdfe_render_fragment_stats), and the pixels drawn;
* beside them the rgbdfe_display_geometry_device time of the same nodes and form in the same run: the renderer runs that
  call itself (twice over the counting half), so it cannot be faster than the stream it consumes.

Prints one JSON line; --out FILE also writes it there.  The line is stamped with `git rev-parse --short HEAD` of the tree, or
BENCH_COMMIT where the tree travels without its history."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbdslam_v2_amd import synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd, render_sensor_camera  # noqa: E402

FORMS = [("POINTS", 0, 1), ("TRIANGLES", 1, 1), ("TRIANGLE_STRIP", 2, 1)]
DEFAULT_GROUP = 1 << 23  # vertices in flight when the caller names no cap (csrc/api_render.hip)


def median_time(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def groups_of(offsets, cap):
    """the groups api_render.hip forms: consecutive nodes whose vertices stay within cap; groups without a vertex are skipped"""
    n, k, out = len(offsets) - 1, 0, 0
    while k < n:
        e = k
        while e < n and offsets[e + 1] - offsets[k] <= cap:
            e += 1
        out += offsets[e] > offsets[k]
        k = e
    return int(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit("at least 7 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_render needs the GPU: no device, no figure")

    base = synth.make_depth_sequence(n_frames=8, nan_fraction=0.10)
    K = (base["fx"], base["fy"], base["cx"], base["cy"])
    depth = (base["depth"] * np.float32(1.5)).astype(np.float32)
    depth[:, 100:220, 80:240] += np.float32(0.8)
    depth[:, 260:400, 380:560] += np.float32(0.8)
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    N, W, H = a.nodes, a.width, a.height
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
    last = Ts[-1].astype(np.float64)
    back = last.copy()
    back[:3, 3] -= 12.0 * last[:3, 2]  # 12 m back along the pose's own viewing axis
    sx, sy = W / depth.shape[2], H / depth.shape[1]
    k_img = (K[0] * sx, K[1] * sy, (K[2] + 0.5) * sx - 0.5, (K[3] + 0.5) * sy - 0.5)
    cams = [("last_pose", render_sensor_camera(*k_img, W, H, pose=last)), ("zoomed_out", render_sensor_camera(*k_img, W, H, pose=back))]
    dev = torch.device("cuda", 0)
    t_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    t_depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    t_ids = torch.empty((H, W), dtype=torch.int64, device=dev)
    t_node = torch.empty((H, W), dtype=torch.int32, device=dev)
    res = {"nodes": N, "cloud": "%dx%d" % (depth.shape[2] // 2, depth.shape[1] // 2), "image": "%dx%d" % (W, H), "reps": a.reps,
           "gl_point_size": 2.0, "cull": 0, "squared_meshing_threshold": 0.0009, "max_vertices_in_flight": 0, "configs": []}
    for name, form, step in FORMS:
        disp = dict(display_type=form, visualization_skip_step=step)
        first = fe.display_geometry(ids[:8], Ts[:8], **disp)  # for the buffers' sizes: the clouds cycle over 8 frames
        nv_cap = int(first["node_offsets"][-1]) * (N // 8 + 1) + 16
        ns_cap = int(first["node_strip_offsets"][-1]) * (N // 8 + 1) + 16
        d_v = torch.empty((nv_cap, 4), dtype=torch.float32, device=dev)
        d_s = torch.empty((ns_cap, 2), dtype=torch.int64, device=dev)
        r = fe.display_geometry_device(ids, d_v, d_s, Ts, **disp)
        t_disp, _, _ = median_time(lambda: fe.display_geometry_device(ids, d_v, d_s, Ts, **disp), a.reps)
        del d_v, d_s
        torch.cuda.empty_cache()
        kinds = len(set(int(t) == 2 for t in r["node_types"]))
        groups = groups_of([int(v) for v in r["node_offsets"]], DEFAULT_GROUP)
        for cam_name, (view, proj) in cams:
            kw = dict(transforms=Ts, view=view, projection=proj, gl_point_size=2.0, cull=False, **disp)

            def to_device():
                fe.render_nodes_device(ids, t_rgba, t_depth, t_ids, t_node, **kw)

            def to_host():
                return fe.render_nodes(ids, width=W, height=H, **kw)
            t_dev, t_dev_min, t_dev_max = median_time(to_device, a.reps)
            t_host, t_host_min, t_host_max = median_time(to_host, a.reps, warmup=1)
            fe.render_fragment_stats(True)
            out = to_host()
            tested, won = fe.render_fragment_stats(False)
            to_device()
            assert out["ids"].tobytes() == t_ids.cpu().numpy().tobytes() and out["rgba"].tobytes() == t_rgba.cpu().numpy().tobytes()
            assert out["depth"].tobytes() == t_depth.cpu().numpy().tobytes()
            res["configs"].append({
                "form": name, "camera": cam_name, "vertices": int(r["n_vertices"]), "strips": int(r["n_strips"]), "groups": groups,
                "launches": (kinds + 1) + 1 + groups * (2 * kinds + 1 + 3), "readbacks": 1 + groups,
                "readbacks_host_entry": 1 + groups + 4,
                "fragments_tested": tested, "fragments_won_on_arrival": won, "pixels_drawn": int(np.sum(out["ids"] >= 0)),
                "device_entry": {"ms": round(t_dev * 1e3, 4), "ms_min": round(t_dev_min * 1e3, 4), "ms_max": round(t_dev_max * 1e3, 4)},
                "host_entry": {"ms": round(t_host * 1e3, 4), "ms_min": round(t_host_min * 1e3, 4), "ms_max": round(t_host_max * 1e3, 4)},
                "display_geometry_device_ms": round(t_disp * 1e3, 4), "device_entry_over_display_geometry": round(t_dev / t_disp, 3),
            })
            print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
    for k in range(N):
        fe.release_node_cloud(k)
    fe.close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res["commit"] = commit or os.environ.get("BENCH_COMMIT") or None
    res["device"] = torch.cuda.get_device_name(0)
    res["note"] = ("one call of tools/bench_render.py on one device (`device`); times are medians of `reps` calls after warm-up, host "
                   "clock around calls that end in a stream synchronise")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
