"""Sensor-frame ingest: a recorded run from the images AS THE SENSOR DELIVERS THEM to matchable nodes, ms per frame at
640 x 480 (colour + depth of one size) and at 1280 x 960 colour with a 640 x 480 depth image (BASELINE configs[4]) for
  a_planes     rgbdfe_detect_describe_batch_nodes on gray / mask / float-depth planes prepared OUTSIDE the timed region
               (the route without this entry point, with its host-side conversion for free)
  b_rgb8_32f   rgbdfe_sensor_detect_describe_batch_nodes on the raw frames, rgb8 + 32FC1
  b_rgb8_16u   the same, rgb8 + 16UC1
  c_h2d        one host-to-device copy of a page-locked buffer of the size the raw frames of b_rgb8_32f occupy (GB/s)
The variants alternate inside every repetition; median of `reps` after two warm-up rounds; ORB detector, max_keypoints
1000 on a 3 x 3 grid; every run restarts from fresh thresholds.  (b) moves 3 W H + 4 w h (or + 2 w h) bytes per frame where
(a) moves 2 W H, so the figure to compare t_b with is 1.10 * (t_a + extra_bytes / bw_c); the tool prints both.  One JSON line.
    python tools/bench_sensor_ingest.py [frames reps]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbdslam_v2_amd import synth
from rgbdslam_v2_amd.frontend import FrontEnd

n_frames, reps = [int(v) for v in (sys.argv[1:3] + ["112", "5"][len(sys.argv) - 1:])]
MAX_KP = 1000


def median(v):
    return sorted(v)[len(v) // 2]


def bench_size(width, height, dw, dh):
    import torch
    seq = synth.make_image_sequence(n_frames=28, width=width, height=height, seed=1)
    dseq = seq if (dw, dh) == (width, height) else synth.make_image_sequence(n_frames=28, width=dw, height=dh, seed=1)
    idx = synth.forth_and_back(n_frames, 28)
    g = seq["gray"]
    # colour: three neighbouring views of the sequence as the three channels
    colour = [np.ascontiguousarray(np.stack([g[i], g[(i + 1) % 28], g[(i + 2) % 28]], -1)) for i in range(28)]
    vis = [colour[i] for i in idx]
    d32 = [np.ascontiguousarray(dseq["depth"][i]) for i in idx]
    d16 = [np.where(np.isnan(d), 0, np.rint(np.nan_to_num(d) * 1000.0)).astype(np.uint16) for d in d32]
    K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
    ids = np.arange(n_frames, dtype=np.int32)
    fe = FrontEnd(max_nodes=n_frames + 2, max_keypoints=1024, max_pairs_per_batch=64)
    fe.detector_configure(max_keypoints=MAX_KP, grid_resolution=3)
    planes = [fe.ingest_frame(v, d, "rgb8") for v, d in zip(vis, d32)]   # outside the timed region
    grays, masks, depths = [p[0] for p in planes], [p[1] for p in planes], [p[2] for p in planes]
    raw_bytes = n_frames * (3 * width * height + 4 * dw * dh)
    pinned = torch.empty(raw_bytes, dtype=torch.uint8).pin_memory()
    dev = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda")

    def a_planes():
        fe.set_detector_type("ORB")
        out = fe.detect_describe_batch(grays, masks, depths, *K, node_ids=ids, copy=False)
        return int(sum(len(o[0]) for o in out))

    def b_raw(dep):
        fe.set_detector_type("ORB")
        out = fe.sensor_detect_describe_batch_nodes(vis, dep, *K, node_ids=ids, visual_encoding="rgb8")
        return int(sum(len(o[0]) for o in out))

    def c_h2d():
        dev.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()
        return 0

    variants = (("a_planes", a_planes), ("b_rgb8_32f", lambda: b_raw(d32)), ("b_rgb8_16u", lambda: b_raw(d16)), ("c_h2d", c_h2d))
    ts = {name: [] for name, _ in variants}
    kps = {}
    for r in range(reps + 2):
        for name, fn in variants:
            t0 = time.perf_counter()
            kps[name] = fn()
            if r >= 2:
                ts[name].append(time.perf_counter() - t0)
    fe.close()
    res = {}
    for name in ("a_planes", "b_rgb8_32f", "b_rgb8_16u"):
        res[name] = {"ms_per_frame": round(median(ts[name]) * 1e3 / n_frames, 4), "keypoints_per_frame": round(kps[name] / n_frames, 1)}
    bw = raw_bytes / median(ts["c_h2d"])
    res["c_h2d_GBps"] = round(bw / 1e9, 2)
    t_a = res["a_planes"]["ms_per_frame"]
    for name, depth_bytes in (("b_rgb8_32f", 4), ("b_rgb8_16u", 2)):
        extra = 3 * width * height + depth_bytes * dw * dh - 2 * width * height
        bound = 1.10 * (t_a + extra / bw * 1e3)
        res[name]["bound_ms_per_frame"] = round(bound, 4)
        res[name]["within_bound"] = bool(res[name]["ms_per_frame"] <= bound)
    return res


out = {"frames": n_frames, "reps": reps, "max_keypoints": MAX_KP, "grid": 3, "detector": "ORB"}
for (w, h), (dw, dh) in (((640, 480), (640, 480)), ((1280, 960), (640, 480))):
    out["%dx%d_depth_%dx%d" % (w, h, dw, dh)] = bench_size(w, h, dw, dh)
try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    commit = ""
out["commit"] = commit or os.environ.get("BENCH_COMMIT") or None
print(json.dumps(out))
