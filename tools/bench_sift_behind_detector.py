"""feature_extractor_type "SIFTGPU" behind the ORB and FAST grid detectors: a recorded run from images to matchable float
nodes at 640 x 480, ms per frame for
  composed    rgbdfe_detect -> rgbdfe_project_to_3d -> rgbdfe_sift_describe -> rgbdfe_sift_node_features ->
              rgbdfe_upload_float_node, frame by frame from Python
  batch_host  rgbdfe_detect_sift_describe_batch_nodes, host outputs filled
  batch_null  rgbdfe_detect_sift_describe_batch_nodes, NULL host outputs
with max_keypoints 1000 on a 3 x 3 grid.  Synthetic frames (a moving camera over a textured plane, masks from the depth);
every mode restarts from fresh thresholds; median of `reps` runs after one warm-up run; one JSON line.
    python tools/bench_sift_behind_detector.py [frames reps]"""
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

n_frames, reps = [int(v) for v in (sys.argv[1:3] + ["56", "5"][len(sys.argv) - 1:])]
MAX_KP = 1000

seq = synth.make_image_sequence(n_frames=28, width=640, height=480, seed=1)
idx = synth.forth_and_back(n_frames, 28)
grays = [seq["gray"][i] for i in idx]
depths = [seq["depth"][i] for i in idx]
masks = [np.where(seq["mask"][i] > 0, 255, 0).astype(np.uint8) for i in idx]
K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
ids = np.arange(n_frames, dtype=np.int32)
fe = FrontEnd(max_nodes=n_frames + 2, max_keypoints=MAX_KP, max_pairs_per_batch=64)
fe.detector_configure(max_keypoints=MAX_KP)


def composed():
    n = 0
    for f in range(n_frames):
        g, m, d = grays[f], masks[f], depths[f]
        agg = fe.detect(g, m)
        kept, _ = fe.project_to_3d(np.stack([agg["x"], agg["y"]], 1), d, *K, 1.0, MAX_KP) if len(agg) else ([], None)
        if len(kept):
            kl, desc = fe.sift_describe(g, agg[np.asarray(kept)])
        else:
            kl, desc = fe.sift_detect(g, None, MAX_KP)
        if len(kl):
            k2, xyz, raw, feat = fe.sift_node_features(np.stack([kl["x"], kl["y"]], 1), desc, d, *K, 1.0, MAX_KP, True)
        else:
            xyz, feat = np.zeros((0, 4), np.float32), np.zeros((0, 128), np.float32)
        fe.upload_float_node(int(ids[f]), feat, xyz)
        n += len(xyz)
    return n


def batch(host):
    out = fe.detect_sift_describe_batch_nodes(grays, masks, depths, *K, ids, return_features=host)
    return int(sum(len(o[0]) for o in out)) if host else int(np.sum(out))


out = {"frames": n_frames, "reps": reps, "max_keypoints": MAX_KP, "grid": 3, "size": "640x480"}
for kind in ("ORB", "FAST"):
    res = {}
    for name, fn in (("composed", composed), ("batch_host", lambda: batch(True)), ("batch_null", lambda: batch(False))):
        fe.set_detector_type(kind)
        fn()
        ts, kps = [], 0
        for _ in range(reps):
            fe.set_detector_type(kind)   # fresh thresholds: every run sees the same sequence from the same state
            t0 = time.perf_counter()
            kps = fn()
            ts.append((time.perf_counter() - t0) * 1e3 / n_frames)
        res[name] = {"ms_per_frame": round(sorted(ts)[len(ts) // 2], 4), "features_per_frame": round(kps / n_frames, 1)}
    out[kind] = res
fe.close()
try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    commit = ""
out["commit"] = commit or os.environ.get("BENCH_COMMIT") or None
print(json.dumps(out))
