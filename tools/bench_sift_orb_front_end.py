"""feature_detector_type "SIFTGPU" with feature_extractor_type "ORB": a recorded run from images to matchable ORB nodes at
640 x 480, ms per frame for
  chained     rgbdfe_sift_detect -> removeDepthless and the cut on the host -> rgbdfe_orb_compute -> rgbdfe_project_to_3d ->
              rgbdfe_upload_node, frame by frame from Python
  batch_host  rgbdfe_sift_detect_orb_describe_batch_nodes, host outputs filled
  batch_null  rgbdfe_sift_detect_orb_describe_batch_nodes, NULL host outputs
  sift_nodes_null  rgbdfe_sift_detect_batch_nodes with NULL host outputs (the SIFTGPU-extractor batch, for comparison)
with max_keypoints 1000, on synthetic frames (a moving camera over a textured plane) and on the photograph fixtures (depth: a
noisy plane with holes); median of `reps` runs after one warm-up run; one JSON line.
    python tools/bench_sift_orb_front_end.py [frames reps]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sift_orb_oracle as soo  # noqa: E402
from rgbdslam_v2_amd import synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402
from test_gpu_orb_photos import binary_mask, intrinsics, plane_depth  # noqa: E402
from test_oracle_orb_photos import load_photos  # noqa: E402

n_frames, reps = [int(v) for v in (sys.argv[1:3] + ["56", "5"][len(sys.argv) - 1:])]
MAX_KP = 1000


def synthetic():
    seq = synth.make_image_sequence(n_frames=28, width=640, height=480, seed=1)
    idx = synth.forth_and_back(n_frames, 28)
    return [seq["gray"][i] for i in idx], [seq["depth"][i] for i in idx], (seq["fx"], seq["fy"], seq["cx"], seq["cy"])


def photographs():
    photos = load_photos()
    names = ["640_1", "640_2", "640_3", "640_4", "640_5"]
    grays = [photos[names[i % len(names)]] for i in range(n_frames)]
    depths = []
    for i, g in enumerate(grays):
        d = plane_depth(g.shape, 2.0, i)
        d[binary_mask(g.shape, i) == 0] = np.nan
        depths.append(d)
    return grays, depths, intrinsics(grays[0].shape)


ids = np.arange(n_frames, dtype=np.int32)
fe = FrontEnd(max_nodes=n_frames + 2, max_keypoints=MAX_KP, max_pairs_per_batch=64)
out = {"frames": n_frames, "reps": reps, "max_keypoints": MAX_KP, "size": "640x480"}
for set_name, make in (("synthetic", synthetic), ("photographs", photographs)):
    grays, depths, K = make()

    def chained():
        n = 0
        for f in range(n_frames):
            g, d = grays[f], depths[f]
            kp, _ = fe.sift_detect(g, None, MAX_KP)
            kp = soo.remove_depthless(kp, d)[:MAX_KP]
            desc, xyz = np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.float32)
            if len(kp):
                kp, desc = fe.orb_compute(g, kp)
                if len(kp):
                    kept, xyz = fe.project_to_3d(np.stack([kp["x"], kp["y"]], 1), d, *K, 1.0, MAX_KP)
                    desc = desc[np.asarray(kept, np.int64)]
            fe.upload_node(int(ids[f]), desc, xyz)
            n += len(xyz)
        return n

    def batch(host):
        r = fe.sift_detect_orb_describe_batch_nodes(grays, depths, *K, ids, max_keypoints=MAX_KP, return_features=host)
        return int(sum(len(o[0]) for o in r)) if host else int(np.sum(r))

    def sift_nodes():
        return int(np.sum(fe.sift_detect_batch_nodes(grays, depths, *K, ids, max_keypoints=MAX_KP, return_features=False)))

    res = {}
    for name, fn in (("chained", chained), ("batch_host", lambda: batch(True)), ("batch_null", lambda: batch(False)),
                     ("sift_nodes_null", sift_nodes)):
        fn()
        ts, kps = [], 0
        for _ in range(reps):
            t0 = time.perf_counter()
            kps = fn()
            ts.append((time.perf_counter() - t0) * 1e3 / n_frames)
        res[name] = {"ms_per_frame": round(sorted(ts)[len(ts) // 2], 4), "features_per_frame": round(kps / n_frames, 1)}
    out[set_name] = res
fe.close()
try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    commit = ""
out["commit"] = commit or os.environ.get("BENCH_COMMIT") or None
print(json.dumps(out))
