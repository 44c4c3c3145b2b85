"""The SIFTGPU front end of a recorded run, from images to matchable float nodes: ms per frame for
  (a) rgbdfe_sift_detect_batch alone (extraction, no nodes),
  (b) the composed chain the host joins frame by frame: sift_detect_batch -> sift_node_features -> upload_float_node,
  (c) rgbdfe_sift_detect_batch_nodes with host outputs, and (d) with NULL host outputs;
(b) - (d) each followed by match_flann_pair_list of every node against its 20 predecessors (reported separately and as a
total).  640 x 480 synthetic frames, 112 frames, median of 7 repetitions after two warm-up runs; one JSON line.
    python tools/bench_sift_front_end.py [frames reps]"""
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

n_frames, reps = [int(v) for v in (sys.argv[1:3] + ["112", "7"][len(sys.argv) - 1:])]
MAX_KP, WINDOW = 1000, 20
seq = synth.make_image_sequence(n_frames=28, seed=1)
idx = synth.forth_and_back(n_frames, 28)
grays = [seq["gray"][i] for i in idx]
depths = [seq["depth"][i] for i in idx]
K = (seq["fx"], seq["fy"], seq["cx"], seq["cy"])
ids = np.arange(n_frames, dtype=np.int32)
pq = np.array([f for f in range(n_frames) for c in range(1, WINDOW + 1) if f - c >= 0], np.int32)
pt = np.array([f - c for f in range(n_frames) for c in range(1, WINDOW + 1) if f - c >= 0], np.int32)
fe = FrontEnd(max_nodes=n_frames + 2, max_keypoints=1024, max_pairs_per_batch=4096)


def extract_only():
    fe.sift_detect_batch(grays, max_keypoints=MAX_KP, copy=False)


def composed():
    dets = fe.sift_detect_batch(grays, max_keypoints=MAX_KP, copy=False)
    for f, (kp, desc) in enumerate(dets):
        xy = np.stack([kp["x"], kp["y"]], 1)
        _, xyz, _, feat = fe.sift_node_features(xy, desc, depths[f], *K, max_keypoints=MAX_KP)
        fe.upload_float_node(int(ids[f]), feat, xyz)


def nodes_host():
    fe.sift_detect_batch_nodes(grays, depths, *K, node_ids=ids, max_keypoints=MAX_KP, copy=False)


def nodes_null():
    fe.sift_detect_batch_nodes(grays, depths, *K, node_ids=ids, max_keypoints=MAX_KP, return_features=False)


def match():
    out, _ = fe.match_flann_pair_list(pq, pt)
    return int((out["id1"] >= 0).sum())


def measure(front, with_match):
    for _ in range(2):
        front()
        if with_match:
            match()
    fr, mt = [], []
    edges = None
    for _ in range(reps):
        t0 = time.perf_counter()
        front()
        t1 = time.perf_counter()
        if with_match:
            edges = match()
        t2 = time.perf_counter()
        fr.append((t1 - t0) * 1e3 / n_frames)
        mt.append((t2 - t1) * 1e3 / n_frames)
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    r = {"front_end_ms_per_frame": med(fr)}
    if with_match:
        r.update({"match_ms_per_frame": med(mt), "total_ms_per_frame": med([a + b for a, b in zip(fr, mt)]), "edges": edges})
    return r


res = {"a_sift_detect_batch": measure(extract_only, False),
       "b_composed_chain": measure(composed, True),
       "c_batch_nodes_host_outputs": measure(nodes_host, True),
       "d_batch_nodes_null_outputs": measure(nodes_null, True)}
fe.close()
try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    commit = ""
commit = commit or os.environ.get("BENCH_COMMIT", "")
print(json.dumps({"width": 640, "height": 480, "frames": n_frames, "reps": reps, "max_keypoints": MAX_KP, "window": WINDOW,
                  "pairs": int(len(pq)), "commit": commit or None, **res,
                  "b_over_c": round(res["b_composed_chain"]["front_end_ms_per_frame"] /
                                    res["c_batch_nodes_host_outputs"]["front_end_ms_per_frame"], 2),
                  "d_over_a": round(res["d_batch_nodes_null_outputs"]["front_end_ms_per_frame"] /
                                    res["a_sift_detect_batch"]["front_end_ms_per_frame"], 2)}))
