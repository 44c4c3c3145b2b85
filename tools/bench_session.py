#!/usr/bin/env python3
"""What a session costs: reading resident nodes back, saving and loading.

--nodes ORB nodes of --rows rows each (200 x 1000 by default), keypoints on every second one, counters allocated.  Medians
of --reps calls (7) after --warmup (2), host clock around calls that end synchronised:

  download        rgbdfe_download_nodes of all of them: one table upload, one launch of node_pack_kernel, four copies, one wait
  copy_loop       the same bytes through rgbdfe_debug_download_nodes_copy_loop: per node one device-to-host copy per array
                  straight out of the slabs (3 - 4 per node), one wait -- the baseline, in the same process: the library had
                  no read-back to compare with before
  save / load     rgbdfe_session_save / _load of the context to and from --dir (/dev/shm), without and with 64 x 48 clouds on
                  every node; load goes into a fresh context each time (its creation is not in the time)

and the launch and copy counts of each read-back.  Prints one JSON line (--out FILE also writes it there), stamped with the
device's name and `git rev-parse --short HEAD` (BENCH_COMMIT where the tree travels without its history; a tree with
uncommitted changes, or BENCH_TREE_DIRTY=1, says so in `commit`)."""
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

from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), reps=reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out")
    a = ap.parse_args()

    rng = np.random.default_rng(1)
    cfg = dict(device_id=0, max_nodes=a.nodes + 1, max_keypoints=a.rows, max_pairs_per_batch=8)
    fe = FrontEnd(**cfg)
    ids = np.arange(a.nodes, dtype=np.int32)
    desc = [rng.integers(0, 256, (a.rows, 32), np.uint8) for _ in ids]
    xyz = [rng.standard_normal((a.rows, 4)).astype(np.float32) for _ in ids]
    fe.upload_nodes(ids, desc, xyz)
    for i in ids[::2]:
        fe.upload_node_keypoints(int(i), rng.uniform(0, 640, (a.rows, 2)).astype(np.float32))
    fe.set_node_feature_stats(0, rng.integers(0, 256, a.rows, np.uint8))   # allocates the counters of every slot
    total = a.nodes * a.rows
    out = {k: np.zeros((total, w), t) for k, w, t in (("desc", 32, np.uint8), ("xyz1", 4, np.float32), ("kp_xy", 2, np.float32), ("stats", 1, np.uint8))}
    off, kinds = np.zeros(a.nodes + 1, np.int64), np.zeros(a.nodes, np.int32)

    def call(fn):
        st = fn(fe._ctx, a.nodes, ids.ctypes.data, total, out["desc"].ctypes.data, out["xyz1"].ctypes.data, out["kp_xy"].ctypes.data,
                out["stats"].ctypes.data, off.ctypes.data, kinds.ctypes.data)
        assert st == 0, st

    res = dict(tool="bench_session", nodes=a.nodes, rows=a.rows, bytes=int(total * 57))
    res["download"] = timed(lambda: call(fe._L.rgbdfe_download_nodes), a.reps, a.warmup)
    res["download"].update({k: v for k, v in fe.download_nodes_stats().items() if k in ("launches", "copies")})
    packed = {k: v.copy() for k, v in out.items()}
    res["copy_loop"] = timed(lambda: call(fe._L.rgbdfe_debug_download_nodes_copy_loop), a.reps, a.warmup)
    res["copy_loop"].update({k: v for k, v in fe.download_nodes_stats().items() if k in ("launches", "copies")})
    assert all(packed[k].tobytes() == out[k].tobytes() for k in out), "the two read-backs differ"
    res["download_speedup"] = res["copy_loop"]["median_ms"] / res["download"]["median_ms"]
    # the spread of the repetitions, for the reader who asks whether the difference is one
    res["download_clearly_faster"] = bool(res["download"]["max_ms"] < res["copy_loop"]["min_ms"])

    path = os.path.join(a.dir, "bench_session_%d.session" % os.getpid())
    depth = np.full((48, 64), 2.0, np.float32)
    try:
        for name, clouds in (("no_clouds", False), ("clouds_64x48", True)):
            if clouds:
                for i in ids:
                    fe.upload_node_cloud(int(i), depth, 60.0, 60.0, 31.5, 23.5, cloud_skip=1)
            save = timed(lambda: fe.save_session(path, clouds=clouds), a.reps, a.warmup)
            loads = []
            for _ in range(a.warmup + a.reps):
                fresh = FrontEnd(**cfg)
                t0 = time.perf_counter()
                fresh.load_session(path)
                loads.append(1e3 * (time.perf_counter() - t0))
                fresh.close()
            loads = loads[a.warmup:]
            res[name] = dict(file_bytes=os.path.getsize(path), save=save,
                             load=dict(median_ms=statistics.median(loads), min_ms=min(loads), max_ms=max(loads), reps=a.reps))
    finally:
        if os.path.exists(path):
            os.remove(path)
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
    import torch
    res["device"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    res["note"] = ("one call of tools/bench_session.py on one device (`device`); host clock around calls that end synchronised; "
                   "medians, minima and maxima of `reps` calls after warm-up")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
