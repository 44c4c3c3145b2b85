"""Measurement of the tree calls of the occupancy map (rgbdfe_octomap_tree_device, rgbdfe_octomap_nodes_at_depth,
rgbdfe_octomap_write; csrc/octomap_tree.hip, csrc/api_octomap.hip).

Maps: those of tools/bench_octomap.py -- NODES (200) nodes of 640x480 depth as resident clouds with a random rigid transform
each, inserted in one call with maximum_depth 3.5 m -- for (cloud_creation_skip_step, voxelfilter_size, octomap_resolution)
in CONFIGS (--all: every combination bench_octomap.py inserts with that range).  Each map is built once; then REPS timed
runs per call, host clock around the call (every call ends in a stream synchronise), median with minimum and maximum:

  tree_device      the node records into a device buffer (one 64-byte read of the sizes, no record crosses to the host)
  nodes_at_depth   depths 16 and 12 with -inf (every node of the depth), records to the host
  write            the .ot file under /dev/shm (removed afterwards); its bytes are checked against tree() once
  d2d_copy         torch's device-to-device copy of the tree_device output: the floor any producer of these bytes has

Reported besides: leaves, nodes, nodes per depth, kernel launches of each call (they do not depend on the map), and the
bytes the kernels move by construction (the formulas are in bytes_by_construction below; gathers count once per element).
The literal pointer tree of this project (tests/octomap_tree_oracle.py) is timed on ORACLE_LEAVES leaves of the map on the
same host and scaled by leaves; its records on that sample are checked against the device byte for byte.  This is the
oracle, not the octomap library: the library is not on this machine and has not been timed.
--kernel-stats FILE: the kernel statistics CSV of a profiler run of this tool (rocprofv3 --kernel-trace --stats, a run of its
own, usually of fewer nodes); the kernels of the tree calls are copied into the record by total time (see top_kernels).

Prints one JSON line; --out FILE also writes it there."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import octomap_tree_oracle as to  # noqa: E402
from bench_map_assembly import median_time  # noqa: E402
from rgbdslam_v2_amd import synth  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd  # noqa: E402

CONFIGS = [(1, None, 0.05), (1, None, 0.1), (2, 0.02, 0.05), (2, 0.02, 0.1)]
ALL = [(s, l, r) for s in (1, 2) for l in (None, 0.02) for r in (0.05, 0.1)]


def bytes_by_construction(n, cap, cnt):
    """What the kernels of one tree call read and write, from the code: n leaves, cap slots, cnt[d] nodes of depth d."""
    gather = 2 * 12 * cap + 20 * n                # key and value per slot in the count and the write pass; code, slot, key, idx
    sort = 6 * 20 * n + 16 * n                    # per pass: keys for the histogram, pairs in and out; the re-keying
    arrange = 36 * n + 24 * n                     # idx, code (own and predecessor's), slot, value, colour; the level-16 rows
    chain = 12 * n                                # top twice, off
    leaves = 16 * n + 8 * n                       # value, colour, top, off; the record
    levels = sum(16 * cnt[d + 1] + 24 * cnt[d + 1] + 28 * cnt[d] for d in range(16))  # flags twice; the walk; parent row + record
    return {"gather": gather, "sort": sort, "arrange": arrange, "chain": chain, "leaf_records": leaves, "levels": levels,
            "total": gather + sort + arrange + chain + leaves + levels}


def top_kernels(path):
    """The kernels a tree call launches, by total time in the profiled run: tree_* (octomap_tree.hip) and the three sort
    kernels of voxel_filter.hip.  The sort kernels also run under the colour pass of the insertion that builds the map in
    the same run (3 of their calls per inserted cloud), so their line is an upper bound for the tree calls' share."""
    rows = list(csv.DictReader(open(path)))
    if not rows:
        return []
    name = [k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name")][0]
    dur = [k for k in rows[0] if "total" in k.lower() and "ns" in k.lower()][0]
    calls = [k for k in rows[0] if k.lower() in ("calls", "count")]
    rows = [r for r in rows if any(w in r[name] for w in ("tree_", "vox_hist_kernel", "vox_digit_scan_kernel", "vox_scatter_kernel"))]
    rows.sort(key=lambda r: -float(r[dur]))
    total = sum(float(r[dur]) for r in rows)
    return [{"kernel": r[name].replace("rgbdfe::(anonymous namespace)::", "").split("(")[0], "total_ns": int(float(r[dur])),
             "share_of_these": round(float(r[dur]) / total, 4), "calls": int(float(r[calls[0]])) if calls else None} for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-leaves", type=int, default=20000)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--configs", type=int, default=None, help="only the first N configurations")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_octomap_tree needs the GPU: no device, no figure")
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
    res = {"nodes": N, "frame": "640x480", "reps": a.reps, "max_range": 3.5, "configs": []}
    shm = "/dev/shm/bench_octomap_tree_%d.ot" % os.getpid()
    configs = (ALL if a.all else CONFIGS)[: a.configs]
    loaded = None
    for skip, leaf, resolution in configs:
        if loaded != (skip, leaf):
            for k in range(N):
                fe.upload_node_cloud(k, depth[k % 8], *K, rgb=rgb[k % 8], min_depth=0.1, cloud_skip=skip)
                if leaf:
                    fe.reduce_node_cloud(k, leaf)
            loaded = (skip, leaf)
        m = fe.octomap(1 << 22, resolution=resolution)
        t0 = time.perf_counter()
        m.insert_nodes(ids, Ts, 3.5)
        t_build = time.perf_counter() - t0
        cap, n = m.capacity, len(m)
        rec = m.tree()
        out = torch.zeros((len(rec), 8), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert m.tree_device(out) == len(rec) and out.cpu().numpy().tobytes() == rec.tobytes()
        t_tree = median_time(lambda: m.tree_device(out), a.reps)
        launches_tree = m.last_tree_launches
        t_d16 = median_time(lambda: m.nodes_at_depth(16), a.reps)
        launches_d16 = m.last_tree_launches
        lv12 = m.nodes_at_depth(12)
        t_d12 = median_time(lambda: m.nodes_at_depth(12), a.reps)
        launches_d12 = m.last_tree_launches
        m.write(shm)
        assert open(shm, "rb").read() == to.ot_file(rec, resolution)
        t_write = median_time(lambda: m.write(shm), a.reps)
        launches_write = m.last_tree_launches
        os.remove(shm)

        def copy():
            out.clone()
            torch.cuda.synchronize()
        t_copy = median_time(copy, a.reps)
        leaves = m.leaves()
        code = to.path_codes(leaves["key"])
        cnt = [int(len(np.unique(code >> np.uint64(3 * (16 - d))))) for d in range(17)]
        assert sum(cnt) == len(rec) and cnt[12] == len(lv12)
        # the literal tree on a sample of the leaves, checked against the device on that sample
        sample = leaves[:: max(1, n // a.oracle_leaves)][: a.oracle_leaves]
        t0 = time.perf_counter()
        lit = to.LiteralTree(sample).records()
        t_or = time.perf_counter() - t0
        with fe.octomap(len(sample) + 1, resolution=resolution) as chk:
            chk.set_leaves(sample)
            assert chk.tree().tobytes() == lit.tobytes()
        m.close()
        by = bytes_by_construction(n, cap, cnt)

        def t3(t):
            return {"s": round(t[0], 6), "s_min": round(t[1], 6), "s_max": round(t[2], 6)}
        res["configs"].append({
            "cloud_skip": skip, "voxelfilter_size": leaf, "resolution": resolution, "leaves": n, "capacity_cells": cap,
            "nodes_in_tree": len(rec), "nodes_per_depth": cnt, "insert_s_once": round(t_build, 3),
            "tree_device": dict(t3(t_tree), launches=launches_tree, host_reads=1, output_bytes=8 * len(rec)),
            "nodes_at_depth_16": dict(t3(t_d16), launches=launches_d16, host_reads=2, records=cnt[16]),
            "nodes_at_depth_12": dict(t3(t_d12), launches=launches_d12, host_reads=2, records=cnt[12]),
            "write_dev_shm": dict(t3(t_write), launches=launches_write, file_bytes=8 * len(rec)),
            "d2d_copy_of_the_output": t3(t_copy),
            "tree_device_over_d2d_copy": round(t_tree[0] / t_copy[0], 1),
            "bytes_by_construction": by,
            "tree_device_GBps_by_construction": round(by["total"] / t_tree[0] / 1e9, 1),
            "literal_tree_of_this_project": {"leaves_timed": int(len(sample)), "s_timed": round(t_or, 3),
                                             "s_scaled_to_all_leaves": round(t_or * n / max(1, len(sample)), 1),
                                             "equal_to_device_on_the_sample": True},
        })
        print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
    for k in range(N):
        fe.release_node_cloud(k)
    fe.close()
    if a.kernel_stats:
        res["tree_call_kernels_by_total_time_in_the_profiled_run"] = top_kernels(a.kernel_stats)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
