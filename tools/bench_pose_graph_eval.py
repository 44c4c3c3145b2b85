"""Measurement of the pose graph's last stage on the device (rgbdfe_pose_graph_evaluate, _prune_edges and the
pose_relative_to strategies; csrc/pose_graph.hip, csrc/api_pose_graph.hip).

Graphs: those of tools/bench_pose_graph.py (200 and 1000 nodes, 20 predecessors each, 5 % loop edges, information I * 1e4,
odometry-chain initial estimates) with 2 % of the edge count added as false loop edges: a random earlier node, a random
measurement.

Per graph, each figure the median of REPS runs on a fresh graph (with minimum and maximum), after one warm-up run:
  optimize_graph   a plain optimize_graph(0.01) with node 0 fixed by the caller: the figure to set beside the others
  evaluate         rgbdfe_pose_graph_evaluate as a whole, and per round (with the round's iterations, edges pruned,
                   launches, read-backs and upload time)
  prune            one prune call at 5.0 alone, on the graph as it is after evaluate's first two rounds
  online           under each strategy, the last FRAMES frames of an online run: the graph up to there is built without
                   optimising; then per frame the node, its edges and optimize_graph(0.01), timed together; the per-frame
                   median, with upload_seconds (the plan build and its copy) separated out

Prints one JSON line; --out FILE also writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pose_graph_oracle as po  # noqa: E402
from bench_pose_graph import make_edges  # noqa: E402

STRATEGIES = ("first", "previous", "largest_loop", "inaffected")


def with_false_edges(n, edges, fraction=0.02, seed=0):
    """The edges per frame [(i, j, Z)], a false loop edge added to int(fraction * edges) random frames."""
    rng = np.random.default_rng(seed + 1)
    frames = [[] for _ in range(n)]
    for i, j, Z in edges:
        frames[j].append((i, j, Z))
    n_false = int(round(fraction * len(edges)))
    for _ in range(n_false):
        j = int(rng.integers(30, n))
        i = int(rng.integers(0, j - 22))
        frames[j].append((i, j, po.pose(rng, 1.0, 0.6)))
    return frames, n_false


def add_frame(pg, v, edges):
    pg.add_node(v)
    for i, j, Z in edges:
        pg.add_edge_se3(i, j, Z, 1e4, set_estimate=(i == j - 1))


def build(frames, upto, strategy=None):
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg = PoseGraph()
    if strategy:
        pg.set_strategy(strategy)
    for v in range(upto):
        add_frame(pg, v, frames[v])
    if not strategy:
        pg.set_fixed(0)
    return pg


def stats(values):
    v = sorted(values)
    return {"median": 1e3 * v[len(v) // 2], "min": 1e3 * v[0], "max": 1e3 * v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--criterion", type=float, default=0.01)
    ap.add_argument("--out")
    a = ap.parse_args()
    from rgbdslam_v2_amd.frontend import FrontEnd
    fe = FrontEnd(device_id=0, max_nodes=8, max_keypoints=64, max_pairs_per_batch=8)
    record = {"tool": "bench_pose_graph_eval", "criterion": a.criterion, "reps": a.reps, "online_frames": a.frames, "unit": "ms",
              "graphs": []}
    for n in a.nodes:
        frames, n_false = with_false_edges(n, make_edges(n, seed=n), seed=n)
        n_edges = sum(len(f) for f in frames)
        print("%d nodes, %d edges (%d false)" % (n, n_edges, n_false), file=sys.stderr, flush=True)
        plain, whole, prune, rounds = [], [], [], []
        for k in range(a.reps + 1):
            pg = build(frames, n)
            t0 = time.perf_counter()
            rep = pg.optimize_graph(fe, a.criterion)
            t_plain = time.perf_counter() - t0
            pg.close()
            pg = build(frames, n, "inaffected")
            t0 = time.perf_counter()
            rd, _ = pg.evaluate(fe, a.criterion)
            t_whole = time.perf_counter() - t0
            active = int(pg.edge_errors(fe)["active"].sum())
            pg.close()
            pg = build(frames, n, "inaffected")
            pg.optimize_graph(fe, a.criterion)
            pg.set_strategy("first")
            pg.optimize_graph(fe, a.criterion)
            t0 = time.perf_counter()
            n_pruned, _ = pg.prune_edges(fe, 5.0, n_edges)
            t_prune = time.perf_counter() - t0
            pg.close()
            if k:
                plain.append(t_plain); whole.append(t_whole); prune.append(t_prune); rounds.append(rd)
            print("  run %d: plain %.1f ms (%d it), evaluate %.1f ms, pruned %s, prune alone %.2f ms (%d)"
                  % (k, 1e3 * t_plain, rep["iterations"], 1e3 * t_whole, [r["pruned"] for r in rd], 1e3 * t_prune, n_pruned),
                  file=sys.stderr, flush=True)
        entry = {"nodes": n, "edges": n_edges, "false_edges": n_false, "active_edges_after_evaluate": active,
                 "optimize_graph": dict(stats(plain), lm_iterations=rep["iterations"], launches=rep["launches"],
                                        upload_ms=1e3 * rep["upload_seconds"]),
                 "evaluate": stats(whole), "prune_alone": dict(stats(prune), pruned=n_pruned), "rounds": []}
        for r in range(5):
            last = rounds[-1][r]
            entry["rounds"].append(dict(stats([rd[r]["seconds"] for rd in rounds]), iterations=last["iterations"], pruned=last["pruned"],
                                        launches=last["launches"], readbacks=last["readbacks"],
                                        upload_ms=1e3 * sorted(rd[r]["upload_seconds"] for rd in rounds)[len(rounds) // 2],
                                        chi2=last["chi2"]))
        entry["online"] = {}
        for strategy in STRATEGIES + ("none",):
            per_frame, uploads, its = [], [], []
            for k in range(a.reps + 1):
                pg = build(frames, n - a.frames, None if strategy == "none" else strategy)
                t_frames, t_up, n_it = [], [], 0
                for v in range(n - a.frames, n):
                    t0 = time.perf_counter()
                    add_frame(pg, v, frames[v])
                    rep = pg.optimize_graph(fe, a.criterion)
                    t_frames.append(time.perf_counter() - t0)
                    t_up.append(rep["upload_seconds"])
                    n_it += rep["iterations"]
                pg.close()
                if k:
                    per_frame.append(sorted(t_frames)[len(t_frames) // 2]); uploads.append(sorted(t_up)[len(t_up) // 2]); its.append(n_it)
            entry["online"][strategy] = dict(stats(per_frame), upload_ms=1e3 * sorted(uploads)[len(uploads) // 2],
                                             lm_iterations_per_frame=its[-1] / a.frames)
            print("  online %-12s %.2f ms per frame, upload %.2f ms" % (strategy, entry["online"][strategy]["median"],
                                                                       entry["online"][strategy]["upload_ms"]), file=sys.stderr, flush=True)
        record["graphs"].append(entry)
    fe.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
