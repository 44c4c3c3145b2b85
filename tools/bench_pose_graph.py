"""Measurement of pose-graph optimisation on the device (rgbdfe_pose_graph_optimize_graph; csrc/pose_graph.hip,
csrc/api_pose_graph.hip).

Graphs: what the front end's record implies -- NODES (200 and 1000) nodes on a random walk, each with an edge to each of its
20 predecessors, plus 5 % loop edges between random earlier nodes; the measurements carry the noise synth.py gives the
observations (depth sigma 0.01 z^2 at some 2 m over a few hundred inliers: about 2 mm and 1 mrad per edge), the information
is I * 1e4, the initial estimates are the odometry chain X_n = X_(n-1) * Z (addEdgeToG2O with set_estimate), node 0 fixed.

Per graph: REPS timed calls of optimize_graph at optimizer_iterations = 0.01 on a fresh copy of the graph each (host clock
around the call, which ends in the read-back of the estimates), median with minimum and maximum after one warm-up call; the
report's Levenberg-Marquardt iterations, trials, PCG iterations, kernel launches, read-backs and the share of the call spent
building and uploading the plan.  --oracle: tests/pose_graph_oracle.py on the same graph on this host beside it, its report
checked against the device's byte for byte (numpy on one thread: the oracle, not g2o; g2o is not on this machine and has not
been timed).

Prints one JSON line; --out FILE also writes it there."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_graph_oracle as po  # noqa: E402


def make_edges(n, predecessors=20, loop_fraction=0.05, seed=0):
    """(id1, id2, Z) with id1 < id2 in the order a front end would add them: per new node its predecessors, nearest first,
    then its loop edges."""
    rng = np.random.default_rng(seed)
    truth = [np.eye(4)]
    for _ in range(1, n):
        truth.append(truth[-1] @ po.pose(rng, 0.05, 0.03))
    n_loops = int(round(loop_fraction * n * predecessors))
    loops = {}
    while sum(len(v) for v in loops.values()) < n_loops:
        j = int(rng.integers(predecessors + 2, n))
        i = int(rng.integers(0, j - predecessors - 1))
        loops.setdefault(j, []).append(i)
    edges = []
    for j in range(1, n):
        for i in list(range(j - 1, max(-1, j - 1 - predecessors), -1)) + loops.get(j, []):
            edges.append((i, j, po.inv(truth[i]) @ truth[j] @ po.pose(rng, 0.002, 0.001)))
    return edges


def library_graph(n, edges):
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg = PoseGraph()
    for v in range(n):
        pg.add_node(v)
    pg.set_fixed(0)
    for i, j, Z in edges:
        pg.add_edge_se3(i, j, Z, 1e4, set_estimate=(i == j - 1))
    return pg


def oracle_graph(n, edges):
    g = po.Graph(n)
    g.fixed[0] = True
    for i, j, Z in edges:
        g.add_edge(i, j, Z, np.eye(6) * 1e4, set_estimate=(i == j - 1))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--criterion", type=float, default=0.01)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--oracle-max-nodes", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    from rgbdslam_v2_amd.frontend import FrontEnd
    fe = FrontEnd(device_id=0, max_nodes=8, max_keypoints=64, max_pairs_per_batch=8)
    record = {"tool": "bench_pose_graph", "criterion": a.criterion, "reps": a.reps, "graphs": [],
              "g2o": "not on this machine, not timed"}
    for n in a.nodes:
        edges = make_edges(n, seed=n)
        print("%d nodes, %d edges" % (n, len(edges)), file=sys.stderr, flush=True)
        times, rep = [], None
        for k in range(a.reps + 1):
            pg = library_graph(n, edges)
            t0 = time.perf_counter()
            rep = pg.optimize_graph(fe, a.criterion)
            if k:
                times.append(time.perf_counter() - t0)
            pg.close()
            print("  call %d: %d iterations, chi2 %.6g" % (k, rep["iterations"], rep["chi2"]), file=sys.stderr, flush=True)
        times.sort()
        entry = {"nodes": n, "edges": len(edges), "ms_per_optimize_graph": {"median": 1e3 * times[len(times) // 2],
                 "min": 1e3 * times[0], "max": 1e3 * times[-1]}, "lm_iterations": rep["iterations"],
                 "trials": sum(r["trials"] for r in rep["its"]), "pcg_iterations": sum(sum(r["pcg"]) for r in rep["its"]),
                 "launches": rep["launches"], "readbacks": rep["readbacks"], "chi2": rep["chi2"],
                 "upload_share": rep["upload_seconds"] / rep["total_seconds"], "upload_ms": 1e3 * rep["upload_seconds"]}
        if a.oracle and n <= a.oracle_max_nodes:
            g = oracle_graph(n, edges)
            want = po.new_report()
            t0 = time.perf_counter()
            po.optimize_graph(g, a.criterion, want)
            entry["oracle_ms"] = 1e3 * (time.perf_counter() - t0)
            entry["oracle_agrees_bytewise"] = bool(
                want["iterations"] == rep["iterations"] and struct.pack("<d", float(want["chi2"])) == struct.pack("<d", rep["chi2"])
                and [r["pcg"] for r in want["its"]] == [r["pcg"] for r in rep["its"]])
        record["graphs"].append(entry)
    fe.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
