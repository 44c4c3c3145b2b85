#!/usr/bin/env python3
"""A synthetic sequence from frames to a trajectory through GraphManager.addNode: what one live frame costs end to end.

Every frame of synth.make_sequence (features given; --images: synth.make_image_sequence through
sensor_detect_describe_batch_nodes, features detected on the device) enters a node slot and goes through
GraphManager.addNode -- candidate selection, the pair batch, the decisions, the pose graph, the optimiser.  Then
saveTrajectory's estimate file is written and tools/evaluate_ate.py compares it with the synthetic poses (feature
sequences only: the image sequence has no camera poses); --map also assembles the clouds of the nodes with a valid
estimate (image sequences: they carry clouds) and inserts them into an OctoMap; --render FILE renders those clouds on the
device, seen through the sensor from the last pose, into a PNG or PPM (tools/render_map.py).  --save-map FILE writes that
map as a file (saveAllCloudsToFile: binary PLY when FILE ends in .ply, else binary PCD), streamed from the device without
ever holding it whole; --save-clouds BASENAME writes BASENAME_%04d.pcd / .txt per node (saveIndividualCloudsToFile).  Both act
on the nodes with a valid estimate, in graph order.

--save-session FILE writes the run's state -- resident nodes, the detector's thresholds, with --map / --render the clouds, the
pose graph and the decision machine -- when the run ends, or after K frames with --stop-after K; --resume FILE loads such a
file into fresh objects and continues with the frame behind the last one the file has seen.  The resumed run's steps, graph
and trajectory are, byte for byte, those of the run that was never stopped (the same --frames, --seed and parameters).

Prints one JSON line (--out FILE also writes it there): frames, frames dropped by status, vertices, edges, keyframes, ATE,
ms per frame in total and per stage (upload, candidates, comparisons, decisions, optimisation) as means and medians of the
step records' times.  The line is stamped with the device's name and with `git rev-parse --short HEAD` of the tree (BENCH_COMMIT
where the tree travels without its history); a tree with changes that are not committed (or BENCH_TREE_DIRTY=1) says so in
the `commit` field itself."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import evaluate_ate  # noqa: E402
from rgbdslam_v2_amd import synth  # noqa: E402
from rgbdslam_v2_amd.candidates import PoseGraph  # noqa: E402
from rgbdslam_v2_amd.frontend import FrontEnd, GraphManager, Node, parse_slam_state, read_session_chunks  # noqa: E402

STAGES = ("candidates", "comparisons", "decisions", "optimisation")


def resident_node(fe, slot):
    node = Node.__new__(Node)   # the rows are in the slot already
    node.frontend, node.id_ = fe, slot
    return node


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--n-kp", type=int, default=1000)
    ap.add_argument("--images", action="store_true", help="detect the features on the device (make_image_sequence)")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--optimizer-skip-step", type=int, default=1)
    ap.add_argument("--strategy", default="first")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--map", action="store_true")
    ap.add_argument("--render", metavar="FILE", help="with --images: the map seen from the last pose, as .png or .ppm")
    ap.add_argument("--save-map", metavar="FILE", help="with --images: the assembled map as a .pcd / .ply file")
    ap.add_argument("--save-clouds", metavar="BASENAME", help="with --images: BASENAME_%%04d.pcd and .txt per node")
    ap.add_argument("--seed", type=int, default=20260923)
    ap.add_argument("--out")
    ap.add_argument("--save-session", metavar="FILE", help="save nodes, detector state, graph and machine when the run ends")
    ap.add_argument("--stop-after", type=int, metavar="K", help="with --save-session: end the run after K frames")
    ap.add_argument("--resume", metavar="FILE", help="load a saved session and continue behind its last frame")
    a = ap.parse_args()

    fe = FrontEnd(device_id=0, max_nodes=a.frames + 1, max_keypoints=max(a.n_kp, 600), max_pairs_per_batch=64)
    gm = GraphManager(fe, PoseGraph())
    gm.set_pose_relative_to(a.strategy)
    slam = gm.slam(optimizer_skip_step=a.optimizer_skip_step, seed=a.seed & 0xFFFFFFFF)
    ns = int(round(1e9 / a.fps))
    stamps = [((k * ns) // 1000000000, (k * ns) % 1000000000) for k in range(a.frames)]
    poses = None
    upload_s = []
    start, stop = 0, a.frames if a.stop_after is None else max(0, min(a.frames, a.stop_after))
    if a.resume:   # before anything enters the context: the file's node ids must not be resident
        start = parse_slam_state(read_session_chunks(a.resume)["SLAM"])["calls"]   # one step per frame so far
        fe.load_session(a.resume, slam, gm.pose_graph)
    if a.images:
        seq = synth.make_image_sequence(n_frames=a.frames, width=a.width, height=a.height, seed=a.seed)
        if not a.resume:   # (a resumed detector has its configuration and thresholds from the file)
            fe.detector_configure(max_keypoints=600)
        t0 = time.perf_counter()
        if stop > start:
            fe.sensor_detect_describe_batch_nodes(list(seq["gray"][start:stop]), list(seq["depth"][start:stop]), seq["fx"], seq["fy"],
                                                  seq["cx"], seq["cy"], node_ids=np.arange(start, stop),
                                                  cloud_skip=8 if (a.map or a.render or a.save_map or a.save_clouds) else None)
        upload_s = [(time.perf_counter() - t0) / max(stop - start, 1)] * (stop - start)
    else:
        seq = synth.make_sequence(n_frames=a.frames, n_kp=a.n_kp, seed=a.seed)
        poses = seq["poses"]
    records, wall = [], []
    for k in range(start, stop):
        if not a.images:
            t0 = time.perf_counter()
            fe.upload_node(k, seq["desc"][k], seq["xyz1"][k])
            upload_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        records.append(gm.addNode(resident_node(fe, k), stamps[k]))
        wall.append(time.perf_counter() - t0)
    if a.save_session:
        fe.save_session(a.save_session, slam, gm.pose_graph, clouds=bool(a.images and (a.map or a.render)))

    ids = list(range(slam.node_count()))
    slots = slam.slots()
    frame_of = {i: slots[i] for i in ids}   # a frame's slot is its index; a cleared node keeps no slot, its stamp is its record's
    state = parse_slam_state(slam.serialize())
    stamp_of = dict(enumerate(state["stamps"]))   # by graph id, the frames of before a --resume included
    res = dict(tool="run_sequence", frames=a.frames, first_frame=start, frames_run=stop - start, resumed=a.resume, saved=a.save_session, images=bool(a.images), n_kp=a.n_kp, optimizer_skip_step=a.optimizer_skip_step,
               strategy=a.strategy, vertices=len(ids), keyframes=len(slam.keyframes()),
               sequential_edges=state["sequential_edges"], loop_closure_edges=state["loop_closure_edges"],
               status={}, optimisations=sum(r.optimized for r in records), stats_launches=sum(r.stats_launches for r in records))
    for r in records:
        res["status"][r.status_name] = res["status"].get(r.status_name, 0) + 1
    res["dropped"] = stop - len(ids)
    ms = lambda v: dict(mean=1e3 * statistics.fmean(v), median=1e3 * statistics.median(v), max=1e3 * max(v)) if len(v) else None
    res["ms_per_frame"] = dict(add_node=ms(wall), upload=ms(upload_s),
                               **{name: ms([r.seconds[i] for r in records]) for i, name in enumerate(STAGES)})
    res["ms_per_frame"]["total"] = ms([w + u for w, u in zip(wall, upload_s)])
    with tempfile.TemporaryDirectory() as d:
        valid = [i for i in ids if slam.valid_tf()[i] and i in stamp_of]
        t_of = lambda i: stamp_of[i][0] + 1e-9 * stamp_of[i][1]
        est = os.path.join(d, "estimate.txt")
        gm.saveTrajectory(est, valid, [t_of(i) for i in valid])
        if poses is not None:
            gt = os.path.join(d, "groundtruth.txt")
            with open(gt, "w") as f:
                for k in range(stop):
                    p = np.linalg.inv(poses[0]) @ poses[k]
                    f.write("%.6f %.6f %.6f %.6f 0 0 0 1\n" % (stamps[k][0] + 1e-9 * stamps[k][1], p[0, 3], p[1, 3], p[2, 3]))
            res["ate"] = evaluate_ate.ate(evaluate_ate.read_trajectory(gt), evaluate_ate.read_trajectory(est))
            res["path_length_m"] = float(sum(np.linalg.norm(poses[k + 1][:3, 3] - poses[k][:3, 3]) for k in range(stop - 1)))
            res["estimate_sha1"] = __import__("hashlib").sha1(open(est, "rb").read()).hexdigest()   # equal for a resumed and an uninterrupted run
    if a.map and a.images:
        valid = [i for i in ids if slam.valid_tf()[i] and frame_of[i] >= 0]
        t0 = time.perf_counter()
        T = gm.pose_graph.transforms(valid)
        cloud = fe.assemble_map([frame_of[i] for i in valid], T)
        res["map"] = dict(nodes=len(valid), points=int(len(cloud)), assemble_ms=1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        with fe.octomap(1 << 20) as om:
            om.insert_nodes([frame_of[i] for i in valid], T)
            res["map"].update(octomap_leaves=len(om), octomap_ms=1e3 * (time.perf_counter() - t0))
    if (a.save_map or a.save_clouds) and a.images:
        valid = [i for i in ids if slam.valid_tf()[i] and frame_of[i] >= 0]
        res["map_files"] = dict(nodes=len(valid))
        if a.save_map:
            t0 = time.perf_counter()
            st = fe.save_map(a.save_map, [frame_of[i] for i in valid], gm.pose_graph.transforms(valid))
            res["map_files"].update(map=st, save_map_ms=1e3 * (time.perf_counter() - t0))
        if a.save_clouds:
            t0 = time.perf_counter()
            n = fe.save_node_clouds(a.save_clouds, [frame_of[i] for i in valid], [gm.pose_graph.get_estimate(i) for i in valid],
                                    graph_ids=valid)
            res["map_files"].update(clouds_basename=a.save_clouds, clouds_written=n, save_clouds_ms=1e3 * (time.perf_counter() - t0))
    if a.render and a.images:
        import render_map
        valid = [i for i in ids if slam.valid_tf()[i] and frame_of[i] >= 0]
        T = gm.pose_graph.transforms(valid)
        view, proj = render_map.camera_for("sensor", np.asarray(T[-1], np.float64), seq["fx"], seq["fy"], seq["cx"], seq["cy"],
                                           a.width, a.height)
        t0 = time.perf_counter()
        img = fe.render_nodes([frame_of[i] for i in valid], T, width=a.width, height=a.height, view=view, projection=proj,
                              gl_point_size=8.0)  # the clouds were made at cloud_skip 8
        res["render"] = dict(file=a.render, nodes=len(valid), render_ms=1e3 * (time.perf_counter() - t0),
                             pixels_drawn=int(np.sum(img["ids"] >= 0)))
        render_map.write_image(a.render, img["rgba"])
    slam.close()
    fe.close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True,
                                    text=True).stdout.strip()) if commit else False
    except OSError:
        commit, dirty = "", False
    commit = commit or os.environ.get("BENCH_COMMIT") or None
    dirty = dirty or os.environ.get("BENCH_TREE_DIRTY", "") not in ("", "0")
    # the field says by itself what ran: the commit, or work that is not committed yet on top of it
    res["commit"] = ("uncommitted changes on top of %s" % commit) if (commit and dirty) else commit
    import torch
    res["device"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    res["note"] = ("one call of tools/run_sequence.py on one device (`device`); host clock around every call, each of which "
                   "ends synchronised; per-stage times are the step records' own")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
