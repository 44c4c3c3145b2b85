#!/usr/bin/env python3
"""A map rendered to an image on the device: node clouds + a trajectory -> PNG (or PPM), without a GL context.

Input: an .npz of frames (`depth` [n, h, w] float32 metres, optionally `rgb` [n, h, w, 3] uint8, and `fx`, `fy`, `cx`, `cy`)
and a trajectory in the format saveTrajectory writes (one line per node: stamp tx ty tz qx qy qz qw; line k is frame k, or
frame `index` when the .npz has `stamps` to match the line's stamp against).  The frames' clouds are built on the device
(createXYZRGBPointCloud at --cloud-skip), rendered by rgbdfe_render_nodes in the chosen form, and written with the standard
library's zlib.

--camera sensor (default): through the sensor's own intrinsics at the pose of --pose-index (default: the last line), so the
picture is directly comparable with the frame the camera delivered there.  --camera viewer: GLViewer's initial position
(50 back, half a turn about x) looking at that pose, with the reference's projection -- its field of view of 1.745 degrees
included (include/rgbdfe.h, "rendering").

write_png / write_ppm / write_image are importable (tools/run_sequence.py --render uses them)."""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = {"POINTS": 0, "TRIANGLES": 1, "TRIANGLE_STRIP": 2}


def write_png(path, rgba):
    """[h, w, 4] or [h, w, 3] uint8 as an 8-bit RGBA / RGB PNG (filter 0 on every row, one zlib stream)"""
    img = np.ascontiguousarray(rgba, np.uint8)
    h, w, ch = img.shape
    if ch not in (3, 4):
        raise ValueError("write_png takes [h, w, 3] or [h, w, 4] uint8")
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * ch)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if ch == 4 else 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_ppm(path, rgba):
    """the r, g, b of [h, w, 3 | 4] uint8 as a binary PPM (P6)"""
    img = np.ascontiguousarray(np.asarray(rgba, np.uint8)[..., :3])
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def write_image(path, rgba, opaque=True):
    """by extension: .ppm, else PNG.  opaque: alpha 255 everywhere (the cleared pixels carry clear_rgba's alpha otherwise)"""
    img = np.array(rgba, np.uint8)
    if opaque and img.shape[2] == 4:
        img[..., 3] = 255
    (write_ppm if path.lower().endswith(".ppm") else write_png)(path, img)


def pose_of(tx, ty, tz, qx, qy, qz, qw):
    n = np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
    x, y, z, w = qx / n, qy / n, qz / n, qw / n
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = (tx, ty, tz)
    return T


def read_trajectory(path):
    """[(stamp, 4 x 4 pose)] of a saveTrajectory / TUM file"""
    out = []
    with open(path) as f:
        for line in f:
            v = line.split()
            if len(v) == 8 and not line.startswith("#"):
                out.append((float(v[0]), pose_of(*[float(t) for t in v[1:]])))
    return out


def camera_for(kind, pose, fx, fy, cx, cy, width, height, z_near=0.1, z_far=1e4):
    """(view, projection) for FrontEnd.render_nodes"""
    from rgbdslam_v2_amd import frontend as F
    if kind == "sensor":
        return F.render_sensor_camera(fx, fy, cx, cy, width, height, z_near, z_far, pose)
    view = F.render_viewer_view(viewpoint=np.linalg.inv(pose))  # setViewPoint (glviewer.cpp:1122-1125)
    return view, F.render_perspective(aspect=float(np.float32(width) / np.float32(height)))


def draw_session(a):
    """The clouds of a session file at the estimates of its pose graph: loaded, not computed again."""
    import struct
    from rgbdslam_v2_amd.candidates import PoseGraph
    from rgbdslam_v2_amd.frontend import FrontEnd, parse_slam_state, read_session_chunks
    chunks = read_session_chunks(a.session)
    if "CLOU" not in chunks or "GRPH" not in chunks or "SLAM" not in chunks:
        raise SystemExit("the session holds no clouds, no graph or no slam state (save_session(..., slam, graph, clouds=True))")
    max_keypoints = struct.unpack_from("<i", chunks["CONF"], 0)[0]
    n_nodes = struct.unpack_from("<I", chunks["NODE"], 0)[0]
    state = parse_slam_state(chunks["SLAM"])
    fe = FrontEnd(device_id=0, max_nodes=n_nodes + 1, max_keypoints=max_keypoints, max_pairs_per_batch=8)
    graph = PoseGraph()
    fe.load_session(a.session, None, graph)   # the machine's chunk stays in the file: its slot table was read above
    clouds = {}
    for i, slot in enumerate(state["slots"]):
        if slot >= 0 and state["valid_tf"][i]:
            try:
                clouds[i] = fe.node_cloud_info(slot)
            except Exception:
                pass   # a node whose cloud the run released
    if not clouds:
        raise SystemExit("no node of the session has both a valid estimate and a cloud")
    ids = sorted(clouds)
    T = graph.transforms(ids)
    c = clouds[ids[a.pose_index]]
    w, h = c["cols"] * c["cloud_skip"], c["rows"] * c["cloud_skip"]
    W, H = a.width or w, a.height or h
    sx, sy = W / w, H / h
    view, proj = camera_for(a.camera, np.asarray(T[a.pose_index], np.float64), c["fx"] * sx, c["fy"] * sy, (c["cx"] + 0.5) * sx - 0.5,
                            (c["cy"] + 0.5) * sy - 0.5, W, H)
    t0 = time.perf_counter()
    out = fe.render_nodes([state["slots"][i] for i in ids], T, width=W, height=H, view=view, projection=proj, display_type=FORMS[a.form],
                          gl_point_size=a.point_size if a.point_size is not None else float(c["cloud_skip"]),
                          max_vertices_in_flight=a.max_vertices_in_flight)
    ms = 1e3 * (time.perf_counter() - t0)
    write_image(a.out, out["rgba"])
    if a.depth_out:
        np.save(a.depth_out, out["depth"])
    fe.close()
    print(json.dumps(dict(tool="render_map", session=a.session, out=a.out, nodes=len(ids), form=a.form, camera=a.camera, width=W, height=H,
                          render_ms=ms, pixels_drawn=int(np.sum(out["ids"] >= 0)))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", help=".npz: depth [n, h, w], rgb [n, h, w, 3] (optional), fx, fy, cx, cy")
    ap.add_argument("--trajectory")
    ap.add_argument("--session", metavar="FILE", help="draw a saved run (FrontEnd.save_session with clouds) instead of --frames and "
                    "--trajectory: its clouds at its graph's estimates, nothing is run again")
    ap.add_argument("--out", required=True, help=".png or .ppm")
    ap.add_argument("--form", choices=sorted(FORMS), default="POINTS")
    ap.add_argument("--camera", choices=("sensor", "viewer"), default="sensor")
    ap.add_argument("--pose-index", type=int, default=-1, help="line of the trajectory to look from")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--cloud-skip", type=int, default=2)
    ap.add_argument("--point-size", type=float, default=None, help="default: the cloud skip, so that the points close up")
    ap.add_argument("--max-vertices-in-flight", type=int, default=0)
    ap.add_argument("--depth-out", default=None, help="also the depth image, as .npy")
    a = ap.parse_args()

    from rgbdslam_v2_amd.frontend import FrontEnd
    if a.session:
        return draw_session(a)
    if not a.frames or not a.trajectory:
        ap.error("--frames and --trajectory, or --session")
    data = np.load(a.frames)
    depth = np.asarray(data["depth"], np.float32)
    rgb = np.asarray(data["rgb"], np.uint8) if "rgb" in data.files else None
    K = [float(data[k]) for k in ("fx", "fy", "cx", "cy")]
    n, h, w = depth.shape
    W, H = a.width or w, a.height or h
    traj = read_trajectory(a.trajectory)
    if "stamps" in data.files:
        stamps = np.asarray(data["stamps"], np.float64)
        frames = [int(np.argmin(np.abs(stamps - s))) for s, _ in traj]
    else:
        frames = list(range(len(traj)))
    if not traj or max(frames) >= n:
        raise SystemExit("the trajectory names %d poses, the file holds %d frames" % (len(traj), n))
    fe = FrontEnd(device_id=0, max_nodes=4, max_keypoints=64, max_pairs_per_batch=8)
    for k in sorted(set(frames)):
        fe.upload_node_cloud(k, depth[k], *K, rgb=rgb[k] if rgb is not None else None, cloud_skip=a.cloud_skip)
    Ts = np.stack([p for _, p in traj]).astype(np.float32)
    sx, sy = W / w, H / h   # a picture of another size than the frames: the same field of view
    view, proj = camera_for(a.camera, traj[a.pose_index][1], K[0] * sx, K[1] * sy, (K[2] + 0.5) * sx - 0.5, (K[3] + 0.5) * sy - 0.5, W, H)
    t0 = time.perf_counter()
    out = fe.render_nodes(frames, Ts, width=W, height=H, view=view, projection=proj, display_type=FORMS[a.form],
                          gl_point_size=a.point_size if a.point_size is not None else float(a.cloud_skip),
                          max_vertices_in_flight=a.max_vertices_in_flight)
    ms = 1e3 * (time.perf_counter() - t0)
    write_image(a.out, out["rgba"])
    if a.depth_out:
        np.save(a.depth_out, out["depth"])
    fe.close()
    print(json.dumps(dict(tool="render_map", out=a.out, nodes=len(frames), form=a.form, camera=a.camera, width=W, height=H,
                          render_ms=ms, pixels_drawn=int(np.sum(out["ids"] >= 0)))))


if __name__ == "__main__":
    main()
