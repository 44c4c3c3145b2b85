"""The map as a coloured triangle mesh: FrontEnd.display_geometry in its TRIANGLES form, with the nodes' transforms, written
as a binary little-endian PLY -- vertices x y z red green blue, one face `3 i j k` per triangle of the soup.  Host code only:
the vertices come from the library, this file packs them.

    from export_mesh import export_mesh
    export_mesh(fe, node_ids, transforms, "map.ply", squared_meshing_threshold=0.0009, maximum_depth=4.0)

Run as a script it meshes a small synthetic scene (two overlapping depth images) into --out."""
import argparse
import os
import sys

import numpy as np

VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
FACE = np.dtype([("n", "u1"), ("i", "<i4"), ("j", "<i4"), ("k", "<i4")])


def write_ply(path, vertices):
    """vertices: [3 m, 4] float32 rows (x, y, z, rgb word) of a triangle soup.  The rgb word's bytes 0, 1, 2 are b, g, r."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
    if len(v) % 3:
        raise ValueError("a triangle soup has three vertices per face")
    rec = np.zeros(len(v), VERTEX)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    bgr = v[:, 3].copy().view(np.uint8).reshape(-1, 4)
    rec["red"], rec["green"], rec["blue"] = bgr[:, 2], bgr[:, 1], bgr[:, 0]
    faces = np.zeros(len(v) // 3, FACE)
    faces["n"] = 3
    first = np.arange(0, len(v), 3, dtype=np.int32)
    faces["i"], faces["j"], faces["k"] = first, first + 1, first + 2
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (len(rec), len(faces)))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())
    return len(rec), len(faces)


def read_ply(path):
    """What write_ply wrote: (vertex records, face records)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    counts = {}
    for line in data[:end].decode("ascii").splitlines():
        if line.startswith("element "):
            _, name, n = line.split()
            counts[name] = int(n)
    nv, nf = counts["vertex"], counts["face"]
    rec = np.frombuffer(data, VERTEX, nv, end)
    faces = np.frombuffer(data, FACE, nf, end + nv * VERTEX.itemsize)
    assert end + nv * VERTEX.itemsize + nf * FACE.itemsize == len(data)
    return rec, faces


def export_mesh(fe, node_ids, transforms, path, squared_meshing_threshold=0.0009, maximum_depth=float("inf")):
    """The listed nodes' resident clouds as one world-frame mesh in `path`; returns (vertices, faces)."""
    from rgbdslam_v2_amd.frontend import DISPLAY_TRIANGLES
    g = fe.display_geometry(node_ids, transforms, display_type=DISPLAY_TRIANGLES,
                            squared_meshing_threshold=squared_meshing_threshold, maximum_depth=maximum_depth)
    tri = g["node_types"] == DISPLAY_TRIANGLES  # a cloud of one row comes as points: no surface
    keep = np.zeros(len(g["vertices"]), bool)
    for k in np.flatnonzero(tri):
        keep[g["node_offsets"][k]:g["node_offsets"][k + 1]] = True
    return write_ply(path, g["vertices"][keep])


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rgbdslam_v2_amd.frontend import FrontEnd
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="mesh.ply")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    fe = FrontEnd(device_id=0, max_nodes=4, max_keypoints=64, max_pairs_per_batch=4)
    Ts = []
    for k in range(2):
        depth = (1.5 + 0.3 * np.sin(np.arange(160) / 25.0)[None, :] + np.zeros((120, 1))).astype(np.float32)
        depth[40:80, 60:100] += 0.8  # a box further back: its rim is a depth jump
        rgb = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
        fe.upload_node_cloud(k, depth, 130.0, 130.0, 80.0, 60.0, rgb=rgb)
        T = np.eye(4, dtype=np.float32)
        T[0, 3] = 0.5 * k
        Ts.append(T)
    nv, nf = export_mesh(fe, [0, 1], Ts, a.out)
    fe.close()
    print("%s: %d vertices, %d faces" % (a.out, nv, nf))


if __name__ == "__main__":
    main()
