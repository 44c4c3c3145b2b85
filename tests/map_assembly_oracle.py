"""Oracle of map assembly (include/rgbdfe.h, "map assembly"; csrc/map_assembly.hip): transformAndAppendPointCloud
(src/misc.cpp:183-238, the non-HEMACLOUDS form) applied to a list of node clouds as GraphManager::saveAllCloudsToFile
(src/graph_mgr_io.cpp:529-552) applies it.

Two restatements that tests/test_oracle_map_assembly.py holds against each other:

* ``assemble``          vectorised numpy, what the GPU tests compare with;
* ``assemble_literal``  the reference loop statement by statement: the `+=` append of the untransformed cloud, the running
                        output index `j`, the writes through `p_out`, the final `resize` -- one float32 rounding per operation.

This function is pinned by transcription, not on the reference's compiled code: besides first-party statements it consists
of PCL's `+=` (a vector append) and squaredEuclideanDistance (dx*dx + dy*dy + dz*dz in float), Eigen's 3x3 product
(((r0*x + r1*y) + r2*z) + t per row) and the tf -> Matrix4f conversion, which stays with the caller.

Clouds are float32 arrays of 4 columns (x, y, z, rgb bits), any leading shape; transforms are 4 x 4 matrices in the usual
row-major numpy sense (the Matrix4f); the rgb column is only ever moved as a 32-bit word."""
import numpy as np

QNAN_BITS = np.uint32(0x7FC00000)  # std::numeric_limits<float>::quiet_NaN()


def _points(cloud):
    pts = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    return pts, pts.view(np.uint32)


def assemble(clouds, transforms, maximum_depth=np.inf, preserve_raster=False):
    """Returns (points [n, 4] float32, node_offsets [len(clouds) + 1] int64)."""
    md = np.float32(maximum_depth)  # `float max_Depth`
    parts, offsets = [], [0]
    with np.errstate(all="ignore"):
        clip_on = bool(md >= np.float32(0))
        md2 = md * md
        for cloud, T in zip(clouds, transforms):
            pts, words = _points(cloud)
            T = np.asarray(T, np.float32).reshape(4, 4)
            x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
            sq = (x * x + y * y) + z * z
            clipped = (sq > md2) if clip_on else np.zeros(len(pts), bool)
            skipped = ~clipped & (np.isnan(x) | np.isnan(y) | np.isnan(z))
            moved = ~clipped & ~skipped
            out = words.copy()
            for r in range(3):
                v = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
                out[moved, r] = v.astype(np.float32).view(np.uint32)[moved]
            out[clipped, :3] = QNAN_BITS
            if not preserve_raster:
                out = out[moved]
            parts.append(out)
            offsets.append(offsets[-1] + len(out))
    allp = np.concatenate(parts) if parts else np.zeros((0, 4), np.uint32)
    return np.ascontiguousarray(allp).view(np.float32).reshape(-1, 4), np.asarray(offsets, np.int64)


def assemble_literal(clouds, transforms, maximum_depth=np.inf, preserve_raster=False):
    """misc.cpp:183-238 statement by statement, called per node as graph_mgr_io.cpp:529-552 does."""
    f32 = np.float32
    qnan = QNAN_BITS.view(np.float32)
    cloud_to_append_to = []  # .points: [x, y, z, rgb word]
    offsets = [0]
    max_Depth = f32(maximum_depth)
    compact = not preserve_raster  # :187
    with np.errstate(all="ignore"):
        for cloud, T in zip(clouds, transforms):
            pts, words = _points(cloud)
            eigen_transform = np.asarray(T, np.float32).reshape(4, 4)
            original_size = len(cloud_to_append_to)  # :190
            cloud_to_append_to += [[pts[i, 0], pts[i, 1], pts[i, 2], words[i, 3]] for i in range(len(pts))]  # :202
            rot, trans = eigen_transform[:3, :3], eigen_transform[:3, 3]  # :204-205
            j = 0  # :210
            for i in range(len(pts)):
                p_in = (pts[i, 0], pts[i, 1], pts[i, 2])
                if compact:  # :215
                    cloud_to_append_to[j + original_size] = [pts[i, 0], pts[i, 1], pts[i, 2], words[i, 3]]
                p_out = cloud_to_append_to[j + original_size]  # :214 (a view of the element's x, y, z)
                if max_Depth >= f32(0):  # :217
                    dx, dy, dz = f32(0) - p_in[0], f32(0) - p_in[1], f32(0) - p_in[2]  # squaredEuclideanDistance(p, origin)
                    if f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz)) > f32(max_Depth * max_Depth):  # :218
                        p_out[0] = p_out[1] = p_out[2] = qnan  # :219-221
                        if not compact:
                            j += 1  # :222
                        continue
                if np.isnan(p_in[0]) or np.isnan(p_in[1]) or np.isnan(p_in[2]):  # :226
                    if not compact:
                        j += 1  # :227
                    continue
                for r in range(3):  # :230, p_out = rot * p_in + trans
                    p_out[r] = f32(f32(f32(f32(rot[r, 0] * p_in[0]) + f32(rot[r, 1] * p_in[1])) + f32(rot[r, 2] * p_in[2])) + trans[r])
                j += 1  # :231
            if compact:
                del cloud_to_append_to[j + original_size:]  # :234
            offsets.append(len(cloud_to_append_to))
    out = np.zeros((len(cloud_to_append_to), 4), np.uint32)
    for k, p in enumerate(cloud_to_append_to):
        out[k, :3] = np.array(p[:3], np.float32).view(np.uint32)
        out[k, 3] = p[3]
    return out.view(np.float32), np.asarray(offsets, np.int64)


def mismatch(got, want):
    """The comparison rule: None when the two assembled clouds are equal -- NaN coordinates in the same places, every other
    coordinate and every rgb word bit for bit -- else a description of the first difference."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    gw, ww = got.view(np.uint32), want.view(np.uint32)
    gn, wn = np.isnan(got[:, :3]), np.isnan(want[:, :3])
    bad = (gn != wn) | (~gn & (gw[:, :3] != ww[:, :3]))
    bad = np.concatenate([bad, (gw[:, 3:] != ww[:, 3:])], axis=1)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        return "row %d column %d: %08x != %08x (%d differences)" % (r, c, gw[r, c], ww[r, c], int(bad.sum()))
    return None


def clipped_rows(clouds, maximum_depth):
    """Rows of the raster-mode output that the range clip hits (they must be exactly QNAN_BITS)."""
    md = np.float32(maximum_depth)
    rows = []
    with np.errstate(all="ignore"):
        for cloud in clouds:
            pts, _ = _points(cloud)
            sq = (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]
            rows.append((sq > md * md) if md >= np.float32(0) else np.zeros(len(pts), bool))
    return np.concatenate(rows) if rows else np.zeros(0, bool)
