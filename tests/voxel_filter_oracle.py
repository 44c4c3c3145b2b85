"""Oracle of the voxel filter (include/rgbdfe.h, "voxel filter"; csrc/voxel_filter.hip): Node::reducePointCloud
(src/node.cpp:1448-1460), a pcl::VoxelGrid<PointXYZRGB> with a cubic leaf of `voxelfilter_size`.

Restated, not pinned: PCL is not part of the reference tree, so what stands here is this project's statement of
pcl::VoxelGrid::applyFilter (PCL 1.7) with the filter's defaults (downsample_all_data, no filter field,
min_points_per_voxel 0, an input that is not dense).  One deliberate difference: PCL orders the points of a cell with an
unstable std::sort; here a cell's members are summed in ascending input index, which makes the result reproducible.
`permuted_bound` is what that choice can cost against any other order.

Two restatements that tests/test_oracle_voxel_filter.py holds against each other:

* ``voxel_filter``          vectorised numpy, what the GPU tests compare with.  The sums are sequential: step j adds the
                            j-th member of every cell that has one (np.sum / np.add.reduce / reduceat add pairwise);
* ``voxel_filter_literal``  loop for loop, one np.float32 per operation.

Points are float32 rows (x, y, z, rgb bits).  Both return (rows [n, 4] float32, flags, info); flags bit 0 = the leaf is
too small for the cloud's extent and the input came back unchanged.  `order`, when given, replaces the order inside the
cells: a permutation of the input indices that the stable sort by cell then runs over."""
import numpy as np

LEAF_TOO_SMALL = 1
INT32_MAX = 2**31 - 1
f32 = np.float32


def leaf_ok(voxelfilter_size):
    """(L, inv) as float32, or None where the C ABI refuses the size."""
    with np.errstate(all="ignore"):
        L = f32(voxelfilter_size)
        if not L > 0:
            return None
        inv = f32(1.0) / L
    if not np.isfinite(inv) or inv == 0:
        return None
    return L, inv


def sort_passes(n_cells):
    """8-bit passes of the key sort for a grid of n_cells cells (keys 0 .. n_cells - 1)."""
    if n_cells > 2**31:
        return 4  # the int32 index has wrapped: all 32 bits
    return max(1, -(-max(int(n_cells) - 1, 1).bit_length() // 8))


def _grid(pts, valid, inv):
    """The bounding box and the grid; None when the leaf is too small."""
    xyz = pts[valid, :3]
    min_p, max_p = xyz.min(axis=0), xyz.max(axis=0)
    with np.errstate(all="ignore"):
        prod = (max_p - min_p) * inv  # float32
    if (prod >= f32(2.0**31)).any():
        return None
    d = [int(prod[a]) + 1 for a in range(3)]
    if d[0] * d[1] * d[2] > INT32_MAX:
        return None
    min_b = [int(np.floor(min_p[a] * inv)) for a in range(3)]
    max_b = [int(np.floor(max_p[a] * inv)) for a in range(3)]
    div = [max_b[a] - min_b[a] + 1 for a in range(3)]
    return dict(d=d, min_b=min_b, div=div, n_cells=div[0] * div[1] * div[2], min_p=min_p, max_p=max_p)


def _wrap32(v):
    return ((np.asarray(v, np.int64) + 2**31) % 2**32 - 2**31).astype(np.int64)


def voxel_filter(points, voxelfilter_size, order=None):
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    words = pts.view(np.uint32)
    lv = leaf_ok(voxelfilter_size)
    if lv is None:
        raise ValueError("voxelfilter_size is refused")
    _, inv = lv
    valid = np.isfinite(pts[:, :3]).all(axis=1)
    if not valid.any():
        return np.zeros((0, 4), np.float32), 0, dict(n_valid=0)
    g = _grid(pts, valid, inv)
    if g is None:
        return pts.copy(), LEAF_TOO_SMALL, dict(n_valid=int(valid.sum()))
    idx_of = np.flatnonzero(valid) if order is None else np.asarray(order)[valid[np.asarray(order)]]
    p = pts[idx_of, :3]
    min_b = np.asarray(g["min_b"], np.float32)
    ijk = (np.floor(p * inv) - min_b).astype(np.int32).astype(np.int64)
    mul1, mul2 = _wrap32(g["div"][0]), _wrap32(g["div"][0] * g["div"][1])
    key = _wrap32(ijk[:, 0] + _wrap32(ijk[:, 1] * mul1) + _wrap32(ijk[:, 2] * mul2))
    perm = np.argsort(key, kind="stable")
    key, idx_of = key[perm], idx_of[perm]
    head = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    count = np.diff(np.r_[head, len(key)])
    w = words[idx_of, 3]
    vals = np.stack([pts[idx_of, 0], pts[idx_of, 1], pts[idx_of, 2], ((w >> 16) & 255).astype(np.float32),
                     ((w >> 8) & 255).astype(np.float32), (w & 255).astype(np.float32)], axis=1)
    acc = vals[head].copy()  # a sum starts from the first member's value
    for j in range(1, int(count.max())):
        live = count > j
        acc[live] = acc[live] + vals[head[live] + j]  # one float32 addition per cell and column
    with np.errstate(all="ignore"):
        mean = acc / count.astype(np.float32)[:, None]
    out = np.zeros((len(head), 4), np.uint32)
    out[:, :3] = mean[:, :3].view(np.uint32)
    rgb = mean[:, 3:].astype(np.int32).astype(np.uint32)
    out[:, 3] = (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
    info = dict(g, n_valid=len(key), count=count, key=key[head], passes=sort_passes(g["n_cells"]))
    return out.view(np.float32), 0, info


def voxel_filter_literal(points, voxelfilter_size, order=None):
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    words = pts.view(np.uint32)
    L = f32(voxelfilter_size)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / L
    if not (L > 0 and np.isfinite(inv) and inv != 0):
        raise ValueError("voxelfilter_size is refused")
    seq = range(len(pts)) if order is None else [int(i) for i in order]
    valid = [i for i in seq if np.isfinite(pts[i, 0]) and np.isfinite(pts[i, 1]) and np.isfinite(pts[i, 2])]
    if not valid:
        return np.zeros((0, 4), np.float32), 0, dict(n_valid=0)
    min_p = [pts[valid[0], a] for a in range(3)]
    max_p = list(min_p)
    for i in valid:
        for a in range(3):
            if pts[i, a] < min_p[a]:
                min_p[a] = pts[i, a]
            if pts[i, a] > max_p[a]:
                max_p[a] = pts[i, a]
    d = []
    for a in range(3):
        with np.errstate(all="ignore"):
            prod = f32(f32(max_p[a] - min_p[a]) * inv)
        if prod >= f32(2.0**31):
            return pts.copy(), LEAF_TOO_SMALL, dict(n_valid=len(valid))
        d.append(int(prod) + 1)
    if d[0] * d[1] * d[2] > INT32_MAX:
        return pts.copy(), LEAF_TOO_SMALL, dict(n_valid=len(valid))
    min_b = [int(np.floor(f32(min_p[a] * inv))) for a in range(3)]
    max_b = [int(np.floor(f32(max_p[a] * inv))) for a in range(3)]
    div = [max_b[a] - min_b[a] + 1 for a in range(3)]
    mul = [1, int(_wrap32(div[0])), int(_wrap32(div[0] * div[1]))]
    pairs = []
    for i in valid:
        ijk = [int(f32(np.floor(f32(pts[i, a] * inv)) - f32(min_b[a]))) for a in range(3)]
        idx = int(_wrap32(ijk[0] + int(_wrap32(ijk[1] * mul[1])) + int(_wrap32(ijk[2] * mul[2]))))
        pairs.append((idx, i))
    pairs.sort(key=lambda t: t[0])  # stable: ascending index (or `order`) inside a cell
    rows, counts, keys = [], [], []
    at = 0
    while at < len(pairs):
        end = at
        while end < len(pairs) and pairs[end][0] == pairs[at][0]:
            end += 1
        n = end - at
        first = pairs[at][1]
        w = int(words[first, 3])
        s = [pts[first, 0], pts[first, 1], pts[first, 2], f32((w >> 16) & 255), f32((w >> 8) & 255), f32(w & 255)]
        for _, i in pairs[at + 1:end]:
            w = int(words[i, 3])
            m = [pts[i, 0], pts[i, 1], pts[i, 2], f32((w >> 16) & 255), f32((w >> 8) & 255), f32(w & 255)]
            s = [f32(s[c] + m[c]) for c in range(6)]
        with np.errstate(all="ignore"):
            s = [f32(v / f32(n)) for v in s]
        r, g, b = int(s[3]), int(s[4]), int(s[5])
        rows.append((s[0], s[1], s[2], (r << 16) | (g << 8) | b))
        counts.append(n)
        keys.append(pairs[at][0])
        at = end
    out = np.zeros((len(rows), 4), np.uint32)
    for k, row in enumerate(rows):
        out[k, :3] = np.array(row[:3], np.float32).view(np.uint32)
        out[k, 3] = row[3]
    info = dict(d=d, min_b=min_b, div=div, n_cells=div[0] * div[1] * div[2], n_valid=len(valid),
                count=np.asarray(counts, np.int64), key=np.asarray(keys, np.int64), passes=sort_passes(div[0] * div[1] * div[2]))
    return out.view(np.float32), 0, info


def order_inside_cells(points, voxelfilter_size, how, seed=0):
    """A permutation of the input indices that leaves every point in its cell and changes the order inside the cells:
    `how` = "reversed" or "random"."""
    n = len(np.asarray(points).reshape(-1, 4))
    if how == "reversed":
        return np.arange(n)[::-1].copy()
    return np.random.default_rng(seed).permutation(n)


def permuted_bound(points, count):
    """|x, y, z difference| allowed per cell between two orders inside the cells: 2 n 2^-24 max|coordinate|, the standard
    bound on a float sum of n terms applied to both orders."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    valid = np.isfinite(pts[:, :3]).all(axis=1)
    biggest = float(np.abs(pts[valid, :3]).max()) if valid.any() else 0.0
    return 2.0 * np.asarray(count, np.float64) * 2.0**-24 * biggest


def cloud(n, seed=0, side=3.0, centre=(0.0, 0.0, 0.0), nan_share=0.1, infs=True):
    """The random family of the tests: n points uniform in a cube of `side` metres, a share of NaN z, one +inf and one -inf
    coordinate, random rgb words with a non-zero top byte."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = (rng.uniform(-side / 2, side / 2, (n, 3)) + np.asarray(centre)).astype(np.float32)
    if nan_share:
        pts[rng.random(n) < nan_share, 2] = np.nan
    if infs and n >= 4:
        a, b = rng.choice(n, 2, replace=False)
        pts[a, rng.integers(3)] = np.inf
        pts[b, rng.integers(3)] = -np.inf
    pts.view(np.uint32)[:, 3] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32) | np.uint32(0x01000000)
    return pts
