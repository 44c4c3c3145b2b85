"""A plain exact restatement of SiftGPUWrapper::match (numpy only), a census of what a pair of nodes can detect about the
second-best dot product, and the input builders that tests/test_oracle_sift_reference.py, tests/test_gpu_sift.py,
tests/test_gpu_sift_variants.py and tests/sift_variant_worker.py share (built from seeds, so that a parent process and
its worker hold identical inputs).

The reference works on the whole integer dot matrix: no tie rule enters, because a tied best is never accepted
(accept(best, best) is false).  A match is an element that is the unique maximum of both its row and its column with both
sides accepted."""
import numpy as np

CAP = 4096            # sift_gpu_wrapper.cpp:231 CreateNewSiftMatchGPU(4096): rows beyond it never enter
DISTMAX = np.float32(0.9)
RATIOMAX = np.float32(0.9)


def quantise(f):
    """SiftMatchCU.cpp:96-99: int((double)(float)(512 * f) + 0.5) stored as unsigned char."""
    prod = (np.float32(512) * np.asarray(f, np.float32)).astype(np.float32)
    return (prod.astype(np.float64) + 0.5).astype(np.int64).astype(np.uint8)


def dot_matrix(d1, d2):
    """The exact int64 dot products of the first 4096 quantised rows of each side (a float64 product of integers below
    2^24 is exact)."""
    q1 = quantise(d1)[:CAP].astype(np.float64)
    q2 = quantise(d2)[:CAP].astype(np.float64)
    return (q1 @ q2.T).astype(np.int64)


def angle(dot):
    """ProgramCU.cu:1738: float product with 2^-18, double min(., 1), double acos, cast to float."""
    prod = np.asarray(dot).astype(np.float32) * np.float32(2.0 ** -18)
    return np.arccos(np.minimum(prod.astype(np.float64), 1.0)).astype(np.float32)


def accept(best, second):
    """angle(best) < 0.9 && angle(best) < 0.9 * angle(second), in float (ProgramCU.cu:1742, :1781)."""
    a, b = angle(best), angle(second)
    return (a < DISTMAX) & (a < (b * RATIOMAX).astype(np.float32))


def _top3(D, axis):
    """(best, second, third, argbest) along `axis`, with multiplicity; missing elements count as dot 0."""
    if axis == 0:
        D = D.T
    n = D.shape[0]
    if D.shape[1] < 3:
        D = np.concatenate([D, np.zeros((n, 3 - D.shape[1]), np.int64)], 1)
    top = np.partition(D, D.shape[1] - 3, axis=1)[:, -3:]
    top.sort(axis=1)
    return top[:, 2], top[:, 1], top[:, 0], D.argmax(1)


def match(d1, d2):
    """(queryIdx, trainIdx) int32 arrays in ascending query order."""
    n1, n2 = min(len(d1), CAP), min(len(d2), CAP)
    if n1 <= 0 or n2 <= 0:           # SiftMatchCU.cpp:141
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    D = dot_matrix(d1, d2)
    rb, rs, _, rj = _top3(D, 1)
    cb, cs, _, ci = _top3(D, 0)
    row_ok = accept(rb, rs)          # implies best > second: the argmax is unique
    col_ok = accept(cb, cs)
    q = np.flatnonzero(row_ok & col_ok[rj] & (ci[rj] == np.arange(n1)))
    t = rj[q]
    # sift_gpu_wrapper.cpp:199-209: more than half of the matches touching index 0 (only possible with <= 3) -> none
    if 2 * (np.count_nonzero((q == 0) | (t == 0))) > len(q):
        q, t = q[:0], t[:0]
    return q.astype(np.int32), t.astype(np.int32)


# ---- census ---------------------------------------------------------------------------------------------------------------
def row_classes(j1, j2, n2):
    """Placement classes of a row's (best column j1, second column j2), from the dot kernels: a lane owns the columns
    j = lane mod 32, 32 columns make a column tile of one MFMA, 128 columns one LDS tile."""
    d = "lt" if j2 < j1 else "gt"
    c = []
    if j1 // 32 == j2 // 32:
        c.append("group_" + d)
    elif j1 % 32 == j2 % 32:
        c.append("lane_" + d)
    if j1 // 128 != j2 // 128:
        c.append("tile_" + d)
    if n2 % 128 and j2 >= n2 // 128 * 128:
        c.append("ragged_" + d)
    if j2 == 0:
        c.append("first")
    if j2 == n2 - 1:
        c.append("last")
    return c


def row_classes_at(n2):
    c = ["group_lt", "group_gt", "first", "last"]
    if n2 > 32:
        c += ["lane_lt", "lane_gt"]
    if n2 > 128:
        c += ["tile_lt", "tile_gt"]
    if n2 % 128:
        c += ["ragged_lt", "ragged_gt"]
    return c


def col_classes(i1, i2, n1):
    """Placement classes of a column's (best row i1, second row i2): 32 rows per MFMA row group, 64 rows per wave,
    256 rows per block of the one-pass kernel, whose per-block column partials the finish kernel merges."""
    c = []
    if i1 // 32 == i2 // 32:
        c.append("group")
    elif i1 // 64 == i2 // 64:
        c.append("wave")
    elif i1 // 256 == i2 // 256:
        c.append("block")
    else:
        c.append("blocks")
    if n1 % 256 and i2 >= n1 // 256 * 256:
        c.append("ragged")
    return c


def col_classes_at(n1):
    c = ["group"]
    if n1 > 32:
        c.append("wave")
    if n1 > 64:
        c.append("block")
    if n1 > 256:
        c.append("blocks")
    if n1 % 256:
        c.append("ragged")
    return c


def census(d1, d2, planted=None):
    """Second-critical rows and columns: the best is unique, accept(best, second) is false and accept(best, third) true --
    a matcher that loses the second accepts them.  With `planted` (planted_case's third result) also the number of
    critical planted pairs per placement class; a planted pair counts where the dot matrix puts the row's best and
    second exactly at the planted positions."""
    D = dot_matrix(d1, d2)
    n1, n2 = D.shape
    out = {}
    for name, axis in (("rows", 1), ("cols", 0)):
        b, s, t, _ = _top3(D, axis)
        out[name] = np.flatnonzero((b > s) & ~accept(b, s) & accept(b, t))
    if planted is not None:
        crit_r, crit_c = set(out["rows"].tolist()), set(out["cols"].tolist())
        rc = {c: 0 for c in row_classes_at(n2)}
        for i, j1, j2 in planted["row"]:
            order = np.argsort(-D[i], kind="stable")
            if i in crit_r and order[0] == j1 and order[1] == j2 and D[i, j2] > D[i, order[2]]:
                for c in row_classes(j1, j2, n2):
                    rc[c] += 1
        cc = {c: 0 for c in col_classes_at(n1)}
        for j, i1, i2 in planted["col"]:
            order = np.argsort(-D[:, j], kind="stable")
            if j in crit_c and order[0] == i1 and order[1] == i2 and D[i2, j] > D[order[2], j]:
                for c in col_classes(i1, i2, n1):
                    cc[c] += 1
        out["row_classes"], out["col_classes"] = rc, cc
    return out


# ---- input builders ---------------------------------------------------------------------------------------------------------
def rand_sift(rng, n):
    v = rng.gamma(0.6, 1.0, (n, 128)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = np.minimum(v, 0.2)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32)


def xyz(rng, n):
    return np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(1, 3, (n, 1)), np.ones((n, 1))], 1).astype(np.float32)


PLANTED_SIZES = ((64, 96), (129, 127), (257, 300), (700, 1023), (1024, 1024), (1100, 900), (900, 1100))
S_BEST, S_SECOND, S_NOISE = 0.955, 0.949, 0.5   # angles ~0.30 and ~0.32: ratio ~0.94 > 0.9, rejected by the second alone


def planted_case(n1, n2, seed):
    """(d1, d2, planted): integer descriptors u / 512 (exact in float, quantise back to u) over a random background, with
    min(n1, n2) // 8 each of
      row-side triples     query row b at i, train rows ~0.955 b at j1 and ~0.949 b at j2: row i is rejected by its second
                           alone, and (i, j1) would be a mutual match without it;
      column-side triples  the same with the roles swapped: train row b at j, query rows at i1 and i2;
      plain matches        query row b at i, train row ~0.955 b at j, no close second: accepted.
    planted = {"row": [(i, j1, j2)], "col": [(j, i1, i2)], "plain": [(i, j)]}.  Positions walk the placement classes
    (row_classes / col_classes) round-robin, every class that exists at the size at least twice; train rows 0 and n2 - 1
    each serve as the second of TWO query rows (a row solved to give both their 0.949 dot products)."""
    rng = np.random.default_rng(seed)
    u1 = quantise(rand_sift(rng, n1)).astype(np.float64)
    u2 = quantise(rand_sift(rng, n2)).astype(np.float64)
    m = min(n1, n2) // 8
    free_q, free_t = np.ones(n1, bool), np.ones(n2, bool)
    planted = {"row": [], "col": [], "plain": []}

    def scaled(b, s):
        return np.clip(np.rint(s * b + rng.normal(0, S_NOISE, 128)), 0, 255)

    def take(free):
        k = int(rng.choice(np.flatnonzero(free)))
        free[k] = False
        return k

    def find(free, n, classes, want, fixed2=None):
        """Free positions (p1, p2) of a best and a second whose classes include `want`, or None."""
        groups = (n + 31) // 32
        for _ in range(20000):
            p1 = int(rng.integers(n))
            kind = want.split("_")[0]
            if fixed2 is not None:
                p2 = fixed2
            elif kind == "group":
                p2 = p1 // 32 * 32 + int(rng.integers(32))
            elif kind == "wave":
                p2 = p1 // 64 * 64 + int(rng.integers(64))
            elif kind == "block":
                p2 = p1 // 256 * 256 + int(rng.integers(256))
            elif kind == "lane":
                p2 = p1 % 32 + 32 * int(rng.integers(groups))
            elif kind == "ragged":
                big = 128 if classes is row_classes else 256
                p2 = int(rng.integers(n // big * big, n))
            else:
                p2 = int(rng.integers(n))
            if p2 >= n or p1 == p2 or not free[p1] or (fixed2 is None and not free[p2]):
                continue
            if want in classes(p1, p2, n):
                free[p1] = free[p2] = False
                return p1, p2
        return None

    def shared_second(u_src, free_src, u_dst, free_dst, n_dst, classes, p2, wants):
        """Row p2 of u_dst as the second of TWO rows of u_src: t = x b + y b' with b.t = 0.949 |b|^2, b'.t = 0.949 |b'|^2."""
        srcs = [take(free_src), take(free_src)]
        b, bp = u_src[srcs[0]], u_src[srcs[1]]
        G = np.array([[b @ b, b @ bp], [b @ bp, bp @ bp]])
        x, y = np.linalg.solve(G, S_SECOND * np.array([b @ b, bp @ bp]))
        u_dst[p2] = np.clip(np.rint(x * b + y * bp), 0, 255)
        out = []
        for s, want in zip(srcs, wants):
            p1 = find(free_dst, n_dst, classes, want, fixed2=p2)[0]
            u_dst[p1] = scaled(u_src[s], S_BEST)
            out.append((s, p1, p2))
        return out

    # train rows 0 and n2 - 1 serve two query rows each; so does query row n1 - 1 where the ragged last block is too short
    # for two seconds of its own
    lane = n2 > 32
    free_t[0] = free_t[n2 - 1] = False
    short_block = 0 < n1 % 256 < 4
    short_tile = 0 < n2 % 128 < 8
    if short_tile:
        assert n2 % 128 >= 4
        free_t[n2 // 128 * 128] = False
    if short_block:
        free_q[n1 - 1] = False
    if short_tile:         # a ragged last tile too short for two disjoint (second below best) pairs: its first row serves two
        planted["row"] += shared_second(u1, free_q, u2, free_t, n2, row_classes, n2 // 128 * 128, ["ragged_lt", "ragged_lt"])
    planted["row"] += shared_second(u1, free_q, u2, free_t, n2, row_classes, 0, ["group_lt", "lane_lt" if lane else "group_lt"])
    planted["row"] += shared_second(u1, free_q, u2, free_t, n2, row_classes, n2 - 1,
                                    ["lane_gt", "tile_gt"] if short_tile else ["group_gt", "lane_gt" if lane else "group_gt"])
    n_row = len(planted["row"])
    rwant = [c for c in row_classes_at(n2) if c not in ("first", "last")]
    k = 0
    while n_row < m:       # round-robin over the classes; a class that has run out of free positions leaves the rotation
        want = rwant[k % len(rwant)]
        pos = find(free_t, n2, row_classes, want)
        if pos is None:
            rwant.remove(want)
            continue
        k += 1
        i = take(free_q)
        u2[pos[0]], u2[pos[1]] = scaled(u1[i], S_BEST), scaled(u1[i], S_SECOND)
        planted["row"].append((i,) + pos)
        n_row += 1
    cwant = col_classes_at(n1)
    n_col = 0
    if short_block:
        planted["col"] += shared_second(u2, free_t, u1, free_q, n1, col_classes, n1 - 1, ["ragged", "ragged"])
        done = [c for _, i1, i2 in planted["col"] for c in col_classes(i1, i2, n1)]
        cwant = [c for c in cwant if done.count(c) < 2]
        n_col = 2
    k = 0
    while n_col < m:
        want = cwant[k % len(cwant)]
        pos = find(free_q, n1, col_classes, want)
        if pos is None:
            cwant.remove(want)
            continue
        k += 1
        j = take(free_t)
        u1[pos[0]], u1[pos[1]] = scaled(u2[j], S_BEST), scaled(u2[j], S_SECOND)
        planted["col"].append((j,) + pos)
        n_col += 1
    for k in range(m):
        i, j = take(free_q), take(free_t)
        u2[j] = scaled(u1[i], S_BEST)
        planted["plain"].append((i, j))
    return (u1 / 512.0).astype(np.float32), (u2 / 512.0).astype(np.float32), planted


def planted_cases():
    return [("planted_%dx%d" % (n1, n2),) + planted_case(n1, n2, 1000 * n1 + n2) for n1, n2 in PLANTED_SIZES]


VS_ORACLE_SIZES = ((1000, 1000), (300, 700), (129, 127), (128, 128), (257, 33), (1, 1), (40, 1), (1, 40))


def vs_oracle_case(n1, n2):
    """test_sift_match_nodes_vs_oracle's recipe: (d1, d2, xyz1, xyz2, k planted neighbours)."""
    rng = np.random.default_rng(n1 * 31 + n2)
    d2 = rand_sift(rng, n2)
    d1 = rand_sift(rng, n1)
    k = min(n1, n2) * 2 // 3
    src = rng.permutation(n2)[:k]
    d1[:k] = d2[src] + rng.normal(0, 0.01, (k, 128)).astype(np.float32)
    d1 = np.abs(d1)
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    return d1, d2, xyz(rng, n1), xyz(rng, n2), k


def _case(rng, name, d1, d2, least=-1):
    d1, d2 = np.ascontiguousarray(d1, np.float32), np.ascontiguousarray(d2, np.float32)
    return {"name": name, "d1": d1, "d2": d2, "xyz1": xyz(rng, len(d1)), "xyz2": xyz(rng, len(d2)), "least": least}


def key_path_cases():
    """test_sift_key_paths' inputs, in its order: `least` is the number of matches a case must exceed."""
    rng = np.random.default_rng(77)
    base = rand_sift(rng, 1200)
    noisy = np.abs(base + rng.normal(0, 0.01, base.shape).astype(np.float32))
    noisy /= np.linalg.norm(noisy, axis=1, keepdims=True)
    perm = rng.permutation(1200)
    c = [_case(rng, "float_keys", noisy[perm][:1000], base[:1000], 300),
         _case(rng, "rows_1100x900", noisy[perm][:1100], base[:900], 300),     # > 1024 rows on one side: integer keys
         _case(rng, "rows_900x1100", noisy[perm][:900], base[:1100], 300),
         _case(rng, "norm_1.6", noisy[perm][:1000] * 1.6, base[:1000], 300),   # |d|^2 = 2.56 * 2^18: integer keys
         _case(rng, "norm_1.6x1.7", noisy[perm][:1000] * 1.6, base[:1000] * 1.7)]   # every angle is acos(1): no match
    # squared norms just under 2^19 (float keys at their upper limit), many exact duplicates -> equal dot products
    u = np.full((48, 128), 64, np.int32)
    u[:, 0] = 63
    for r in range(48):
        k = rng.integers(1, 128, 6)
        u[r, k] -= rng.integers(1, 20, 6)
    assert ((u * u).sum(1) < (1 << 19)).all() and ((u * u).sum(1) > (1 << 19) - 40000).all()
    f = (u / 512.0).astype(np.float32)
    d2 = f[rng.integers(0, 48, 1024)]
    d1 = f[rng.integers(0, 48, 1000)]
    c.append(_case(rng, "near_2^19_duplicates", d1, d2))
    d2n = np.abs(d2 + rng.normal(0, 2e-3, d2.shape).astype(np.float32))
    c.append(_case(rng, "near_2^19_noisy", d1, np.minimum(d2n, 0.1249)))
    # one row over the limit switches the whole node to integer keys
    d1b = d1.copy()
    d1b[500, :] = 0.126
    c.append(_case(rng, "one_row_over_2^19", d1b, d2))
    # saturated / wrapping u8 values (SiftMatchCU.cpp:96-99 stores an unsigned char): 0.6 * 512 = 307 -> 51
    d1c = rand_sift(rng, 300)
    d1c[::7, 3] = 0.6
    c.append(_case(rng, "wrapping_0.6", d1c, base[:400]))
    return c


BLOCK_SHAPE_SIZES = ((1, 1), (31, 128), (128, 33), (129, 64), (64, 129), (127, 255), (256, 256), (257, 129), (193, 385),
                     (320, 511), (513, 640), (700, 1023), (1024, 767), (1024, 1024), (65, 1000))


def block_shape_cases():
    """test_sift_block_shapes' inputs: sizes around every block / tile boundary, every fifth row an exact duplicate."""
    rng = np.random.default_rng(4242)
    base = rand_sift(rng, 1024)
    base[1::5] = base[0::5][: len(base[1::5])]          # exact duplicates
    noisy = np.abs(base + rng.normal(0, 0.01, base.shape).astype(np.float32))
    noisy /= np.linalg.norm(noisy, axis=1, keepdims=True)
    perm = rng.permutation(1024)
    return [_case(rng, "shape_%dx%d" % (n1, n2), noisy[perm][:n1], base[:n2]) for n1, n2 in BLOCK_SHAPE_SIZES]


MIXED_SIZES = (1000, 1024, 1025, 1536, 700, 300, 1, 0)


def mixed_batch_nodes():
    """Eight related nodes for one batch that mixes float-key and integer-key pairs: [(desc, xyz1)] and the key kind of
    every ordered pair by the rule of sift_fast_keys (both nodes <= 1024 rows, every quantised squared norm < 2^19)."""
    from rgbdslam_v2_amd import synth
    F = len(MIXED_SIZES)
    seq = synth.make_sequence(n_frames=F, n_kp=1536, n_world=5000, seed=2718)
    sd = synth.sift_descriptors_like(seq["desc"], seed=2718)
    nodes = [(sd[f][:n].copy(), seq["xyz1"][f][:n].copy()) for f, n in enumerate(MIXED_SIZES)]
    nodes[4] = (nodes[4][0] * np.float32(1.6), nodes[4][1])                      # the norm flag is off
    nodes[5][0][1::2] = nodes[5][0][0::2][: len(nodes[5][0][1::2])]              # exact duplicates: tie rules
    pq = np.array([q for q in range(F) for t in range(F)], np.int32)
    pt = np.array([t for q in range(F) for t in range(F)], np.int32)
    return nodes, pq, pt


def fast_key_node(desc):
    """The node flag of rgbdfe_upload_sift_node together with the row limit of sift_fast_keys."""
    u = quantise(desc).astype(np.int64)
    return len(desc) <= 1024 and bool(((u * u).sum(1) < (1 << 19)).all())


CAP_SIZES = ((4096, 4096), (4097, 5000), (5000, 1000))


def cap_nodes():
    """(noisy, base, xyz of noisy, xyz of base): 5000 related rows, noisy = a permutation of base plus noise (enough of it
    that a fifth of the rows fail the ratio test), the 3-d points permuted alike; a case takes the first n1 / n2 rows."""
    rng = np.random.default_rng(4096)
    base = rand_sift(rng, 5000)
    noisy = np.abs(base + rng.normal(0, 0.09, base.shape).astype(np.float32))
    noisy /= np.linalg.norm(noisy, axis=1, keepdims=True)
    # a permutation that keeps most partners inside the first 4096 rows of both sides
    perm = np.concatenate([rng.permutation(4096), 4096 + rng.permutation(904)])
    xb = xyz(rng, 5000)
    return noisy[perm], base, xb[perm], xb


def extreme_cases():
    """The ends of the dot value.  saturated: one all-255 query row against one all-255 train row among sparse rows
    (<= 8 non-zero bytes): dot 8 323 200, the largest an integer key holds, the angle clips to 0 and the match stands.
    zero_rows: a tenth of the rows all-zero (dot 0, the index sentinel), among them rows 0 and n - 1 and rows of the ragged
    last tile."""
    rng = np.random.default_rng(255)
    out = []

    def sparse(n):
        u = np.zeros((n, 128), np.float32)
        for r in range(n):
            u[r, rng.choice(128, 8, replace=False)] = rng.integers(1, 101, 8)   # 255 * 800 < 2^18: a second with an angle
        return u

    u1, u2 = sparse(150), sparse(200)
    u1[77] = 255
    u2[133] = 255
    assert quantise(np.float32(0.4985)) == 255
    out.append(_case(rng, "saturated", u1 / 512.0, u2 / 512.0))
    out[-1]["d1"][77] = out[-1]["d2"][133] = np.float32(0.4985)
    for n1, n2 in ((300, 333), (1100, 700)):
        base = rand_sift(rng, max(n1, n2))
        noisy = np.abs(base + rng.normal(0, 0.01, base.shape).astype(np.float32))
        noisy /= np.linalg.norm(noisy, axis=1, keepdims=True)
        d1, d2 = noisy[rng.permutation(len(base))][:n1].copy(), base[:n2].copy()
        for d in (d1, d2):
            n = len(d)
            z = set(rng.choice(n, n // 10, replace=False).tolist()) | {0, n - 1, n - 2, n // 128 * 128, n // 128 * 128 + 1}
            d[sorted(z)] = 0.0
        out.append(_case(rng, "zero_rows_%dx%d" % (n1, n2), d1, d2))
    return out


def worker_cases():
    """The fixed case list of tests/sift_variant_worker.py: the planted cases, test_sift_block_shapes' sizes with their
    duplicated rows and test_sift_key_paths' cases."""
    rng = np.random.default_rng(31337)
    return ([_case(rng, name, d1, d2) for name, d1, d2, _ in planted_cases()] + block_shape_cases() + key_path_cases())
