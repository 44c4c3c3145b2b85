"""A plain numpy restatement of Node::featureMatching's FLANN branch with exact neighbours (node.cpp:610-667), censuses
that prove the planted inputs decide an outcome, and the input builders that tests/test_oracle_flann_reference.py and
tests/test_gpu_flann.py share (every builder is deterministic from its seed).

The branch: squared L2 distances in float32 in the order of flann::L2<float>::operator() (four differences per step,
result += ((d0*d0 + d1*d1) + d2*d2) + d3*d3), the two smallest per query with strict <, so the lowest train row wins a
tie; ratio = b1 / b2 in float32; accepted iff nn_distance_ratio > (double)ratio; a train row is used once, first come
first served in query order; DMatch.distance = the ratio.  The result record lists the accepted matches sorted by
(ratio, queryIdx), at most max_matches of them."""
import math

import numpy as np

F32 = np.float32


# ---- the reference --------------------------------------------------------------------------------------------------------
def l2sq_flann(q, t):
    """[nq, nt] float32 squared distances, accumulated four dimensions per step in flann::L2's order."""
    q = np.asarray(q, F32)
    t = np.asarray(t, F32)
    assert q.shape[1] == t.shape[1] and q.shape[1] % 4 == 0
    result = np.zeros((q.shape[0], t.shape[0]), F32)
    for k in range(0, q.shape[1], 4):
        d0, d1, d2, d3 = (q[:, None, k + i] - t[None, :, k + i] for i in range(4))
        result = result + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3)
    return result


def l2sq_left_to_right(q, t):
    """The same distances summed one dimension at a time in float32 (what flann::L2 does NOT do): census only."""
    q = np.asarray(q, F32)
    t = np.asarray(t, F32)
    result = np.zeros((q.shape[0], t.shape[0]), F32)
    for k in range(q.shape[1]):
        d = q[:, None, k] - t[None, :, k]
        result = result + d * d
    return result


def l2sq_float64(q, t):
    """The distance matrix in float64 (exact for the integer-built families, 2^-29 relative otherwise): census only."""
    q = np.asarray(q, F32).astype(np.float64)
    t = np.asarray(t, F32).astype(np.float64)
    result = np.zeros((q.shape[0], t.shape[0]), np.float64)
    for k in range(q.shape[1]):
        d = q[:, None, k] - t[None, :, k]
        result += d * d
    return result


def knn2(D):
    """(b1, b2, i1) of every row: smallest distance, second smallest with multiplicity, the lowest index of the smallest."""
    i1 = D.argmin(1)                      # the first of equal minima: strict <
    rows = np.arange(D.shape[0])
    b1 = D[rows, i1]
    rest = D.copy()
    rest[rows, i1] = np.inf
    return b1, rest.min(1), i1


def ratios(q, t):
    """(ratio float32 [nq], nearest train row [nq]); NaN where b1 = b2 = 0."""
    b1, b2, i1 = knn2(l2sq_flann(q, t))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (b1 / b2).astype(F32), i1


def passes(ratio, nn_distance_ratio):
    return np.float64(nn_distance_ratio) > ratio.astype(np.float64)   # node.cpp:648; False for NaN


def match(q, t, nn_distance_ratio):
    """(queryIdx, trainIdx, ratio) in query order."""
    q = np.asarray(q, F32)
    t = np.asarray(t, F32)
    if q.shape[0] <= 0 or t.shape[0] < 2:       # knnSearch with k = 2
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, F32)
    ratio, i1 = ratios(q, t)
    ok = passes(ratio, nn_distance_ratio)
    used = set()
    mq, mt, md = [], [], []
    for i in np.flatnonzero(ok):
        if int(i1[i]) in used:
            continue
        used.add(int(i1[i]))
        mq.append(i); mt.append(i1[i]); md.append(ratio[i])
    return np.array(mq, np.int32), np.array(mt, np.int32), np.array(md, F32)


def record_view(mq, mt, md, max_matches=300):
    """What the result record holds: the matches sorted by (ratio, queryIdx), the first max_matches of them."""
    o = np.lexsort((mq, md))[:max_matches]
    return mq[o], mt[o], md[o]


def expected_record(q, t, nn_distance_ratio, max_matches=300):
    return record_view(*match(q, t, nn_distance_ratio), max_matches)


# ---- builders -------------------------------------------------------------------------------------------------------------
def root_sift(rng, n, dim=128):
    v = rng.gamma(0.6, 1.0, (n, dim)).astype(F32)
    v /= np.abs(v).sum(1, keepdims=True)
    return np.sqrt(v).astype(F32)


def above(r):
    """The next double above r: it rounds to the float r, so a ratio test narrowed to float rejects what this accepts."""
    return math.nextafter(r, math.inf)


EXACT_RATIOS = (0.25, 0.5, 1.0)
TINY = 5e-324     # the smallest positive double: only a ratio of +0.0 passes (the entry point refuses a ratio <= 0)


def exact_ratio(seed=0, per_ratio=10):
    """Rows of small integers times a power of two: every distance and every ratio is exact in any summation order.
    Query i sits alone on coordinate i; its two nearest train rows differ from it on coordinates 40 + i and 80 + i."""
    rng = np.random.default_rng(seed)
    nq = 3 * per_ratio
    q = np.zeros((nq, 128), F32)
    t = np.zeros((2 * nq, 128), F32)
    want = np.zeros(nq, F32)
    for i in range(nq):
        s = F32(2.0) ** int(rng.integers(-2, 3))
        q[i, i] = 64
        a, b = q[i].copy(), q[i].copy()
        kind = i % 3
        sign = 1 if rng.random() < 0.5 else -1
        if kind == 0:      # 1 / 4
            a[40 + i] = sign; b[40 + i] = -2 * sign
        elif kind == 1:    # 2 / 4
            a[40 + i] = sign; a[80 + i] = -sign; b[80 + i] = 2 * sign
        else:              # 1 / 1: two equal nearest rows
            a[40 + i] = sign; b[80 + i] = -sign
        q[i] *= s; a *= s; b *= s
        t[2 * i], t[2 * i + 1] = a, b
        want[i] = EXACT_RATIOS[kind]
    qo, to = rng.permutation(nq), rng.permutation(2 * nq)
    runs = [r for e in EXACT_RATIOS for r in (e, above(e))]
    return dict(name="exact_ratio", q=q[qo], t=t[to], ratios=runs, want=want[qo])


def census_exact_ratio(fam):
    """Counts of queries per ratio; asserts that each ratio is hit >= 8 times, exactly, and that the run at the ratio and
    the run just above it differ by exactly those queries."""
    ratio, _ = ratios(fam["q"], fam["t"])
    assert np.array_equal(ratio, fam["want"])
    D64 = l2sq_float64(fam["q"], fam["t"])
    assert np.array_equal(l2sq_flann(fam["q"], fam["t"]).astype(np.float64), D64)    # exact distances
    out = {}
    for e in EXACT_RATIOS:
        hit = int((ratio == F32(e)).sum())
        n_at, n_above = len(match(fam["q"], fam["t"], e)[0]), len(match(fam["q"], fam["t"], above(e))[0])
        assert hit >= 8 and n_above - n_at == hit and F32(above(e)) == F32(e)
        out[e] = (hit, n_at, n_above)
    return out


def ties_and_nan(seed=0):
    """Exact duplicate train rows at both ends of the train set and across the 256-row boundary, queries equal to one
    train row (ratio +0.0), equal to two (0/0), and equidistant from two (ratio 1.0, the lower row wins)."""
    rng = np.random.default_rng(seed)
    nt = 520
    t = root_sift(rng, nt)
    dup = [(0, 1), (255, 256), (nt - 2, nt - 1), (7, 300)]
    for a, b in dup:
        t[b] = t[a]
    # mirrored pairs: rows c + h e_k and c - h e_k with dyadic c_k, h; a query at c is equidistant from both, exactly
    mirror = [(40, 41), (500, 30), (250, 260)]
    centres = []
    for a, b in mirror:
        c = t[a].copy()
        c[5] = 0.5
        t[a], t[b] = c, c
        t[a, 5], t[b, 5] = 0.625, 0.375
        centres.append(c)
    single = [10, 100, 254, 257, 400, nt - 3]
    q = [t[i] for i in single]                                          # ratio +0.0
    q += [t[a] for a, _ in dup] + [t[b] for _, b in dup[:2]]            # 0/0
    q += centres                                                        # ratio 1.0, mirrored rows
    noisy = [(t[a] + rng.normal(0, 0.002, 128)).astype(F32) for a, _ in dup]
    q += noisy                                                          # ratio 1.0, duplicated rows: equal sums
    k = 40
    q += list((t[rng.integers(0, nt, k)] + rng.normal(0, 0.003, (k, 128))).astype(F32))
    q = np.array(q, F32)
    o = rng.permutation(len(q))
    kind = np.array(["zero"] * len(single) + ["nan"] * (len(dup) + 2) + ["one"] * (len(centres) + len(noisy)) + ["other"] * k)
    lower = np.array(single + [a for a, _ in dup] + [a for a, _ in dup[:2]] + [min(m) for m in mirror] + [a for a, _ in dup]
                     + [-1] * k)
    return dict(name="ties_and_nan", q=q[o], t=t, ratios=[2.0, above(1.0), 1.0, 0.95, TINY], kind=kind[o], lower=lower[o])


def census_ties_and_nan(fam):
    ratio, i1 = ratios(fam["q"], fam["t"])
    kind = fam["kind"]
    zero, nan, one = kind == "zero", kind == "nan", kind == "one"
    assert np.all(ratio[zero] == 0) and not np.any(np.signbit(ratio[zero]))
    assert np.all(np.isnan(ratio[nan])) and np.all(ratio[one] == 1)
    assert np.array_equal(i1[zero | nan | one], fam["lower"][zero | nan | one])    # the lowest of the tied rows
    assert not np.any(np.isnan(ratio[kind == "other"]))
    m2, m1 = set(match(fam["q"], fam["t"], 2.0)[0].tolist()), set(match(fam["q"], fam["t"], 1.0)[0].tolist())
    idx = lambda mask: set(np.flatnonzero(mask).tolist())
    assert not (idx(nan) & m2) and not (idx(one) & m1) and len(idx(one) & m2) >= 4   # (a later 'one' may lose its row)
    assert len(match(fam["q"], fam["t"], 0.0)[0]) == 0
    assert set(match(fam["q"], fam["t"], TINY)[0].tolist()) == idx(zero) and F32(TINY) == 0
    return dict(zero=int(zero.sum()), nan=int(nan.sum()), one=int(one.sum()), one_accepted_at_2=len(idx(one) & m2))


CLAIM_ROWS = (0, 3, 6)
CLAIM_RATIO = 0.7


def claims(seed=1, reverse=False):
    """600 queries against 8 train rows: noisy copies of rows 0, 3 and 6; every 5th query is a weighted midpoint of its row
    and another, which has the row as its nearest but fails the ratio test.  Queries 0-4, 5-9 and 10-14 belong to rows 0, 3
    and 6, so each claimer (1, 6, 11) has a failing query below it; the last 260 queries are all midpoints, so in the
    reversed copy the claimers sit past the first 256-query round.  About a hundred passing queries lose each row."""
    rng = np.random.default_rng(seed)
    nt, nq = 8, 600
    t = root_sift(rng, nt)
    q = np.zeros((nq, 128), F32)
    for i in range(nq):
        r = CLAIM_ROWS[int(rng.integers(0, 3))]
        if i < 15:
            r = CLAIM_ROWS[i // 5]
        if i % 5 == 0 or i >= 340:
            other = (r + 1 + int(rng.integers(0, nt - 1))) % nt
            q[i] = F32(0.52) * t[r] + F32(0.48) * t[other]
        else:
            q[i] = t[r] + rng.normal(0, 0.004, 128).astype(F32)
    if reverse:
        q = q[::-1].copy()
    return dict(name="claims_reversed" if reverse else "claims", q=q, t=t, ratios=[CLAIM_RATIO], reverse=reverse)


def census_claims(fam):
    ratio, i1 = ratios(fam["q"], fam["t"])
    ok = passes(ratio, CLAIM_RATIO)
    mq, mt, _ = match(fam["q"], fam["t"], CLAIM_RATIO)
    assert sorted(mt.tolist()) == list(CLAIM_ROWS)
    out = {}
    for claimer, row in zip(mq.tolist(), mt.tolist()):
        nearest = np.flatnonzero(i1 == row)
        losers = np.flatnonzero(ok & (i1 == row))
        losers = losers[losers != claimer]
        assert len(losers) >= 50
        assert len(set(((losers % 256) // 64).tolist())) == 4       # all four waves of the ratio kernel's block
        assert len(set((losers // 256).tolist())) >= 2              # and more than one of its 256-query rounds
        assert nearest[0] < claimer and not ok[nearest[0]]          # a failing query sits below the claimer
        if fam["reverse"]:
            assert claimer >= 256                                   # the claimers sit past the first round
        out[row] = dict(claimer=claimer, losers=len(losers), last_loser=int(losers[-1]))
    return out


def cap(seed=0):
    """450 queries against 500 train rows, 400 of them exact copies of distinct train rows: more accepted matches than the
    record holds, and more than 300 of them with ratio +0.0, so the kept set is decided by queryIdx alone."""
    rng = np.random.default_rng(seed)
    nq, nt = 450, 500
    t = root_sift(rng, nt)
    rows = rng.permutation(nt)
    q = np.zeros((nq, 128), F32)
    q[:400] = t[rows[:400]]
    q[400:] = t[rows[400:450]] + rng.normal(0, 0.003, (50, 128)).astype(F32)
    return dict(name="cap", q=q[rng.permutation(nq)], t=t, ratios=[0.95])


def census_cap(fam, capacity=320):
    mq, mt, md = match(fam["q"], fam["t"], 0.95)
    zeros = int((md == 0).sum())
    assert len(mq) > capacity and zeros >= 300
    k300, k320 = record_view(mq, mt, md, 300)[0], record_view(mq, mt, md, 320)[0]
    assert np.array_equal(k300, np.sort(mq[md == 0])[:300])         # decided by queryIdx alone
    assert len(k320) == 320 and not np.array_equal(k320[:300], mq[:300])    # and not the first 300 in query order
    return dict(matches=len(mq), zero_ratio=zeros)


def dims(seed=0):
    """dim 4, 64, 124, 128: the slab zero-pads every row to 128 floats, which must add +0.0 terms only."""
    fams = []
    for dim in (4, 64, 124, 128):
        rng = np.random.default_rng(seed * 1000 + dim)
        nq, nt = 70, 40
        t = root_sift(rng, nt, dim)
        q = root_sift(rng, nq, dim)
        q[:30] = t[rng.integers(0, nt, 30)] + rng.normal(0, 0.01, (30, dim)).astype(F32)
        fams.append(dict(name="dim%d" % dim, q=q, t=t, ratios=[0.95, 0.6]))
    return fams


def winner_by_rounding(seed=0, nq=96):
    """Train pairs t_b = q + P(q - t_a), P a permutation of the coordinates: the two exact distances are nearly equal, and
    the float32 sum in FLANN's order picks the winner."""
    rng = np.random.default_rng(seed)
    q = root_sift(rng, nq)
    ta = (q + rng.normal(0, 0.01, (nq, 128))).astype(F32)
    tb = np.zeros_like(ta)
    for i in range(nq):
        tb[i] = q[i] + (q[i] - ta[i])[rng.permutation(128)]
    t = np.concatenate([ta, tb])[rng.permutation(2 * nq)]
    return dict(name="winner_by_rounding", q=q, t=t, ratios=[2.0, 1.0])


def census_winner_by_rounding(fam):
    """How many queries change their nearest row when the sum is taken in float64, or left to right in float32."""
    D = l2sq_flann(fam["q"], fam["t"])
    i1 = knn2(D)[2]
    i64 = knn2(l2sq_float64(fam["q"], fam["t"]))[2]
    ilr = knn2(l2sq_left_to_right(fam["q"], fam["t"]))[2]
    vs64, vslr = int((i1 != i64).sum()), int((i1 != ilr).sum())
    assert vs64 >= 8 and vslr >= 8
    return dict(differs_from_float64=vs64, differs_from_left_to_right=vslr)


def all_families():
    """Every family as (name, q, t, ratios); built once per process."""
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = [exact_ratio(), ties_and_nan(), claims(), claims(reverse=True), cap()] + dims() + [winner_by_rounding()]
    return _FAMILIES


_FAMILIES = None


# ---- the ragged batch -----------------------------------------------------------------------------------------------------
RAGGED_ROWS = (0, 1, 2, 3, 255, 256, 257, 511, 513, 768)
RAGGED_PAIRS = ((768, 768), (1, 768), (768, 1), (257, 2), (2, 257), (255, 513), (256, 256), (513, 3), (3, 3), (0, 257),
                (511, 0))


def ragged_nodes(seed=0):
    """{rows: descriptors}: every node draws noisy copies of rows of one pool, so that nodes of any two sizes match."""
    rng = np.random.default_rng(seed)
    pool = root_sift(rng, 768)
    nodes = {}
    for n in RAGGED_ROWS:
        rows = rng.permutation(768)[:n]
        nodes[n] = (pool[rows] + rng.normal(0, 0.003, (n, 128)).astype(F32)).astype(F32).reshape(n, 128)
    return nodes
