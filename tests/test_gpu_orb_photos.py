"""-m gpu: the ORB front end on photographs against oracle/orb_oracle.c -- the ten pictures of SiftGPU's test data
(640x480, 800x600, and 2048x1536 mirrored from the central quarter of the largest picture; see
tests/test_oracle_orb_photos.py) and three photometric variants of each (dark,
saturating gain, inverted).  Same rules as test_gpu_orb.py: positions, octaves, sizes, FAST/NMS decisions and descriptor
bytes exact, Harris responses and angles bit-equal.  Natural texture brings what the synthetic images of test_gpu_orb.py do
not: FAST-score ties, 255 plateaus next to detail, JPEG 8x8 blocking, very uneven corner density across the grid cells, and
cv::ORB's per-level retainBest cut through runs of equal scores (most photographs reach its 10000-keypoint cap at low
thresholds).  The oracle runs in a thread pool next to the GPU calls."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle as po
from oracle import pyorb
from test_oracle_orb_photos import load_photos, variant

pytestmark = pytest.mark.gpu

KINDS = ("orig", "dark", "sat", "inv")
CAPACITY = 16384                     # cv::ORB(10000)'s per-level caps sum to 10000: room for threshold 5 at 2048x1536
_POOL = ThreadPoolExecutor(max_workers=min(16, po.usable_cpus()))
_CACHE = {}


def _oracle(key, fn, *args):
    """A future of fn(*args), computed once per module run."""
    if key not in _CACHE:
        pyorb.lib()
        _CACHE[key] = _POOL.submit(fn, *args)
    return _CACHE[key]


@pytest.fixture(scope="module")
def photos():
    P = load_photos()
    big = P["1600"]
    P["1600_c1280"] = np.ascontiguousarray(big[288:1248, 384:1664])     # 1280x960, the BASELINE size (across both mirror seams)
    P["1600_c1283"] = np.ascontiguousarray(big[57:1014, 411:1694])      # 1283x957: odd, off every tile and level seam
    return P


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=48, max_keypoints=4096, max_pairs_per_batch=512)
    yield f
    f.close()


def assert_kps_equal(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "octave", "size"):
        assert np.array_equal(a[f], b[f]), f
    assert np.allclose(a["response"], b["response"], rtol=1e-6, atol=0)
    assert np.allclose(a["angle"], b["angle"], rtol=1e-6, atol=0)
    assert np.array_equal(a["response"], b["response"]) and np.array_equal(a["angle"], b["angle"])


def binary_mask(shape, seed):
    """20 % of a grid of 37 x 29 blocks off (edges on none of the kernels' tile seams) and a band without depth on the left."""
    h, w = shape
    rng = np.random.default_rng(seed)
    off = np.repeat(np.repeat(rng.random((h // 29 + 1, w // 37 + 1)) < 0.2, 29, 0), 37, 1)[:h, :w]
    m = np.where(off, 0, 255).astype(np.uint8)
    m[:, : w // 10] = 0
    return m


def depth_mask(shape, seed):
    """A mask of depth values (the reference's depth * 100 as mono8): 50 .. 254 over most of the frame, 255 where the depth
    saturates (the bottom third), 0 in the binary mask's holes.  cv::ORB's threshold(254) wipes the pyramid levels >= 1
    everywhere but in the saturated part."""
    h, w = shape
    ramp = np.linspace(50, 350, h)[:, None] * np.ones((1, w))
    m = np.clip(ramp, 0, 255).astype(np.uint8)
    m[binary_mask(shape, seed) == 0] = 0
    return m


def plane_depth(shape, z, seed, noise=0.001):
    """A fronto-parallel plane at depth z with seeded sensor noise sigma = noise * z^2 (f32, metres)."""
    rng = np.random.default_rng(seed)
    return (z + rng.normal(0.0, noise * z * z, shape)).astype(np.float32)


def intrinsics(shape):
    h, w = shape
    return 525.0 * w / 640, 525.0 * w / 640, (w - 1) / 2.0, (h - 1) / 2.0


def frame_image(photos, name, kind):
    if name == "flat":
        g = np.full((480, 640), 128, np.uint8)
        g[200:280, 300:340] = 140
        return g
    return variant(photos[name], kind)


# ---- 3a / 3b: orb_detect against pyorb.detect ----------------------------------------------------------------------------
IMAGES = ["640_1", "640_2", "640_3", "640_4", "640_5", "800_1", "800_2", "800_3", "800_4", "1600", "1600_c1280", "1600_c1283"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", IMAGES)
def test_orb_detect_photo_matches_oracle(fe, photos, name, kind):
    """cv::ORB::detect at FAST thresholds 5, 20, 60 without a mask, with a binary mask and with a depth-valued mask.  A dark
    frame has no corner at 60 (its contrast is 0.3 of the original's): it also runs at 18."""
    g = variant(photos[name], kind)
    masks = {"none": None, "binary": binary_mask(g.shape, 3), "depth": depth_mask(g.shape, 3)}
    thrs = (5, 18, 20, 60) if kind == "dark" else (5, 20, 60)
    refs = {(t, mk): _POOL.submit(pyorb.detect, g, m, t, CAPACITY) for t in thrs for mk, m in masks.items()}
    for (t, mk), fut in refs.items():
        kp = fe.orb_detect(g, masks[mk], t, capacity=CAPACITY)
        ref = fut.result()
        assert_kps_equal(kp, ref)
        if kind == "dark" and t == 60:
            assert len(kp) < 10                           # (640-2 keeps one corner)
        else:
            assert len(kp) > 50, (t, mk, len(kp))
        if mk != "none" and len(kp):
            l0 = kp[kp["octave"] == 0]
            assert len(l0) and np.all(masks[mk][l0["y"].astype(int), l0["x"].astype(int)] > 0)
        if mk == "depth" and len(kp):                      # levels >= 1: only the saturated bottom third survives
            assert np.all(kp["y"][kp["octave"] > 0] >= g.shape[0] * 0.6), (t, len(kp))


def test_orb_detect_capacity_overflow_leaves_the_context_usable(fe, photos):
    """More keypoints than the output rows: RGBDFE_ERR_CAPACITY, nothing written; the next calls -- another size, then
    the same image -- still equal the oracle."""
    from rgbdslam_v2_amd.frontend import RgbdfeError
    big, small = photos["1600"], photos["640_3"]
    ref_small = _POOL.submit(pyorb.detect, small, None, 20, CAPACITY)
    ref_big = _POOL.submit(pyorb.detect, big, None, 5, CAPACITY)
    for g, t in ((big, 5), (small, 20)):
        with pytest.raises(RgbdfeError, match="capacity"):
            fe.orb_detect(g, None, t, capacity=500)
    assert_kps_equal(fe.orb_detect(small, None, 20, capacity=CAPACITY), ref_small.result())
    kp = fe.orb_detect(big, None, 5, capacity=CAPACITY)
    ref = ref_big.result()
    assert_kps_equal(kp, ref)
    assert len(kp) >= 10000                              # (retainBest keeps the ties at its cut: a few more than 10000)
    assert_kps_equal(fe.orb_detect(big, None, 5, capacity=len(ref)), ref)                 # exactly enough rows
    with pytest.raises(RgbdfeError, match="capacity"):
        fe.orb_detect(big, None, 5, capacity=len(ref) - 1)                                # one row short
    assert_kps_equal(fe.orb_detect(big, None, 5, capacity=CAPACITY), ref)


# ---- 3c: orb_compute against pyorb.compute --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["640_1", "640_3", "640_5", "800_2", "800_4", "1600"])
def test_orb_compute_photo_matches_oracle(fe, photos, name, kind):
    """The photograph's own keypoints at threshold 20, shuffled across levels, plus some moved to straddle the 31 px border
    (fractional positions): the same keypoints survive, regrouped by level, with the same descriptor bytes."""
    g = variant(photos[name], kind)
    kp = pyorb.detect(g, None, 20, CAPACITY)
    assert len(kp) > 500
    rng = np.random.default_rng(7)
    sel = kp[rng.permutation(len(kp))].copy()
    edge = sel[:200].copy()
    h, w = g.shape
    edge["x"][:100] = rng.uniform(20, 45, 100).astype(np.float32)
    edge["y"][100:] = (h - 1 - rng.uniform(20, 45, 100)).astype(np.float32)
    sel = np.concatenate([sel, edge])[rng.permutation(len(sel) + 200)]
    k1, d1 = fe.orb_compute(g, sel)
    k2, d2 = pyorb.compute(g, sel)
    assert_kps_equal(k1, k2)
    assert np.array_equal(d1, d2)
    assert np.all(np.diff(k1["octave"]) >= 0)
    assert 100 < len(sel) - len(k1) < len(sel) // 2          # the border drop ran, on the moved keypoints and others
    assert 60 < np.unpackbits(d1, axis=1).sum(1).mean() < 196


# ---- 3d: the grid-adaptive detector over photograph sequences ------------------------------------------------------------
# A sparse frame (dark, flat) comes directly before the densest photograph (640-3): the speculative read-back of the dense
# frame's first pass is sized from the sparse frame's last pass, and the rest of its corners take the second trip.
SEQ_640 = [("640_1", "orig"), ("640_2", "orig"), ("640_4", "sat"), ("640_5", "inv"), ("640_1", "dark"), ("640_3", "orig"),
           ("640_4", "orig"), ("flat", ""), ("640_3", "inv"), ("640_2", "dark"), ("640_5", "orig"), ("640_3", "sat")]
SEQ_800 = [("800_1", "orig"), ("800_2", "inv"), ("800_4", "dark"), ("800_3", "orig"), ("800_4", "sat"), ("800_2", "orig"),
           ("800_1", "dark"), ("800_3", "inv"), ("800_1", "sat"), ("800_4", "orig"), ("800_2", "dark"), ("800_3", "sat"),
           ("800_1", "inv"), ("800_4", "inv"), ("800_2", "sat"), ("800_3", "dark")]
SEQ_1600 = [("1600", "orig"), ("1600", "dark"), ("1600", "inv"), ("1600", "sat")]


def _frames(photos, seq):
    grays = [frame_image(photos, n, k) for n, k in seq]
    shape = grays[0].shape
    masks = [binary_mask(shape, f) if f % 3 != 2 else np.full(shape, 255, np.uint8) for f in range(len(seq))]
    depths = [plane_depth(shape, 2.0 + 0.1 * (f % 4), f) for f in range(len(seq))]
    return grays, masks, depths, intrinsics(shape)


def _oracle_run(grays, masks, depths, K, budget, grid):
    """Node::Node's feature path frame by frame: [(keypoints, descriptors, xyz1, thresholds after the frame)]."""
    st = pyorb.grid_state(budget, grid)
    out = []
    for g, m, d in zip(grays, masks, depths):
        rk, rdesc = pyorb.node_features(st, g, m, d, budget)
        kept, rxyz = po.project_to_3d(np.stack([rk["x"], rk["y"]], 1), d, *K, 1.0, budget)
        assert len(kept) == len(rk)
        out.append((rk, rdesc, rxyz, np.array(st.thresh[: grid * grid])))
    return out


def _oracle_seq(photos, seq_name, seq, budget, grid):
    grays, masks, depths, K = _frames(photos, seq)
    return _oracle(("seq", seq_name, budget, grid), _oracle_run, grays, masks, depths, K, budget, grid)


class _Env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check_frames(res, ref):
    assert len(res) == len(ref)
    for f, ((kp, desc, xyz), (rk, rdesc, rxyz, _)) in enumerate(zip(res, ref)):
        assert_kps_equal(kp, rk)
        assert np.array_equal(desc, rdesc), f
        assert np.array_equal(xyz, rxyz), f


GRID_CASES = [(b, g) for b in (600, 1000, 1500, 4000) for g in (2, 3, 6)]


@pytest.mark.parametrize("budget,grid", GRID_CASES)
def test_detect_describe_photo_sequence_matches_oracle(fe, photos, budget, grid):
    """detect -> removeDepthless -> retainBest -> compute -> projectTo3D over SEQ_640: after every frame the keypoints,
    descriptors, points and per-cell thresholds equal the oracle's.  The same run through detect_describe_batch with the
    measure kernel's own read-back and with the copy behind it (RGBDFE_DETECT_HOSTWRITE=0) gives the same frames and leaves
    the same thresholds."""
    for b, g in GRID_CASES:                              # the oracle of every case starts now, in the pool
        _oracle_seq(photos, "640", SEQ_640, b, g)
    ref = _oracle_seq(photos, "640", SEQ_640, budget, grid).result()
    grays, masks, depths, K = _frames(photos, SEQ_640)
    fe.detector_configure(max_keypoints=budget, grid_resolution=grid)
    for f, (g, m, d) in enumerate(zip(grays, masks, depths)):
        kp, desc, xyz = fe.detect_describe(g, m if f != 8 else None, d, *K)     # frame 8 without a mask: all valid
        rk, rdesc, rxyz, rthr = ref[f]
        assert_kps_equal(kp, rk)
        assert np.array_equal(desc, rdesc) and np.array_equal(xyz, rxyz), f
        assert np.array_equal(fe.detector_thresholds(), rthr), f
        assert len(kp) <= budget
        if SEQ_640[f][0] != "flat":
            assert len(kp) > min(budget // 3, 300), (f, len(kp))
    assert min(r[3].min() for r in ref) < 4              # the x0.7 re-detection drove thresholds from 20 down near the floor (2)
    for hw in ("1", "0"):
        with _Env(RGBDFE_DETECT_HOSTWRITE=hw):
            fe.detector_configure(max_keypoints=budget, grid_resolution=grid)
            res = fe.detect_describe_batch(grays, masks, depths, *K)
            _check_frames(res, ref)
            assert np.array_equal(fe.detector_thresholds(), ref[-1][3]), hw


@pytest.mark.parametrize("grid", [3, 6])
def test_detect_describe_largest_photograph_sequence(fe, photos, grid):
    """The 2048x1536 image and its variants at configs[4]'s budget of 4000."""
    ref = _oracle_seq(photos, "1600", SEQ_1600, 4000, grid).result()
    grays, masks, depths, K = _frames(photos, SEQ_1600)
    fe.detector_configure(max_keypoints=4000, grid_resolution=grid)
    for f, (g, m, d) in enumerate(zip(grays, masks, depths)):
        kp, desc, xyz = fe.detect_describe(g, m, d, *K)
        rk, rdesc, rxyz, rthr = ref[f]
        assert_kps_equal(kp, rk)
        assert np.array_equal(desc, rdesc) and np.array_equal(xyz, rxyz), f
        assert np.array_equal(fe.detector_thresholds(), rthr), f
        assert 1500 < len(kp) <= 4000
    for hw in ("1", "0"):
        with _Env(RGBDFE_DETECT_HOSTWRITE=hw):
            fe.detector_configure(max_keypoints=4000, grid_resolution=grid)
            _check_frames(fe.detect_describe_batch(grays, masks, depths, *K), ref)
            assert np.array_equal(fe.detector_thresholds(), ref[-1][3])


# ---- 3e: detect_describe_batch on photographs ----------------------------------------------------------------------------
@pytest.mark.parametrize("seq_name", ["640", "800"])
def test_detect_describe_batch_photos_equals_single_calls_and_oracle(photos, seq_name):
    """More frames than one super-frame (7 at grid 3) with a ragged tail: 19 frames at 640x480, 16 at 800x600.  Every frame
    equals its single call and the oracle; the thresholds left behind are those of single calls; copy=False too."""
    from rgbdslam_v2_amd.frontend import FrontEnd
    seq = SEQ_640 + SEQ_640[:7] if seq_name == "640" else SEQ_800
    ref = _oracle_seq(photos, seq_name + "_batch", seq, 1000, 3).result()
    grays, masks, depths, K = _frames(photos, seq)
    masks[11] = None                                        # (the oracle's mask of frame 11 is all 255)
    outs = []
    for mode in ("single", "batch", "views"):
        f = FrontEnd(device_id=0, max_nodes=2, max_keypoints=1024, max_pairs_per_batch=8)
        f.detector_configure(max_keypoints=1000)
        if mode == "single":
            res = [f.detect_describe(g, m, d, *K) for g, m, d in zip(grays, masks, depths)]
        else:
            res = f.detect_describe_batch(grays, masks, depths, *K, copy=(mode == "batch"))
            res = [tuple(a.copy() for a in r) for r in res]
        outs.append((res, f.detector_thresholds().copy()))
        f.close()
    for res, thr in outs:
        _check_frames(res, ref)
        assert np.array_equal(thr, outs[0][1]) and np.array_equal(thr, ref[-1][3])
    assert sum(len(r[0]) for r in outs[0][0]) > 400 * len(seq)


# ---- 3f: the pair path on photograph features ----------------------------------------------------------------------------
def check_against_oracle(rec, ref):
    from rgbdslam_v2_amd.frontend import inlier_indices
    n = ref["n_all"]
    assert rec["n_all"] == n
    assert np.array_equal(rec["all_q"][:n], ref["all_q"])
    assert np.array_equal(rec["all_t"][:n], ref["all_t"])
    assert np.array_equal(rec["all_hd"][:n], ref["all_hd"])
    assert (rec["id1"], rec["id2"]) == (ref["id1"], ref["id2"])
    assert rec["real_iterations"] == ref["real_iterations"]
    assert rec["valid_iterations"] == ref["valid_iterations"]
    assert rec["n_inl"] == ref["n_inl"]
    assert np.array_equal(inlier_indices(rec), ref["inl_idx"])
    T = np.array(rec["trafo"], np.float32).reshape(4, 4).T
    assert np.array_equal(T, ref["T"]), "pose bits differ from the oracle"
    assert np.float32(rec["rmse"]) == ref["rmse"]
    assert rec["info_scale"] == ref["info_scale"]


@pytest.mark.parametrize("size", ["640", "800"])
def test_match_pair_list_on_photo_features(fe, photos, size):
    """The photographs and their variants of one size class, detected and described with a plane depth, become nodes; all
    ordered pairs run through match + RANSAC on the one-wave kernel (set_latency_mode(0, 0)) and on the default record /
    replay plan, against the oracle.  Real descriptors bring many equal Hamming distances and repeated structure: the
    first-minimum tie rule and the match order RANSAC sees.  A variant of the same photograph registers with it."""
    names = [n for n in ("640_1", "640_2", "640_3", "640_4", "640_5", "800_1", "800_2", "800_3", "800_4") if n[:3] == size]
    seq = [(n, k) for n in names for k in KINDS]
    grays, masks, depths, K = _frames(photos, seq)
    base = 0 if size == "640" else 100
    fe.detector_configure(max_keypoints=1000)
    descs, xyzs = [], []
    for f, (g, d) in enumerate(zip(grays, depths)):
        kp, desc, xyz = fe.detect_describe(g, None, d, *K)
        assert len(kp) > 300
        fe.upload_node(base + f, desc, xyz)
        descs.append(desc)
        xyzs.append(xyz)
    n = len(seq)
    qi = np.array([q for q in range(n) for t in range(n) if q != t], np.int32)
    ti = np.array([t for q in range(n) for t in range(n) if q != t], np.int32)
    prm = po.default_params(seed=fe.params.seed, depth_cov=fe.params.depth_cov)
    refs = [po.result_to_dict(r) for r in po.match_pairs_mt(descs, xyzs, base + np.arange(n), qi, ti, prm)]
    try:
        for mode in ((0, 0), ()):
            fe.set_latency_mode(*mode)
            out = fe.match_pair_list(base + qi, base + ti)
            for rec, ref in zip(out, refs):
                check_against_oracle(rec, ref)
    finally:
        fe.set_latency_mode()
        for f in range(n):
            fe.release_node(base + f)
    reached = sum(r["n_all"] > prm.min_matches for r in refs)
    edges = sum(r["id1"] >= 0 for r in refs)
    print("pairs %s: %d, reached RANSAC %d, edges %d" % (size, len(refs), reached, edges))
    assert reached >= 10 and edges >= 15
