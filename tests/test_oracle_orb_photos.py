"""CPU checks of the ORB oracle (oracle/orb_oracle.c) on photographs: the pictures of SiftGPU's test data
(tests/golden/sift_photo_pairs.npz: 640-1, 640-2, 800-1, 800-2; tests/golden/orb_photos_640.npz, orb_photos_800.npz and
orb_photos_1600.npz, made by tests/golden/make_orb_photos.py: 640-3, 640-4, 640-5, 800-3, 800-4 and the central quarter of
the 2048x1536 picture, mirrored here into a seamless 2048x1536 image) and three photometric variants of each.  Natural
texture -- FAST-score ties, saturated regions next to detail, JPEG 8x8 blocking, very uneven corner density across the grid
cells -- is a different input class from the synthetic images of test_oracle_orb.py; tests/test_gpu_orb_photos.py runs the
kernels on it against this oracle."""
import lzma
import os
import time
import zlib

import numpy as np
import pytest

from oracle import pyorb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SHAPES = {"640_1": (480, 640), "640_2": (480, 640), "640_3": (480, 640), "640_4": (480, 640), "640_5": (480, 640),
          "800_1": (600, 800), "800_2": (600, 800), "800_3": (600, 800), "800_4": (600, 800), "1600": (1536, 2048)}
# CRC32 of the luminance bytes of the four pictures sift_photo_pairs.npz holds (the orb_photos_*.npz files store their
# own), and of the 2048x1536 mirror mosaic load_photos() builds from the stored quarter of 1600.jpg
PAIR_CRCS = {"640_1": 0x45487BE5, "640_2": 0xB92332ED, "800_1": 0x817256F3, "800_2": 0x951148FC}
MOSAIC_CRC = 0xD193A2AE
STORED = {"orb_photos_640.npz": ("640_3", "640_4", "640_5"), "orb_photos_800.npz": ("800_3", "800_4"),
          "orb_photos_1600.npz": ("1600q",)}


def decode(xz, shape):
    """make_orb_photos.py's storage: the xz-compressed second difference (mod 256) of the picture."""
    r = np.frombuffer(lzma.decompress(xz.tobytes()), np.uint8).reshape(tuple(int(s) for s in shape))
    return np.ascontiguousarray(np.cumsum(np.cumsum(r, axis=0, dtype=np.uint8), axis=1, dtype=np.uint8))


def load_stored():
    """{name: (decoded uint8 luminance, stored shape, stored CRC32)} of the pictures in the orb_photos_*.npz files."""
    out = {}
    for fname, names in STORED.items():
        z = np.load(os.path.join(GOLDEN, fname))
        for name in names:
            out[name] = (decode(z["xz_" + name], z["shape_" + name]), tuple(int(s) for s in z["shape_" + name]),
                         int(z["crc_" + name]))
    return out


def load_photos():
    """{name: uint8 luminance} of all ten photographs, names as in SHAPES.  "1600" is the central 1024x768 quarter of the
    2048x1536 picture mirrored into a 2048x1536 image (continuous across both seams): that picture's own texture at its
    own resolution, at the size of the original."""
    pairs = np.load(os.path.join(GOLDEN, "sift_photo_pairs.npz"))
    stored = load_stored()
    out = {}
    for name in SHAPES:
        if name in PAIR_CRCS:
            out[name] = np.ascontiguousarray(pairs["img_" + name])
        elif name == "1600":
            q = stored["1600q"][0]
            out[name] = np.ascontiguousarray(np.block([[q, q[:, ::-1]], [q[::-1, :], q[::-1, ::-1]]]))
        else:
            out[name] = stored[name][0]
    return out


def variant(g, kind):
    """Photometric variants: "dark" (low contrast: drives the adjuster's x0.7 re-detection down to its floor), "sat"
    (saturating gain: large 255 plateaus next to detail), "inv" (FAST's brighter and darker arcs swap roles)."""
    if kind == "orig":
        return g
    if kind == "dark":
        return (g.astype(np.float32) * 0.3 + 80).astype(np.uint8)
    if kind == "sat":
        return np.clip(g.astype(np.int32) * 2, 0, 255).astype(np.uint8)
    if kind == "inv":
        return (255 - g).astype(np.uint8)
    raise ValueError(kind)


@pytest.fixture(scope="module")
def photos():
    return load_photos()


def test_fixture_integrity(photos):
    stored = load_stored()
    assert sorted(photos) == sorted(SHAPES)
    for name, (g, shape, crc) in stored.items():
        assert g.shape == shape and zlib.crc32(g.tobytes()) == crc, name
    assert stored["1600q"][0].shape == (768, 1024)
    for name, g in photos.items():
        assert g.dtype == np.uint8 and g.shape == SHAPES[name] and g.flags.c_contiguous, name
        crc = zlib.crc32(g.tobytes())
        if name in PAIR_CRCS:
            assert crc == PAIR_CRCS[name], name
            assert all(name not in names for names in STORED.values())     # not stored twice
        elif name == "1600":
            assert crc == MOSAIC_CRC, "%08x" % crc
        else:
            assert crc == stored[name][2], name
        assert 40 < g.std() and g.min() < 30 and g.max() > 220   # a real photograph, not a flat or blank array


def _key(k):
    return sorted(zip(k["octave"].tolist(), k["y"].tolist(), k["x"].tolist(), k["response"].tolist(), k["angle"].tolist(),
                      k["size"].tolist()))


@pytest.mark.skipif(pyorb.ref_adjuster_lib() is None, reason="reference pin (oracle/_ref/libref_adjuster.so) not built")
@pytest.mark.parametrize("max_kp,grid,iters", [(1000, 3, 5), (600, 2, 3), (4000, 6, 5)])
def test_grid_detect_on_photos_matches_live_reference_code(photos, max_kp, grid, iters):
    """pyorb.grid_detect against the reference's own createDetector("ORB") wiring and feature_adjuster.cpp compiled around
    the oracle's cv::ORB::detect (as test_oracle_orb.py's test_grid_and_threshold_adaptation_match_live_reference_code
    does on synthetic frames), over sequences of photographs and their variants: a dark frame directly before the densest
    photograph, saturated and inverted frames, a frame with a partial mask; the per-cell thresholds persist on both sides."""
    R = pyorb.ref_adjuster_lib()
    seqs = {"640": [("640_1", "orig"), ("640_2", "orig"), ("640_1", "dark"), ("640_3", "orig"), ("640_4", "sat"),
                    ("640_5", "inv"), ("640_3", "dark"), ("640_2", "sat")],
            "800": [("800_1", "orig"), ("800_4", "dark"), ("800_4", "orig"), ("800_3", "inv"), ("800_2", "sat")]}
    if max_kp == 4000:
        seqs["1600"] = [("1600", "orig"), ("1600", "dark"), ("1600", "inv")]
    for size, seq in seqs.items():
        st = pyorb.grid_state(max_kp, grid, iters)
        h = R.ref_grid_detector_create(max_kp, grid, iters)
        try:
            for f, (name, kind) in enumerate(seq):
                img = variant(photos[name], kind)
                mask = np.full(img.shape, 255, np.uint8)
                if f == 3:
                    mask[:, (img.shape[1] * 2) // 3:] = 0     # the right third has no depth: cells with an all-zero mask
                a = pyorb.grid_detect(st, img, mask)
                b = pyorb.ref_grid_detect(h, img, mask)
                assert len(a) == len(b) and len(a) > 0, (size, f)
                assert _key(a) == _key(b), (size, f, name, kind)
        finally:
            R.ref_grid_detector_destroy(h)


def test_node_features_on_the_largest_photograph_is_fast_enough(photos):
    """The GPU tests run the oracle on the 2048x1536 image many times: one Node::Node feature pass of it stays far
    inside their time budget (about 1 s on one core)."""
    g = photos["1600"]
    st = pyorb.grid_state(4000)
    depth = np.full(g.shape, 2.0, np.float32)
    mask = np.full(g.shape, 255, np.uint8)
    t0 = time.perf_counter()
    kp, desc = pyorb.node_features(st, g, mask, depth, 4000)
    dt = time.perf_counter() - t0
    assert 3000 < len(kp) <= 4000 and desc.shape == (len(kp), 32)
    assert dt < 15.0, dt
