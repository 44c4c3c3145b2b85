"""The oracle of feature_detector_type "FAST" (TEST INFRASTRUCTURE ONLY), composed from the pinned restatements of
oracle/orb_oracle.c and oracle/rgbd_oracle.c:

  cv::FastFeatureDetector::create(t)->detect   pyorb.fast_score_map + pyorb.fast_keypoints (3-pixel border, mask)
  VideoGridAdaptedFeatureDetector +            Grid below (feature_adjuster.cpp:185-317; orb_grid_detect restated in
  VideoDynamicAdaptedFeatureDetector           Python), with the cell detector as a function: pyorb.detect plugged in gives
                                               pyorb.grid_detect back (tests/test_oracle_fast.py)
  Node::Node, ORB extractor                    node_features (node.cpp:183-210; orb_node_features restated): removeDepthless
                                               (or its min-depth form), the max_keypoints cut, cv::ORB::compute
  projectTo3D                                  pyoracle.project_to_3d / project_to_3d_min_depth

orb_keep_strongest and orb_compute are called through a private ctypes handle of liboracle.so with their own argtypes."""
import ctypes as C
import math

import numpy as np

from oracle import pyoracle as po
from oracle import pyorb

KP = pyorb.KP_DTYPE
_L = None


def _lib():
    global _L
    if _L is None:
        pyorb.lib()   # builds / loads liboracle.so
        L = C.CDLL(po.lib()._name)
        vp, i = C.c_void_p, C.c_int
        L.orb_keep_strongest.restype = i
        L.orb_keep_strongest.argtypes = [vp, i, i]
        L.orb_compute.restype = i
        L.orb_compute.argtypes = [vp, i, i, vp, i, vp]
        _L = L
    return _L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fast_detect(img, mask, threshold):
    """cv::FastFeatureDetector::create(threshold)->detect(img, kps, mask)."""
    return pyorb.fast_keypoints(pyorb.fast_score_map(img, threshold), mask, 3)


def keep_strongest(kp, n):
    """keepStrongest(N) (feature_adjuster.cpp:247-255) with the oracle's tie rule (orb_keep_strongest)."""
    kp = np.ascontiguousarray(kp.copy())
    if len(kp) == 0:
        return kp
    m = _lib().orb_keep_strongest(_p(kp), len(kp), n)
    return kp[:m].copy()


def orb_compute(gray, kp):
    """cv::ORB::create()->compute (orb_compute): (kept keypoints, descriptors [n, 32])."""
    gray = np.ascontiguousarray(gray, np.uint8)
    kp = np.ascontiguousarray(kp.copy())
    desc = np.zeros((max(len(kp), 1), 32), np.uint8)
    n = _lib().orb_compute(_p(gray), gray.shape[1], gray.shape[0], _p(kp), len(kp), _p(desc))
    return kp[:n].copy(), desc[:n].copy()


def _roundf(x):
    return int(math.floor(float(x) + 0.5))   # C roundf of a positive float


class Grid:
    """The reference's detector object: grid x grid threshold-adaptive cell detectors (features.cpp:42-60,
    feature_adjuster.cpp:185-317).  thresh[cell] persists across frames; a new Grid is a fresh createDetector."""

    def __init__(self, max_keypoints=600, grid=3, max_iters=5):
        cells = grid * grid
        mn, mx = max_keypoints, int(max_keypoints * 1.5)
        self.grid, self.max_iters = grid, max_iters
        self.cell_min = _roundf(np.float32(mn) / np.float32(cells))
        self.cell_max = _roundf(np.float32(mx) / np.float32(cells))
        self.max_total, self.edge = mx, 31
        self.thresh = [20.0] * cells

    def detect(self, img, mask, cell_detect):
        """cell_detect(sub_image, sub_mask or None, int threshold) -> keypoints of the sub-image (KP_DTYPE)."""
        rows, cols = img.shape
        G, e = self.grid, self.edge
        max_per_cell = self.max_total // (G * G)
        out = []
        for i in range(G):
            r0, r1 = max(i * rows // G - e, 0), min(rows, (i + 1) * rows // G + e)
            for j in range(G):
                c0, c1 = max(j * cols // G - e, 0), min(cols, (j + 1) * cols // G + e)
                sub = np.ascontiguousarray(img[r0:r1, c0:c1])
                sub_mask = None if mask is None else np.ascontiguousarray(mask[r0:r1, c0:c1])
                c = i * G + j
                it, checked = self.max_iters, False
                while True:   # VideoDynamicAdaptedFeatureDetector::detect
                    kp = cell_detect(sub, sub_mask, int(self.thresh[c]))
                    n = len(kp)
                    if n < self.cell_min:
                        self.thresh[c] *= 0.7
                        if self.thresh[c] < 2:
                            self.thresh[c] = 2.0
                        if n == 0 and not checked:
                            checked = True
                            if sub_mask is None or not sub_mask.any():
                                break
                    elif n > self.cell_max:
                        self.thresh[c] *= 1.3
                        if self.thresh[c] > 10000:
                            self.thresh[c] = 10000.0
                        break
                    else:
                        break
                    it -= 1
                    if not (it > 0 and 2 < self.thresh[c] < 10000):
                        break
                kp = keep_strongest(kp, max_per_cell)
                kp["x"] += np.float32(c0)
                kp["y"] += np.float32(r0)
                out.append(kp)
        return np.concatenate(out) if out else np.zeros(0, KP)


def remove_depthless(kp, depth):
    """removeDepthless (node.cpp:67-97), as orb_oracle.c:635-647 restates it."""
    rows, cols = depth.shape
    x, y = kp["x"], kp["y"]
    ok = (x < cols) & (x >= 0) & (y < rows) & (y >= 0) & ~np.isnan(x) & ~np.isnan(y)
    keep = np.zeros(len(kp), bool)
    for k in np.nonzero(ok)[0]:
        r = min(int(np.floor(y[k] + 0.5)), rows - 1)
        c = min(int(np.floor(x[k] + 0.5)), cols - 1)
        keep[k] = not np.isnan(depth[r, c])
    return kp[keep].copy()


def node_features(grid, gray, mask, depth, max_keypoints, cell_detect=None, min_depth=False):
    """Node::Node's ORB-extractor steps (node.cpp:160-210) behind the grid detector: (keypoints, descriptors)."""
    gray = np.ascontiguousarray(gray, np.uint8)
    depth = np.ascontiguousarray(depth, np.float32)
    kp = grid.detect(gray, mask, cell_detect or fast_detect)
    if min_depth:
        kept = po.remove_depthless_min_depth(np.stack([kp["x"], kp["y"]], 1), kp["size"], depth)
        kp = kp[kept].copy()
    else:
        kp = remove_depthless(kp, depth)
    if len(kp) > max_keypoints:   # retainBest + resize: the max_keypoints largest responses, ties in order
        order = sorted(range(len(kp)), key=lambda i: (-float(kp["response"][i]), i))[:max_keypoints]
        kp = kp[np.sort(np.array(order, np.int64))].copy()
    return orb_compute(gray, kp)


def project(kp, depth, K, depth_scaling=1.0, max_keypoints=1000, min_depth=False):
    """projectTo3D of the final keypoints: xyz1 [n, 4]."""
    xy = np.stack([kp["x"], kp["y"]], 1)
    if min_depth:
        kept, xyz = po.project_to_3d_min_depth(xy, kp["size"], depth, *K, depth_scaling, max_keypoints)
    else:
        kept, xyz = po.project_to_3d(xy, depth, *K, depth_scaling, max_keypoints)
    assert len(kept) == len(kp)
    return xyz


def run_sequence(grays, masks, depths, K, max_keypoints, grid, min_depth=False, max_iters=5):
    """Node::Node frame by frame through one detector: [(keypoints, descriptors, xyz1, thresholds after the frame)]."""
    g = Grid(max_keypoints, grid, max_iters)
    out = []
    for im, m, d in zip(grays, masks, depths):
        kp, desc = node_features(g, im, m, d, max_keypoints, min_depth=min_depth)
        out.append((kp, desc, project(kp, d, K, 1.0, max_keypoints, min_depth), np.array(g.thresh)))
    return out
