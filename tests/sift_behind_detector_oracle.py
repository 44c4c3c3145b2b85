"""The oracle of feature_extractor_type SIFTGPU behind the ORB or FAST grid detector (Node::Node, node.cpp:160, 165-176),
composed from the pinned restatements:

  1. detector->detect: the ORB grid detector of oracle/orb_oracle.c (pyorb.grid_detect) or the FAST composition of
     tests/fast_oracle.py -- the aggregate, before removeDepthless;
  2. projectTo3D (node.cpp:900-965): pyoracle.project_to_3d(_min_depth), whose kept indices are the first max_keypoints
     keypoints with depth, in aggregate order;
  3. SiftGPUWrapper::detect with that list (sift_gpu_wrapper.cpp:132-165): s = size / 12.0, o = angle / 180.0 * 3.1415927 in
     double, stored as float; the keypoints come back as (12.0 * s, o * 180.0 / 3.1415927).  Descriptors: the compiled
     reference (pyoracle.ref_sift_describe), where it is available;
  4. projectTo3DSiftGPU + RootSIFT (pyoracle.sift_node_features).

The empty-list rule: when step 2 keeps nothing, the wrapper skips SetKeypointList (sift_gpu_wrapper.cpp:133) and SiftGPU runs
its own detection -- a list never carries over, SiftPyramid::RunSIFT resets _existing_keypoints and _keypoint_index after
every run (SiftPyramid.cpp:154-156) -- so the frame gets SiftGPU's own keypoints and descriptors ("-tc2 max_keypoints")."""
import numpy as np

import fast_oracle as fo
from oracle import pyorb
from oracle import pyoracle as po


class Detector:
    """createDetector(type) for type ORB or FAST: the grid of adaptive detectors; the thresholds persist across frames."""

    def __init__(self, kind, max_keypoints=600, grid=3, max_iters=5):
        self.kind, self.cells = kind, grid * grid
        if kind == "ORB":
            self.st = pyorb.grid_state(max_keypoints, grid, max_iters)
            self.max_total = self.st.max_total
        else:
            self.g = fo.Grid(max_keypoints, grid, max_iters)
            self.max_total = self.g.max_total

    def detect(self, img, mask):
        if self.kind == "ORB":
            return pyorb.grid_detect(self.st, img, mask)
        return self.g.detect(np.ascontiguousarray(img, np.uint8), mask, fo.fast_detect)

    def thresholds(self):
        if self.kind == "ORB":
            return np.array(self.st.thresh[: self.cells], np.float64)
        return np.array(self.g.thresh, np.float64)


def project_kept(kp, depth, K, max_keypoints, min_depth=False):
    """Step 2: the indices projectTo3D keeps (feature_locations_2d_ after its erase and cut)."""
    if len(kp) == 0:
        return np.zeros(0, np.int64)
    xy = np.stack([kp["x"], kp["y"]], 1)
    if min_depth:
        kept, _ = po.project_to_3d_min_depth(xy, kp["size"], depth, *K, 1.0, max_keypoints)
    else:
        kept, _ = po.project_to_3d(xy, depth, *K, 1.0, max_keypoints)
    return np.asarray(kept, np.int64)


def wrapper_keys(kp):
    """Step 3's conversions: the (x, y, s, o) the wrapper hands to SiftGPU and the keypoints it rebuilds."""
    s = (kp["size"].astype(np.float64) / 12.0).astype(np.float32)
    o = (kp["angle"].astype(np.float64) / 180.0 * 3.1415927).astype(np.float32)
    out = np.zeros(len(kp), kp.dtype)
    out["x"], out["y"] = kp["x"], kp["y"]
    out["size"] = (12.0 * s.astype(np.float64)).astype(np.float32)
    out["angle"] = (o.astype(np.float64) * 180.0 / 3.1415927).astype(np.float32)
    return np.stack([kp["x"], kp["y"], s, o], 1).astype(np.float32), out


def sift_keypoints(keys, dtype):
    """SiftGPU's own keys (x, y, s, o) as the wrapper rebuilds them (sift_gpu_wrapper.cpp:156-160)."""
    out = np.zeros(len(keys), dtype)
    out["x"], out["y"] = keys[:, 0], keys[:, 1]
    out["size"] = (12.0 * keys[:, 2].astype(np.float64)).astype(np.float32)
    out["angle"] = (keys[:, 3].astype(np.float64) * 180.0 / 3.1415927).astype(np.float32)
    return out


def frame(det, gray, mask, depth, K, max_keypoints, min_depth=False, use_root_sift=True, describe=None, detect_own=None):
    """Node::Node for one frame: (keypoints, xyz1, siftgpu_descriptors, feature_descriptors, aggregate, quirk).
    describe(gray, keys [n, 4]) -> [n, 128] and detect_own(gray, max_keypoints) -> (keys [n, 4], desc [n, 128]) default to
    the compiled reference."""
    describe = describe or po.ref_sift_describe
    detect_own = detect_own or (lambda g, m: po.ref_sift_detect(g, m)[:2])
    depth = np.ascontiguousarray(depth, np.float32)
    agg = det.detect(gray, mask)
    kept = project_kept(agg, depth, K, max_keypoints, min_depth)
    quirk = len(kept) == 0
    if quirk:   # the empty-list rule
        keys, desc = detect_own(gray, max_keypoints)
        kl = sift_keypoints(keys, agg.dtype)
    else:
        keys, kl = wrapper_keys(agg[kept])
        desc = describe(gray, keys)
    if len(kl) == 0:
        z = np.zeros((0, 128), np.float32)
        return kl, np.zeros((0, 4), np.float32), z, z, agg, quirk
    k2, xyz, raw, feat = po.sift_node_features(np.stack([kl["x"], kl["y"]], 1), desc, depth, *K, 1.0, max_keypoints,
                                               use_root_sift, kp_size=kl["size"] if min_depth else None)
    return kl[k2].copy(), xyz, raw, feat, agg, quirk
