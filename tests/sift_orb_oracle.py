"""The oracle of feature_detector_type SIFTGPU with feature_extractor_type ORB (Node::Node, node.cpp:149-152, 183-210),
composed from the pinned pieces:

  1. SiftGPUWrapper::detect with an empty list (node.cpp:149-152): SiftGPU's own keys (x, y, s, o) -- the compiled reference
     (pyoracle.ref_sift_detect) where oracle/_ref exists, else the reference pipeline's recorded rows
     (tests/golden/sift_extract_golden.npz); the 128-d descriptors are never read;
  2. the wrapper's conversions (sift_gpu_wrapper.cpp:156-160): KeyPoint(x, y, 12.0 * s, o * 180.0 / 3.1415927) in double,
     stored as float, response = octave = 0;
  3. removeDepthless (node.cpp:186; :82 under use_feature_min_depth), then retainBest(max_keypoints) + resize (:188-191):
     every response is 0, so the repository's stable retainBest keeps the first max_keypoints survivors in SiftGPU's order;
  4. cv::ORB::create()->compute (:202): pyorb.compute -- the 31-pixel border filter, rBRIEF at each keypoint's own angle on
     level 0 (every octave is 0);
  5. the second removeDepthless (:206) and projectTo3D (:210): pyoracle.project_to_3d(_min_depth).

The cut of step 3 comes BEFORE the border filter of step 4: a frame can end with fewer than max_keypoints rows although
SiftGPU found more."""
import os

import numpy as np

import fast_oracle as fo
from oracle import pyorb
from oracle import pyoracle as po

GOLD = os.path.join(os.path.dirname(__file__), "golden", "sift_extract_golden.npz")


def sift_keys(name):
    """Step 1 on a fixture image ("c": 640 x 480, "d": 320 x 240): (gray, keys [n, 4], max_features)."""
    g = np.load(GOLD)
    img = np.ascontiguousarray(g[name + "_img"])
    maxf = int(g[name + "_meta"][2])
    if po.ref_siftgpu_lib() is not None:
        keys = po.ref_sift_detect(img, maxf)[0]
    else:
        keys = np.asarray(g[name + "_keys"], np.float32)
    return img, keys, maxf


def wrapper_keypoints(keys):
    """Step 2: SiftGPU keys (x, y, s, o) -> the cv::KeyPoints the wrapper builds."""
    out = np.zeros(len(keys), pyorb.KP_DTYPE)
    out["x"], out["y"] = keys[:, 0], keys[:, 1]
    out["size"] = (12.0 * keys[:, 2].astype(np.float64)).astype(np.float32)
    out["angle"] = (keys[:, 3].astype(np.float64) * 180.0 / 3.1415927).astype(np.float32)
    return out


def remove_depthless(kp, depth, min_depth=False):
    """removeDepthless (node.cpp:67-97), the rounded lookup or getMinDepthInNeighborhood over the keypoint's size."""
    if len(kp) == 0:
        return kp.copy()
    if min_depth:
        kept = po.remove_depthless_min_depth(np.stack([kp["x"], kp["y"]], 1), kp["size"], depth)
        return kp[np.asarray(kept, np.int64)].copy()
    return fo.remove_depthless(kp, depth)


def project(kp, depth, K, depth_scaling, max_keypoints, min_depth=False):
    """projectTo3D (node.cpp:900-965): (kept indices, xyz1)."""
    xy = np.stack([kp["x"], kp["y"]], 1)
    if min_depth:
        return po.project_to_3d_min_depth(xy, kp["size"], depth, *K, depth_scaling, max_keypoints)
    return po.project_to_3d(xy, depth, *K, depth_scaling, max_keypoints)


def frame_from_keypoints(gray, kp, depth, K, max_keypoints, min_depth=False, depth_scaling=1.0):
    """Steps 3-5 for the wrapper's keypoints of one frame: (keypoints, descriptors [n, 32], xyz1 [n, 4])."""
    gray = np.ascontiguousarray(gray, np.uint8)
    depth = np.ascontiguousarray(depth, np.float32)
    kp = remove_depthless(kp, depth, min_depth)[:max_keypoints]
    if len(kp) == 0:
        return kp, np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.float32)
    kp, desc = pyorb.compute(gray, kp)
    kp2 = remove_depthless(kp, depth, min_depth)
    assert len(kp2) == len(kp)   # the positions and sizes the first pass kept: the second keeps them all
    if len(kp) == 0:
        return kp, desc, np.zeros((0, 4), np.float32)
    kept, xyz = project(kp, depth, K, depth_scaling, max_keypoints, min_depth)
    kept = np.asarray(kept, np.int64)
    return kp[kept].copy(), desc[kept].copy(), xyz


def frame(gray, keys, depth, K, max_keypoints, min_depth=False, depth_scaling=1.0):
    """Node::Node for one frame from SiftGPU's keys (x, y, s, o): (keypoints, descriptors, xyz1)."""
    return frame_from_keypoints(gray, wrapper_keypoints(keys), depth, K, max_keypoints, min_depth, depth_scaling)
