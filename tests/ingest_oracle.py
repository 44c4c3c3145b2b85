"""numpy restatement of the image preparation in front of Node::Node's feature path (include/rgbdfe.h, "sensor frames",
steps 1-3) -- test infrastructure for tests/test_oracle_ingest.py and tests/test_gpu_sensor_ingest.py.

  1. resize_nearest   cv::resize(depth, visual size, INTER_NEAREST) on the raw samples (openni_listener.cpp:651-655);
                      OpenCV 3.3 resizeNN: x_ofs[x] = min(cvFloor(x * ifx), src.cols - 1), ifx = 1 / ((double)dst.cols / src.cols)
  2. po.depth_to_mono8 depthToCV8UC1 (misc.cpp:414-430), the oracle's orc_depth_* functions
  3. gray_of          cv::cvtColor(CV_RGB2GRAY) on the channels as stored (node.cpp:139-144); OpenCV 3.3 RGB2Gray<uchar>:
                      (c0 * 4899 + c1 * 9617 + c2 * 1868 + 8192) >> 14.  Third-party arithmetic restated from the portable
                      OpenCV path, not pinned by an executable of the reference.
"""
import numpy as np

from oracle import pyoracle as po

R2Y, G2Y, B2Y, YUV_SHIFT = 4899, 9617, 1868, 14


def gray_of(visual):
    """[H, W] uint8 -> itself; [H, W, 3] uint8 -> CV_RGB2GRAY of the channels as stored (rgb8 and bgr8 alike)."""
    v = np.asarray(visual)
    if v.ndim == 2:
        return np.ascontiguousarray(v, np.uint8)
    c = v.astype(np.uint32)
    return ((c[..., 0] * R2Y + c[..., 1] * G2Y + c[..., 2] * B2Y + (1 << (YUV_SHIFT - 1))) >> YUV_SHIFT).astype(np.uint8)


def index_table(dst, src):
    """Source index of every destination index, in resizeNN's double arithmetic."""
    inv = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * inv).astype(np.int64), src - 1)


def resize_nearest(img, shape):
    """img resampled to shape (rows, cols) by nearest neighbour, on the raw samples."""
    rows, cols = shape
    if img.shape == (rows, cols):
        return np.ascontiguousarray(img)
    return np.ascontiguousarray(img[index_table(rows, img.shape[0])][:, index_table(cols, img.shape[1])])


def prepared_planes(visual, depth):
    """(gray uint8, mono8 mask uint8, depth float32 metres) at the visual image's size: what the listener and Node::Node hand
    to detector->detect / removeDepthless / projectTo3D for a sensor frame."""
    gray = gray_of(visual)
    d = resize_nearest(np.asarray(depth), gray.shape)
    if d.dtype == np.uint16:
        mono8, dm = po.depth_to_mono8(d)
        return gray, mono8, dm
    d = np.ascontiguousarray(d, np.float32)
    return gray, po.depth_to_mono8(d), d


# ---- the test frames: colour composed from the luminance photographs under tests/golden (no new fixtures)
PHOTO_NAMES = ("640_1", "640_2", "640_3", "640_4", "640_5")


def colour_frame(photos, k):
    """Frame k: channels (640_{k}, 640_{k+1}, 640_{k+2}), cyclically."""
    return np.ascontiguousarray(np.stack([photos[PHOTO_NAMES[(k + c) % 5]] for c in range(3)], axis=-1))


def depth_frame(shape, k, encoding, plane_depth, binary_mask):
    """plane_depth(shape, 2.0, k) with binary_mask(shape, k) holes: NaN for "32FC1"; rint(1000 d) with 0 in the holes for
    "16UC1"."""
    d = plane_depth(shape, 2.0, k)
    holes = binary_mask(shape, k) == 0
    if encoding == "32FC1":
        d = d.copy()
        d[holes] = np.nan
        return d
    mm = np.rint(d.astype(np.float64) * 1000.0).astype(np.uint16)
    mm[holes] = 0
    return mm
