"""Host-side mirror of the reference's front-end interface over the C ABI.

The reference's seam is a set of C++ methods (there is no FFI):
``Node::matchNodePair`` (src/node.h:85), ``Node::featureMatching`` (:117),
``Node::getRelativeTransformationTo`` (:102), ``bruteForceSearchORB``
(src/features.h:14) and ``GraphManager::nodeComparisons``'s
``QtConcurrent::blockingMapped`` fan-out (src/graph_manager.cpp:541-548).
This module keeps those names and argument meanings so the parity tests read
like tests of the reference; all arithmetic happens in librgbdfe.so on the GPU.
"""
import ctypes as C
import os
import threading
import warnings
import weakref
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import DEFAULT_HAMMING_MODE, RESULT_DTYPE, RgbdfeConfig, RgbdfeError, RgbdfeParams
from ._lib import DISPLAY_POINTS, DISPLAY_TRIANGLES, DISPLAY_TRIANGLE_STRIP  # noqa: F401


@dataclass
class DMatch:
    """cv::DMatch as the reference fills it (node.cpp:573): distance = hd/256 (jitter dropped)."""
    queryIdx: int
    trainIdx: int
    distance: float


@dataclass
class LoadedEdge3D:
    """src/edge.h:24-32"""
    id1: int = -1
    id2: int = -1
    transform: np.ndarray = field(default_factory=lambda: np.eye(4))
    informationMatrix: np.ndarray = field(default_factory=lambda: np.zeros((6, 6)))


@dataclass
class MatchingResult:
    """src/matching_result.h:24-46"""
    inlier_matches: List[DMatch] = field(default_factory=list)
    all_matches: List[DMatch] = field(default_factory=list)
    edge: LoadedEdge3D = field(default_factory=LoadedEdge3D)
    rmse: float = 0.0
    ransac_trafo: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    final_trafo: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    valid_iterations: int = 0
    real_iterations: int = 0


def inlier_indices(rec) -> np.ndarray:
    """Positions (into all_*) of the inlier matches of one RESULT_DTYPE record."""
    bits = np.unpackbits(np.asarray(rec["inlier_mask"]).view(np.uint8), bitorder="little")
    return np.flatnonzero(bits[: int(rec["n_all"])]).astype(np.int32)


def record_to_matching_result(rec) -> MatchingResult:
    n_all = int(rec["n_all"])
    q = rec["all_q"][:n_all].astype(np.int32)
    t = rec["all_t"][:n_all].astype(np.int32)
    d = rec["all_hd"][:n_all].astype(np.float32) / np.float32(256.0)
    all_matches = [DMatch(int(a), int(b), float(c)) for a, b, c in zip(q, t, d)]
    inl = inlier_indices(rec)
    T = np.array(rec["trafo"], np.float32).reshape(4, 4).T.copy()  # column-major storage
    mr = MatchingResult(all_matches=all_matches, inlier_matches=[all_matches[i] for i in inl],
                        rmse=float(rec["rmse"]), ransac_trafo=T, final_trafo=T.copy(),
                        valid_iterations=int(rec["valid_iterations"]),
                        real_iterations=int(rec["real_iterations"]))
    mr.edge.id1, mr.edge.id2 = int(rec["id1"]), int(rec["id2"])
    if mr.edge.id1 >= 0:
        mr.edge.transform = T.astype(np.float64)                        # node.cpp:1339
        mr.edge.informationMatrix = np.eye(6) * float(rec["info_scale"])  # node.cpp:1335
    return mr


def _matrix_out(buf):
    return np.array(buf, np.float64).reshape(4, 4).T.copy()


def _matrix_in(M):
    return (C.c_double * 16)(*[float(v) for v in np.asarray(M, np.float64).reshape(4, 4).T.reshape(-1)])


REFERENCE_FOVY = 100.0 / 180.0 * 3.14159265358979323846   # fov_ (glviewer.cpp:118): radians, handed to gluPerspective as degrees


def render_perspective(fovy=REFERENCE_FOVY, aspect=float(np.float32(640) / np.float32(480)), z_near=0.1, z_far=1e4):
    """gluPerspective as a 4 x 4 float64 matrix (row-major numpy sense); the defaults are what the reference passes."""
    out = (C.c_double * 16)()
    _lib.load().rgbdfe_render_perspective(fovy, aspect, z_near, z_far, out)
    return _matrix_out(out)


def render_viewer_view(x_tra=0.0, y_tra=0.0, z_tra=-50.0, x_rot=180.0 * 16.0, y_rot=0.0, z_rot=0.0, rotation_stepping=1.0,
                       viewpoint=None):
    """The modelview of GLViewer::drawClouds (glviewer.cpp:356-377); viewpoint: the INVERSE of a camera pose, 4 x 4."""
    out = (C.c_double * 16)()
    _lib.load().rgbdfe_render_viewer_view(x_tra, y_tra, z_tra, x_rot, y_rot, z_rot, rotation_stepping,
                                          _matrix_in(viewpoint) if viewpoint is not None else None, out)
    return _matrix_out(out)


def render_sensor_camera(fx, fy, cx, cy, width, height, z_near=0.1, z_far=1e4, pose=None):
    """(view, projection) of the sensor's own pinhole at the rigid 4 x 4 pose: point (u, v) of a cloud lands on pixel (u, v)."""
    view, proj = (C.c_double * 16)(), (C.c_double * 16)()
    _lib.load().rgbdfe_render_sensor_camera(fx, fy, cx, cy, int(width), int(height), z_near, z_far,
                                            _matrix_in(pose) if pose is not None else None, view, proj)
    return _matrix_out(view), _matrix_out(proj)


def render_unproject(x, y, depth, view, projection, width, height):
    """gluUnProject as GLViewer::setClickedPosition uses it: window x, y (y up: height - image row) and a depth image value
    to the world point, or None when projection . view is singular."""
    out = (C.c_double * 3)()
    st = _lib.load().rgbdfe_render_unproject(float(x), float(y), float(depth), _matrix_in(view), _matrix_in(projection),
                                             int(width), int(height), out)
    return np.array(out, np.float64) if st == 0 else None


class FrontEnd:
    """One rgbdfe context = one GPU: resident node features + the batched pair op."""

    def __init__(self, device_id: int = 0, max_nodes: int = 256, max_keypoints: int = 1024,
                 max_pairs_per_batch: int = 4096, device_ids: Optional[Sequence[int]] = None, **params):
        """device_ids: several GPUs behind this one handle (rgbdfe_create_multi): node features replicated,
        pairs sharded pair k -> device k mod G, results gathered; a device may be listed twice."""
        self._L = _lib.load()
        self._batch_lock = threading.Lock()
        cfg = RgbdfeConfig()
        self._L.rgbdfe_default_config(C.byref(cfg))
        cfg.device_id = device_id
        cfg.max_nodes = max_nodes
        cfg.max_keypoints = max_keypoints
        cfg.max_pairs_per_batch = max_pairs_per_batch
        for k, v in params.items():
            if not hasattr(cfg.params, k):
                raise TypeError(f"unknown front-end parameter {k!r}")
            setattr(cfg.params, k, v)
        self.cfg = cfg
        self._ctx = C.c_void_p()
        if device_ids is not None:
            ids = np.ascontiguousarray(device_ids, np.int32)
            st = self._L.rgbdfe_create_multi(C.byref(cfg), ids.ctypes.data, len(ids), C.byref(self._ctx))
        else:
            st = self._L.rgbdfe_create(C.byref(cfg), C.byref(self._ctx))
        if st != 0:
            self._ctx = C.c_void_p()
            raise RgbdfeError(f"rgbdfe_create failed: {self._L.rgbdfe_status_string(st).decode()}")

    @property
    def device_count(self) -> int:
        return int(self._L.rgbdfe_device_count(self._ctx))

    def set_hamming_mode(self, mode: int):
        """0 = popcount kernel, 1 = fp4 MFMA kernel, 2 = MFMA kernel with the VALU row term, 3 = the MFMA kernel as a
        software pipeline inside every wave with 256 queries per block, 4 = that kernel with 512 queries per block
        (include/rgbdfe.h; _lib.DEFAULT_HAMMING_MODE is what a new context uses: mode 3 with the block width chosen per batch)."""
        self._check(self._L.rgbdfe_set_hamming_mode(self._ctx, mode))
        self._hamming_mode = int(mode)

    @property
    def hamming_wide_last(self) -> int:
        """1 = the latest Hamming launch ran the pipelined kernel's 512-query blocks, 0 = it did not, -1 = none yet."""
        return int(self._L.rgbdfe_hamming_wide_last(self._ctx))

    def set_hamming_shape(self, shape: int):
        """The MFMA tile of mode 3's 512-query blocks: 16 = 16x16x128, 32 = 32x32x64, 0 = the library's choice
        (include/rgbdfe.h; every other kernel is 32x32x64 whatever this says)."""
        self._check(self._L.rgbdfe_set_hamming_shape(self._ctx, shape))

    @property
    def hamming_shape_last(self) -> int:
        """16 / 32 = the MFMA tile of the latest Hamming launch, 0 = it ran the popcount kernel, -1 = none yet."""
        return int(self._L.rgbdfe_hamming_shape_last(self._ctx))

    @property
    def hamming_mode(self) -> int:
        """The Hamming kernel in use (the library falls back to 0 above 32768 keypoints per node)."""
        import os
        m = getattr(self, "_hamming_mode", None)
        if m is None:
            try:
                m = int(os.environ.get("RGBDFE_HAMMING_MODE", str(DEFAULT_HAMMING_MODE)))
            except ValueError:
                m = DEFAULT_HAMMING_MODE
            m = m if 0 <= m <= 4 else DEFAULT_HAMMING_MODE
        return 0 if self.cfg.max_keypoints > 32768 else m

    def group_submit_us(self) -> float:
        """Host microseconds the calling thread spent enqueueing the latest sharded batch on all devices."""
        v = C.c_double(0.0)
        self._check(self._L.rgbdfe_group_submit_us(self._ctx, C.byref(v)))
        return float(v.value)

    def gather_transport(self) -> str:
        return self._L.rgbdfe_gather_transport(self._ctx).decode()

    def gather_exchanges(self) -> int:
        """Exchanges the latest match_pair_list_allgather_inliers issued (1: one collective, no host read in front of it)."""
        return int(self._L.rgbdfe_gather_exchanges(self._ctx))

    def match_pair_list_allgather(self, query_ids, train_ids, d_out_ptrs: Sequence[int]) -> int:
        """All results on every device (ncclAllGather / peer copies).  d_out_ptrs: one device buffer per device,
        each device_count * ceil(n / device_count) records.  Returns records per device."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        ptrs = (C.c_void_p * len(d_out_ptrs))(*[C.c_void_p(int(p)) for p in d_out_ptrs])
        per = C.c_int32(0)
        self._check(self._L.rgbdfe_match_pair_list_allgather(self._ctx, q.ctypes.data, t.ctypes.data, len(q),
                                                             C.cast(ptrs, C.c_void_p), C.byref(per)))
        return int(per.value)

    def match_pair_list_allgather_compact(self, query_ids, train_ids, d_out_ptrs: Sequence[int]) -> int:
        """rgbdfe_match_pair_list_allgather with COMPACT_DTYPE records (144 B: no all_matches lists) as the payload."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        ptrs = (C.c_void_p * len(d_out_ptrs))(*[C.c_void_p(int(p)) for p in d_out_ptrs])
        per = C.c_int32(0)
        self._check(self._L.rgbdfe_match_pair_list_allgather_compact(self._ctx, q.ctypes.data, t.ctypes.data, len(q),
                                                                     C.cast(ptrs, C.c_void_p), C.byref(per)))
        return int(per.value)

    def match_pair_list_allgather_inliers(self, query_ids, train_ids, d_out_ptrs: Sequence[int]):
        """rgbdfe_match_pair_list_allgather_inliers: every device buffer ends up with every device's inlier stream.
        Returns (records per device, list entries per device, stride in bytes)."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        g = len(d_out_ptrs)
        ptrs = (C.c_void_p * g)(*[C.c_void_p(int(p)) for p in d_out_ptrs])
        per, stride = C.c_int32(0), C.c_int64(0)
        totals = np.zeros(g, np.int32)
        self._check(self._L.rgbdfe_match_pair_list_allgather_inliers(self._ctx, q.ctypes.data, t.ctypes.data, len(q),
                                                                     C.cast(ptrs, C.c_void_p), C.byref(per), totals.ctypes.data,
                                                                     C.byref(stride)))
        return int(per.value), totals, int(stride.value)

    def pack_compact(self, d_records_ptr: int, n: int, d_compact_ptr: int, stream: Optional[int] = None):
        """n records in HBM -> n compact records in HBM on `stream` (rgbdfe_pack_compact)."""
        self._check(self._L.rgbdfe_pack_compact(self._ctx, C.c_void_p(int(d_records_ptr)), int(n),
                                                C.c_void_p(int(d_compact_ptr)), C.c_void_p(stream or 0)))

    def pack_inliers(self, d_records_ptr: int, n: int, n_headers: int, d_stream_ptr: int, d_total_ptr: int,
                     stream: Optional[int] = None):
        """n records in HBM -> the shard's inlier stream in HBM on `stream` (rgbdfe_pack_inliers: n_headers headers of 104
        bytes, then query | train << 16 of every inlier; the entry count goes to the device int32 at d_total_ptr)."""
        self._check(self._L.rgbdfe_pack_inliers(self._ctx, C.c_void_p(int(d_records_ptr)), int(n), int(n_headers),
                                                C.c_void_p(int(d_stream_ptr)), C.c_void_p(int(d_total_ptr)),
                                                C.c_void_p(stream or 0)))

    def match_pair_list_allgather_edges(self, query_ids, train_ids, d_out_ptrs: Sequence[int], d_index_ptrs=None):
        """Only the accepted edges travel (rgbdfe_match_pair_list_allgather_edges).  Returns (counts per device, stride):
        device i's edges sit at records [i * stride, i * stride + counts[i]) of every buffer, their positions in the pair
        list at the same offsets of the index buffers."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        g = len(d_out_ptrs)
        ptrs = (C.c_void_p * g)(*[C.c_void_p(int(p)) for p in d_out_ptrs])
        iptrs = None if d_index_ptrs is None else (C.c_void_p * g)(*[C.c_void_p(int(p)) for p in d_index_ptrs])
        counts = np.zeros(g, np.int32)
        stride = C.c_int32(0)
        self._check(self._L.rgbdfe_match_pair_list_allgather_edges(
            self._ctx, q.ctypes.data, t.ctypes.data, len(q), C.cast(ptrs, C.c_void_p),
            None if iptrs is None else C.cast(iptrs, C.c_void_p), counts.ctypes.data, C.byref(stride)))
        return counts, int(stride.value)

    # -- plumbing --------------------------------------------------------------
    def _check(self, st):
        if st != 0:
            msg = self._L.rgbdfe_last_error(self._ctx).decode()
            raise RgbdfeError(f"{self._L.rgbdfe_status_string(st).decode()}: {msg}")

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            for ref in getattr(self, "_octomaps", []) + getattr(self, "_slams", []):  # a map or a SLAM object goes before the context it lives on
                m = ref()
                if m is not None:
                    m.close()
            self._L.rgbdfe_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def params(self) -> RgbdfeParams:
        return self.cfg.params

    def set_params(self, **params):
        for k, v in params.items():
            setattr(self.cfg.params, k, v)
        self._check(self._L.rgbdfe_set_params(self._ctx, C.byref(self.cfg.params)))

    # -- node residency ----------------------------------------------------------
    def upload_node(self, node_id: int, desc: np.ndarray, xyz1: np.ndarray):
        desc = np.ascontiguousarray(desc, np.uint8)
        xyz1 = np.ascontiguousarray(xyz1, np.float32)
        n = desc.shape[0]
        if desc.ndim != 2 or desc.shape[1] != 32 or xyz1.shape != (n, 4):
            raise ValueError("desc must be [n,32] uint8 and xyz1 [n,4] float32")
        self._check(self._L.rgbdfe_upload_node(self._ctx, node_id, desc.ctypes.data,
                                               xyz1.ctypes.data, n))

    def upload_node_device(self, node_id: int, d_desc_ptr: int, d_xyz1_ptr: int, n: int,
                           stream: Optional[int] = None):
        self._check(self._L.rgbdfe_upload_node_device(self._ctx, node_id, d_desc_ptr, d_xyz1_ptr,
                                                      n, stream))

    def upload_node_keypoints(self, node_id: int, kp_xy: np.ndarray):
        """Node::feature_locations_2d_ (KeyPoint.pt) of a resident node, for the g2o refinement."""
        kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        self._check(self._L.rgbdfe_upload_node_keypoints(self._ctx, node_id, kp_xy.ctypes.data, kp_xy.shape[0]))

    def release_node(self, node_id: int):
        self._check(self._L.rgbdfe_release_node(self._ctx, node_id))

    def node_count(self, node_id: int) -> int:
        return self._L.rgbdfe_node_count(self._ctx, node_id)

    def node_feature_stats(self, node_id: int) -> np.ndarray:
        """Node::feature_matching_stats_ of a resident node: a saturating 8-bit counter per row (updateInlierFeatures)."""
        out = np.zeros(max(self.node_count(node_id), 0), np.uint8)
        n = self._L.rgbdfe_node_feature_stats(self._ctx, int(node_id), out.ctypes.data, len(out))
        if n < 0:
            self._check(n)
        return out[:n]

    def set_node_feature_stats(self, node_id: int, stats):
        """Writes a resident node's counters back (one byte per row): what a restore needs behind the upload."""
        s = np.ascontiguousarray(stats, np.uint8).reshape(-1)
        self._check(self._L.rgbdfe_set_node_feature_stats(self._ctx, int(node_id), s.ctypes.data, len(s)))

    def download_nodes(self, node_ids, fields=("desc", "xyz1", "kp_xy", "stats")) -> dict:
        """rgbdfe_download_nodes: the listed resident nodes (of one kind) in the order given, packed without gaps.  Returns
        {"row_offsets": [n + 1] int64, "kinds": [n] (0 ORB, 1 SIFT, 2 float), "has_keypoints": [n] bool} plus the arrays named
        in `fields`: desc [rows, 32] uint8 (ORB) or [rows, 128] float32, xyz1 [rows, 4], kp_xy [rows, 2] (zeros for a node
        without keypoints), stats [rows] uint8.  Node i's rows are row_offsets[i] : row_offsets[i + 1] of each."""
        ids = np.ascontiguousarray(node_ids, np.int32).reshape(-1)
        unknown = set(fields) - {"desc", "xyz1", "kp_xy", "stats"}
        if unknown:
            raise ValueError("unknown fields: %s" % sorted(unknown))
        n = len(ids)
        off = np.zeros(n + 1, np.int64)
        kinds = np.zeros(n, np.int32)
        # sizing call: no array given, so any capacity serves and no device work happens; offsets and kinds come back
        self._check(self._L.rgbdfe_download_nodes(self._ctx, n, ids.ctypes.data, 2 ** 62, None, None, None, None, off.ctypes.data,
                                                  kinds.ctypes.data))
        rows = int(off[n])
        orb = n == 0 or (int(kinds[0]) & 0xff) == 0
        shapes = {"desc": ((rows, 32), np.uint8) if orb else ((rows, 128), np.float32), "xyz1": ((rows, 4), np.float32),
                  "kp_xy": ((rows, 2), np.float32), "stats": ((rows,), np.uint8)}
        out = {f: np.zeros(*shapes[f]) for f in fields}
        if rows and out:
            ptr = {f: (out[f].ctypes.data if f in out else None) for f in shapes}
            self._check(self._L.rgbdfe_download_nodes(self._ctx, n, ids.ctypes.data, rows, ptr["desc"], ptr["xyz1"], ptr["kp_xy"],
                                                      ptr["stats"], off.ctypes.data, kinds.ctypes.data))
        out["row_offsets"] = off
        out["kinds"] = kinds & 0xff
        out["has_keypoints"] = (kinds & _lib.RGBDFE_NODE_HAS_KEYPOINTS) != 0
        return out

    # -- session files (include/rgbdfe.h, "session files") -----------------------------------------
    def save_session(self, path, slam=None, graph=None, clouds=False):
        """rgbdfe_session_save: the resident nodes (features, keypoints, counters), the detector's state, with clouds=True the
        resident clouds, and the graph's and the Slam's byte strings when given.  The same state gives the same bytes."""
        self._check(self._L.rgbdfe_session_save(self._ctx, None if slam is None else slam._s, None if graph is None else graph._g,
                                                _lib.RGBDFE_SESSION_CLOUDS if clouds else 0, str(path).encode()))

    def load_session(self, path, slam=None, graph=None):
        """rgbdfe_session_load into this context and (when the file holds them) a fresh Slam and an empty PoseGraph: validated
        as a whole before anything changes.  RANSAC / matcher parameters are the caller's to set again (set_params)."""
        self._check(self._L.rgbdfe_session_load(self._ctx, None if slam is None else slam._s, None if graph is None else graph._g,
                                                str(path).encode()))
        if graph is not None:
            graph._sync_ids()
        with open(path, "rb") as f:   # the detector's max_keypoints sizes detect_describe's outputs on this side
            f.seek(80)                # header 32, CONF chunk 16 + 16, DETE chunk header 16: its payload, i32 type, i32 max_keypoints
            self._max_keypoints = int(np.frombuffer(f.read(8), np.int32)[1])

    def node_cloud_info(self, node_id) -> dict:
        """rows, cols, cloud_skip and the intrinsics (as the floats they are kept as) of a node's resident cloud."""
        v = np.zeros(8, np.float64)
        self._check(self._L.rgbdfe_node_cloud_info(self._ctx, int(node_id), v.ctypes.data))
        return dict(rows=int(v[0]), cols=int(v[1]), cloud_skip=int(v[2]), fx=float(v[3]), fy=float(v[4]), cx=float(v[5]), cy=float(v[6]))

    def restore_node_cloud(self, node_id, points, fx, fy, cx, cy, cloud_skip=1):
        """A resident cloud from node_cloud's points [rows, cols, 4] and node_cloud_info's fields."""
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 3 or pts.shape[2] != 4:
            raise ValueError("points must be [rows, cols, 4] float32")
        self._check(self._L.rgbdfe_restore_node_cloud(self._ctx, int(node_id), pts.ctypes.data, pts.shape[0], pts.shape[1],
                                                      float(fx), float(fy), float(cx), float(cy), int(cloud_skip)))

    def download_nodes_stats(self) -> dict:
        """The latest download_nodes call: kernel launches, device-to-host copies, bytes of the staging buffer, and whether the
        context's feature counters have been allocated."""
        v = np.zeros(4, np.int64)
        self._check(self._L.rgbdfe_download_nodes_stats(self._ctx, v.ctypes.data, len(v)))
        return {"launches": int(v[0]), "copies": int(v[1]), "staging_bytes": int(v[2]), "feature_stats_allocated": bool(v[3])}

    def update_inlier_features(self, d_records_ptr: int, query_ids, train_ids, accept) -> int:
        """updateInlierFeatures over n records in device memory for the pairs with accept != 0; returns the kernel launches."""
        q, t = np.ascontiguousarray(query_ids, np.int32), np.ascontiguousarray(train_ids, np.int32)
        a = np.ascontiguousarray(accept, np.uint8)
        launched = C.c_int32(0)
        self._check(self._L.rgbdfe_update_inlier_features(self._ctx, d_records_ptr, q.ctypes.data, t.ctypes.data, a.ctypes.data,
                                                          len(q), C.byref(launched)))
        return launched.value

    # -- the pair op ---------------------------------------------------------------
    def match_pair_list(self, query_ids: Sequence[int], train_ids: Sequence[int]) -> np.ndarray:
        """Batched Node::matchNodePair; returns a RESULT_DTYPE array (one record per pair)."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        if q.shape != t.shape or q.ndim != 1:
            raise ValueError("query_ids / train_ids must be 1-D and of equal length")
        out = np.zeros(q.shape[0], RESULT_DTYPE)
        self._check(self._L.rgbdfe_match_pair_list(self._ctx, q.ctypes.data, t.ctypes.data,
                                                   q.shape[0], out.ctypes.data))
        return out

    def match_node_pairs(self, new_node_id: int, candidate_ids: Sequence[int]) -> np.ndarray:
        """1:1 replacement of blockingMapped(nodes_to_comp, matchNodePair) (graph_manager.cpp:548)."""
        c = np.ascontiguousarray(candidate_ids, np.int32)
        out = np.zeros(c.shape[0], RESULT_DTYPE)
        self._check(self._L.rgbdfe_match_node_pairs(self._ctx, new_node_id, c.ctypes.data,
                                                    c.shape[0], out.ctypes.data))
        return out

    def match_pair_list_device(self, query_ids: np.ndarray, train_ids: np.ndarray,
                               d_out_ptr: int, stream: Optional[int] = None):
        """Asynchronous variant: results stay in HBM at d_out_ptr (n x sizeof(result))."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        self._check(self._L.rgbdfe_match_pair_list_device(self._ctx, q.ctypes.data, t.ctypes.data,
                                                          q.shape[0], d_out_ptr, stream))

    def submit_pair_list(self, query_ids: np.ndarray, train_ids: np.ndarray, d_out_ptr: int) -> int:
        """Pipelined variant: enqueue on an internal stream, return a ticket (see wait_ticket)."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        ticket = C.c_int64(0)
        self._check(self._L.rgbdfe_submit_pair_list(self._ctx, q.ctypes.data, t.ctypes.data,
                                                    q.shape[0], d_out_ptr, C.byref(ticket)))
        return ticket.value

    def wait_ticket(self, ticket: int, stream: Optional[int] = None):
        """Make `stream` (hipStream_t as int) wait for the batch, or block the host if None."""
        self._check(self._L.rgbdfe_wait_ticket(self._ctx, ticket, stream))

    def submit_pair_list_host(self, query_ids, train_ids, out: np.ndarray, inliers: bool = False) -> int:
        """rgbdfe_submit_pair_list_host: results into the HOST array `out` (RESULT_DTYPE records, or -- inliers=True -- a
        uint8 buffer for the batch's inlier stream); returns the ticket for wait_host.  `out` must stay alive and untouched
        until then; pinned arrays (host_register) are written by the download itself."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        if not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be contiguous")
        ticket = C.c_int64(0)
        self._check(self._L.rgbdfe_submit_pair_list_host(self._ctx, q.ctypes.data, t.ctypes.data, q.shape[0], out.ctypes.data,
                                                         out.nbytes, 1 if inliers else 0, C.byref(ticket)))
        return ticket.value

    def wait_host(self, ticket: int) -> int:
        """rgbdfe_wait_host: block until the job's results are in its `out`; returns the payload's size in bytes."""
        nb = C.c_int64(0)
        self._check(self._L.rgbdfe_wait_host(self._ctx, ticket, C.byref(nb)))
        return nb.value

    def wait_host_into(self, ticket: int, out) -> int:
        """rgbdfe_wait_host_into: collect a job whose payload did not fit its buffer into `out` (None: drop the job)."""
        nb = C.c_int64(0)
        if out is None:
            self._check(self._L.rgbdfe_wait_host_into(self._ctx, ticket, None, 0, C.byref(nb)))
            return 0
        if not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be contiguous")
        self._check(self._L.rgbdfe_wait_host_into(self._ctx, ticket, out.ctypes.data, out.nbytes, C.byref(nb)))
        return nb.value

    def synchronize(self):
        self._check(self._L.rgbdfe_synchronize(self._ctx))

    # -- per-frame feature path (Node::Node, node.cpp:139-210) ------------------------------
    def detector_configure(self, max_keypoints=600, grid_resolution=3, adjuster_max_iterations=5):
        """createDetector("ORB") (features.cpp:63-113): resets the per-cell FAST thresholds."""
        self._max_keypoints = max_keypoints
        self._check(self._L.rgbdfe_detector_configure(self._ctx, max_keypoints, grid_resolution,
                                                      adjuster_max_iterations))

    DETECTOR_TYPES = {"ORB": 0, "FAST": 1}

    def set_detector_type(self, name: str):
        """Parameter "feature_detector_type" with the default ORB extractor: "ORB" (the default) or "FAST"
        (rgbdfe_set_detector_type).  detect_describe(_batch), detect_describe_cloud and detector_thresholds follow it;
        the per-cell thresholds restart at 20, as a fresh createDetector does."""
        if name not in self.DETECTOR_TYPES:
            raise ValueError("feature_detector_type must be one of %s" % sorted(self.DETECTOR_TYPES))
        self._check(self._L.rgbdfe_set_detector_type(self._ctx, self.DETECTOR_TYPES[name]))

    def fast_detect(self, gray, mask, threshold, capacity=60000):
        """cv::FastFeatureDetector::create(threshold)->detect(gray, kps, mask) on the whole image (no grid).
        Raises RgbdfeError (RGBDFE_ERR_CAPACITY) when more than `capacity` keypoints are found."""
        gray = np.ascontiguousarray(gray, np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        kp = np.zeros(max(capacity, 1), _lib.KEYPOINT_DTYPE)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_fast_detect(self._ctx, gray.ctypes.data, None if m is None else m.ctypes.data,
                                               gray.shape[0], gray.shape[1], threshold, kp.ctypes.data, capacity,
                                               C.byref(n)))
        return kp[: n.value].copy()

    def detector_thresholds(self):
        t = np.zeros(64, np.float64)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_detector_thresholds(self._ctx, t.ctypes.data, C.byref(n)))
        return t[: n.value].copy()

    def detector_set_thresholds(self, thresholds):
        """The inverse of detector_thresholds (grid_resolution^2 values): all a grid detector carries between frames."""
        t = np.ascontiguousarray(thresholds, np.float64).reshape(-1)
        self._check(self._L.rgbdfe_detector_set_thresholds(self._ctx, t.ctypes.data, len(t)))

    def host_register(self, array):
        """Page-locks a numpy array's memory (rgbdfe_host_register): detect_describe then copies it to the device directly
        instead of through the library's staging buffer.  Keep the array alive and call host_unregister before freeing it."""
        self._check(self._L.rgbdfe_host_register(self._ctx, array.ctypes.data, array.nbytes))

    def host_unregister(self, array):
        self._check(self._L.rgbdfe_host_unregister(self._ctx, array.ctypes.data))

    def detect_describe(self, gray, mask, depth, fx, fy, cx, cy, depth_scaling=1.0):
        """detect -> removeDepthless -> retainBest -> compute -> projectTo3D for one frame.
        Returns (keypoints KEYPOINT_DTYPE, descriptors [n,32] uint8, xyz1 [n,4] float32)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        cap = getattr(self, "_max_keypoints", 600)
        kp = np.zeros(cap, _lib.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        xyz = np.zeros((cap, 4), np.float32)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_detect_describe(
            self._ctx, gray.ctypes.data, None if m is None else m.ctypes.data, depth.ctypes.data,
            gray.shape[0], gray.shape[1], fx, fy, cx, cy, depth_scaling, kp.ctypes.data, desc.ctypes.data,
            xyz.ctypes.data, C.byref(n)))
        return kp[: n.value].copy(), desc[: n.value].copy(), xyz[: n.value].copy()

    def set_feature_min_depth(self, on: bool):
        """Parameter "use_feature_min_depth" (parameter_server.cpp:90) for detect_describe(_batch)."""
        self._check(self._L.rgbdfe_set_feature_min_depth(self._ctx, 1 if on else 0))

    def project_to_3d_min_depth(self, kp_xy, kp_size, depth, fx, fy, cx, cy, depth_scaling=1.0, max_keypoints=1000):
        """projectTo3D with use_feature_min_depth (node.cpp:940): returns (kept_idx, xyz1)."""
        kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        kp_size = np.ascontiguousarray(kp_size, np.float32)
        depth = np.ascontiguousarray(depth, np.float32)
        n = kp_xy.shape[0]
        kept = np.zeros(max(n, 1), np.int32)
        xyz = np.zeros((max(n, 1), 4), np.float32)
        k = C.c_int32(0)
        self._check(self._L.rgbdfe_project_to_3d_min_depth(
            self._ctx, kp_xy.ctypes.data, kp_size.ctypes.data, n, depth.ctypes.data, depth.shape[0], depth.shape[1],
            fx, fy, cx, cy, depth_scaling, max_keypoints, kept.ctypes.data, xyz.ctypes.data, C.byref(k)))
        return kept[: k.value].copy(), xyz[: k.value].copy()

    def detect_describe_batch(self, grays, masks, depths, fx, fy, cx, cy, depth_scaling=1.0, node_ids=None, copy=True,
                              host_outputs=True):
        """A run of frames through the same detector state, in order (rgbdfe_detect_describe_batch): the results of
        calling detect_describe frame by frame, with frame k+1's upload overlapped with frame k's detection.
        Returns a list of (keypoints, descriptors, xyz1) per frame.  node_ids: frame f's features also become the resident
        node node_ids[f] (rgbdfe_detect_describe_batch_nodes; a negative id: no node).  copy=False returns views of the
        output arrays this object keeps and reuses for its next call (what an integration with its own buffers does;
        sift_detect_batch has the same switch): valid until then.  host_outputs=False (with node_ids, under the FAST
        detector): the features go to the nodes only and the per-frame counts are returned."""
        n = len(grays)
        if n == 0:
            return []
        g = [np.ascontiguousarray(x, np.uint8) for x in grays]
        d = [np.ascontiguousarray(x, np.float32) for x in depths]
        m = [None if (masks is None or masks[i] is None) else np.ascontiguousarray(masks[i], np.uint8) for i in range(n)]
        rows, cols = g[0].shape
        for a in g + d + [x for x in m if x is not None]:
            if a.shape != (rows, cols):
                raise ValueError("all frames of a batch share one size")
        cap = getattr(self, "_max_keypoints", 600)
        # the ABI's output arrays (n * cap rows each: 8.7 MB for 112 frames of 1024) are scratch of this object, kept between
        # calls of the same shape: fresh np.zeros arrays of that size are fresh mmap'ed pages every call, i.e. ~2000 page
        # faults inside the library's result copies (10 us per frame of a 640 x 480 run); what is returned are copies of the
        # rows in use
        with self._batch_lock:   # (the scratch is one per object)
            key = (n, cap)
            if getattr(self, "_batch_out_key", None) != key:
                self._batch_out = (np.zeros((n, cap), _lib.KEYPOINT_DTYPE), np.zeros((n, cap, 32), np.uint8),
                                   np.zeros((n, cap, 4), np.float32), np.zeros(n, np.int32))
                self._batch_out_key = key
            kp, desc, xyz, cnt = self._batch_out
            cnt[:] = 0
            vp = C.c_void_p * n
            pg = vp(*[x.ctypes.data for x in g])
            pd = vp(*[x.ctypes.data for x in d])
            pm = vp(*[None if x is None else x.ctypes.data for x in m])
            if node_ids is not None:
                ids = np.ascontiguousarray(node_ids, np.int32)
                if ids.shape != (n,):
                    raise ValueError("node_ids must hold one id per frame")
                outs = (kp.ctypes.data, desc.ctypes.data, xyz.ctypes.data) if host_outputs else (None, None, None)
                self._check(self._L.rgbdfe_detect_describe_batch_nodes(
                    self._ctx, n, C.cast(pg, C.c_void_p), C.cast(pm, C.c_void_p), C.cast(pd, C.c_void_p), rows, cols, fx, fy, cx, cy,
                    depth_scaling, cap, *outs, cnt.ctypes.data, ids.ctypes.data))
                if not host_outputs:
                    return cnt.copy()
            else:
                self._check(self._L.rgbdfe_detect_describe_batch(
                    self._ctx, n, C.cast(pg, C.c_void_p), C.cast(pm, C.c_void_p), C.cast(pd, C.c_void_p), rows, cols, fx, fy, cx, cy,
                    depth_scaling, cap, kp.ctypes.data, desc.ctypes.data, xyz.ctypes.data, cnt.ctypes.data))
            if not copy:
                return [(kp[f, : cnt[f]], desc[f, : cnt[f]], xyz[f, : cnt[f]]) for f in range(n)]
            return [(kp[f, : cnt[f]].copy(), desc[f, : cnt[f]].copy(), xyz[f, : cnt[f]].copy()) for f in range(n)]

    # ---- sensor frames: the images as the sensor messages carry them (include/rgbdfe.h, "sensor frames")
    @staticmethod
    def _sensor_frame(visual, depth, visual_encoding=None):
        """(rgbdfe_sensor_frame, the arrays it points into) of a visual image ([H, W] uint8 = mono8, [H, W, 3] uint8 = "rgb8" or
        "bgr8") and a depth image (float32 = 32FC1 metres, uint16 = 16UC1 millimetres).  Row strides are taken from the arrays;
        the pixels of a row must be contiguous."""
        v = np.asarray(visual)
        d = np.asarray(depth)
        if v.dtype != np.uint8 or v.ndim not in (2, 3) or (v.ndim == 3 and v.shape[2] != 3):
            raise ValueError("visual image: [H, W] or [H, W, 3] uint8")
        if d.ndim != 2 or d.dtype not in (np.dtype(np.float32), np.dtype(np.uint16)):
            raise ValueError("depth image: [H, W] float32 (metres) or uint16 (millimetres)")
        ch = 1 if v.ndim == 2 else 3
        if (v.ndim == 3 and v.strides[2] != 1) or v.strides[1] != ch or v.strides[0] < v.shape[1] * ch:
            v = np.ascontiguousarray(v)
        if d.strides[1] != d.itemsize or d.strides[0] < d.shape[1] * d.itemsize:
            d = np.ascontiguousarray(d)
        if ch == 1:
            enc = _lib.VISUAL_MONO8
        else:
            enc = {None: _lib.VISUAL_RGB8, "rgb8": _lib.VISUAL_RGB8, "bgr8": _lib.VISUAL_BGR8}[visual_encoding]
        fr = _lib.RgbdfeSensorFrame(
            v.ctypes.data, v.shape[0], v.shape[1], v.strides[0], enc,
            d.ctypes.data, d.shape[0], d.shape[1], d.strides[0], _lib.DEPTH_16UC1 if d.dtype == np.uint16 else _lib.DEPTH_32FC1)
        return fr, (v, d)

    def ingest_frame(self, visual, depth, visual_encoding=None, gray=True, mono8=True, depth_m=True):
        """The listener's and Node::Node's image preparation of one sensor frame on the device (rgbdfe_ingest_frame): returns
        (gray, mono8 mask, depth in metres) at the visual image's size; an output that is switched off is None."""
        fr, keep = self._sensor_frame(visual, depth, visual_encoding)
        shape = (fr.visual_rows, fr.visual_cols)
        g = np.zeros(shape, np.uint8) if gray else None
        m = np.zeros(shape, np.uint8) if mono8 else None
        dm = np.zeros(shape, np.float32) if depth_m else None
        self._check(self._L.rgbdfe_ingest_frame(self._ctx, C.byref(fr), None if g is None else g.ctypes.data,
                                                None if m is None else m.ctypes.data, None if dm is None else dm.ctypes.data))
        del keep
        return g, m, dm

    def sensor_detect_describe(self, visual, depth, fx, fy, cx, cy, depth_scaling=1.0, visual_encoding=None):
        """detect_describe on a sensor frame (rgbdfe_sensor_detect_describe): the results of detect_describe on the planes of
        ingest_frame.  Returns (keypoints KEYPOINT_DTYPE, descriptors [n,32] uint8, xyz1 [n,4] float32)."""
        fr, keep = self._sensor_frame(visual, depth, visual_encoding)
        cap = getattr(self, "_max_keypoints", 600)
        kp = np.zeros(cap, _lib.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        xyz = np.zeros((cap, 4), np.float32)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_sensor_detect_describe(self._ctx, C.byref(fr), fx, fy, cx, cy, depth_scaling, kp.ctypes.data,
                                                          desc.ctypes.data, xyz.ctypes.data, C.byref(n)))
        del keep
        return kp[: n.value].copy(), desc[: n.value].copy(), xyz[: n.value].copy()

    def sensor_detect_describe_batch_nodes(self, visuals, depths, fx, fy, cx, cy, depth_scaling=1.0, node_ids=None,
                                           visual_encoding=None, host_outputs=True, cloud_skip=None, cloud_encoding_bgr=False,
                                           cloud_min_depth=0.0):
        """detect_describe_batch on a run of sensor frames of one geometry (rgbdfe_sensor_detect_describe_batch_nodes).  Returns
        a list of (keypoints, descriptors, xyz1) per frame, or the per-frame counts with host_outputs=False (node_ids, FAST
        detector).  cloud_skip: frame f's structured cloud is also kept under node_ids[f] (upload_node_cloud's)."""
        n = len(visuals)
        if n == 0:
            return []
        built = [self._sensor_frame(visuals[i], depths[i], visual_encoding) for i in range(n)]
        frames = (_lib.RgbdfeSensorFrame * n)(*[b[0] for b in built])
        cap = getattr(self, "_max_keypoints", 600)
        kp = np.zeros((n, cap), _lib.KEYPOINT_DTYPE)
        desc = np.zeros((n, cap, 32), np.uint8)
        xyz = np.zeros((n, cap, 4), np.float32)
        cnt = np.zeros(n, np.int32)
        ids = None
        if node_ids is not None:
            ids = np.ascontiguousarray(node_ids, np.int32)
            if ids.shape != (n,):
                raise ValueError("node_ids must hold one id per frame")
        cloud = None
        if cloud_skip is not None:
            cloud = C.pointer(_lib.RgbdfeSensorCloud(int(cloud_skip), 1 if cloud_encoding_bgr else 0, float(cloud_min_depth)))
        outs = (kp.ctypes.data, desc.ctypes.data, xyz.ctypes.data) if host_outputs else (None, None, None)
        self._check(self._L.rgbdfe_sensor_detect_describe_batch_nodes(
            self._ctx, n, frames, fx, fy, cx, cy, depth_scaling, cap, *outs, cnt.ctypes.data,
            None if ids is None else ids.ctypes.data, cloud))
        del built
        if not host_outputs:
            return cnt.copy()
        return [(kp[f, : cnt[f]].copy(), desc[f, : cnt[f]].copy(), xyz[f, : cnt[f]].copy()) for f in range(n)]

    def orb_detect(self, gray, mask, fast_threshold, capacity=60000):
        """cv::ORB::create(10000,1.2,8,15,0,2,HARRIS,31,thr)->detect(gray, kps, mask) (feature_adjuster.cpp:94).
        Raises RgbdfeError (RGBDFE_ERR_CAPACITY) when more than `capacity` keypoints are found."""
        gray = np.ascontiguousarray(gray, np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        kp = np.zeros(capacity, _lib.KEYPOINT_DTYPE)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_orb_detect(self._ctx, gray.ctypes.data, None if m is None else m.ctypes.data,
                                              gray.shape[0], gray.shape[1], fast_threshold, kp.ctypes.data,
                                              capacity, C.byref(n)))
        return kp[: n.value].copy()

    def orb_compute(self, gray, keypoints):
        """cv::ORB::create()->compute(gray, kps, desc) (features.cpp:117-119)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        kp = np.ascontiguousarray(keypoints.copy())
        desc = np.zeros((max(len(kp), 1), 32), np.uint8)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_orb_compute(self._ctx, gray.ctypes.data, gray.shape[0], gray.shape[1],
                                               kp.ctypes.data, len(kp), desc.ctypes.data, C.byref(n)))
        return kp[: n.value].copy(), desc[: n.value].copy()

    # -- SIFT (128-d float descriptors, matcher_type == SIFTGPU) ---------------------------
    def sift_detect(self, gray, mask=None, max_keypoints: int = 1000):
        """SiftGPUWrapper::detect (sift_gpu_wrapper.cpp:113-167): (keypoints KEYPOINT_DTYPE [n], descriptors [n, 128] f32,
        unnormalised) of a mono8 image.  `mask` is ignored, as in the reference."""
        gray = np.ascontiguousarray(gray, np.uint8)
        rows, cols = gray.shape
        cap = min(max(2 * int(max_keypoints) + 4096, 8192), 1 << 16)
        max_keypoints = min(int(max_keypoints), (1 << 31) - 1)
        while True:
            kp = np.zeros(cap, _lib.KEYPOINT_DTYPE)
            desc = np.zeros((cap, 128), np.float32)
            n = C.c_int32(0)
            st = self._L.rgbdfe_sift_detect(self._ctx, gray.ctypes.data, None, rows, cols, int(max_keypoints), kp.ctypes.data,
                                            desc.ctypes.data, cap, C.byref(n))
            if st == -5 and n.value > cap:        # RGBDFE_ERR_CAPACITY: *n_out = the number of features
                cap = n.value + 64
                continue
            self._check(st)
            return kp[: n.value].copy(), desc[: n.value].copy()

    def sift_describe(self, gray, keypoints):
        """SiftGPUWrapper::detect with a given keypoint list (sift_gpu_wrapper.cpp:132-142): descriptors at the keypoints'
        positions, sizes and angles.  Returns (keypoints as the wrapper rebuilds them, descriptors [n, 128])."""
        gray = np.ascontiguousarray(gray, np.uint8)
        kp = np.ascontiguousarray(keypoints.copy())
        n = len(kp)
        desc = np.zeros((max(n, 1), 128), np.float32)
        self._check(self._L.rgbdfe_sift_describe(self._ctx, gray.ctypes.data, gray.shape[0], gray.shape[1], kp.ctypes.data, n,
                                                 desc.ctypes.data))
        return kp, desc[:n]

    def sift_detect_batch(self, grays, max_keypoints: int = 1000, out_stride=None, copy=True):
        """rgbdfe_sift_detect_batch: sift_detect over a run of frames of one size, up to 8 frames per launch chain.
        Returns a list of (keypoints, descriptors) per frame.  copy=False returns views of output arrays this object keeps
        and reuses for the next call of the same shape (what an integration with its own buffers does)."""
        n = len(grays)
        if n == 0:
            return []
        g = [np.ascontiguousarray(x, np.uint8) for x in grays]
        rows, cols = g[0].shape
        for a in g:
            if a.shape != (rows, cols):
                raise ValueError("all frames of a batch share one size")
        max_keypoints = min(int(max_keypoints), (1 << 31) - 1)
        stride = int(out_stride) if out_stride else min(2 * max_keypoints + 1024, 1 << 16)
        while True:
            cache = getattr(self, "_sift_out", None)
            if copy or cache is None or cache[0] != (n, stride):
                kp = np.zeros((n, stride), _lib.KEYPOINT_DTYPE)
                desc = np.zeros((n, stride, 128), np.float32)
                if not copy:
                    self._sift_out = ((n, stride), kp, desc)
            else:
                kp, desc = cache[1], cache[2]
            cnt = np.zeros(n, np.int32)
            pg = (C.c_void_p * n)(*[x.ctypes.data for x in g])
            rc = self._L.rgbdfe_sift_detect_batch(self._ctx, n, C.cast(pg, C.c_void_p), rows, cols, max_keypoints, stride,
                                                  kp.ctypes.data, desc.ctypes.data, cnt.ctypes.data)
            if rc == -5 and int(cnt.max()) > stride and not out_stride:   # RGBDFE_ERR_CAPACITY: cnt holds the counts
                stride = int(cnt.max())
                continue
            self._check(rc)
            if not copy:
                return [(kp[f, : cnt[f]], desc[f, : cnt[f]]) for f in range(n)]
            return [(kp[f, : cnt[f]].copy(), desc[f, : cnt[f]].copy()) for f in range(n)]

    def sift_detect_batch_nodes(self, grays, depths, fx, fy, cx, cy, node_ids, depth_scaling=1.0, max_keypoints: int = 1000,
                                use_root_sift=True, return_features=True, copy=True):
        """rgbdfe_sift_detect_batch_nodes: Node::Node's SIFTGPU branch over a run of frames of one size -- SIFT extraction,
        projectTo3DSiftGPU and RootSIFT -- with frame f's features becoming the resident float node node_ids[f] (a negative
        id: no node) without passing through the host.  The nodes equal sift_detect_batch -> sift_node_features ->
        upload_float_node.  Returns per frame (keypoints, xyz1, feature_descriptors), or only the counts (an int32 array)
        when return_features is False (no host outputs: nothing but the counts comes back).  copy=False returns views of
        output arrays this object keeps and reuses for the next call of the same shape."""
        n = len(grays)
        if n == 0:
            return [] if return_features else np.zeros(0, np.int32)
        g = [np.ascontiguousarray(x, np.uint8) for x in grays]
        d = [np.ascontiguousarray(x, np.float32) for x in depths]
        rows, cols = g[0].shape
        if len(d) != n:
            raise ValueError("one depth image per frame")
        for a in g + d:
            if a.shape != (rows, cols):
                raise ValueError("all frames of a batch share one size")
        ids = np.ascontiguousarray(node_ids, np.int32)
        if ids.shape != (n,):
            raise ValueError("node_ids must hold one id per frame")
        max_keypoints = int(max_keypoints)
        vp = C.c_void_p * n
        pg = vp(*[x.ctypes.data for x in g])
        pd = vp(*[x.ctypes.data for x in d])
        cnt = np.zeros(n, np.int32)
        if not return_features:
            self._check(self._L.rgbdfe_sift_detect_batch_nodes(
                self._ctx, n, C.cast(pg, C.c_void_p), C.cast(pd, C.c_void_p), rows, cols, fx, fy, cx, cy, depth_scaling,
                max_keypoints, int(bool(use_root_sift)), ids.ctypes.data, 0, None, None, None, cnt.ctypes.data))
            return cnt
        stride = max(max_keypoints, 1)   # a frame keeps at most max_keypoints rows
        cache = getattr(self, "_sift_nodes_out", None)
        if copy or cache is None or cache[0] != (n, stride):
            kp = np.zeros((n, stride), _lib.KEYPOINT_DTYPE)
            xyz = np.zeros((n, stride, 4), np.float32)
            feat = np.zeros((n, stride, 128), np.float32)
            if not copy:
                self._sift_nodes_out = ((n, stride), kp, xyz, feat)
        else:
            kp, xyz, feat = cache[1], cache[2], cache[3]
        self._check(self._L.rgbdfe_sift_detect_batch_nodes(
            self._ctx, n, C.cast(pg, C.c_void_p), C.cast(pd, C.c_void_p), rows, cols, fx, fy, cx, cy, depth_scaling,
            max_keypoints, int(bool(use_root_sift)), ids.ctypes.data, stride, kp.ctypes.data, xyz.ctypes.data,
            feat.ctypes.data, cnt.ctypes.data))
        if not copy:
            return [(kp[f, : cnt[f]], xyz[f, : cnt[f]], feat[f, : cnt[f]]) for f in range(n)]
        return [(kp[f, : cnt[f]].copy(), xyz[f, : cnt[f]].copy(), feat[f, : cnt[f]].copy()) for f in range(n)]

    def _detector_max_total(self):
        return int(1.5 * getattr(self, "_max_keypoints", 600))

    def detect(self, gray, mask=None, capacity=None):
        """rgbdfe_detect: detector->detect alone (node.cpp:160) -- the grid detector's aggregate, in aggregate order, before
        removeDepthless; the per-cell thresholds advance as in detect_describe.  capacity defaults to max_total =
        floor(1.5 * max_keypoints), the aggregate's bound; less is refused (RGBDFE_ERR_INVALID_ARG)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        cap = self._detector_max_total() if capacity is None else int(capacity)
        kp = np.zeros(max(cap, 1), _lib.KEYPOINT_DTYPE)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_detect(self._ctx, gray.ctypes.data, None if m is None else m.ctypes.data, gray.shape[0],
                                          gray.shape[1], kp.ctypes.data, cap, C.byref(n)))
        return kp[: n.value].copy()

    def detect_sift_describe(self, gray, mask, depth, fx, fy, cx, cy, depth_scaling=1.0, use_root_sift=True):
        """rgbdfe_detect_sift_describe: Node::Node with feature_detector_type ORB / FAST (the context's detector type) and
        feature_extractor_type SIFTGPU for one frame -- detect -> projectTo3D -> SiftGPU descriptors at the kept keypoints ->
        projectTo3DSiftGPU (+ RootSIFT).  A frame whose keypoints all lack depth gets SiftGPU's own detection (the wrapper's
        empty-list behaviour).  Returns (keypoints, xyz1 [n,4], siftgpu_descriptors [n,128], feature_descriptors [n,128])."""
        gray = np.ascontiguousarray(gray, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        cap = max(getattr(self, "_max_keypoints", 600), 1)
        kp = np.zeros(cap, _lib.KEYPOINT_DTYPE)
        xyz = np.zeros((cap, 4), np.float32)
        raw = np.zeros((cap, 128), np.float32)
        feat = np.zeros((cap, 128), np.float32)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_detect_sift_describe(
            self._ctx, gray.ctypes.data, None if m is None else m.ctypes.data, depth.ctypes.data, gray.shape[0], gray.shape[1],
            fx, fy, cx, cy, depth_scaling, int(bool(use_root_sift)), kp.ctypes.data, xyz.ctypes.data, raw.ctypes.data,
            feat.ctypes.data, C.byref(n)))
        k = n.value
        return kp[:k].copy(), xyz[:k].copy(), raw[:k].copy(), feat[:k].copy()

    def detect_sift_describe_batch_nodes(self, grays, masks, depths, fx, fy, cx, cy, node_ids, depth_scaling=1.0,
                                         use_root_sift=True, return_features=True):
        """rgbdfe_detect_sift_describe_batch_nodes: detect_sift_describe over a run of frames of one size (the thresholds
        carry over), frame f's features becoming the float node node_ids[f] (a negative id: no node).  masks may be None or
        hold None entries.  Returns per frame (keypoints, xyz1, feature_descriptors), or only the counts (an int32 array)
        when return_features is False (no host outputs)."""
        n = len(grays)
        if n == 0:
            return [] if return_features else np.zeros(0, np.int32)
        g = [np.ascontiguousarray(x, np.uint8) for x in grays]
        d = [np.ascontiguousarray(x, np.float32) for x in depths]
        rows, cols = g[0].shape
        if len(d) != n or (masks is not None and len(masks) != n):
            raise ValueError("one depth image (and mask, when given) per frame")
        ms = [None] * n if masks is None else [None if x is None else np.ascontiguousarray(x, np.uint8) for x in masks]
        for a in g + d + [x for x in ms if x is not None]:
            if a.shape != (rows, cols):
                raise ValueError("all frames of a batch share one size")
        ids = np.ascontiguousarray(node_ids, np.int32)
        if ids.shape != (n,):
            raise ValueError("node_ids must hold one id per frame")
        vp = C.c_void_p * n
        pg = vp(*[x.ctypes.data for x in g])
        pd = vp(*[x.ctypes.data for x in d])
        pm = vp(*[None if x is None else x.ctypes.data for x in ms])
        stride = max(getattr(self, "_max_keypoints", 600), 1)
        cnt = np.zeros(n, np.int32)
        args = (self._ctx, n, C.cast(pg, C.c_void_p), C.cast(pm, C.c_void_p), C.cast(pd, C.c_void_p), rows, cols, fx, fy, cx,
                cy, depth_scaling, int(bool(use_root_sift)), ids.ctypes.data, stride)
        if not return_features:
            self._check(self._L.rgbdfe_detect_sift_describe_batch_nodes(*args, None, None, None, cnt.ctypes.data))
            return cnt
        kp = np.zeros((n, stride), _lib.KEYPOINT_DTYPE)
        xyz = np.zeros((n, stride, 4), np.float32)
        feat = np.zeros((n, stride, 128), np.float32)
        self._check(self._L.rgbdfe_detect_sift_describe_batch_nodes(*args, kp.ctypes.data, xyz.ctypes.data, feat.ctypes.data,
                                                                    cnt.ctypes.data))
        return [(kp[f, : cnt[f]].copy(), xyz[f, : cnt[f]].copy(), feat[f, : cnt[f]].copy()) for f in range(n)]

    def sift_detect_orb_describe(self, gray, depth, fx, fy, cx, cy, depth_scaling=1.0, max_keypoints: int = 1000):
        """rgbdfe_sift_detect_orb_describe: Node::Node with feature_detector_type SIFTGPU and feature_extractor_type ORB for one
        frame -- SiftGPU's own detection, removeDepthless, the max_keypoints cut, cv::ORB::compute, projectTo3D.  Returns
        (keypoints, descriptors [n, 32] uint8, xyz1 [n, 4])."""
        gray = np.ascontiguousarray(gray, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        cap = max(int(max_keypoints), 1)
        kp = np.zeros(cap, _lib.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        xyz = np.zeros((cap, 4), np.float32)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_sift_detect_orb_describe(
            self._ctx, gray.ctypes.data, depth.ctypes.data, gray.shape[0], gray.shape[1], fx, fy, cx, cy, depth_scaling,
            int(max_keypoints), kp.ctypes.data, desc.ctypes.data, xyz.ctypes.data, C.byref(n)))
        k = n.value
        return kp[:k].copy(), desc[:k].copy(), xyz[:k].copy()

    def sift_detect_orb_describe_batch_nodes(self, grays, depths, fx, fy, cx, cy, node_ids, depth_scaling=1.0,
                                             max_keypoints: int = 1000, return_features=True):
        """rgbdfe_sift_detect_orb_describe_batch_nodes: sift_detect_orb_describe over a run of frames of one size, frame f's
        features becoming the ORB node node_ids[f] (a negative id: no node).  Returns per frame (keypoints, descriptors,
        xyz1), or only the counts (an int32 array) when return_features is False (no host outputs)."""
        n = len(grays)
        if n == 0:
            return [] if return_features else np.zeros(0, np.int32)
        g = [np.ascontiguousarray(x, np.uint8) for x in grays]
        d = [np.ascontiguousarray(x, np.float32) for x in depths]
        rows, cols = g[0].shape
        if len(d) != n:
            raise ValueError("one depth image per frame")
        for a in g + d:
            if a.shape != (rows, cols):
                raise ValueError("all frames of a batch share one size")
        ids = np.ascontiguousarray(node_ids, np.int32)
        if ids.shape != (n,):
            raise ValueError("node_ids must hold one id per frame")
        vp = C.c_void_p * n
        pg = vp(*[x.ctypes.data for x in g])
        pd = vp(*[x.ctypes.data for x in d])
        cnt = np.zeros(n, np.int32)
        args = (self._ctx, n, C.cast(pg, C.c_void_p), C.cast(pd, C.c_void_p), rows, cols, fx, fy, cx, cy, depth_scaling,
                int(max_keypoints), ids.ctypes.data)
        if not return_features:
            self._check(self._L.rgbdfe_sift_detect_orb_describe_batch_nodes(*args, 0, None, None, None, cnt.ctypes.data))
            return cnt
        stride = max(int(max_keypoints), 1)
        kp = np.zeros((n, stride), _lib.KEYPOINT_DTYPE)
        desc = np.zeros((n, stride, 32), np.uint8)
        xyz = np.zeros((n, stride, 4), np.float32)
        self._check(self._L.rgbdfe_sift_detect_orb_describe_batch_nodes(*args, stride, kp.ctypes.data, desc.ctypes.data,
                                                                        xyz.ctypes.data, cnt.ctypes.data))
        return [(kp[f, : cnt[f]].copy(), desc[f, : cnt[f]].copy(), xyz[f, : cnt[f]].copy()) for f in range(n)]

    def sift_geometry(self):
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.rgbdfe_sift_geometry(self._ctx, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(octave_min=a.value, octave_num=b.value, levels=c.value, dog_levels=d.value)

    def sift_debug_plane(self, octave: int, level: int) -> np.ndarray:
        """A Gaussian plane [h, w] of the latest sift_detect frame (tests)."""
        buf = np.zeros(1 << 25, np.float32)
        w, h = C.c_int32(), C.c_int32()
        self._check(self._L.rgbdfe_sift_debug_plane(self._ctx, octave, level, buf.ctypes.data, buf.size, C.byref(w),
                                                    C.byref(h)))
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

    def sift_debug_candidates(self, octave: int, dog_level: int) -> np.ndarray:
        """The keypoint candidates [n, 6] = (x, y, sign, dx, dy, ds) of one (octave, dog level), list order (tests)."""
        buf = np.zeros((1 << 20, 6), np.float32)
        n = C.c_int32()
        self._check(self._L.rgbdfe_sift_debug_candidates(self._ctx, octave, dog_level, buf.ctypes.data, buf.shape[0],
                                                         C.byref(n)))
        return buf[: n.value].copy()

    def upload_nodes(self, node_ids, descs, xyz1s):
        """rgbdfe_upload_nodes: upload_node for a list of nodes in one call (one wait, pinned staging)."""
        n = len(node_ids)
        d = [np.ascontiguousarray(x, np.uint8) for x in descs]
        p = [np.ascontiguousarray(x, np.float32) for x in xyz1s]
        for a, b in zip(d, p):
            if a.ndim != 2 or a.shape[1] != 32 or b.shape != (a.shape[0], 4):
                raise ValueError("desc must be [n,32] uint8 and xyz1 [n,4] float32")
        ids = np.ascontiguousarray(node_ids, np.int32)
        cnt = np.array([a.shape[0] for a in d], np.int32)
        vp = C.c_void_p * max(n, 1)
        pd = vp(*[a.ctypes.data for a in d])
        pp = vp(*[b.ctypes.data for b in p])
        self._check(self._L.rgbdfe_upload_nodes(self._ctx, n, ids.ctypes.data, C.cast(pd, C.c_void_p), C.cast(pp, C.c_void_p),
                                                cnt.ctypes.data))

    def upload_sift_node(self, node_id: int, desc128: np.ndarray, xyz1: np.ndarray):
        desc128 = np.ascontiguousarray(desc128, np.float32)
        xyz1 = np.ascontiguousarray(xyz1, np.float32)
        n = desc128.shape[0]
        if desc128.ndim != 2 or desc128.shape[1] != 128 or xyz1.shape != (n, 4):
            raise ValueError("desc128 must be [n,128] float32 and xyz1 [n,4] float32")
        self._check(self._L.rgbdfe_upload_sift_node(self._ctx, node_id, desc128.ctypes.data,
                                                    xyz1.ctypes.data, n))

    def match_sift_pair_list(self, query_ids, train_ids):
        """Batched matchNodePair for SIFT nodes; returns (records, all_dist [n, 320] float32)."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        out = np.zeros(q.shape[0], RESULT_DTYPE)
        dist = np.zeros((q.shape[0], _lib.RGBDFE_MAX_MATCHES), np.float32)
        self._check(self._L.rgbdfe_match_sift_pair_list(self._ctx, q.ctypes.data, t.ctypes.data,
                                                        q.shape[0], out.ctypes.data, dist.ctypes.data))
        return out, dist

    def upload_float_node(self, node_id: int, desc: np.ndarray, xyz1: np.ndarray):
        """Node::feature_descriptors_ (N x dim CV_32F) for the FLANN branch (node.cpp:610-667)."""
        desc = np.ascontiguousarray(desc, np.float32)
        xyz1 = np.ascontiguousarray(xyz1, np.float32)
        n = desc.shape[0]
        if desc.ndim != 2 or xyz1.shape != (n, 4):
            raise ValueError("desc must be [n, dim] float32 and xyz1 [n, 4] float32")
        self._check(self._L.rgbdfe_upload_float_node(self._ctx, node_id, desc.ctypes.data, desc.shape[1],
                                                     xyz1.ctypes.data, n))

    def match_flann_pair_list(self, query_ids, train_ids, nn_distance_ratio: float = 0.95):
        """Batched matchNodePair on the FLANN branch with exact neighbours; returns (records, ratios [n, 320])."""
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        out = np.zeros(q.shape[0], RESULT_DTYPE)
        dist = np.zeros((q.shape[0], _lib.RGBDFE_MAX_MATCHES), np.float32)
        self._check(self._L.rgbdfe_match_flann_pair_list(self._ctx, q.ctypes.data, t.ctypes.data, q.shape[0],
                                                         nn_distance_ratio, out.ctypes.data, dist.ctypes.data))
        return out, dist

    def submit_sift_pair_list(self, query_ids, train_ids, d_out_ptr: int, d_dist_ptr: Optional[int] = None) -> int:
        q = np.ascontiguousarray(query_ids, np.int32)
        t = np.ascontiguousarray(train_ids, np.int32)
        ticket = C.c_int64(0)
        self._check(self._L.rgbdfe_submit_sift_pair_list(self._ctx, q.ctypes.data, t.ctypes.data,
                                                         q.shape[0], d_out_ptr, d_dist_ptr,
                                                         C.byref(ticket)))
        return ticket.value

    def sift_match_nodes(self, query_id: int, train_id: int):
        """SiftGPUWrapper::match twin (sift_gpu_wrapper.cpp:169-227): (queryIdx, trainIdx, L2)."""
        n = max(self.node_count(query_id), 1)
        mq = np.empty(n, np.int32)
        mt = np.empty(n, np.int32)
        md = np.empty(n, np.float32)
        k = C.c_int32(0)
        self._check(self._L.rgbdfe_sift_match_nodes(self._ctx, query_id, train_id, mq.ctypes.data,
                                                    mt.ctypes.data, md.ctypes.data, C.byref(k)))
        return mq[: k.value].copy(), mt[: k.value].copy(), md[: k.value].copy()

    def place_recognition(self, query_id: int, candidate_ids, k_neighbours: int = 2, max_hd: int = 128,
                          max_out: Optional[int] = None):
        """Descriptor-vote ranking of loop-closure candidates (loop_closing.cpp:190-277 with exact neighbours).
        Returns (ids, scores) in descending score order."""
        c = np.ascontiguousarray(candidate_ids, np.int32)
        max_out = len(c) if max_out is None else max_out
        ids = np.zeros(max(max_out, 1), np.int32)
        sc = np.zeros(max(max_out, 1), np.float32)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_place_recognition(self._ctx, query_id, c.ctypes.data, len(c), k_neighbours, max_hd,
                                                     max_out, ids.ctypes.data, sc.ctypes.data, C.byref(n)))
        return ids[: n.value].copy(), sc[: n.value].copy()

    def place_recognition_batch(self, query_ids, candidate_lists, k_neighbours: int = 2, max_hd: int = 128,
                                max_out: int = 16):
        """Many queries in one launch.  candidate_lists[s] = the candidate ids of query_ids[s].
        Returns a list of (ids, scores) per query."""
        qs = np.ascontiguousarray(query_ids, np.int32)
        offs = np.zeros(len(qs) + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in candidate_lists])
        cands = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32) for c in candidate_lists])
                                     if len(candidate_lists) else np.zeros(0, np.int32), np.int32)
        ids = np.zeros((max(len(qs), 1), max(max_out, 1)), np.int32)
        sc = np.zeros((max(len(qs), 1), max(max_out, 1)), np.float32)
        cnt = np.zeros(max(len(qs), 1), np.int32)
        self._check(self._L.rgbdfe_place_recognition_batch(self._ctx, qs.ctypes.data, len(qs), offs.ctypes.data,
                                                           cands.ctypes.data, k_neighbours, max_hd, max_out,
                                                           ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data))
        return [(ids[s, : cnt[s]].copy(), sc[s, : cnt[s]].copy()) for s in range(len(qs))]

    # -- pieces -----------------------------------------------------------------------
    def hamming_nn_nodes(self, query_id: int, train_id: int):
        n = self.node_count(query_id)
        if n < 0:
            raise RgbdfeError("unknown node id")
        hd = np.empty(n, np.int32)
        idx = np.empty(n, np.int32)
        self._check(self._L.rgbdfe_hamming_nn_nodes(self._ctx, query_id, train_id,
                                                    hd.ctypes.data, idx.ctypes.data))
        return hd, idx

    def bruteForceSearchORB_batch(self, qdesc: np.ndarray, tdesc: np.ndarray):
        """Every row of qdesc through bruteForceSearchORB(row, tdesc, len(tdesc)) (features.h:14)."""
        qdesc = np.ascontiguousarray(qdesc, np.uint8)
        tdesc = np.ascontiguousarray(tdesc, np.uint8)
        hd = np.empty(qdesc.shape[0], np.int32)
        idx = np.empty(qdesc.shape[0], np.int32)
        self._check(self._L.rgbdfe_hamming_nn_host(self._ctx, qdesc.ctypes.data, qdesc.shape[0],
                                                   tdesc.ctypes.data, tdesc.shape[0],
                                                   hd.ctypes.data, idx.ctypes.data))
        return hd, idx

    def project_to_3d(self, kp_xy, depth, fx, fy, cx, cy, depth_scaling=1.0, max_keypoints=1000):
        """removeDepthless + projectTo3D (node.cpp:67-97, 900-965)."""
        kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        depth = np.ascontiguousarray(depth, np.float32)
        n = kp_xy.shape[0]
        kept = np.empty(max(n, 1), np.int32)
        xyz1 = np.empty((max(n, 1), 4), np.float32)
        n_out = C.c_int32(0)
        self._check(self._L.rgbdfe_project_to_3d(
            self._ctx, kp_xy.ctypes.data, n, depth.ctypes.data, depth.shape[0], depth.shape[1],
            fx, fy, cx, cy, depth_scaling, max_keypoints, kept.ctypes.data, xyz1.ctypes.data,
            C.byref(n_out)))
        return kept[: n_out.value].copy(), xyz1[: n_out.value].copy()

    def project_to_3d_cloud(self, kp_xy, cloud, maximum_depth, max_keypoints=1000):
        """Node::projectTo3D, point-cloud overload (node.cpp:855-898).  cloud: [rows, cols, 4] float32."""
        kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        cloud = np.ascontiguousarray(cloud, np.float32)
        n = kp_xy.shape[0]
        kept = np.empty(max(n, 1), np.int32)
        xyz1 = np.empty((max(n, 1), 4), np.float32)
        n_out = C.c_int32(0)
        self._check(self._L.rgbdfe_project_to_3d_cloud(self._ctx, kp_xy.ctypes.data, n, cloud.ctypes.data, cloud.shape[0],
                                                       cloud.shape[1], maximum_depth, max_keypoints, kept.ctypes.data,
                                                       xyz1.ctypes.data, C.byref(n_out)))
        return kept[: n_out.value].copy(), xyz1[: n_out.value].copy()

    def detect_describe_cloud(self, gray, mask, cloud, maximum_depth):
        """The feature path of the Node constructor that is given the organised cloud (node.cpp:252-369)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        cloud = np.ascontiguousarray(cloud, np.float32)
        cap = int(1.5 * getattr(self, "_max_keypoints", 600)) + 64
        kps = np.zeros(cap, _lib.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        xyz = np.zeros((cap, 4), np.float32)
        n = C.c_int32(0)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._check(self._L.rgbdfe_detect_describe_cloud(self._ctx, gray.ctypes.data, None if m is None else m.ctypes.data,
                                                         cloud.ctypes.data, gray.shape[0], gray.shape[1], maximum_depth,
                                                         kps.ctypes.data, desc.ctypes.data, xyz.ctypes.data, C.byref(n)))
        return kps[: n.value].copy(), desc[: n.value].copy(), xyz[: n.value].copy()

    def sift_node_features(self, kp_xy, desc, depth, fx, fy, cx, cy, depth_scaling=1.0, max_keypoints=1000,
                           use_root_sift=True, kp_size=None):
        """projectTo3DSiftGPU (node.cpp:695-769) + squareroot_descriptor_space (node.cpp:1557-1571):
        returns (kept_idx, xyz1, siftgpu_descriptors, feature_descriptors).  kp_size (cv::KeyPoint::size per keypoint)
        selects the use_feature_min_depth variant (node.cpp:727-731)."""
        kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        desc = np.ascontiguousarray(desc, np.float32)
        depth = np.ascontiguousarray(depth, np.float32)
        n = kp_xy.shape[0]
        if desc.shape != (n, 128):
            raise ValueError("desc must be n_kp x 128 float32")
        cap = max(min(n, max_keypoints), 1)
        kept = np.empty(cap, np.int32)
        xyz1 = np.empty((cap, 4), np.float32)
        raw = np.empty((cap, 128), np.float32)
        feat = np.empty((cap, 128), np.float32)
        n_out = C.c_int32(0)
        if kp_size is not None:
            kp_size = np.ascontiguousarray(kp_size, np.float32).reshape(-1)
            if kp_size.shape[0] != n:
                raise ValueError("kp_size must hold one size per keypoint")
            self._check(self._L.rgbdfe_sift_node_features_min_depth(
                self._ctx, kp_xy.ctypes.data, kp_size.ctypes.data, n, desc.ctypes.data, depth.ctypes.data, depth.shape[0],
                depth.shape[1], fx, fy, cx, cy, depth_scaling, max_keypoints, int(bool(use_root_sift)),
                kept.ctypes.data, xyz1.ctypes.data, raw.ctypes.data, feat.ctypes.data, C.byref(n_out)))
        else:
            self._check(self._L.rgbdfe_sift_node_features(
                self._ctx, kp_xy.ctypes.data, n, desc.ctypes.data, depth.ctypes.data, depth.shape[0],
                depth.shape[1], fx, fy, cx, cy, depth_scaling, max_keypoints, int(bool(use_root_sift)),
                kept.ctypes.data, xyz1.ctypes.data, raw.ctypes.data, feat.ctypes.data, C.byref(n_out)))
        k = n_out.value
        return kept[:k].copy(), xyz1[:k].copy(), raw[:k].copy(), feat[:k].copy()

    # -- frame-level data either side of the pair path ------
    def depth_to_mono8(self, depth):
        """depthToCV8UC1 (misc.cpp:414-430).  float32 metres -> mono8; uint16 millimetres -> (mono8, metres)."""
        depth = np.ascontiguousarray(depth)
        rows, cols = depth.shape
        mono8 = np.empty((rows, cols), np.uint8)
        if depth.dtype == np.uint16:
            dm = np.empty((rows, cols), np.float32)
            self._check(self._L.rgbdfe_depth_to_mono8(self._ctx, depth.ctypes.data, 1, rows, cols,
                                                      mono8.ctypes.data, dm.ctypes.data))
            return mono8, dm
        depth = np.ascontiguousarray(depth, np.float32)
        self._check(self._L.rgbdfe_depth_to_mono8(self._ctx, depth.ctypes.data, 0, rows, cols,
                                                  mono8.ctypes.data, None))
        return mono8

    def upload_node_cloud(self, node_id, depth, fx, fy, cx, cy, rgb=None, encoding_bgr=False, depth_scaling=1.0,
                          min_depth=0.1, cloud_skip=2, return_cloud=False):
        """createXYZRGBPointCloud (misc.cpp:467-556): builds and keeps the node's structured cloud."""
        depth = np.ascontiguousarray(depth, np.float32)
        rows, cols = depth.shape
        ch = 0
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, np.uint8)
            ch = 1 if rgb.ndim == 2 else rgb.shape[2]
            if rgb.shape[:2] != (rows, cols):
                raise ValueError("rgb and depth must have the same size")
        out = np.empty((rows // cloud_skip, cols // cloud_skip, 4), np.float32) if return_cloud else None
        self._check(self._L.rgbdfe_upload_node_cloud(
            self._ctx, int(node_id), depth.ctypes.data, rows, cols, rgb.ctypes.data if rgb is not None else None,
            ch, int(bool(encoding_bgr)), fx, fy, cx, cy, depth_scaling, min_depth, int(cloud_skip),
            out.ctypes.data if out is not None else None))
        return out

    def release_node_cloud(self, node_id):
        self._check(self._L.rgbdfe_release_node_cloud(self._ctx, int(node_id)))

    def node_cloud(self, node_id):
        """The node's resident structured cloud, rows x cols x 4 float32 (x, y, z, rgb bits): what upload_node_cloud's
        return_cloud=True returned; also for the clouds sensor_detect_describe_batch_nodes keeps."""
        rows, cols = C.c_int32(0), C.c_int32(0)
        st = self._L.rgbdfe_download_node_cloud(self._ctx, int(node_id), None, 0, C.byref(rows), C.byref(cols))
        if st != -5:  # RGBDFE_ERR_CAPACITY: rows, cols are set (anything else: an unknown node)
            self._check(st)
        out = np.empty((rows.value, cols.value, 4), np.float32)
        self._check(self._L.rgbdfe_download_node_cloud(self._ctx, int(node_id), out.ctypes.data, rows.value * cols.value,
                                                       C.byref(rows), C.byref(cols)))
        return out

    def _map_args(self, node_ids, transforms):
        node_ids = np.ascontiguousarray(node_ids, np.int32).reshape(-1)
        T = np.ascontiguousarray(np.asarray(transforms, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))  # column-major
        if len(T) != len(node_ids):
            raise ValueError("one 4 x 4 transform per listed node")
        return node_ids, T

    def assemble_map(self, node_ids, transforms, maximum_depth=float("inf"), preserve_raster=False, return_offsets=False,
                     capacity=None, out=None):
        """transformAndAppendPointCloud (misc.cpp:183-238) over the resident clouds of node_ids, in that order:
        GraphManager::saveAllCloudsToFile's aggregate cloud.  transforms: n x 4 x 4 (row-major numpy matrices, the
        Matrix4f of world2cam per node).  Returns the [n, 4] float32 points (x, y, z, rgb bits), with return_offsets also
        the int64 first row of every node (n_nodes + 1 entries).  capacity: rows of the output buffer; by default the
        kept points are counted first (compact mode) and the buffer is sized to them.  out: a contiguous [capacity, 4]
        float32 array to assemble into (the result is a view of its first rows)."""
        node_ids, T = self._map_args(node_ids, transforms)
        n = len(node_ids)
        n_out = C.c_int64(0)
        offsets = np.zeros(n + 1, np.int64)

        def call(out, cap):
            return self._L.rgbdfe_assemble_map(self._ctx, n, node_ids.ctypes.data, T.ctypes.data, float(maximum_depth),
                                               int(bool(preserve_raster)), out.ctypes.data if out is not None else None,
                                               cap, C.byref(n_out), offsets.ctypes.data)
        if out is not None:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.ndim == 2 and out.shape[1] == 4 and
                    out.flags.c_contiguous):
                raise ValueError("out must be a contiguous [capacity, 4] float32 array")
            capacity = len(out)
        elif capacity is None:
            st = call(None, 0)  # the size: RGBDFE_ERR_CAPACITY with n_out set, or OK for an empty cloud
            if st != -5:
                self._check(st)
            capacity = n_out.value
        if out is None:
            out = np.empty((int(capacity), 4), np.float32)
        self._check(call(out, int(capacity)))
        out = out[:n_out.value]
        return (out, offsets) if return_offsets else out

    def assemble_map_device(self, node_ids, transforms, out, maximum_depth=float("inf"), preserve_raster=False,
                            return_offsets=False, stream=None):
        """assemble_map into `out`, a contiguous float32 torch tensor [capacity, 4] on this context's device; no point
        crosses to the host.  Returns the number of rows written (and the offsets)."""
        node_ids, T = self._map_args(node_ids, transforms)
        if not (out.is_cuda and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 4 and out.element_size() == 4):
            raise ValueError("out must be a contiguous [capacity, 4] float32 tensor on the device")
        n = len(node_ids)
        n_out = C.c_int64(0)
        offsets = np.zeros(n + 1, np.int64)
        self._check(self._L.rgbdfe_assemble_map_device(
            self._ctx, n, node_ids.ctypes.data, T.ctypes.data, float(maximum_depth), int(bool(preserve_raster)),
            out.data_ptr() if out.shape[0] else None, int(out.shape[0]), C.byref(n_out), offsets.ctypes.data, stream))
        return (n_out.value, offsets) if return_offsets else n_out.value

    def save_map(self, path, node_ids, transforms, maximum_depth=float("inf"), preserve_raster=False, chunk_points=0):
        """GraphManager::saveAllCloudsToFile: assemble_map's rows as a binary PCD file, or as a binary PLY file when `path`
        ends in .ply (any case; otherwise .pcd is appended unless it is there).  The map is streamed group by group through
        two device buffers and two page-locked slots of at most max(chunk_points, the largest cloud) rows (0: 2^20), so it
        is never whole in memory; the file does not depend on chunk_points.  Returns a dict: path (as written), points,
        bytes_written, format ("pcd" / "ply"), groups, device_scratch_bytes, pinned_bytes, table_bytes.  No point: no file."""
        node_ids, T = self._map_args(node_ids, transforms)
        stats = _lib.MapFileStats()
        written = C.create_string_buffer(len(os.fsencode(path)) + 8)
        self._check(self._L.rgbdfe_save_map(self._ctx, len(node_ids), node_ids.ctypes.data, T.ctypes.data, float(maximum_depth),
                                            int(bool(preserve_raster)), os.fsencode(path), int(chunk_points), written,
                                            len(written), C.byref(stats)))
        out = {name: getattr(stats, name) for name, _ in stats._fields_}
        out["format"] = ("pcd", "ply")[stats.format]
        out["path"] = os.fsdecode(written.value)
        return out

    def save_node_clouds(self, basename, node_ids, poses, graph_ids=None, transform_individual_clouds=False):
        """GraphManager::saveIndividualCloudsToFile: <basename>_%04d.pcd and .txt for every listed node with a non-empty
        cloud, numbered by graph_ids (default: node_ids).  poses: n x 4 x 4 (row-major numpy matrices, float64: the vertex
        estimates).  The resident clouds stay as they are.  Returns the number of nodes written."""
        node_ids = np.ascontiguousarray(node_ids, np.int32).reshape(-1)
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))  # column-major
        if len(P) != len(node_ids):
            raise ValueError("one 4 x 4 pose per listed node")
        gids = None if graph_ids is None else np.ascontiguousarray(graph_ids, np.int32).reshape(-1)
        if gids is not None and len(gids) != len(node_ids):
            raise ValueError("one graph id per listed node")
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_save_node_clouds(self._ctx, len(node_ids), node_ids.ctypes.data,
                                                    None if gids is None else gids.ctypes.data, P.ctypes.data,
                                                    int(bool(transform_individual_clouds)), os.fsencode(basename), C.byref(n)))
        return n.value

    def _display_args(self, node_ids, transforms, display_type, visualization_skip_step, squared_meshing_threshold,
                      maximum_depth):
        node_ids = np.ascontiguousarray(node_ids, np.int32).reshape(-1)
        T = None
        if transforms is not None:
            node_ids, T = self._map_args(node_ids, transforms)
        prm = _lib.RgbdfeDisplayParams(int(display_type), int(visualization_skip_step), float(squared_meshing_threshold),
                                       float(maximum_depth))
        return node_ids, T, prm

    def display_geometry(self, node_ids, transforms=None, display_type=DISPLAY_POINTS, visualization_skip_step=1,
                         squared_meshing_threshold=0.0009, maximum_depth=float("inf")):
        """GLViewer::addPointCloud (glviewer.cpp:693-711) over the resident clouds of node_ids, in that order: the
        glVertex3f calls of pointCloud2GLPoints / pointCloud2GLTriangleList / pointCloud2GLStrip as rows (x, y, z, rgb
        bits).  transforms: n x 4 x 4 as assemble_map takes them, or None for the node frame.  The sizes are counted first
        and the buffers sized to them.  Returns a dict: vertices [n, 4] float32, node_offsets [n_nodes + 1] int64, strips
        [m, 2] int64 (first vertex in the whole stream, vertex count; one per glBegin(GL_TRIANGLE_STRIP)),
        node_strip_offsets [n_nodes + 1] int64, node_types [n_nodes] int32 (the form each node was drawn in)."""
        node_ids, T, prm = self._display_args(node_ids, transforms, display_type, visualization_skip_step,
                                              squared_meshing_threshold, maximum_depth)
        n = len(node_ids)
        nv, ns = C.c_int64(0), C.c_int64(0)
        off, soff, types = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(n, np.int32)

        def call(v, s):
            return self._L.rgbdfe_display_geometry(
                self._ctx, n, node_ids.ctypes.data, T.ctypes.data if T is not None else None, C.byref(prm),
                v.ctypes.data if v is not None and len(v) else None, len(v) if v is not None else 0, C.byref(nv),
                off.ctypes.data, s.ctypes.data if s is not None and len(s) else None, len(s) if s is not None else 0,
                C.byref(ns), soff.ctypes.data, types.ctypes.data)
        st = call(None, None)  # the sizes: RGBDFE_ERR_CAPACITY with both set, or OK for an empty stream
        if st != -5:
            self._check(st)
        v, s = np.empty((nv.value, 4), np.float32), np.empty((ns.value, 2), np.int64)
        if st == -5:
            self._check(call(v, s))
        return dict(vertices=v, node_offsets=off, strips=s, node_strip_offsets=soff, node_types=types)

    def display_geometry_device(self, node_ids, vertices, strips, transforms=None, display_type=DISPLAY_POINTS,
                                visualization_skip_step=1, squared_meshing_threshold=0.0009, maximum_depth=float("inf"),
                                stream=None):
        """display_geometry into `vertices`, a contiguous float32 torch tensor [capacity, 4], and `strips`, a contiguous
        int64 torch tensor [capacity, 2], on this context's device; no vertex crosses to the host.  Returns a dict:
        n_vertices, n_strips, node_offsets, node_strip_offsets, node_types.  A buffer that is too small raises
        RgbdfeError (RGBDFE_ERR_CAPACITY)."""
        node_ids, T, prm = self._display_args(node_ids, transforms, display_type, visualization_skip_step,
                                              squared_meshing_threshold, maximum_depth)
        for t, cols, size, name in ((vertices, 4, 4, "vertices"), (strips, 2, 8, "strips")):
            if not (t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == cols and t.element_size() == size):
                raise ValueError("%s must be a contiguous [capacity, %d] tensor of %d-byte elements on the device" %
                                 (name, cols, size))
        n = len(node_ids)
        nv, ns = C.c_int64(0), C.c_int64(0)
        off, soff, types = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
        self._check(self._L.rgbdfe_display_geometry_device(
            self._ctx, n, node_ids.ctypes.data, T.ctypes.data if T is not None else None, C.byref(prm),
            vertices.data_ptr() if vertices.shape[0] else None, int(vertices.shape[0]), C.byref(nv), off.ctypes.data,
            strips.data_ptr() if strips.shape[0] else None, int(strips.shape[0]), C.byref(ns), soff.ctypes.data,
            types.ctypes.data, stream))
        return dict(n_vertices=nv.value, n_strips=ns.value, node_offsets=off, node_strip_offsets=soff, node_types=types)

    def _render_args(self, node_ids, transforms, width, height, view, projection, gl_point_size, cull, clear_rgba,
                     max_vertices_in_flight, display):
        node_ids, T, dp = self._display_args(node_ids, transforms, display.get("display_type", DISPLAY_POINTS),
                                             display.get("visualization_skip_step", 1),
                                             display.get("squared_meshing_threshold", 0.0009),
                                             display.get("maximum_depth", float("inf")))
        rp = _lib.RgbdfeRenderParams()
        self._L.rgbdfe_render_default_params(C.byref(rp))
        rp.width, rp.height = int(width), int(height)
        if projection is None:  # the viewer's own, at this size (resizeGL, glviewer.cpp:443-444)
            projection = render_perspective(aspect=float(np.float32(width) / np.float32(height)))
        for name, M in (("view", view), ("projection", projection)):
            if M is not None:
                getattr(rp, name)[:] = [float(v) for v in np.asarray(M, np.float64).reshape(4, 4).T.reshape(-1)]
        rp.gl_point_size, rp.cull = float(gl_point_size), int(cull)
        rp.clear_rgba[:] = [int(v) for v in clear_rgba]
        rp.max_vertices_in_flight = int(max_vertices_in_flight)
        return node_ids, T, dp, rp

    def render_nodes(self, node_ids, transforms=None, width=640, height=480, view=None, projection=None, gl_point_size=1.0,
                     cull=True, clear_rgba=(3, 3, 3, 3), max_vertices_in_flight=0, return_ids=True, **display):
        """What GLViewer::paintGL draws of the listed nodes' clouds (include/rgbdfe.h, "rendering"): their display-geometry
        stream (display_type, visualization_skip_step, squared_meshing_threshold, maximum_depth as display_geometry takes
        them) rasterised on the device.  view / projection: 4 x 4 matrices in the row-major numpy sense (render_viewer_view,
        render_perspective, render_sensor_camera make them); None: the viewer's initial position and its projection at
        this size.  Returns a dict of [height, width] images, row 0 at the top: rgba uint8 [.., 4], depth float32 (1.0 where
        nothing was drawn), and with return_ids also ids int64 (the primitive's first vertex in the stream, -1) and
        node_index int32 (position in node_ids, -1)."""
        node_ids, T, dp, rp = self._render_args(node_ids, transforms, width, height, view, projection, gl_point_size, cull,
                                                clear_rgba, max_vertices_in_flight, display)
        H, W = int(height), int(width)
        out = dict(rgba=np.empty((H, W, 4), np.uint8), depth=np.empty((H, W), np.float32))
        if return_ids:
            out.update(ids=np.empty((H, W), np.int64), node_index=np.empty((H, W), np.int32))
        self._check(self._L.rgbdfe_render_nodes(
            self._ctx, len(node_ids), node_ids.ctypes.data, T.ctypes.data if T is not None else None, C.byref(dp), C.byref(rp),
            out["rgba"].ctypes.data, out["depth"].ctypes.data, out["ids"].ctypes.data if return_ids else None,
            out["node_index"].ctypes.data if return_ids else None))
        return out

    def render_nodes_device(self, node_ids, rgba, depth, ids=None, node_index=None, transforms=None, view=None,
                            projection=None, gl_point_size=1.0, cull=True, clear_rgba=(3, 3, 3, 3), max_vertices_in_flight=0,
                            stream=None, **display):
        """render_nodes into contiguous torch tensors on this context's device: rgba uint8 [H, W, 4], depth float32 [H, W],
        and optionally ids int64 [H, W], node_index int32 [H, W]; no pixel crosses to the host."""
        H, W = int(depth.shape[0]), int(depth.shape[1])
        for t, shape, size, name in ((rgba, (H, W, 4), 1, "rgba"), (depth, (H, W), 4, "depth"), (ids, (H, W), 8, "ids"),
                                     (node_index, (H, W), 4, "node_index")):
            if t is not None and not (t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape and t.element_size() == size):
                raise ValueError("%s must be a contiguous %s tensor of %d-byte elements on the device" % (name, shape, size))
        node_ids, T, dp, rp = self._render_args(node_ids, transforms, W, H, view, projection, gl_point_size, cull, clear_rgba,
                                                max_vertices_in_flight, display)
        self._check(self._L.rgbdfe_render_nodes_device(
            self._ctx, len(node_ids), node_ids.ctypes.data, T.ctypes.data if T is not None else None, C.byref(dp), C.byref(rp),
            rgba.data_ptr(), depth.data_ptr(), ids.data_ptr() if ids is not None else None,
            node_index.data_ptr() if node_index is not None else None, stream))

    def render_fragment_stats(self, enable=None):
        """Diagnostics: (fragments offered, fragments that lowered a pixel's word on arrival) of the latest render call while
        counting was on; enable = True / False turns the counting kernels on / off for the calls that follow."""
        out = np.zeros(2, np.int64)
        self._check(self._L.rgbdfe_render_fragment_stats(self._ctx, -1 if enable is None else int(bool(enable)), out.ctypes.data))
        return int(out[0]), int(out[1])

    def voxel_filter(self, points, voxelfilter_size, return_flags=False):
        """pcl::VoxelGrid with a cubic leaf of voxelfilter_size (Node::reducePointCloud, node.cpp:1448-1460) over points,
        [n, 4] float32 (x, y, z, rgb bits): one centroid row per occupied cell, in ascending cell index.  return_flags:
        also the flags (bit 0: the leaf is too small for the cloud's extent and the input came back unchanged)."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        n_out, flags = C.c_int64(0), C.c_int32(0)

        def call(out, cap):
            return self._L.rgbdfe_voxel_filter(self._ctx, pts.ctypes.data if len(pts) else None, len(pts), float(voxelfilter_size),
                                               out.ctypes.data if out is not None else None, cap, C.byref(n_out), C.byref(flags))
        st = call(None, 0)  # the size: RGBDFE_ERR_CAPACITY with n_out set, or OK for an empty result
        if st != -5:
            self._check(st)
        out = np.empty((n_out.value, 4), np.float32)
        self._check(call(out, len(out)))
        out = out[:n_out.value]
        return (out, flags.value) if return_flags else out

    def voxel_filter_device(self, points, voxelfilter_size, out, stream=None, return_flags=False):
        """voxel_filter from `points` into `out`, contiguous float32 torch tensors [n, 4] and [capacity, 4] on this
        context's device that do not overlap; no point crosses to the host.  Returns the number of rows written."""
        for t, name in ((points, "points"), (out, "out")):
            if not (t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 4 and t.element_size() == 4):
                raise ValueError("%s must be a contiguous [n, 4] float32 tensor on the device" % name)
        n_out, flags = C.c_int64(0), C.c_int32(0)
        self._check(self._L.rgbdfe_voxel_filter_device(
            self._ctx, points.data_ptr() if points.shape[0] else None, int(points.shape[0]), float(voxelfilter_size),
            out.data_ptr() if out.shape[0] else None, int(out.shape[0]), C.byref(n_out), C.byref(flags), stream))
        return (n_out.value, flags.value) if return_flags else n_out.value

    def reduce_node_cloud(self, node_id, voxelfilter_size):
        """Node::reducePointCloud (node.cpp:1448-1460): the node's resident cloud becomes its voxel-filtered cloud,
        unstructured (node_cloud() then has the shape (1, n, 4)).  Like the reference, voxelfilter_size <= 0 warns and
        does nothing (returns None); otherwise returns (rows of the cloud, flags)."""
        if not voxelfilter_size > 0:
            warnings.warn("Point Clouds can't be reduced because of invalid voxelfilter_size")  # node.cpp:1458
            return None
        n_out, flags = C.c_int64(0), C.c_int32(0)
        self._check(self._L.rgbdfe_reduce_node_cloud(self._ctx, int(node_id), float(voxelfilter_size), C.byref(n_out),
                                                     C.byref(flags)))
        return n_out.value, flags.value

    def octomap(self, capacity_cells, **params):
        """A persistent occupancy map on this context's device (ColorOctomapServer): see OctoMap."""
        return OctoMap(self, capacity_cells, **params)

    def observation_likelihood(self, new_ids, old_ids, transforms, emm_skip_step=8):
        """observationLikelihood (misc.cpp:814-969) for a batch of directed edges; transforms: n x 4 x 4
        (row-major numpy matrices, new -> old).  Returns an n x 4 uint32 array (inliers, outliers, occluded, all)."""
        new_ids = np.ascontiguousarray(new_ids, np.int32)
        old_ids = np.ascontiguousarray(old_ids, np.int32)
        T = np.ascontiguousarray(np.asarray(transforms, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))  # column-major
        n = len(new_ids)
        out = np.zeros((max(n, 1), 4), np.uint32)
        self._check(self._L.rgbdfe_observation_likelihood(self._ctx, n, new_ids.ctypes.data, old_ids.ctypes.data,
                                                          T.ctypes.data, int(emm_skip_step), out.ctypes.data))
        return out[:n]

    def pairwise_observation_likelihood(self, results, observability_threshold, emm_skip_step=8):
        """pairwiseObservationLikelihood (node.cpp:1520-1554) + observation_criterion_met (misc.cpp:1136-1148)
        for match results with an edge: returns (counts n x 4 summed over both directions, criterion_met)."""
        results = np.asarray(results)
        n = len(results)
        T = np.array([np.array(r["trafo"], np.float32).reshape(4, 4).T for r in results], np.float32).reshape(-1, 4, 4)
        Tinv = np.array([np.linalg.inv(t.astype(np.float64)).astype(np.float32) for t in T], np.float32).reshape(-1, 4, 4)
        newer, older = results["id2"].astype(np.int32), results["id1"].astype(np.int32)
        a = self.observation_likelihood(newer, older, T, emm_skip_step)
        b = self.observation_likelihood(older, newer, Tinv, emm_skip_step)
        c = a + b
        met = np.zeros(n, bool)
        q = C.c_double(0)
        for i in range(n):
            met[i] = bool(self._L.rgbdfe_observation_criterion_met(
                int(c[i, 0]), int(c[i, 1]), int(c[i, 2] + c[i, 0] + c[i, 1]), observability_threshold, C.byref(q)))
        return c, met

    # -- the ICP fallback --------------------------------------------------------------------
    def icp_params(self, **kw):
        """rgbdfe_icp_default_params (icpAlignment's settings and gicp_max_cloud_size), with keyword overrides."""
        p = _lib.IcpParams()
        self._L.rgbdfe_icp_default_params(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise TypeError("no ICP parameter %r" % k)
            setattr(p, k, v)
        return p

    def filter_cloud(self, cloud, desired_size):
        """filterCloud (icp.cpp:20-45): returns (indices, rows) of the sampled rows of cloud, [n, 4] float32."""
        pts = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        n_out = C.c_int64(0)
        cap = len(pts)
        idx, rows = np.empty(cap, np.int32), np.empty((cap, 4), np.float32)
        self._check(self._L.rgbdfe_filter_cloud(self._ctx, pts.ctypes.data if len(pts) else None, len(pts), int(desired_size),
                                                idx.ctypes.data, rows.ctypes.data, cap, C.byref(n_out)))
        return idx[:n_out.value].copy(), rows[:n_out.value].copy()

    def icp_align_clouds(self, source, target, guess=None, params=None, debug=False):
        """icpAlignment (icp.cpp:47-89) of two host clouds, [n, 4] float32, after filterCloud on both.  guess: a 4 x 4
        numpy matrix (row-major; None = identity).  Returns (T, report) -- T a 4 x 4 float32 numpy matrix, report a
        record of ICP_REPORT_DTYPE -- and with debug also (nn_index, nn_d2) of the last iteration's sampled source rows."""
        src = np.ascontiguousarray(source, np.float32).reshape(-1, 4)
        tgt = np.ascontiguousarray(target, np.float32).reshape(-1, 4)
        prm = params if params is not None else self.icp_params()
        G = None if guess is None else np.ascontiguousarray(np.asarray(guess, np.float32).reshape(4, 4).T)
        T = np.empty(16, np.float32)
        rep = np.zeros(1, _lib.ICP_REPORT_DTYPE)
        cap = len(src) if debug else 0
        nn_j, nn_d2 = np.full(cap, -1, np.int32), np.zeros(cap, np.float32)
        self._check(self._L.rgbdfe_icp_align_clouds(
            self._ctx, src.ctypes.data if len(src) else None, len(src), tgt.ctypes.data if len(tgt) else None, len(tgt),
            G.ctypes.data if G is not None else None, C.byref(prm), T.ctypes.data, rep.ctypes.data,
            nn_j.ctypes.data if debug else None, nn_d2.ctypes.data if debug else None, cap))
        T = T.reshape(4, 4).T.copy()
        if debug:
            ns = int(rep[0]["n_source"])
            return T, rep[0], nn_j[:ns], nn_d2[:ns]
        return T, rep[0]

    def icp_align_nodes(self, source_ids, target_ids, guesses=None, params=None):
        """rgbdfe_icp_align_nodes: one batch of alignments over resident node clouds.  guesses: n x 4 x 4 numpy matrices
        (None = identity).  Returns (T, reports): n x 4 x 4 float32 numpy matrices and ICP_REPORT_DTYPE records."""
        src = np.ascontiguousarray(source_ids, np.int32).reshape(-1)
        tgt = np.ascontiguousarray(target_ids, np.int32).reshape(-1)
        if len(src) != len(tgt):
            raise ValueError("one target per source")
        n = len(src)
        prm = params if params is not None else self.icp_params()
        G = None
        if guesses is not None:
            G = np.ascontiguousarray(np.asarray(guesses, np.float32).reshape(n, 4, 4).transpose(0, 2, 1))
        T = np.empty((n, 16), np.float32)
        rep = np.zeros(n, _lib.ICP_REPORT_DTYPE)
        self._check(self._L.rgbdfe_icp_align_nodes(self._ctx, n, src.ctypes.data, tgt.ctypes.data,
                                                   G.ctypes.data if G is not None else None, C.byref(prm), T.ctypes.data,
                                                   rep.ctypes.data))
        return T.reshape(n, 4, 4).transpose(0, 2, 1).copy(), rep

    def icp_fallback(self, results, new_id, candidate_ids, params=None):
        """Node::matchNodePair's ICP branch (node.cpp:1356-1377) for the records of one new node against candidate_ids:
        every record WITHOUT an edge (id1 < 0) whose new_id - candidate_id <= 1 is served.  The source is the OLDER node's
        cloud, the target the new node's, the guess the identity (:1362-1364).  When the alignment converged -- the
        reference then sets found_transformation = true regardless of any quality measure -- the record's trafo
        (final_trafo) becomes icp_trafo and id1 / id2 the older / the new id (:1370-1373); nothing else changes, the
        information scale included.  The assignment final_trafo = icp_trafo is reproduced literally: icp_trafo maps the
        older cloud onto the newer one, whatever direction the RANSAC transform of the other records has.
        Returns (records, served, icp_trafos, reports): a copy of results, the positions served, their n x 4 x 4
        transforms and ICP_REPORT_DTYPE records."""
        out = np.array(results, copy=True)
        cand = np.asarray(candidate_ids, np.int64).reshape(-1)
        if len(cand) != len(out):
            raise ValueError("one candidate id per record")
        served = np.array([i for i in range(len(out)) if int(out[i]["id1"]) < 0 and int(new_id) - int(cand[i]) <= 1], np.int64)
        if len(served) == 0:
            return out, served, np.zeros((0, 4, 4), np.float32), np.zeros(0, _lib.ICP_REPORT_DTYPE)
        T, rep = self.icp_align_nodes(cand[served].astype(np.int32), np.full(len(served), int(new_id), np.int32), None, params)
        for k, i in enumerate(served):
            if rep[k]["converged"]:
                out[i]["trafo"] = T[k].T.reshape(16)   # column-major storage
                out[i]["id1"], out[i]["id2"] = int(cand[i]), int(new_id)
        return out, served, T, rep

    def set_latency_mode(self, max_pairs=(1 << 31) - 1, chunk_iterations=0):
        """Batches of at most max_pairs pairs spread each pair's RANSAC iterations over several waves (record /
        replay, identical results; the default for every batch size); max_pairs = 0 forces one wave per pair,
        chunk_iterations = 0 is automatic."""
        self._check(self._L.rgbdfe_set_latency_mode(self._ctx, int(max_pairs), int(chunk_iterations)))

    # -- measurement ----------------------------------------------------------------------
    def set_profiling(self, enable: bool):
        self._check(self._L.rgbdfe_set_profiling(self._ctx, int(enable)))

    def reset_kernel_time(self):
        self._check(self._L.rgbdfe_reset_kernel_time(self._ctx))

    def set_graph_capture(self, enable: bool):
        """Cached hipGraphs for ORB pair batches (rgbdfe_set_graph_capture): off by default -- an open capture makes
        device-wide synchronisations on other threads of the process fail; for callers that own every HIP-calling thread."""
        self._check(self._L.rgbdfe_set_graph_capture(self._ctx, int(bool(enable))))

    def graph_stats(self):
        """The hipGraph cache of the ORB pair path (rgbdfe_graph_stats)."""
        v = (C.c_int64 * 8)()
        self._check(self._L.rgbdfe_graph_stats(self._ctx, v, 8))
        names = ("captures", "launches", "misses", "plain_batches", "capture_failures", "launch_failures", "cached", "enabled")
        return dict(zip(names, (int(x) for x in v)))

    def kernel_time(self, which: int):
        ms, n, p = C.c_double(0), C.c_int64(0), C.c_int64(0)
        self._check(self._L.rgbdfe_get_kernel_time(self._ctx, which, C.byref(ms), C.byref(n),
                                                   C.byref(p)))
        return ms.value, n.value, p.value


class Node:
    """The slice of the reference's Node (src/node.h) that the pair path touches."""

    def __init__(self, frontend: FrontEnd, node_id: int, feature_descriptors: np.ndarray,
                 feature_locations_3d: np.ndarray):
        self.frontend = frontend
        self.id_ = node_id
        self.feature_descriptors_ = np.ascontiguousarray(feature_descriptors, np.uint8)
        self.feature_locations_3d_ = np.ascontiguousarray(feature_locations_3d, np.float32)
        self.matchable_ = True
        frontend.upload_node(node_id, self.feature_descriptors_, self.feature_locations_3d_)

    def matchNodePair(self, older_node: "Node") -> MatchingResult:
        """src/node.cpp:1305-1429"""
        rec = self.frontend.match_node_pairs(self.id_, [older_node.id_])[0]
        return record_to_matching_result(rec)

    def featureMatching(self, other: "Node") -> List[DMatch]:
        """ORB branch of src/node.cpp:535-690 (matches sorted by (hd, queryIdx))."""
        rec = self.frontend.match_node_pairs(self.id_, [other.id_])[0]
        return record_to_matching_result(rec).all_matches

    def clearFeatureInformation(self):
        """src/node.cpp:1431-1443"""
        self.frontend.release_node(self.id_)
        self.matchable_ = False


class GraphManager:
    """The fan-out of GraphManager::nodeComparisons (src/graph_manager.cpp:531-583) and, over a candidates.PoseGraph,
    addEdgeToG2O (:811-909), optimizeGraph (:938-1066), pruneEdgesWithErrorAbove (:1106-1246), sanityCheck (:1347-1360),
    the rounds of OpenNIListener::evaluation and saveTrajectory's estimate file."""

    def __init__(self, frontend: FrontEnd, pose_graph=None):
        self.frontend = frontend
        self.pose_graph = pose_graph

    def _graph(self):
        if self.pose_graph is None:
            from .candidates import PoseGraph
            self.pose_graph = PoseGraph()
        return self.pose_graph

    def addEdgeToG2O(self, edge, set_estimate: bool = False):
        """edge: a LoadedEdge3D (MatchingResult.edge); both nodes must be in the pose graph."""
        self._graph().add_edge_se3(edge.id1, edge.id2, edge.transform, edge.informationMatrix, set_estimate)

    def optimize_graph(self, break_criterion: float = 0.01):
        """optimizeGraph with optimizer_iterations = break_criterion; the report (its "chi2" is what the reference returns)."""
        return self._graph().optimize_graph(self.frontend, break_criterion)

    def set_pose_relative_to(self, strategy: str):
        """pose_relative_to: "first", "previous", "largest_loop", "inaffected" ("none": the flags of set_fixed as they are)."""
        self._graph().set_strategy(strategy)

    def pruneEdgesWithErrorAbove(self, thresh: float):
        """pruneEdgesWithErrorAbove (:1106-1246) on the device; returns the number of edges pruned."""
        return self._graph().prune_edges(self.frontend, thresh)[0]

    def sanityCheck(self, thresh: float):
        """sanityCheck (:1347-1360); returns the number of edges whose information became 0.000001 I."""
        return self._graph().sanity_check(thresh)

    def evaluation(self, optimizer_iterations: float = 0.01):
        """The five optimisation rounds of OpenNIListener::evaluation (openni_listener.cpp:431-518):
        (a dict per round, the estimates after every round as [5, n, 4, 4])."""
        return self._graph().evaluate(self.frontend, optimizer_iterations)

    def saveTrajectory(self, path, node_ids, timestamps, base2points=None, init_base_pose=None, frame_id=None,
                       child_frame_id=None):
        """saveTrajectory's estimate file (graph_mgr_io.cpp:615-677) in TUM format, for tools/evaluate_ate.py."""
        self._graph().write_trajectory(path, node_ids, timestamps, base2points, init_base_pose, frame_id, child_frame_id)

    def nodeComparisons(self, new_node: Node, nodes_to_comp: Sequence[Node]) -> List[MatchingResult]:
        recs = self.frontend.match_node_pairs(new_node.id_, [n.id_ for n in nodes_to_comp])
        return [record_to_matching_result(r) for r in recs]

    def slam(self, **params) -> "Slam":
        """The SLAM-step object over this manager's front end and pose graph (made by the first addNode with the defaults)."""
        if getattr(self, "_slam", None) is None:
            self._slam = Slam(self.frontend, self._graph(), **params)
        elif params:
            raise ValueError("the SLAM step's parameters are fixed when it is made")
        return self._slam

    def addNode(self, node: Node, stamp=(0, 0)) -> "SlamStepRecord":
        """GraphManager::addNode (src/graph_manager.cpp:681-782) for a node that is resident under node.id_ (its slot);
        stamp = (sec, nsec).  The step record says what happened; record.id is the graph id (node.id_ stays the slot)."""
        return self.slam().add_node(node.id_, stamp)

    def firstNode(self, node: Node, stamp=(0, 0)) -> "SlamStepRecord":
        """GraphManager::firstNode (:360-402): addNode on an empty graph."""
        if self.slam().node_count() != 0:
            raise ValueError("firstNode: the graph is not empty")
        return self.addNode(node, stamp)


def _check_contextless(L, st):
    if st != 0:
        raise RgbdfeError(f"{L.rgbdfe_status_string(st).decode()}: {L.rgbdfe_last_error(None).decode()}")


def cloud_file_path(path):
    """The reference's name rule: (path as it is written, "pcd" / "ply")."""
    L = _lib.load()
    out = C.create_string_buffer(len(os.fsencode(path)) + 8)
    fmt = C.c_int32(0)
    _check_contextless(L, L.rgbdfe_cloud_file_path(os.fsencode(path), out, len(out), C.byref(fmt)))
    return os.fsdecode(out.value), ("pcd", "ply")[fmt.value]


def save_cloud_file(path, points, viewpoint=None, format=None):
    """A cloud held in host memory as a binary PCD / PLY file (include/rgbdfe.h, "map files"); no device.  points: [n, 4] (written
    as WIDTH n, HEIGHT 1) or [rows, cols, 4] float32 (x, y, z, rgb bits); viewpoint: ox oy oz qw qx qy qz (PCD only).  `path` is
    written as given; format: "pcd" / "ply", by default by the name rule's reading of the path."""
    L = _lib.load()
    pts = np.ascontiguousarray(points, np.float32)
    if pts.ndim not in (2, 3) or pts.shape[-1] != 4:
        raise ValueError("points must be [n, 4] or [rows, cols, 4]")
    height, width = (1, pts.shape[0]) if pts.ndim == 2 else pts.shape[:2]
    fmt = cloud_file_path(path)[1] if format is None else format
    vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(7)
    _check_contextless(L, L.rgbdfe_save_cloud_file(pts.ctypes.data, int(width), int(height), None if vp is None else vp.ctypes.data,
                                                   ("pcd", "ply").index(fmt), os.fsencode(path)))


def read_cloud_file(path, header_only=False):
    """A file of one of the two layouts this library writes: (points [height, width, 4] float32, info) with info = format,
    width, height, points, header_bytes, data_bytes, viewpoint.  A PLY vertex's rgb word has a zero top byte.  Anything else is
    refused.  header_only: info alone."""
    L = _lib.load()
    h = _lib.CloudFileHeader()
    _check_contextless(L, L.rgbdfe_cloud_file_info(os.fsencode(path), C.byref(h)))
    info = dict(format=("pcd", "ply")[h.format], width=h.width, height=h.height, points=h.points, header_bytes=h.header_bytes,
                data_bytes=h.data_bytes, viewpoint=np.array(h.viewpoint[:], np.float32))
    if header_only:
        return info
    out = np.empty((h.height, h.width, 4), np.float32)
    _check_contextless(L, L.rgbdfe_load_cloud_file(os.fsencode(path), out.ctypes.data, int(h.points), C.byref(h)))
    return out, info


def read_session_chunks(path) -> dict:
    """The chunks of a session file by tag ("CONF", "DETE", "NODE", "CLOU", "GRPH", "SLAM"), every CRC checked: for tools that
    need a field before they can build the objects to load into (include/rgbdfe.h, "session files")."""
    import struct
    import zlib
    with open(path, "rb") as f:
        b = f.read()
    if b[:8] != b"RGBDFESS" or len(b) < 32 or struct.unpack_from("<IIQ", b, 8)[0::2] != (1, len(b)):
        raise RgbdfeError("not a session file: " + str(path))
    at, out = 32, {}
    while at + 16 <= len(b):
        tag = b[at:at + 4].decode("ascii", "replace")
        crc, n = struct.unpack_from("<IQ", b, at + 4)
        payload = b[at + 16:at + 16 + n]
        if len(payload) != n or zlib.crc32(payload) != crc:
            raise RgbdfeError("session file: bad chunk " + tag)
        if tag == "END ":
            return out
        out[tag] = payload
        at += 16 + n + (-n % 8)
    raise RgbdfeError("session file: no END chunk")


def parse_slam_state(data: bytes) -> dict:
    """Slam.serialize()'s string (a session file's SLAM chunk) as a dict: params (the 13 int32 in the order of
    rgbdfe_slam_params, seed, the 6 doubles, init_base_pose), calls (steps begun), per graph id slots / rows / stamps /
    valid_tf, keyframes, the edge counters."""
    import struct
    if data[:8] != b"RGBDFESM":
        raise RgbdfeError("not a slam state")
    names_i = [n for n, _ in _lib.SlamParams._fields_][:13]
    names_d = [n for n, _ in _lib.SlamParams._fields_][14:20]
    at = 24
    params = dict(zip(names_i, struct.unpack_from("<13i", data, at)))
    params["seed"] = struct.unpack_from("<I", data, at + 52)[0]
    params.update(zip(names_d, struct.unpack_from("<6d", data, at + 56)))
    params["init_base_pose"] = np.array(struct.unpack_from("<16d", data, at + 104)).reshape(4, 4).T
    at += 232
    n, n_kf, next_seq_id, calls, seq_edges, loop_edges, b1, b2, bn, _ = struct.unpack_from("<IIiIiiiiiI", data, at)
    at += 40
    slots = list(struct.unpack_from("<%di" % n, data, at)); at += 4 * n
    rows = list(struct.unpack_from("<%di" % n, data, at)); at += 4 * n
    sec = struct.unpack_from("<%dq" % n, data, at); at += 8 * n
    nsec = struct.unpack_from("<%di" % n, data, at); at += 4 * n
    valid = list(struct.unpack_from("<%dB" % n, data, at)); at += n + (-n % 4)
    keyframes = list(struct.unpack_from("<%di" % n_kf, data, at))
    return dict(params=params, calls=calls, slots=slots, rows=rows, stamps=list(zip(sec, nsec)), valid_tf=valid, keyframes=keyframes,
                sequential_edges=seq_edges, loop_closure_edges=loop_edges, best=(b1, b2, bn), next_seq_id=next_seq_id)


class SlamStepRecord:
    """An rgbdfe_slam_step with names for its codes."""

    def __init__(self, raw: "_lib.SlamStep"):
        self.raw = raw
        for name, _ in raw._fields_:
            v = getattr(raw, name)
            setattr(self, name, v if isinstance(v, (int, float)) else list(v))
        n = raw.n_candidates
        self.candidates, self.verdicts = self.candidates[:n], self.verdicts[:n]
        self.status_name = _lib.SLAM_STATUS.get(raw.status, "?")
        self.verdict_names = [_lib.SLAM_VERDICTS[v & 15] + ("+icp" if v & _lib.SLAM_VERDICT_ICP else "") for v in self.verdicts]
        self.motion_estimate = np.array(raw.motion_estimate).reshape(4, 4).T
        self.broadcast_pose = np.array(raw.broadcast_pose).reshape(4, 4).T

    def __bool__(self):   # addNode's return value: "iff the node could be added"
        return self.raw.status in (2, 4, 6)


class Slam:
    """rgbdfe_slam: GraphManager::addNode as one call (add_node), or as the decision machine alone (begin / feed) for callers
    that run the comparisons themselves.  frontend may be None (no device: begin / feed only)."""

    def __init__(self, frontend: Optional[FrontEnd], pose_graph, **params):
        self._L = _lib.load()
        self.frontend, self.pose_graph = frontend, pose_graph
        self.params = _lib.SlamParams()
        self._L.rgbdfe_slam_default_params(C.byref(self.params))
        for k, v in params.items():
            if k == "init_base_pose":
                v = (C.c_double * 16)(*np.asarray(v, np.float64).reshape(4, 4).T.reshape(16))
            elif not hasattr(self.params, k):
                raise ValueError("unknown SLAM parameter " + k)
            setattr(self.params, k, v)
        self._s = C.c_void_p()
        st = self._L.rgbdfe_slam_create(frontend._ctx if frontend is not None else None, pose_graph._g, C.byref(self.params),
                                        C.byref(self._s))
        if st != 0:
            raise RgbdfeError(self._L.rgbdfe_status_string(st).decode())
        self._ids = np.zeros(_lib.SLAM_MAX_CANDIDATES, np.int32)
        if frontend is not None:
            if not hasattr(frontend, "_slams"):
                frontend._slams = []
            frontend._slams.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_s", None) and self._s.value:
            self._L.rgbdfe_slam_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            msg = self._L.rgbdfe_last_error(self.frontend._ctx).decode() if self.frontend is not None else ""
            raise RgbdfeError(f"{self._L.rgbdfe_status_string(st).decode()}: {msg}")

    def reset(self):
        self._check(self._L.rgbdfe_slam_reset(self._s))

    def _check_string(self, st):
        if st != 0:
            raise RgbdfeError(f"{self._L.rgbdfe_status_string(st).decode()}: {self._L.rgbdfe_last_error(None).decode()}")

    def serialize(self) -> bytes:
        """The machine between two steps -- slot table, stamps, valid_tf, keyframes, counters, curr_best_result_, the draw
        counter and the parameters -- as one byte string; refused while a step is in flight (between begin and feed)."""
        n = C.c_int64(0)
        st = self._L.rgbdfe_slam_serialize(self._s, None, 0, C.byref(n))
        if st not in (0, -5):  # RGBDFE_ERR_CAPACITY: the length is set
            self._check_string(st)
        buf = np.zeros(max(n.value, 1), np.uint8)
        self._check_string(self._L.rgbdfe_slam_serialize(self._s, buf.ctypes.data, n.value, C.byref(n)))
        return buf[: n.value].tobytes()

    def deserialize(self, data: bytes):
        """Into a fresh or reset Slam created with the stored parameters (the error names the first field that differs).  The
        pose graph is not part of the string: PoseGraph.deserialize."""
        buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        self._check_string(self._L.rgbdfe_slam_deserialize(self._s, buf.ctypes.data, len(data)))

    def add_node(self, slot: int, stamp=(0, 0)) -> SlamStepRecord:
        st = _lib.SlamStep()
        self._check(self._L.rgbdfe_slam_add_node(self._s, int(slot), int(stamp[0]), int(stamp[1]), C.byref(st)))
        return SlamStepRecord(st)

    def begin(self, slot: int, n_rows: int, stamp=(0, 0)):
        """-> (graph ids to compare the new node with, None) or ([], the finished step record)."""
        st, n = _lib.SlamStep(), C.c_int32(0)
        self._check(self._L.rgbdfe_slam_begin(self._s, int(slot), int(n_rows), int(stamp[0]), int(stamp[1]), self._ids.ctypes.data,
                                              len(self._ids), C.byref(n), C.byref(st)))
        return ([int(i) for i in self._ids[:n.value]], None) if n.value else ([], SlamStepRecord(st))

    def feed(self, results, flags=None):
        """results: RESULT_DTYPE or COMPACT_DTYPE records, one per id handed out; -> as begin."""
        results = np.asarray(results)
        rec = results if results.dtype == _lib.COMPACT_DTYPE else _lib.compact_of(results)
        rec = np.ascontiguousarray(rec)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        st, n = _lib.SlamStep(), C.c_int32(0)
        self._check(self._L.rgbdfe_slam_feed(self._s, rec.ctypes.data, None if fl is None else fl.ctypes.data, len(rec),
                                             self._ids.ctypes.data, len(self._ids), C.byref(n), C.byref(st)))
        return ([int(i) for i in self._ids[:n.value]], None) if n.value else ([], SlamStepRecord(st))

    def node_count(self) -> int:
        return self._L.rgbdfe_slam_node_count(self._s)

    def slot_of(self, graph_id: int) -> int:
        return self._L.rgbdfe_slam_slot_of(self._s, int(graph_id))

    def slots(self) -> List[int]:
        return [self.slot_of(i) for i in range(self.node_count())]

    def valid_tf(self) -> List[int]:
        return [self._L.rgbdfe_slam_valid_tf(self._s, i) for i in range(self.node_count())]

    def keyframes(self) -> List[int]:
        ids, n = np.zeros(self.node_count() + 1, np.int32), C.c_int32(0)
        self._check(self._L.rgbdfe_slam_keyframes(self._s, ids.ctypes.data, len(ids), C.byref(n)))
        return [int(i) for i in ids[:n.value]]


class OctoMap:
    """ColorOctomapServer on the device (ColorOctomapServer.cpp:61-129; the seam of GraphManager::renderToOctomap /
    saveOctomapImpl, graph_mgr_io.cpp:253-329): the leaves of a colour OctoMap, fed by ray-casting clouds one after another.
    params: resolution, prob_hit, prob_miss, clamping_min, clamping_max, occupancy_threshold (defaults:
    parameter_server.cpp:56-64).  tree / tree_device / nodes_at_depth / write / read / set_leaves: the octree over the leaves
    (updateInnerOccupancy), the node set of render() and the .ot file of save(), built on the device.  Close the map before
    its FrontEnd."""

    def __init__(self, fe: "FrontEnd", capacity_cells: int, **params):
        self._fe, self._L = fe, fe._L
        self.params = _lib.OctomapParams()
        self._L.rgbdfe_octomap_default_params(C.byref(self.params))
        for k, v in params.items():
            if not hasattr(self.params, k):
                raise TypeError("unknown octomap parameter %r" % k)
            setattr(self.params, k, float(v))
        self._map = C.c_void_p()
        fe._check(self._L.rgbdfe_octomap_create(fe._ctx, C.byref(self.params), int(capacity_cells), C.byref(self._map)))
        if not hasattr(fe, "_octomaps"):
            fe._octomaps = []
        fe._octomaps.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_map", None) and self._map.value:
            self._L.rgbdfe_octomap_destroy(self._map)
            self._map = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        """ColorOctomapServer::reset: no leaves, the same parameters and capacity."""
        self._fe._check(self._L.rgbdfe_octomap_reset(self._map))

    def reserve(self, capacity_cells: int):
        """The leaves re-housed in a table of capacity_cells cells, on the device."""
        self._fe._check(self._L.rgbdfe_octomap_reserve(self._map, int(capacity_cells)))

    def insert_nodes_status(self, node_ids, transforms, max_range=-1.0):
        """(status, clouds applied): status -5 (RGBDFE_ERR_CAPACITY) when a cloud did not fit; the map is then the map
        after the clouds applied.  Other failures raise."""
        node_ids, T = self._fe._map_args(node_ids, transforms)
        done = C.c_int32(0)
        st = self._L.rgbdfe_octomap_insert_nodes(self._map, len(node_ids), node_ids.ctypes.data, T.ctypes.data,
                                                 float(max_range), C.byref(done))
        if st != -5:
            self._fe._check(st)
        return st, done.value

    def insert_nodes(self, node_ids, transforms, max_range=-1.0, grow=True):
        """insertCloudCallback for the resident clouds of node_ids, in that order; transforms: n x 4 x 4 (row-major numpy
        matrices, world2cam per node, as assemble_map takes them); max_range: the parameter maximum_depth (negative: off).
        grow: a full table is doubled and the remaining clouds follow; otherwise a full table raises with the clouds
        applied so far in place."""
        node_ids = np.ascontiguousarray(node_ids, np.int32).reshape(-1)
        T = np.asarray(transforms, np.float32).reshape(-1, 4, 4)
        at = 0
        while True:
            st, done = self.insert_nodes_status(node_ids[at:], T[at:], max_range)
            if st == 0:
                return
            at += done
            if not grow:
                self._fe._check(st)
            self.reserve(2 * self.capacity)

    def insert_cloud(self, points, transform, max_range=-1.0):
        """The same for one host cloud, [n, 4] float32 (x, y, z, rgb bits), and one row-major 4 x 4 transform."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(np.asarray(transform, np.float32).reshape(4, 4).T)  # column-major
        self._fe._check(self._L.rgbdfe_octomap_insert_cloud(self._map, pts.ctypes.data if len(pts) else None, len(pts),
                                                            T.ctypes.data, float(max_range)))

    def _stats(self):
        out = np.zeros(3, np.int64)
        self._fe._check(self._L.rgbdfe_octomap_stats(self._map, out.ctypes.data, 3))
        return out

    @property
    def capacity(self) -> int:
        return int(self._stats()[0])

    @property
    def last_launches(self) -> int:
        """Kernel launches of the last insert call."""
        return int(self._stats()[2])

    def __len__(self):
        n = C.c_int64(0)
        self._fe._check(self._L.rgbdfe_octomap_size(self._map, C.byref(n)))
        return n.value

    def leaves(self):
        """The leaves as a structured array (key[3], log_odds, rgb[3]; _lib.OCTOMAP_LEAF_DTYPE), in ascending
        key[0] | key[1] << 16 | key[2] << 32."""
        out = np.zeros(len(self), _lib.OCTOMAP_LEAF_DTYPE)
        n = C.c_int64(0)
        self._fe._check(self._L.rgbdfe_octomap_leaves(self._map, out.ctypes.data if len(out) else None, len(out), C.byref(n)))
        return out[:n.value]

    @property
    def last_tree_launches(self) -> int:
        """Kernel launches of the last tree / tree_device / nodes_at_depth / write call."""
        out = np.zeros(4, np.int64)
        self._fe._check(self._L.rgbdfe_octomap_stats(self._map, out.ctypes.data, 4))
        return int(out[3])

    def tree_status(self, out):
        """(status, nodes needed) of rgbdfe_octomap_tree into `out` (a _lib.OCTOMAP_NODE_DTYPE array): status -5
        (RGBDFE_ERR_CAPACITY) when `out` is too short, and nothing is written then.  Other failures raise."""
        n = C.c_int64(0)
        st = self._L.rgbdfe_octomap_tree(self._map, out.ctypes.data if len(out) else None, len(out), C.byref(n))
        if st != -5:
            self._fe._check(st)
        return st, n.value

    def tree(self):
        """Every node of the octree over the leaves (inner values as updateInnerOccupancy leaves them) in depth-first
        pre-order, children in ascending index: a structured array (log_odds, rgb[3], children;
        _lib.OCTOMAP_NODE_DTYPE), the payload of an .ot file.  An empty map has no nodes."""
        out = np.zeros(0, _lib.OCTOMAP_NODE_DTYPE)
        st, n = self.tree_status(out)
        if st == 0:
            return out
        out = np.zeros(n, _lib.OCTOMAP_NODE_DTYPE)
        self._fe._check(self.tree_status(out)[0])
        return out

    def tree_device(self, out, stream=None):
        """The same records into `out`, a contiguous uint8 torch tensor [capacity, 8] on the map's device; no record
        crosses to the host.  Returns the number of nodes; raises when the room is too small."""
        if not (out.is_cuda and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 8 and out.element_size() == 1):
            raise ValueError("out must be a contiguous [capacity, 8] uint8 tensor on the device")
        n = C.c_int64(0)
        self._fe._check(self._L.rgbdfe_octomap_tree_device(self._map, out.data_ptr() if out.shape[0] else None,
                                                           int(out.shape[0]), C.byref(n), stream))
        return n.value

    def nodes_at_depth(self, depth, min_log_odds=-np.inf):
        """The nodes of one depth (0 .. 16) with log_odds >= min_log_odds, in tree order, as leaf records
        (_lib.OCTOMAP_LEAF_DTYPE) whose key is the node's first cell with the low 16 - depth bits cleared: what
        ColorOctomapServer::render walks at octomap_display_level.  A node's edge is resolution * 2 ** (16 - depth)."""
        bound = len(self) if depth >= 11 else min(len(self), 8 ** max(int(depth), 0))
        out = np.zeros(bound, _lib.OCTOMAP_LEAF_DTYPE)
        n = C.c_int64(0)
        self._fe._check(self._L.rgbdfe_octomap_nodes_at_depth(self._map, int(depth), float(min_log_odds),
                                                              out.ctypes.data if len(out) else None, len(out), C.byref(n)))
        return out[:n.value].copy()

    def write(self, path):
        """ColorOctomapServer::save: the map as an .ot file (id ColorOcTree)."""
        self._fe._check(self._L.rgbdfe_octomap_write(self._map, os.fsencode(path)))

    def read(self, path):
        """The leaves of an .ot file written with the same resolution become the map's contents."""
        self._fe._check(self._L.rgbdfe_octomap_read(self._map, os.fsencode(path)))

    def set_leaves(self, leaves):
        """The map's contents replaced by these leaves (_lib.OCTOMAP_LEAF_DTYPE records, any order)."""
        lv = np.ascontiguousarray(leaves, _lib.OCTOMAP_LEAF_DTYPE).reshape(-1)
        self._fe._check(self._L.rgbdfe_octomap_set_leaves(self._map, lv.ctypes.data if len(lv) else None, len(lv)))

    # ---- the read side (include/rgbdfe.h, "occupancy map: the read side") ------------------------------------------------
    @property
    def last_query_launches(self) -> int:
        """Kernel launches of the last search / cast_rays / view_cloud / view_cloud_device call."""
        out = np.zeros(5, np.int64)
        self._fe._check(self._L.rgbdfe_octomap_stats(self._map, out.ctypes.data, 5))
        return int(out[4])

    @property
    def occupied_log_odds(self) -> float:
        """logodds(occupancy_threshold): the threshold a query uses when it is given none."""
        v = C.c_float(0.0)
        self._fe._check(self._L.rgbdfe_octomap_occupied_log_odds(self._map, C.byref(v)))
        return v.value

    def _query(self, call, grow):
        """call() -> status.  A table loaded above 3/4 refuses queries (RGBDFE_ERR_CAPACITY): with grow, the leaves are
        re-housed at a load of at most 0.5 and the call repeated, as insert_nodes doubles a full table."""
        st = call()
        if st == -5 and grow and 4 * len(self) > 3 * self.capacity:
            self.reserve(2 * len(self))
            st = call()
        self._fe._check(st)

    @staticmethod
    def _threshold(occupied_log_odds):
        return float("nan") if occupied_log_odds is None else float(occupied_log_odds)

    def search(self, points, grow=True):
        """OcTreeBaseImpl::search for n world-frame points ([n, 3] float32): (found, leaves) with found[i] = 0 (no leaf),
        1 (leaves[i] is the leaf of the point's cell) or 2 (a non-finite coordinate or a key out of range), leaves as
        _lib.OCTOMAP_LEAF_DTYPE records."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(pts)
        found, leaves = np.zeros(n, np.int32), np.zeros(n, _lib.OCTOMAP_LEAF_DTYPE)
        self._query(lambda: self._L.rgbdfe_octomap_search(self._map, pts.ctypes.data if n else None, n,
                                                          found.ctypes.data if n else None, leaves.ctypes.data if n else None), grow)
        return found, leaves

    def cast_rays(self, origins, directions, ignore_unknown=False, max_range=-1.0, occupied_log_odds=None, grow=True):
        """OccupancyOcTreeBase::castRay for n rays ([n, 3] float32 origins and directions, world frame; a direction need not
        be normalised): _lib.OCTOMAP_RAY_HIT_DTYPE records (status: _lib.OCTOMAP_RAY_*; steps; the end cell's key and
        centre; log_odds and rgb of the leaf for a hit).  max_range <= 0: no limit; occupied_log_odds None: the map's
        occupancy_threshold."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("as many directions as origins")
        n = len(o)
        hits = np.zeros(n, _lib.OCTOMAP_RAY_HIT_DTYPE)
        self._query(lambda: self._L.rgbdfe_octomap_cast_rays(
            self._map, o.ctypes.data if n else None, d.ctypes.data if n else None, n, int(bool(ignore_unknown)), float(max_range),
            self._threshold(occupied_log_odds), hits.ctypes.data if n else None), grow)
        return hits

    def _view_args(self, transform, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range, occupied_log_odds):
        T = np.ascontiguousarray(np.asarray(transform, np.float32).reshape(4, 4).T)  # column-major
        return T, (T.ctypes.data, float(fx), float(fy), float(cx), float(cy), int(rows), int(cols), int(bool(ignore_unknown)),
                   float(max_range), self._threshold(occupied_log_odds))

    def view_cloud(self, transform, fx, fy, cx, cy, rows, cols, ignore_unknown=False, max_range=-1.0, occupied_log_odds=None,
                   with_status=False, grow=True):
        """The map seen from a pose: an organised cloud [rows, cols, 4] float32 in the node-cloud row format (x, y, z in the
        camera frame, rgb bits; NaN rows and word 0 where the pixel's ray hits nothing).  transform: camera -> world, a
        row-major 4 x 4 matrix as insert_cloud takes it.  with_status: also the rays' statuses, [rows, cols] uint8."""
        T, args = self._view_args(transform, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range, occupied_log_odds)
        n = int(rows) * int(cols)
        out = np.zeros((max(int(rows), 0), max(int(cols), 0), 4), np.float32)
        status = np.zeros(out.shape[:2], np.uint8) if with_status else None
        self._query(lambda: self._L.rgbdfe_octomap_view_cloud(
            self._map, *args, out.ctypes.data if n > 0 else None, status.ctypes.data if with_status and n > 0 else None), grow)
        return (out, status) if with_status else out

    def view_cloud_device(self, out, transform, fx, fy, cx, cy, ignore_unknown=False, max_range=-1.0, occupied_log_odds=None,
                          status=None, stream=None, grow=True):
        """The same into `out`, a contiguous float32 torch tensor [rows, cols, 4] on the map's device (status: a contiguous
        uint8 tensor [rows, cols] there, or None); nothing crosses to the host."""
        if not (out.is_cuda and out.is_contiguous() and out.dim() == 3 and out.shape[2] == 4 and out.element_size() == 4):
            raise ValueError("out must be a contiguous [rows, cols, 4] float32 tensor on the device")
        rows, cols = int(out.shape[0]), int(out.shape[1])
        if status is not None and not (status.is_cuda and status.is_contiguous() and tuple(status.shape) == (rows, cols)
                                       and status.element_size() == 1):
            raise ValueError("status must be a contiguous [rows, cols] uint8 tensor on the device")
        T, args = self._view_args(transform, fx, fy, cx, cy, rows, cols, ignore_unknown, max_range, occupied_log_odds)
        n = rows * cols
        self._query(lambda: self._L.rgbdfe_octomap_view_cloud_device(
            self._map, *args, out.data_ptr() if n else None, status.data_ptr() if status is not None and n else None, stream), grow)
