"""ctypes binding of librgbdfe.so (the C ABI in include/rgbdfe.h).

The library is built in-tree by ``rgbdslam_v2_amd.build.build()`` (hipcc, gfx950).
There is no CPU fallback anywhere in this package: if the shared library is
missing, or no HIP device is present, the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RGBDFE_LIB", os.path.join(_HERE, "librgbdfe.so"))  # RGBDFE_LIB: diagnostics builds

RGBDFE_MAX_MATCHES = 320
RGBDFE_MASK_WORDS = 5
RGBDFE_NODE_HAS_KEYPOINTS = 0x100   # or-ed into rgbdfe_download_nodes' kinds
RGBDFE_SESSION_CLOUDS = 1   # rgbdfe_session_save's flags

DEFAULT_HAMMING_MODE = 3   # RGBDFE_HAMMING_MODE_DEFAULT of include/rgbdfe.h (tests/test_abi.py keeps the two equal)
KERNEL_HAMMING = 0
KERNEL_RANSAC = 1
KERNEL_SIFT_DOT = 2
KERNEL_SIFT_FINISH = 3
KERNEL_EMM = 4
KERNEL_ICP_NN = 5   # the ICP fallback's nearest-neighbour kernel (pairs = job-iterations)


class RgbdfeParams(C.Structure):
    _fields_ = [
        ("max_matches", C.c_int32),
        ("min_matches", C.c_int32),
        ("ransac_iterations", C.c_int32),
        ("max_dist_for_inliers", C.c_float),
        ("depth_cov", C.c_double),
        ("seed", C.c_uint32),
        ("g2o_iterations", C.c_uint32),
    ]


class RgbdfeConfig(C.Structure):
    _fields_ = [
        ("device_id", C.c_int32),
        ("max_nodes", C.c_int32),
        ("max_keypoints", C.c_int32),
        ("max_pairs_per_batch", C.c_int32),
        ("params", RgbdfeParams),
    ]


class RgbdfeMatchResult(C.Structure):
    _fields_ = [
        ("id1", C.c_int32),
        ("id2", C.c_int32),
        ("n_all", C.c_int32),
        ("n_inl", C.c_int32),
        ("rmse", C.c_float),
        ("trafo", C.c_float * 16),
        ("pad0", C.c_uint32),
        ("info_scale", C.c_double),
        ("valid_iterations", C.c_int32),
        ("real_iterations", C.c_int32),
        ("all_q", C.c_uint16 * RGBDFE_MAX_MATCHES),
        ("all_t", C.c_uint16 * RGBDFE_MAX_MATCHES),
        ("all_hd", C.c_uint8 * RGBDFE_MAX_MATCHES),
        ("inlier_mask", C.c_uint64 * RGBDFE_MASK_WORDS),
    ]


VISUAL_MONO8, VISUAL_RGB8, VISUAL_BGR8 = 0, 1, 2   # RGBDFE_VISUAL_*
DEPTH_32FC1, DEPTH_16UC1 = 0, 1                     # RGBDFE_DEPTH_*


class RgbdfeSensorFrame(C.Structure):   # rgbdfe_sensor_frame
    _fields_ = [
        ("visual", C.c_void_p), ("visual_rows", C.c_int32), ("visual_cols", C.c_int32), ("visual_step", C.c_int32),
        ("visual_encoding", C.c_int32),
        ("depth", C.c_void_p), ("depth_rows", C.c_int32), ("depth_cols", C.c_int32), ("depth_step", C.c_int32),
        ("depth_encoding", C.c_int32),
    ]


class RgbdfeSensorCloud(C.Structure):   # rgbdfe_sensor_cloud
    _fields_ = [("cloud_skip", C.c_int32), ("encoding_bgr", C.c_int32), ("min_depth", C.c_double)]


class OctomapParams(C.Structure):   # rgbdfe_octomap_params
    _fields_ = [("resolution", C.c_double), ("prob_hit", C.c_double), ("prob_miss", C.c_double),
                ("clamping_min", C.c_double), ("clamping_max", C.c_double), ("occupancy_threshold", C.c_double)]


POSE_GRAPH_REPORT_ITERATIONS = 64
POSE_GRAPH_MAX_TRIALS = 10


class PoseGraphIteration(C.Structure):   # rgbdfe_pose_graph_iteration
    _fields_ = [("trials", C.c_int32), ("pcg_iterations", C.c_int32 * POSE_GRAPH_MAX_TRIALS), ("pad", C.c_int32),
                ("chi2_before", C.c_double), ("chi2_after", C.c_double), ("lam", C.c_double)]


POSE_GRAPH_EVALUATION_ROUNDS = 5
POSE_RELATIVE_TO = dict(none=0, first=1, previous=2, largest_loop=3, inaffected=4)   # RGBDFE_POSE_RELATIVE_TO_*
PRUNE_VERDICTS = ("kept", "removed", "discounted", "zero_motion")                    # RGBDFE_PRUNE_*


class PoseGraphRound(C.Structure):   # rgbdfe_pose_graph_round
    _fields_ = [("chi2", C.c_double), ("iterations", C.c_int32), ("pruned", C.c_int32), ("launches", C.c_int64),
                ("readbacks", C.c_int64), ("upload_seconds", C.c_double), ("seconds", C.c_double)]


class PoseGraphEvaluation(C.Structure):   # rgbdfe_pose_graph_evaluation
    _fields_ = [("round", PoseGraphRound * POSE_GRAPH_EVALUATION_ROUNDS)]


class PoseGraphReport(C.Structure):   # rgbdfe_pose_graph_report
    _fields_ = [("iterations", C.c_int32), ("recorded", C.c_int32), ("chi2", C.c_double), ("launches", C.c_int64),
                ("readbacks", C.c_int64), ("upload_seconds", C.c_double), ("total_seconds", C.c_double),
                ("it", PoseGraphIteration * POSE_GRAPH_REPORT_ITERATIONS)]


class IcpParams(C.Structure):   # rgbdfe_icp_params
    _fields_ = [("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double), ("max_iterations", C.c_int32), ("desired_size", C.c_int32)]


SLAM_MAX_CANDIDATES = 64   # RGBDFE_SLAM_MAX_CANDIDATES
SLAM_STATUS = {1: "too_few_features", 2: "first", 3: "motion_out_of_bounds", 4: "added", 5: "no_match",
               6: "replaced_first"}                                                  # RGBDFE_SLAM_*
SLAM_VERDICTS = ("no_edge", "accepted", "not_small", "too_short", "withdrawn", "out_of_bounds")   # RGBDFE_SLAM_VERDICT_*
SLAM_VERDICT_ICP = 16
SLAM_RESULT_ICP, SLAM_RESULT_WITHDRAWN = 1, 2
SLAM_CONSTANT_NONE, SLAM_CONSTANT_ADDED, SLAM_CONSTANT_SKIPPED = 0, 1, 2


class SlamParams(C.Structure):   # rgbdfe_slam_params
    _fields_ = [("min_matches", C.c_int32), ("predecessor_candidates", C.c_int32), ("neighbor_candidates", C.c_int32),
                ("min_sampled_candidates", C.c_int32), ("geodesic_depth", C.c_int32), ("keep_all_nodes", C.c_int32),
                ("keep_good_nodes", C.c_int32), ("clear_non_keyframes", C.c_int32),
                ("create_cloud_every_nth_node", C.c_int32), ("optimizer_skip_step", C.c_int32), ("use_icp", C.c_int32),
                ("emm__skip_step", C.c_int32), ("have_odometry_frame", C.c_int32), ("seed", C.c_uint32),
                ("min_translation_meter", C.c_double), ("min_rotation_degree", C.c_double),
                ("max_translation_meter", C.c_double), ("max_rotation_degree", C.c_double),
                ("optimizer_iterations", C.c_double), ("observability_threshold", C.c_double),
                ("init_base_pose", C.c_double * 16)]


class SlamStep(C.Structure):   # rgbdfe_slam_step
    _fields_ = [("status", C.c_int32), ("id", C.c_int32), ("found", C.c_int32), ("initial_id", C.c_int32),
                ("initial_verdict", C.c_int32), ("n_candidates", C.c_int32),
                ("candidates", C.c_int32 * SLAM_MAX_CANDIDATES), ("verdicts", C.c_uint8 * SLAM_MAX_CANDIDATES),
                ("best_id1", C.c_int32), ("best_id2", C.c_int32), ("best_n_inl", C.c_int32),
                ("predecessor_matched", C.c_int32), ("edge_to_keyframe", C.c_int32), ("keyframe_added", C.c_int32),
                ("cleared_first", C.c_int32), ("cleared_last", C.c_int32), ("released_slot", C.c_int32),
                ("constant_position", C.c_int32), ("cloud_released", C.c_int32), ("has_broadcast_pose", C.c_int32),
                ("optimize_due", C.c_int32), ("optimized", C.c_int32), ("lm_iterations", C.c_int32),
                ("sequential_edges", C.c_int32), ("loop_closure_edges", C.c_int32), ("stats_launches", C.c_int32),
                ("motion_estimate", C.c_double * 16), ("broadcast_pose", C.c_double * 16), ("chi2", C.c_double),
                ("seconds", C.c_double * 4)]


class RgbdfeDisplayParams(C.Structure):   # rgbdfe_display_params
    _fields_ = [("display_type", C.c_int32), ("visualization_skip_step", C.c_int32),
                ("squared_meshing_threshold", C.c_double), ("maximum_depth", C.c_double)]


DISPLAY_POINTS, DISPLAY_TRIANGLES, DISPLAY_TRIANGLE_STRIP = 0, 1, 2


class RgbdfeRenderParams(C.Structure):   # rgbdfe_render_params
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("view", C.c_double * 16), ("projection", C.c_double * 16),
                ("gl_point_size", C.c_double), ("cull", C.c_int32), ("clear_rgba", C.c_uint8 * 4),
                ("max_vertices_in_flight", C.c_int64)]


# rgbdfe_icp_report
ICP_REPORT_DTYPE = np.dtype([("converged", "<i4"), ("state", "<i4"), ("iterations", "<i4"), ("correspondences", "<i4"),
                             ("mse", "<f8"), ("n_source", "<i4"), ("n_target", "<i4"), ("launches", "<i8"),
                             ("readbacks", "<i8")])
ICP_NO_CORRESPONDENCES, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE = 1, 2, 3, 4, 5


# rgbdfe_octomap_leaf
OCTOMAP_LEAF_DTYPE = np.dtype([("key", "<u2", (3,)), ("zero0", "<u2"), ("log_odds", "<f4"), ("rgb", "u1", (3,)),
                               ("zero1", "u1")])

# rgbdfe_octomap_ray_hit: the result of one ray (status: OCTOMAP_RAY_*)
OCTOMAP_RAY_HIT_DTYPE = np.dtype([("status", "<i4"), ("steps", "<u4"), ("key", "<u2", (3,)), ("zero0", "<u2"),
                                  ("centre", "<f4", (3,)), ("log_odds", "<f4"), ("rgb", "u1", (3,)), ("zero1", "u1")])
assert OCTOMAP_RAY_HIT_DTYPE.itemsize == 36
(OCTOMAP_RAY_HIT, OCTOMAP_RAY_UNKNOWN, OCTOMAP_RAY_OUT_OF_RANGE, OCTOMAP_RAY_OUT_OF_BOUNDS, OCTOMAP_RAY_BAD_ORIGIN,
 OCTOMAP_RAY_BAD_DIRECTION, OCTOMAP_RAY_STEP_LIMIT) = range(1, 8)
# rgbdfe_octomap_node: the 8 bytes of a node in an .ot file
OCTOMAP_NODE_DTYPE = np.dtype([("log_odds", "<f4"), ("rgb", "u1", (3,)), ("children", "u1")])

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4")])

# numpy view of the same POD (used for bulk result handling and the all-gather payload)
RESULT_DTYPE = np.dtype([
    ("id1", "<i4"), ("id2", "<i4"), ("n_all", "<i4"), ("n_inl", "<i4"), ("rmse", "<f4"),
    ("trafo", "<f4", (16,)), ("pad0", "<u4"), ("info_scale", "<f8"),
    ("valid_iterations", "<i4"), ("real_iterations", "<i4"),
    ("all_q", "<u2", (RGBDFE_MAX_MATCHES,)), ("all_t", "<u2", (RGBDFE_MAX_MATCHES,)),
    ("all_hd", "u1", (RGBDFE_MAX_MATCHES,)), ("inlier_mask", "<u8", (RGBDFE_MASK_WORDS,)),
], align=True)

# rgbdfe_compact_result: the record without its all_matches lists (the default multi-GPU gather payload, 144 B)
COMPACT_DTYPE = np.dtype([
    ("id1", "<i4"), ("id2", "<i4"), ("n_all", "<i4"), ("n_inl", "<i4"), ("rmse", "<f4"),
    ("trafo", "<f4", (16,)), ("pad0", "<u4"), ("info_scale", "<f8"),
    ("valid_iterations", "<i4"), ("real_iterations", "<i4"), ("inlier_mask", "<u8", (RGBDFE_MASK_WORDS,)),
], align=True)
COMPACT_FIELDS = [n for n in COMPACT_DTYPE.names]
# rgbdfe_inlier_header: the leading 104 bytes of a record, pad0 = first_inlier
INLIER_HEADER_DTYPE = np.dtype([
    ("id1", "<i4"), ("id2", "<i4"), ("n_all", "<i4"), ("n_inl", "<i4"), ("rmse", "<f4"),
    ("trafo", "<f4", (16,)), ("first_inlier", "<u4"), ("info_scale", "<f8"),
    ("valid_iterations", "<i4"), ("real_iterations", "<i4"),
], align=True)


def compact_of(records: np.ndarray) -> np.ndarray:
    """Host twin of compact_pack_kernel: RESULT_DTYPE records -> COMPACT_DTYPE records (tests)."""
    out = np.zeros(len(records), COMPACT_DTYPE)
    for f in COMPACT_FIELDS:
        out[f] = records[f]
    return out


def inlier_stream_of(records: np.ndarray, n_headers: int):
    """Host twin of rgbdfe_pack_inliers: RESULT_DTYPE records -> (headers INLIER_HEADER_DTYPE [n_headers], list uint32 [total])."""
    n = len(records)
    hdr = np.zeros(n_headers, INLIER_HEADER_DTYPE)
    hdr["id1"][n:] = -1
    hdr["id2"][n:] = -1
    for f in INLIER_HEADER_DTYPE.names:
        if f != "first_inlier":
            hdr[f][:n] = records[f]
    bits = np.unpackbits(np.ascontiguousarray(records["inlier_mask"]).view(np.uint8).reshape(n, -1), axis=1, bitorder="little") \
        if n else np.zeros((0, 64 * RGBDFE_MASK_WORDS), np.uint8)
    counts = bits.sum(1).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(counts)])
    hdr["first_inlier"][:n] = first[:n]
    hdr["first_inlier"][n:] = first[n]
    lst = np.zeros(int(first[n]), np.uint32)
    for k in range(n):
        m = np.nonzero(bits[k])[0]
        lst[first[k]:first[k + 1]] = records["all_q"][k][m].astype(np.uint32) | (records["all_t"][k][m].astype(np.uint32) << 16)
    return hdr, lst


def parse_inlier_stream(buf: np.ndarray, n_headers: int, total: int):
    """A shard's inlier stream (uint8) -> (headers, list uint32 [total])."""
    b = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    hb = n_headers * INLIER_HEADER_DTYPE.itemsize
    return b[:hb].view(INLIER_HEADER_DTYPE), b[hb:hb + 4 * total].view(np.uint32)


def inlier_pairs(hdr, lst, k):
    """(query rows, train rows) of pair k's inlier matches from a parsed inlier stream."""
    a = int(hdr["first_inlier"][k])
    e = lst[a:a + int(hdr["n_inl"][k])]
    return (e & 0xFFFF).astype(np.int32), (e >> 16).astype(np.int32)


_lib = None


class RgbdfeError(RuntimeError):
    pass


CLOUD_FILE_PCD, CLOUD_FILE_PLY = 0, 1   # RGBDFE_CLOUD_FILE_*


class MapFileStats(C.Structure):   # rgbdfe_map_file_stats
    _fields_ = [("points", C.c_int64), ("bytes_written", C.c_int64), ("format", C.c_int32), ("groups", C.c_int32),
                ("device_scratch_bytes", C.c_int64), ("pinned_bytes", C.c_int64), ("table_bytes", C.c_int64)]


class CloudFileHeader(C.Structure):   # rgbdfe_cloud_file_header
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32),
                ("points", C.c_int64), ("header_bytes", C.c_int64), ("data_bytes", C.c_int64),
                ("viewpoint", C.c_float * 7), ("reserved2", C.c_float)]


def load():
    """Load librgbdfe.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RgbdfeError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # PyTorch wheels bundle their own libamdhip64; two HIP runtimes in one process cannot both see the
    # GPU.  Loading torch first makes its runtime the process-wide one (librgbdfe.so then binds to it
    # through the soname), whatever order the caller imports things in.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    i32 = C.c_int32
    ctx = vp
    L.rgbdfe_default_config.restype = None
    L.rgbdfe_default_config.argtypes = [C.POINTER(RgbdfeConfig)]
    L.rgbdfe_create.restype = C.c_int
    L.rgbdfe_create.argtypes = [C.POINTER(RgbdfeConfig), C.POINTER(vp)]
    L.rgbdfe_destroy.restype = None
    L.rgbdfe_destroy.argtypes = [ctx]
    L.rgbdfe_set_params.restype = C.c_int
    L.rgbdfe_set_params.argtypes = [ctx, C.POINTER(RgbdfeParams)]
    L.rgbdfe_status_string.restype = C.c_char_p
    L.rgbdfe_status_string.argtypes = [C.c_int]
    L.rgbdfe_last_error.restype = C.c_char_p
    L.rgbdfe_last_error.argtypes = [ctx]
    L.rgbdfe_upload_node.restype = C.c_int
    L.rgbdfe_upload_node.argtypes = [ctx, i32, vp, vp, i32]
    L.rgbdfe_upload_nodes.restype = C.c_int
    L.rgbdfe_upload_nodes.argtypes = [ctx, i32, vp, vp, vp, vp]
    L.rgbdfe_upload_node_device.restype = C.c_int
    L.rgbdfe_upload_node_device.argtypes = [ctx, i32, vp, vp, i32, vp]
    L.rgbdfe_release_node.restype = C.c_int
    L.rgbdfe_release_node.argtypes = [ctx, i32]
    L.rgbdfe_node_count.restype = C.c_int
    L.rgbdfe_node_count.argtypes = [ctx, i32]
    L.rgbdfe_match_node_pairs.restype = C.c_int
    L.rgbdfe_match_node_pairs.argtypes = [ctx, i32, vp, i32, vp]
    L.rgbdfe_match_pair_list.restype = C.c_int
    L.rgbdfe_match_pair_list.argtypes = [ctx, vp, vp, i32, vp]
    L.rgbdfe_match_pair_list_device.restype = C.c_int
    L.rgbdfe_match_pair_list_device.argtypes = [ctx, vp, vp, i32, vp, vp]
    L.rgbdfe_submit_pair_list.restype = C.c_int
    L.rgbdfe_submit_pair_list.argtypes = [ctx, vp, vp, i32, vp, C.POINTER(C.c_int64)]
    L.rgbdfe_wait_ticket.restype = C.c_int
    L.rgbdfe_wait_ticket.argtypes = [ctx, C.c_int64, vp]
    L.rgbdfe_submit_pair_list_host.restype = C.c_int
    L.rgbdfe_submit_pair_list_host.argtypes = [ctx, vp, vp, i32, vp, C.c_size_t, C.c_int, C.POINTER(C.c_int64)]
    L.rgbdfe_wait_host.restype = C.c_int
    L.rgbdfe_wait_host.argtypes = [ctx, C.c_int64, C.POINTER(C.c_int64)]
    L.rgbdfe_wait_host_into.restype = C.c_int
    L.rgbdfe_wait_host_into.argtypes = [ctx, C.c_int64, vp, C.c_size_t, C.POINTER(C.c_int64)]
    L.rgbdfe_upload_sift_node.restype = C.c_int
    L.rgbdfe_upload_sift_node.argtypes = [ctx, i32, vp, vp, i32]
    L.rgbdfe_match_sift_pair_list.restype = C.c_int
    L.rgbdfe_match_sift_pair_list.argtypes = [ctx, vp, vp, i32, vp, vp]
    L.rgbdfe_submit_sift_pair_list.restype = C.c_int
    L.rgbdfe_submit_sift_pair_list.argtypes = [ctx, vp, vp, i32, vp, vp, C.POINTER(C.c_int64)]
    L.rgbdfe_sift_match_nodes.restype = C.c_int
    L.rgbdfe_sift_match_nodes.argtypes = [ctx, i32, i32, vp, vp, vp, C.POINTER(i32)]
    L.rgbdfe_detector_configure.restype = C.c_int
    L.rgbdfe_detector_configure.argtypes = [ctx, i32, i32, i32]
    L.rgbdfe_detector_thresholds.restype = C.c_int
    L.rgbdfe_detector_thresholds.argtypes = [ctx, vp, C.POINTER(i32)]
    L.rgbdfe_detect_describe.restype = C.c_int
    L.rgbdfe_detect_describe.argtypes = [ctx, vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double,
                                         C.c_double, C.c_double, vp, vp, vp, C.POINTER(i32)]
    L.rgbdfe_orb_detect.restype = C.c_int
    L.rgbdfe_orb_detect.argtypes = [ctx, vp, vp, i32, i32, i32, vp, i32, C.POINTER(i32)]
    L.rgbdfe_set_detector_type.restype = C.c_int
    L.rgbdfe_set_detector_type.argtypes = [ctx, i32]
    L.rgbdfe_fast_detect.restype = C.c_int
    L.rgbdfe_fast_detect.argtypes = [ctx, vp, vp, i32, i32, i32, vp, i32, C.POINTER(i32)]
    L.rgbdfe_orb_compute.restype = C.c_int
    L.rgbdfe_orb_compute.argtypes = [ctx, vp, i32, i32, vp, i32, vp, C.POINTER(i32)]
    L.rgbdfe_synchronize.restype = C.c_int
    L.rgbdfe_synchronize.argtypes = [ctx]
    L.rgbdfe_hamming_nn_nodes.restype = C.c_int
    L.rgbdfe_hamming_nn_nodes.argtypes = [ctx, i32, i32, vp, vp]
    L.rgbdfe_hamming_nn_host.restype = C.c_int
    L.rgbdfe_hamming_nn_host.argtypes = [ctx, vp, i32, vp, i32, vp, vp]
    L.rgbdfe_project_to_3d.restype = C.c_int
    L.rgbdfe_project_to_3d.argtypes = [ctx, vp, i32, vp, i32, i32, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_double, i32, vp, vp,
                                       C.POINTER(i32)]
    L.rgbdfe_project_to_3d_cloud.restype = C.c_int
    L.rgbdfe_project_to_3d_cloud.argtypes = [ctx, vp, i32, vp, i32, i32, C.c_double, i32, vp, vp, C.POINTER(i32)]
    L.rgbdfe_set_feature_min_depth.restype = C.c_int
    L.rgbdfe_set_feature_min_depth.argtypes = [ctx, i32]
    L.rgbdfe_project_to_3d_min_depth.restype = C.c_int
    L.rgbdfe_project_to_3d_min_depth.argtypes = [ctx, vp, vp, i32, vp, i32, i32, C.c_double, C.c_double, C.c_double,
                                                 C.c_double, C.c_double, i32, vp, vp, C.POINTER(i32)]
    L.rgbdfe_detect_describe_batch.restype = C.c_int
    L.rgbdfe_detect_describe_batch.argtypes = [ctx, i32, vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double,
                                               C.c_double, C.c_double, i32, vp, vp, vp, vp]
    L.rgbdfe_detect_describe_batch_nodes.restype = C.c_int
    L.rgbdfe_detect_describe_batch_nodes.argtypes = [ctx, i32, vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double,
                                                     C.c_double, C.c_double, i32, vp, vp, vp, vp, vp]
    L.rgbdfe_detect_describe_cloud.restype = C.c_int
    L.rgbdfe_detect_describe_cloud.argtypes = [ctx, vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, C.POINTER(i32)]
    L.rgbdfe_place_recognition.restype = C.c_int
    L.rgbdfe_place_recognition.argtypes = [ctx, i32, vp, i32, i32, i32, i32, vp, vp, C.POINTER(i32)]
    L.rgbdfe_place_recognition_batch.restype = C.c_int
    L.rgbdfe_place_recognition_batch.argtypes = [ctx, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp]
    L.rgbdfe_upload_float_node.restype = C.c_int
    L.rgbdfe_upload_float_node.argtypes = [ctx, i32, vp, i32, vp, i32]
    L.rgbdfe_match_flann_pair_list.restype = C.c_int
    L.rgbdfe_match_flann_pair_list.argtypes = [ctx, vp, vp, i32, C.c_double, vp, vp]
    L.rgbdfe_upload_node_keypoints.restype = C.c_int
    L.rgbdfe_upload_node_keypoints.argtypes = [ctx, i32, vp, i32]
    L.rgbdfe_sift_node_features.restype = C.c_int
    L.rgbdfe_sift_node_features.argtypes = [ctx, vp, i32, vp, vp, i32, i32, C.c_double, C.c_double,
                                            C.c_double, C.c_double, C.c_double, i32, i32, vp, vp, vp, vp,
                                            C.POINTER(i32)]
    L.rgbdfe_sift_node_features_min_depth.restype = C.c_int
    L.rgbdfe_sift_node_features_min_depth.argtypes = [ctx, vp, vp, i32, vp, vp, i32, i32, C.c_double, C.c_double,
                                                      C.c_double, C.c_double, C.c_double, i32, i32, vp, vp, vp, vp,
                                                      C.POINTER(i32)]
    L.rgbdfe_host_register.restype = C.c_int
    L.rgbdfe_host_register.argtypes = [ctx, vp, C.c_size_t]
    L.rgbdfe_host_unregister.restype = C.c_int
    L.rgbdfe_host_unregister.argtypes = [ctx, vp]
    L.rgbdfe_depth_to_mono8.restype = C.c_int
    L.rgbdfe_depth_to_mono8.argtypes = [ctx, vp, i32, i32, i32, vp, vp]
    L.rgbdfe_upload_node_cloud.restype = C.c_int
    L.rgbdfe_upload_node_cloud.argtypes = [ctx, i32, vp, i32, i32, vp, i32, i32, C.c_double, C.c_double,
                                           C.c_double, C.c_double, C.c_double, C.c_double, i32, vp]
    L.rgbdfe_release_node_cloud.restype = C.c_int
    L.rgbdfe_release_node_cloud.argtypes = [ctx, i32]
    L.rgbdfe_observation_likelihood.restype = C.c_int
    L.rgbdfe_observation_likelihood.argtypes = [ctx, i32, vp, vp, vp, i32, vp]
    L.rgbdfe_assemble_map.restype = C.c_int
    L.rgbdfe_assemble_map.argtypes = [ctx, i32, vp, vp, C.c_double, i32, vp, C.c_int64, C.POINTER(C.c_int64), vp]
    L.rgbdfe_assemble_map_device.restype = C.c_int
    L.rgbdfe_assemble_map_device.argtypes = [ctx, i32, vp, vp, C.c_double, i32, vp, C.c_int64, C.POINTER(C.c_int64), vp, vp]
    L.rgbdfe_display_default_params.restype = None
    L.rgbdfe_display_default_params.argtypes = [C.POINTER(RgbdfeDisplayParams)]
    L.rgbdfe_display_geometry.restype = C.c_int
    L.rgbdfe_display_geometry.argtypes = [ctx, i32, vp, vp, C.POINTER(RgbdfeDisplayParams), vp, C.c_int64, C.POINTER(C.c_int64),
                                          vp, vp, C.c_int64, C.POINTER(C.c_int64), vp, vp]
    L.rgbdfe_display_geometry_device.restype = C.c_int
    L.rgbdfe_display_geometry_device.argtypes = L.rgbdfe_display_geometry.argtypes + [vp]
    dbl = C.c_double
    L.rgbdfe_render_default_params.restype = None
    L.rgbdfe_render_default_params.argtypes = [C.POINTER(RgbdfeRenderParams)]
    L.rgbdfe_render_nodes.restype = C.c_int
    L.rgbdfe_render_nodes.argtypes = [ctx, i32, vp, vp, C.POINTER(RgbdfeDisplayParams), C.POINTER(RgbdfeRenderParams), vp, vp, vp, vp]
    L.rgbdfe_render_nodes_device.restype = C.c_int
    L.rgbdfe_render_nodes_device.argtypes = L.rgbdfe_render_nodes.argtypes + [vp]
    L.rgbdfe_render_perspective.restype = None
    L.rgbdfe_render_perspective.argtypes = [dbl, dbl, dbl, dbl, vp]
    L.rgbdfe_render_viewer_view.restype = None
    L.rgbdfe_render_viewer_view.argtypes = [dbl] * 7 + [vp, vp]
    L.rgbdfe_render_sensor_camera.restype = None
    L.rgbdfe_render_sensor_camera.argtypes = [dbl, dbl, dbl, dbl, i32, i32, dbl, dbl, vp, vp, vp]
    L.rgbdfe_render_unproject.restype = C.c_int
    L.rgbdfe_render_unproject.argtypes = [dbl, dbl, dbl, vp, vp, i32, i32, vp]
    L.rgbdfe_render_fragment_stats.restype = C.c_int
    L.rgbdfe_render_fragment_stats.argtypes = [ctx, i32, vp]
    L.rgbdfe_download_node_cloud.restype = C.c_int
    L.rgbdfe_download_node_cloud.argtypes = [ctx, i32, vp, C.c_int64, C.POINTER(i32), C.POINTER(i32)]
    L.rgbdfe_voxel_filter.restype = C.c_int
    L.rgbdfe_voxel_filter.argtypes = [ctx, vp, C.c_int64, C.c_double, vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(i32)]
    L.rgbdfe_voxel_filter_device.restype = C.c_int
    L.rgbdfe_voxel_filter_device.argtypes = [ctx, vp, C.c_int64, C.c_double, vp, C.c_int64, C.POINTER(C.c_int64),
                                             C.POINTER(i32), vp]
    L.rgbdfe_reduce_node_cloud.restype = C.c_int
    L.rgbdfe_reduce_node_cloud.argtypes = [ctx, i32, C.c_double, C.POINTER(C.c_int64), C.POINTER(i32)]
    omap = vp
    L.rgbdfe_octomap_default_params.restype = None
    L.rgbdfe_octomap_default_params.argtypes = [C.POINTER(OctomapParams)]
    L.rgbdfe_octomap_create.restype = C.c_int
    L.rgbdfe_octomap_create.argtypes = [ctx, C.POINTER(OctomapParams), C.c_int64, C.POINTER(vp)]
    L.rgbdfe_octomap_destroy.restype = None
    L.rgbdfe_octomap_destroy.argtypes = [omap]
    L.rgbdfe_octomap_reset.restype = C.c_int
    L.rgbdfe_octomap_reset.argtypes = [omap]
    L.rgbdfe_octomap_reserve.restype = C.c_int
    L.rgbdfe_octomap_reserve.argtypes = [omap, C.c_int64]
    L.rgbdfe_octomap_insert_nodes.restype = C.c_int
    L.rgbdfe_octomap_insert_nodes.argtypes = [omap, i32, vp, vp, C.c_double, C.POINTER(i32)]
    L.rgbdfe_octomap_insert_cloud.restype = C.c_int
    L.rgbdfe_octomap_insert_cloud.argtypes = [omap, vp, C.c_int64, vp, C.c_double]
    L.rgbdfe_octomap_size.restype = C.c_int
    L.rgbdfe_octomap_size.argtypes = [omap, C.POINTER(C.c_int64)]
    L.rgbdfe_octomap_leaves.restype = C.c_int
    L.rgbdfe_octomap_leaves.argtypes = [omap, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rgbdfe_octomap_stats.restype = C.c_int
    L.rgbdfe_octomap_stats.argtypes = [omap, vp, i32]
    L.rgbdfe_octomap_tree.restype = C.c_int
    L.rgbdfe_octomap_tree.argtypes = [omap, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rgbdfe_octomap_tree_device.restype = C.c_int
    L.rgbdfe_octomap_tree_device.argtypes = [omap, vp, C.c_int64, C.POINTER(C.c_int64), vp]
    L.rgbdfe_octomap_nodes_at_depth.restype = C.c_int
    L.rgbdfe_octomap_nodes_at_depth.argtypes = [omap, i32, C.c_float, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rgbdfe_octomap_write.restype = C.c_int
    L.rgbdfe_octomap_write.argtypes = [omap, C.c_char_p]
    L.rgbdfe_octomap_set_leaves.restype = C.c_int
    L.rgbdfe_octomap_set_leaves.argtypes = [omap, vp, C.c_int64]
    L.rgbdfe_octomap_read.restype = C.c_int
    L.rgbdfe_octomap_read.argtypes = [omap, C.c_char_p]
    L.rgbdfe_sizeof_octomap_ray_hit.restype = C.c_int
    L.rgbdfe_sizeof_octomap_ray_hit.argtypes = []
    L.rgbdfe_octomap_occupied_log_odds.restype = C.c_int
    L.rgbdfe_octomap_occupied_log_odds.argtypes = [omap, C.POINTER(C.c_float)]
    L.rgbdfe_octomap_search.restype = C.c_int
    L.rgbdfe_octomap_search.argtypes = [omap, vp, C.c_int64, vp, vp]
    L.rgbdfe_octomap_cast_rays.restype = C.c_int
    L.rgbdfe_octomap_cast_rays.argtypes = [omap, vp, vp, C.c_int64, i32, C.c_double, C.c_float, vp]
    view = [omap, vp] + [C.c_double] * 4 + [i32, i32, i32, C.c_double, C.c_float]
    L.rgbdfe_octomap_view_cloud.restype = C.c_int
    L.rgbdfe_octomap_view_cloud.argtypes = view + [vp, vp]
    L.rgbdfe_octomap_view_cloud_device.restype = C.c_int
    L.rgbdfe_octomap_view_cloud_device.argtypes = view + [vp, vp, vp]
    L.rgbdfe_observation_criterion_met.restype = C.c_int
    L.rgbdfe_observation_criterion_met.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                                                   C.POINTER(C.c_double)]
    L.rgbdfe_set_latency_mode.restype = C.c_int
    L.rgbdfe_set_latency_mode.argtypes = [ctx, i32, i32]
    L.rgbdfe_set_profiling.restype = C.c_int
    L.rgbdfe_set_profiling.argtypes = [ctx, C.c_int]
    L.rgbdfe_get_kernel_time.restype = C.c_int
    L.rgbdfe_get_kernel_time.argtypes = [ctx, C.c_int, C.POINTER(C.c_double),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rgbdfe_reset_kernel_time.restype = C.c_int
    L.rgbdfe_reset_kernel_time.argtypes = [ctx]
    L.rgbdfe_set_graph_capture.restype = C.c_int
    L.rgbdfe_set_graph_capture.argtypes = [ctx, C.c_int]
    L.rgbdfe_graph_stats.restype = C.c_int
    L.rgbdfe_graph_stats.argtypes = [ctx, C.POINTER(C.c_int64), C.c_int32]
    L.rgbdfe_create_multi.restype = C.c_int
    L.rgbdfe_create_multi.argtypes = [C.POINTER(RgbdfeConfig), vp, i32, C.POINTER(vp)]
    L.rgbdfe_device_count.restype = C.c_int
    L.rgbdfe_device_count.argtypes = [ctx]
    L.rgbdfe_device_context.restype = vp
    L.rgbdfe_device_context.argtypes = [ctx, i32]
    L.rgbdfe_match_pair_list_allgather.restype = C.c_int
    L.rgbdfe_match_pair_list_allgather.argtypes = [ctx, vp, vp, i32, vp, C.POINTER(i32)]
    L.rgbdfe_match_pair_list_allgather_edges.restype = C.c_int
    L.rgbdfe_match_pair_list_allgather_edges.argtypes = [ctx, vp, vp, i32, vp, vp, vp, C.POINTER(i32)]
    L.rgbdfe_group_submit_us.restype = C.c_int
    L.rgbdfe_group_submit_us.argtypes = [ctx, C.POINTER(C.c_double)]
    L.rgbdfe_gather_transport.restype = C.c_char_p
    L.rgbdfe_gather_transport.argtypes = [ctx]
    L.rgbdfe_gather_exchanges.restype = C.c_int
    L.rgbdfe_gather_exchanges.argtypes = [ctx]
    L.rgbdfe_set_hamming_mode.restype = C.c_int
    L.rgbdfe_set_hamming_mode.argtypes = [ctx, i32]
    L.rgbdfe_hamming_wide_last.restype = C.c_int
    L.rgbdfe_hamming_wide_last.argtypes = [ctx]
    L.rgbdfe_set_hamming_shape.restype = C.c_int
    L.rgbdfe_set_hamming_shape.argtypes = [ctx, i32]
    L.rgbdfe_hamming_shape_last.restype = C.c_int
    L.rgbdfe_hamming_shape_last.argtypes = [ctx]
    L.rgbdfe_match_pair_list_allgather_compact.restype = C.c_int
    L.rgbdfe_match_pair_list_allgather_compact.argtypes = [ctx, vp, vp, i32, vp, C.POINTER(i32)]
    L.rgbdfe_pack_compact.restype = C.c_int
    L.rgbdfe_pack_compact.argtypes = [ctx, vp, i32, vp, vp]
    L.rgbdfe_sizeof_compact_result.restype = C.c_int
    L.rgbdfe_match_pair_list_allgather_inliers.restype = C.c_int
    L.rgbdfe_match_pair_list_allgather_inliers.argtypes = [ctx, vp, vp, i32, vp, C.POINTER(i32), vp, C.POINTER(C.c_int64)]
    L.rgbdfe_pack_inliers.restype = C.c_int
    L.rgbdfe_pack_inliers.argtypes = [ctx, vp, i32, i32, vp, vp, vp]
    L.rgbdfe_sizeof_inlier_header.restype = C.c_int
    if L.rgbdfe_sizeof_inlier_header() != INLIER_HEADER_DTYPE.itemsize:
        raise RgbdfeError("rgbdfe_inlier_header layout mismatch between librgbdfe.so and the binding")
    if L.rgbdfe_sizeof_compact_result() != COMPACT_DTYPE.itemsize:
        raise RgbdfeError("rgbdfe_compact_result layout mismatch between librgbdfe.so and the binding")
    L.rgbdfe_sift_detect.restype = C.c_int
    L.rgbdfe_sift_detect.argtypes = [ctx, vp, vp, i32, i32, i32, vp, vp, i32, C.POINTER(i32)]
    L.rgbdfe_sift_describe.restype = C.c_int
    L.rgbdfe_sift_describe.argtypes = [ctx, vp, i32, i32, vp, i32, vp]
    L.rgbdfe_sift_detect_batch.restype = C.c_int
    L.rgbdfe_sift_detect_batch.argtypes = [ctx, i32, vp, i32, i32, i32, i32, vp, vp, vp]
    L.rgbdfe_sift_detect_batch_nodes.restype = C.c_int
    L.rgbdfe_sift_detect_batch_nodes.argtypes = [ctx, i32, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double,
                                                 C.c_double, i32, i32, vp, i32, vp, vp, vp, vp]
    L.rgbdfe_detect.restype = C.c_int
    L.rgbdfe_detect.argtypes = [ctx, vp, vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.rgbdfe_detect_sift_describe.restype = C.c_int
    L.rgbdfe_detect_sift_describe.argtypes = [ctx, vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double,
                                              C.c_double, i32, vp, vp, vp, vp, C.POINTER(i32)]
    L.rgbdfe_detect_sift_describe_batch_nodes.restype = C.c_int
    L.rgbdfe_detect_sift_describe_batch_nodes.argtypes = [ctx, i32, vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double,
                                                          C.c_double, C.c_double, i32, vp, i32, vp, vp, vp, vp]
    L.rgbdfe_sift_detect_orb_describe.restype = C.c_int
    L.rgbdfe_sift_detect_orb_describe.argtypes = [ctx, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double,
                                                  C.c_double, i32, vp, vp, vp, C.POINTER(i32)]
    L.rgbdfe_sift_detect_orb_describe_batch_nodes.restype = C.c_int
    L.rgbdfe_sift_detect_orb_describe_batch_nodes.argtypes = [ctx, i32, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double,
                                                              C.c_double, C.c_double, i32, vp, i32, vp, vp, vp, vp]
    L.rgbdfe_sizeof_sensor_frame.restype = C.c_int
    if L.rgbdfe_sizeof_sensor_frame() != C.sizeof(RgbdfeSensorFrame):
        raise RgbdfeError("rgbdfe_sensor_frame layout mismatch between librgbdfe.so and the binding")
    L.rgbdfe_ingest_frame.restype = C.c_int
    L.rgbdfe_ingest_frame.argtypes = [ctx, C.POINTER(RgbdfeSensorFrame), vp, vp, vp]
    L.rgbdfe_sensor_detect_describe.restype = C.c_int
    L.rgbdfe_sensor_detect_describe.argtypes = [ctx, C.POINTER(RgbdfeSensorFrame), C.c_double, C.c_double, C.c_double, C.c_double,
                                                C.c_double, vp, vp, vp, C.POINTER(i32)]
    L.rgbdfe_sensor_detect_describe_batch_nodes.restype = C.c_int
    L.rgbdfe_sensor_detect_describe_batch_nodes.argtypes = [ctx, i32, C.POINTER(RgbdfeSensorFrame), C.c_double, C.c_double,
                                                            C.c_double, C.c_double, C.c_double, i32, vp, vp, vp, vp, vp,
                                                            C.POINTER(RgbdfeSensorCloud)]
    L.rgbdfe_sift_geometry.restype = C.c_int
    L.rgbdfe_sift_geometry.argtypes = [ctx] + [C.POINTER(i32)] * 4
    L.rgbdfe_sift_debug_plane.restype = C.c_int
    L.rgbdfe_sift_debug_plane.argtypes = [ctx, i32, i32, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.rgbdfe_sift_debug_candidates.restype = C.c_int
    L.rgbdfe_sift_debug_candidates.argtypes = [ctx, i32, i32, vp, i32, C.POINTER(i32)]
    L.rgbdfe_sizeof_match_result.restype = C.c_int
    L.rgbdfe_abi_version.restype = C.c_int
    if L.rgbdfe_sizeof_match_result() != C.sizeof(RgbdfeMatchResult) or \
            RESULT_DTYPE.itemsize != C.sizeof(RgbdfeMatchResult):
        raise RgbdfeError("rgbdfe_match_result layout mismatch between librgbdfe.so and the binding")
    RAND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
    L.rgbdfe_rand_fn = RAND_FN
    L.rgbdfe_pose_graph_create.restype = vp
    L.rgbdfe_pose_graph_create.argtypes = []
    L.rgbdfe_pose_graph_destroy.restype = None
    L.rgbdfe_pose_graph_destroy.argtypes = [vp]
    L.rgbdfe_pose_graph_add_node.restype = C.c_int
    L.rgbdfe_pose_graph_add_node.argtypes = [vp, i32, i32, i32, i32]
    L.rgbdfe_pose_graph_add_edge.restype = C.c_int
    L.rgbdfe_pose_graph_add_edge.argtypes = [vp, i32, i32]
    L.rgbdfe_pose_graph_set_matchable.restype = C.c_int
    L.rgbdfe_pose_graph_set_matchable.argtypes = [vp, i32, i32]
    L.rgbdfe_pose_graph_set_estimate.restype = C.c_int
    L.rgbdfe_pose_graph_set_estimate.argtypes = [vp, i32, vp]
    L.rgbdfe_pose_graph_get_estimate.restype = C.c_int
    L.rgbdfe_pose_graph_get_estimate.argtypes = [vp, i32, vp]
    L.rgbdfe_pose_graph_set_fixed.restype = C.c_int
    L.rgbdfe_pose_graph_set_fixed.argtypes = [vp, i32, i32]
    L.rgbdfe_pose_graph_add_edge_se3.restype = C.c_int
    L.rgbdfe_pose_graph_add_edge_se3.argtypes = [vp, i32, i32, vp, vp, i32]
    L.rgbdfe_pose_graph_chi2.restype = C.c_int
    L.rgbdfe_pose_graph_chi2.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.rgbdfe_pose_graph_linearize.restype = C.c_int
    L.rgbdfe_pose_graph_linearize.argtypes = [vp, vp, vp, vp, i32, C.POINTER(i32), vp, vp, vp, i32, C.POINTER(i32), vp, vp, vp,
                                              i32, C.POINTER(i32), C.POINTER(C.c_double)]
    L.rgbdfe_pose_graph_optimize.restype = C.c_int
    L.rgbdfe_pose_graph_optimize.argtypes = [vp, vp, i32, C.POINTER(PoseGraphReport)]
    L.rgbdfe_pose_graph_optimize_graph.restype = C.c_int
    L.rgbdfe_pose_graph_optimize_graph.argtypes = [vp, vp, C.c_double, C.POINTER(PoseGraphReport)]
    L.rgbdfe_pose_graph_transforms.restype = C.c_int
    L.rgbdfe_pose_graph_transforms.argtypes = [vp, i32, vp, vp]
    L.rgbdfe_pose_graph_set_strategy.restype = C.c_int
    L.rgbdfe_pose_graph_set_strategy.argtypes = [vp, i32]
    L.rgbdfe_pose_graph_get_fixed.restype = C.c_int
    L.rgbdfe_pose_graph_get_fixed.argtypes = [vp, i32, C.POINTER(i32)]
    L.rgbdfe_pose_graph_get_edge.restype = C.c_int
    L.rgbdfe_pose_graph_get_edge.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), vp, vp, C.POINTER(i32)]
    L.rgbdfe_pose_graph_sanity_check.restype = C.c_int
    L.rgbdfe_pose_graph_sanity_check.argtypes = [vp, C.c_float]
    L.rgbdfe_pose_graph_edge_errors.restype = C.c_int
    L.rgbdfe_pose_graph_edge_errors.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.rgbdfe_pose_graph_prune_edges.restype = C.c_int
    L.rgbdfe_pose_graph_prune_edges.argtypes = [vp, vp, C.c_float, vp, i32, C.POINTER(i32)]
    L.rgbdfe_pose_graph_evaluate.restype = C.c_int
    L.rgbdfe_pose_graph_evaluate.argtypes = [vp, vp, C.c_double, C.POINTER(PoseGraphEvaluation), vp, i32]
    L.rgbdfe_pose_graph_write_trajectory.restype = C.c_int
    L.rgbdfe_pose_graph_write_trajectory.argtypes = [vp, C.c_char_p, i32, vp, vp, vp, vp, C.c_char_p, C.c_char_p]
    L.rgbdfe_potential_edge_targets.restype = C.c_int
    L.rgbdfe_potential_edge_targets.argtypes = [vp, i32, i32, i32, i32, i32, i32, RAND_FN, vp, C.c_uint32, vp, i32,
                                                C.POINTER(i32)]
    L.rgbdfe_icp_default_params.restype = None
    L.rgbdfe_icp_default_params.argtypes = [C.POINTER(IcpParams)]
    L.rgbdfe_icp_align_nodes.restype = C.c_int
    L.rgbdfe_icp_align_nodes.argtypes = [vp, i32, vp, vp, vp, C.POINTER(IcpParams), vp, vp]
    L.rgbdfe_icp_align_clouds.restype = C.c_int
    L.rgbdfe_icp_align_clouds.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, vp, C.POINTER(IcpParams), vp, vp, vp, vp, C.c_int64]
    L.rgbdfe_filter_cloud.restype = C.c_int
    L.rgbdfe_filter_cloud.argtypes = [vp, vp, C.c_int64, i32, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rgbdfe_slam_default_params.restype = None
    L.rgbdfe_slam_default_params.argtypes = [C.POINTER(SlamParams)]
    L.rgbdfe_slam_create.restype = C.c_int
    L.rgbdfe_slam_create.argtypes = [vp, vp, C.POINTER(SlamParams), C.POINTER(vp)]
    L.rgbdfe_slam_destroy.restype = None
    L.rgbdfe_slam_destroy.argtypes = [vp]
    L.rgbdfe_slam_reset.restype = C.c_int
    L.rgbdfe_slam_reset.argtypes = [vp]
    L.rgbdfe_slam_set_rand.restype = C.c_int
    L.rgbdfe_slam_set_rand.argtypes = [vp, RAND_FN, vp]
    L.rgbdfe_slam_add_node.restype = C.c_int
    L.rgbdfe_slam_add_node.argtypes = [vp, i32, C.c_int64, i32, C.POINTER(SlamStep)]
    L.rgbdfe_slam_begin.restype = C.c_int
    L.rgbdfe_slam_begin.argtypes = [vp, i32, i32, C.c_int64, i32, vp, i32, C.POINTER(i32), C.POINTER(SlamStep)]
    L.rgbdfe_slam_feed.restype = C.c_int
    L.rgbdfe_slam_feed.argtypes = [vp, vp, vp, i32, vp, i32, C.POINTER(i32), C.POINTER(SlamStep)]
    for name in ("rgbdfe_slam_node_count", "rgbdfe_slam_slot_of", "rgbdfe_slam_valid_tf"):
        getattr(L, name).restype = C.c_int
    L.rgbdfe_slam_node_count.argtypes = [vp]
    L.rgbdfe_slam_slot_of.argtypes = [vp, i32]
    L.rgbdfe_slam_valid_tf.argtypes = [vp, i32]
    L.rgbdfe_slam_keyframes.restype = C.c_int
    L.rgbdfe_slam_keyframes.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.rgbdfe_sizeof_slam_step.restype = C.c_int
    L.rgbdfe_sizeof_slam_step.argtypes = []
    L.rgbdfe_update_inlier_features.restype = C.c_int
    L.rgbdfe_update_inlier_features.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.rgbdfe_node_feature_stats.restype = C.c_int
    L.rgbdfe_node_feature_stats.argtypes = [vp, i32, vp, i32]
    L.rgbdfe_pose_graph_add_keyframe.restype = C.c_int
    L.rgbdfe_pose_graph_add_keyframe.argtypes = [vp, i32]
    L.rgbdfe_pose_graph_clear.restype = C.c_int
    L.rgbdfe_pose_graph_clear.argtypes = [vp]
    L.rgbdfe_download_nodes.restype = C.c_int
    L.rgbdfe_download_nodes.argtypes = [vp, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.rgbdfe_debug_download_nodes_copy_loop.restype = C.c_int
    L.rgbdfe_debug_download_nodes_copy_loop.argtypes = [vp, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.rgbdfe_download_node.restype = C.c_int
    L.rgbdfe_download_node.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.rgbdfe_download_nodes_stats.restype = C.c_int
    L.rgbdfe_download_nodes_stats.argtypes = [vp, vp, i32]
    L.rgbdfe_set_node_feature_stats.restype = C.c_int
    L.rgbdfe_set_node_feature_stats.argtypes = [vp, i32, vp, i32]
    L.rgbdfe_detector_set_thresholds.restype = C.c_int
    L.rgbdfe_detector_set_thresholds.argtypes = [vp, vp, i32]
    i64 = C.c_int64
    L.rgbdfe_pose_graph_serialize.restype = C.c_int
    L.rgbdfe_pose_graph_serialize.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.rgbdfe_pose_graph_deserialize.restype = C.c_int
    L.rgbdfe_pose_graph_deserialize.argtypes = [vp, vp, i64]
    L.rgbdfe_pose_graph_node_ids.restype = C.c_int
    L.rgbdfe_pose_graph_node_ids.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.rgbdfe_slam_serialize.restype = C.c_int
    L.rgbdfe_slam_serialize.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.rgbdfe_slam_deserialize.restype = C.c_int
    L.rgbdfe_slam_deserialize.argtypes = [vp, vp, i64]
    L.rgbdfe_session_save.restype = C.c_int
    L.rgbdfe_session_save.argtypes = [vp, vp, vp, C.c_uint32, C.c_char_p]
    L.rgbdfe_session_load.restype = C.c_int
    L.rgbdfe_session_load.argtypes = [vp, vp, vp, C.c_char_p]
    L.rgbdfe_restore_node_cloud.restype = C.c_int
    L.rgbdfe_restore_node_cloud.argtypes = [vp, i32, vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double, i32]
    L.rgbdfe_node_cloud_info.restype = C.c_int
    L.rgbdfe_node_cloud_info.argtypes = [vp, i32, vp]
    L.rgbdfe_save_map.restype = C.c_int
    L.rgbdfe_save_map.argtypes = [ctx, i32, vp, vp, C.c_double, i32, C.c_char_p, i64, vp, i64, vp]
    L.rgbdfe_save_node_clouds.restype = C.c_int
    L.rgbdfe_save_node_clouds.argtypes = [ctx, i32, vp, vp, vp, i32, C.c_char_p, C.POINTER(i32)]
    L.rgbdfe_save_cloud_file.restype = C.c_int
    L.rgbdfe_save_cloud_file.argtypes = [vp, i32, i32, vp, i32, C.c_char_p]
    L.rgbdfe_cloud_file_info.restype = C.c_int
    L.rgbdfe_cloud_file_info.argtypes = [C.c_char_p, vp]
    L.rgbdfe_load_cloud_file.restype = C.c_int
    L.rgbdfe_load_cloud_file.argtypes = [C.c_char_p, vp, i64, vp]
    L.rgbdfe_cloud_file_path.restype = C.c_int
    L.rgbdfe_cloud_file_path.argtypes = [C.c_char_p, vp, i64, C.POINTER(i32)]
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "rgbdfe_default_config", "rgbdfe_create", "rgbdfe_destroy", "rgbdfe_set_params",
    "rgbdfe_status_string", "rgbdfe_last_error", "rgbdfe_upload_node", "rgbdfe_upload_nodes",
    "rgbdfe_upload_node_device", "rgbdfe_release_node", "rgbdfe_node_count",
    "rgbdfe_match_node_pairs", "rgbdfe_match_pair_list", "rgbdfe_match_pair_list_device",
    "rgbdfe_detector_configure", "rgbdfe_detector_thresholds", "rgbdfe_detect_describe",
    "rgbdfe_orb_detect", "rgbdfe_orb_compute",
    "rgbdfe_submit_pair_list", "rgbdfe_wait_ticket", "rgbdfe_submit_pair_list_host", "rgbdfe_wait_host", "rgbdfe_wait_host_into", "rgbdfe_upload_sift_node",
    "rgbdfe_match_sift_pair_list", "rgbdfe_submit_sift_pair_list", "rgbdfe_sift_match_nodes",
    "rgbdfe_synchronize", "rgbdfe_hamming_nn_nodes", "rgbdfe_hamming_nn_host",
    "rgbdfe_project_to_3d", "rgbdfe_sift_node_features", "rgbdfe_sift_node_features_min_depth", "rgbdfe_depth_to_mono8",
    "rgbdfe_host_register", "rgbdfe_host_unregister",
    "rgbdfe_upload_node_cloud", "rgbdfe_release_node_cloud", "rgbdfe_observation_likelihood",
    "rgbdfe_assemble_map", "rgbdfe_assemble_map_device", "rgbdfe_download_node_cloud",
    "rgbdfe_voxel_filter", "rgbdfe_voxel_filter_device", "rgbdfe_reduce_node_cloud",
    "rgbdfe_display_default_params", "rgbdfe_display_geometry", "rgbdfe_display_geometry_device",
    "rgbdfe_render_default_params", "rgbdfe_render_nodes", "rgbdfe_render_nodes_device", "rgbdfe_render_perspective",
    "rgbdfe_render_viewer_view", "rgbdfe_render_sensor_camera", "rgbdfe_render_unproject", "rgbdfe_render_fragment_stats",
    "rgbdfe_octomap_default_params", "rgbdfe_octomap_create", "rgbdfe_octomap_destroy", "rgbdfe_octomap_reset",
    "rgbdfe_octomap_reserve", "rgbdfe_octomap_insert_nodes", "rgbdfe_octomap_insert_cloud", "rgbdfe_octomap_size",
    "rgbdfe_octomap_leaves", "rgbdfe_octomap_stats",
    "rgbdfe_octomap_tree", "rgbdfe_octomap_tree_device", "rgbdfe_octomap_nodes_at_depth", "rgbdfe_octomap_write",
    "rgbdfe_octomap_set_leaves", "rgbdfe_octomap_read",
    "rgbdfe_sizeof_octomap_ray_hit", "rgbdfe_octomap_occupied_log_odds", "rgbdfe_octomap_search", "rgbdfe_octomap_cast_rays",
    "rgbdfe_octomap_view_cloud", "rgbdfe_octomap_view_cloud_device",
    "rgbdfe_observation_criterion_met", "rgbdfe_set_latency_mode", "rgbdfe_set_profiling", "rgbdfe_get_kernel_time",
    "rgbdfe_reset_kernel_time", "rgbdfe_graph_stats", "rgbdfe_set_graph_capture", "rgbdfe_match_pair_list_allgather_inliers", "rgbdfe_pack_inliers", "rgbdfe_sizeof_inlier_header", "rgbdfe_sizeof_match_result", "rgbdfe_abi_version",
    "rgbdfe_pose_graph_create", "rgbdfe_pose_graph_destroy", "rgbdfe_pose_graph_add_node",
    "rgbdfe_pose_graph_add_edge", "rgbdfe_pose_graph_set_matchable", "rgbdfe_potential_edge_targets",
    "rgbdfe_pose_graph_set_estimate", "rgbdfe_pose_graph_get_estimate", "rgbdfe_pose_graph_set_fixed",
    "rgbdfe_pose_graph_add_edge_se3", "rgbdfe_pose_graph_chi2", "rgbdfe_pose_graph_linearize",
    "rgbdfe_pose_graph_optimize", "rgbdfe_pose_graph_optimize_graph", "rgbdfe_pose_graph_transforms",
    "rgbdfe_pose_graph_set_strategy", "rgbdfe_pose_graph_get_fixed", "rgbdfe_pose_graph_get_edge",
    "rgbdfe_pose_graph_sanity_check", "rgbdfe_pose_graph_edge_errors", "rgbdfe_pose_graph_prune_edges",
    "rgbdfe_pose_graph_evaluate", "rgbdfe_pose_graph_write_trajectory",
    "rgbdfe_create_multi", "rgbdfe_device_count", "rgbdfe_device_context", "rgbdfe_match_pair_list_allgather",
    "rgbdfe_gather_transport", "rgbdfe_gather_exchanges", "rgbdfe_set_hamming_mode", "rgbdfe_hamming_wide_last", "rgbdfe_set_hamming_shape", "rgbdfe_hamming_shape_last", "rgbdfe_project_to_3d_cloud", "rgbdfe_detect_describe_cloud",
    "rgbdfe_detect_describe_batch", "rgbdfe_detect_describe_batch_nodes", "rgbdfe_match_pair_list_allgather_edges",
    "rgbdfe_set_feature_min_depth", "rgbdfe_project_to_3d_min_depth",
    "rgbdfe_place_recognition", "rgbdfe_place_recognition_batch", "rgbdfe_upload_float_node",
    "rgbdfe_match_flann_pair_list", "rgbdfe_upload_node_keypoints",
    "rgbdfe_match_pair_list_allgather_compact", "rgbdfe_pack_compact", "rgbdfe_sizeof_compact_result",
    "rgbdfe_group_submit_us", "rgbdfe_sift_detect", "rgbdfe_sift_detect_batch", "rgbdfe_sift_describe", "rgbdfe_sift_geometry", "rgbdfe_sift_debug_plane", "rgbdfe_sift_debug_candidates",
    "rgbdfe_sift_detect_batch_nodes", "rgbdfe_set_detector_type", "rgbdfe_fast_detect",
    "rgbdfe_detect", "rgbdfe_detect_sift_describe", "rgbdfe_detect_sift_describe_batch_nodes",
    "rgbdfe_sift_detect_orb_describe", "rgbdfe_sift_detect_orb_describe_batch_nodes",
    "rgbdfe_sizeof_sensor_frame", "rgbdfe_ingest_frame", "rgbdfe_sensor_detect_describe",
    "rgbdfe_sensor_detect_describe_batch_nodes",
    "rgbdfe_icp_default_params", "rgbdfe_icp_align_nodes", "rgbdfe_icp_align_clouds", "rgbdfe_filter_cloud",
    "rgbdfe_slam_default_params", "rgbdfe_slam_create", "rgbdfe_slam_destroy", "rgbdfe_slam_reset", "rgbdfe_slam_set_rand",
    "rgbdfe_slam_add_node", "rgbdfe_slam_begin", "rgbdfe_slam_feed", "rgbdfe_slam_node_count", "rgbdfe_slam_slot_of",
    "rgbdfe_slam_valid_tf", "rgbdfe_slam_keyframes", "rgbdfe_sizeof_slam_step", "rgbdfe_update_inlier_features",
    "rgbdfe_node_feature_stats", "rgbdfe_pose_graph_add_keyframe", "rgbdfe_pose_graph_clear",
    "rgbdfe_download_nodes", "rgbdfe_debug_download_nodes_copy_loop", "rgbdfe_download_node", "rgbdfe_download_nodes_stats", "rgbdfe_set_node_feature_stats",
    "rgbdfe_detector_set_thresholds",
    "rgbdfe_pose_graph_serialize", "rgbdfe_pose_graph_deserialize", "rgbdfe_pose_graph_node_ids", "rgbdfe_slam_serialize",
    "rgbdfe_slam_deserialize", "rgbdfe_session_save", "rgbdfe_session_load", "rgbdfe_restore_node_cloud", "rgbdfe_node_cloud_info",
    "rgbdfe_save_map", "rgbdfe_save_node_clouds", "rgbdfe_save_cloud_file", "rgbdfe_cloud_file_info", "rgbdfe_load_cloud_file",
    "rgbdfe_cloud_file_path",
]
