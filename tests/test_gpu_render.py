"""-m gpu: rendering (include/rgbdfe.h, "rendering"; csrc/render.hip) through the C ABI and FrontEnd against
tests/render_oracle.py, byte for byte: the four images of every planted scene of tests/render_cases.py, and a node seen
through its own sensor with no oracle involved.

The clouds come from upload_node_cloud(..., return_cloud=True), whose output tests/test_gpu_emm.py pins bit for bit; the
streams the oracle draws are tests/display_oracle.py's over those clouds.  Images are 32 x 24 to 96 x 64, clouds 3 x 4 to
66 x 11.  The sizes sit either side of the kernels' tiles (csrc/render.h): the lane pass and the clear take 256 vertices /
pixels per workgroup (12 to 5106 vertices, 768 to 6144 pixels), a primitive goes to the workgroup pass when its box holds more
than 64 pixels (boxes of 64, 81 and a whole image; points of 1 to 4 and of 64 pixels), the shading pass takes 8 x 8 pixels per
wave and four waves per workgroup (widths and heights that are and are not multiples of 8: 32 x 24, 64 x 33, 33 x 25, 40 x 36,
96 x 64)."""
import ctypes as C

import numpy as np
import pytest

import display_oracle as do
import render_cases as rc
import render_oracle as ro

pytestmark = pytest.mark.gpu

INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
CASES = rc.cases()
BY_NAME = {c["name"]: c for c in CASES}
IMAGES = ("rgba", "depth", "ids", "node_index")
NODE0 = 100  # frame k of tests/render_cases.py is node NODE0 + k


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    yield f
    f.close()


def upload(fe, node_id, fr):
    return fe.upload_node_cloud(node_id, fr["depth"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], rgb=fr["rgb"], encoding_bgr=False,
                                depth_scaling=1.0, min_depth=fr["min_depth"], cloud_skip=1, return_cloud=True)


@pytest.fixture(scope="module")
def clouds(fe):
    out = {k: upload(fe, NODE0 + k, fr) for k, fr in rc.frames().items()}
    yield out
    for k in out:
        fe.release_node_cloud(NODE0 + k)


def render_params(rp):
    from rgbdslam_v2_amd import _lib
    p = _lib.RgbdfeRenderParams()
    p.width, p.height = rp["width"], rp["height"]
    p.view[:] = rp["view"]
    p.projection[:] = rp["projection"]
    p.gl_point_size, p.cull = rp["gl_point_size"], rp["cull"]
    p.clear_rgba[:] = rp["clear_rgba"]
    p.max_vertices_in_flight = rp["max_vertices_in_flight"]
    return p


def display_params(dp):
    from rgbdslam_v2_amd import _lib
    return _lib.RgbdfeDisplayParams(dp["display_type"], dp["visualization_skip_step"], dp["squared_meshing_threshold"],
                                    dp["maximum_depth"])


def raw(fe, ids, Ts, dp, rp, guard=2, shape=None, null=()):
    """The C call as it is, into poisoned images with `guard` rows behind them (shape: the buffers' H, W when the call's own
    are not valid)."""
    H, W = shape or (rp["height"], rp["width"])
    ids = np.ascontiguousarray(ids, np.int32)
    T = None if Ts is None else np.ascontiguousarray(np.asarray(Ts, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
    buf = dict(rgba=np.full((H + guard, W, 4), 0xAB, np.uint8), depth=np.full((H + guard, W), -7.0, np.float32),
               ids=np.full((H + guard, W), -77, np.int64), node_index=np.full((H + guard, W), -77, np.int32))
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in buf.items()}
    p, d = render_params(rp), display_params(dp)
    st = fe._L.rgbdfe_render_nodes(fe._ctx, len(ids), ids.ctypes.data if len(ids) else None, None if T is None else T.ctypes.data,
                                   C.byref(d), C.byref(p), ptr["rgba"], ptr["depth"], ptr["ids"], ptr["node_index"])
    out = dict(status=st, buffers=buf)
    for k, v in buf.items():
        out[k] = v[:H]
    return out


def untouched(got, rows=None):
    b = got["buffers"]
    sl = slice(rows, None)
    return bool(np.all(b["rgba"][sl] == 0xAB) and np.all(b["depth"][sl] == -7.0) and np.all(b["ids"][sl] == -77) and
                np.all(b["node_index"][sl] == -77))


def same(got, want, images=IMAGES):
    for name in images:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert got[name].tobytes() == want[name].tobytes(), name


def run_case(fe, clouds, case, **rp_over):
    rp = dict(case["rp"], **rp_over)
    got = raw(fe, [NODE0 + k for k in case["nodes"]], case["transforms"], case["disp"], rp)
    assert got["status"] == 0 and untouched(got, rp["height"])
    return got


def test_the_device_made_the_clouds_the_host_tests_drew(fe, clouds):
    """tests/test_emu_render_kernels.py runs the same cases over render_cases.cloud_of's restatement of these clouds."""
    for k, fr in rc.frames().items():
        assert clouds[k].tobytes() == rc.cloud_of(fr).tobytes(), k


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_planted_scene(fe, clouds, case):
    """Depth test, point clipping, point sizes and borders, the shared-edge fan, zero area, culling from both sides, the near
    plane and the guard band, boxes either side of the lane / workgroup threshold and a triangle over the whole image, strips of
    every length and both windings, mixed forms, repeated ids, no transforms, no nodes, perspective: the four images."""
    stream = do.display([clouds[k] for k in case["nodes"]], case["disp"], case["transforms"])
    want = ro.render_stream(stream, case["rp"])
    case["planted"](stream, case["rp"], want)
    same(run_case(fe, clouds, case), want)


@pytest.mark.parametrize("with_pose", [False, True])
def test_a_node_through_its_own_sensor_owns_its_own_pixels(fe, with_pose):
    """No oracle: a cloud rendered as POINTS through rgbdfe_render_sensor_camera with its own intrinsics and size puts every valid
    point (u, v) on pixel (u, v) with its own colour, its position in POINTS order (x outer, y inner) as id, and nothing else
    anywhere.  The reprojection error is about 1e-7 |u - cx| pixels against a margin of 1/2."""
    from rgbdslam_v2_amd.frontend import render_sensor_camera
    rng = np.random.default_rng(17)
    h, w = 24, 32
    depth = (1.2 + 0.01 * np.arange(w)[None, :] + rng.uniform(0, 0.3, (h, w))).astype(np.float32)
    depth[rng.random((h, w)) < 0.2] = np.nan
    depth[rng.random((h, w)) < 0.05] = 0.2  # under min_depth
    fr = rc.frame(depth, 50, fx=30.0, fy=31.0, cx=15.5, cy=11.5)
    cloud = upload(fe, 60, fr)
    try:
        T = np.eye(4, dtype=np.float32)
        if with_pose:
            c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
            T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
            T[:3, 3] = (0.25, -0.5, 1.0)
        view, proj = render_sensor_camera(fr["fx"], fr["fy"], fr["cx"], fr["cy"], w, h, pose=T.astype(np.float64) if with_pose else None)
        out = fe.render_nodes([60], transforms=[T] if with_pose else None, width=w, height=h, view=view, projection=proj)
        valid = np.isfinite(cloud[..., 2])
        assert 0.6 * h * w < valid.sum() < 0.9 * h * w
        order = np.full((h, w), -1, np.int64)
        order.T[valid.T] = np.arange(valid.sum())  # x outer, y inner
        words = cloud.view(np.uint32)[..., 3]
        rgba = np.stack([(words >> 16) & 255, (words >> 8) & 255, words & 255, np.full_like(words, 255)], -1).astype(np.uint8)
        rgba[~valid] = 3
        assert np.array_equal(out["ids"], order)
        assert np.array_equal(out["node_index"], np.where(valid, 0, -1))
        assert np.array_equal(out["rgba"], rgba)
        assert np.all(out["depth"][~valid] == 1.0) and np.all(out["depth"][valid] < 1.0) and np.all(out["depth"][valid] > 0.0)
    finally:
        fe.release_node_cloud(60)


@pytest.mark.parametrize("name", ["perspective_form1_step1", "perspective_form2_step1", "mixed_forms", "depth_near_second"])
def test_the_images_do_not_depend_on_the_grouping(fe, clouds, name):
    case = BY_NAME[name]
    stream = do.display([clouds[k] for k in case["nodes"]], case["disp"], case["transforms"])
    counts = np.diff(stream["node_offsets"])
    whole = run_case(fe, clouds, case)
    cap = int(counts.max())  # the largest node alone fills a group
    if name != "mixed_forms":
        assert np.all(counts == cap) and len(counts) == 2  # a group per node
    same(run_case(fe, clouds, case, max_vertices_in_flight=cap), whole)
    same(run_case(fe, clouds, case, max_vertices_in_flight=int(counts.sum())), whole)
    too_small = raw(fe, [NODE0 + k for k in case["nodes"]], case["transforms"], case["disp"], dict(case["rp"], max_vertices_in_flight=cap - 1))
    assert too_small["status"] == CAPACITY and untouched(too_small)


def test_the_device_variant_on_a_callers_stream_and_the_wrapper(fe, clouds):
    import torch
    case = BY_NAME["perspective_form1_step1"]
    rp, dp = case["rp"], case["disp"]
    H, W = rp["height"], rp["width"]
    host = run_case(fe, clouds, case)
    ids = [NODE0 + k for k in case["nodes"]]
    kw = dict(transforms=case["transforms"], view=np.asarray(rp["view"]).reshape(4, 4).T, projection=np.asarray(rp["projection"]).reshape(4, 4).T,
              gl_point_size=rp["gl_point_size"], cull=rp["cull"], clear_rgba=rp["clear_rgba"], **dp)
    wrapped = fe.render_nodes(ids, width=W, height=H, **kw)
    same(wrapped, host)
    assert set(fe.render_nodes(ids, width=W, height=H, return_ids=False, **kw)) == {"rgba", "depth"}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    t = dict(rgba=torch.full((H, W, 4), 0xAB, dtype=torch.uint8, device=dev), depth=torch.full((H, W), -7.0, dtype=torch.float32, device=dev),
             ids=torch.full((H, W), -77, dtype=torch.int64, device=dev), node_index=torch.full((H, W), -77, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    fe.render_nodes_device(ids, t["rgba"], t["depth"], t["ids"], t["node_index"], stream=stream.cuda_stream, **kw)
    same({k: v.cpu().numpy() for k, v in t.items()}, host)
    t["rgba"].fill_(0xAB)
    t["depth"].fill_(-7.0)
    torch.cuda.synchronize(dev)
    fe.render_nodes_device(ids, t["rgba"], t["depth"], **kw)  # no ids, the context's own stream
    same({k: t[k].cpu().numpy() for k in ("rgba", "depth")}, host, ("rgba", "depth"))


def test_one_call_repeated_gives_the_same_bytes(fe, clouds):
    case = BY_NAME["mixed_forms"]
    same(run_case(fe, clouds, case), run_case(fe, clouds, case))


def test_outputs_that_may_be_null(fe, clouds):
    case = BY_NAME["fan_front_k8"]
    whole = run_case(fe, clouds, case)
    part = raw(fe, [NODE0 + k for k in case["nodes"]], case["transforms"], case["disp"], case["rp"], null=("ids", "node_index"))
    assert part["status"] == 0 and np.all(part["buffers"]["ids"] == -77) and np.all(part["buffers"]["node_index"] == -77)
    same(part, whole, ("rgba", "depth"))


BAD_RENDER = [dict(width=0), dict(width=4097), dict(height=0), dict(height=-3), dict(gl_point_size=float("nan")),
              dict(gl_point_size=0.0), dict(gl_point_size=float("inf")), dict(cull=2), dict(cull=-1), dict(max_vertices_in_flight=-1),
              dict(view=[float("nan")] + [0.0] * 15), dict(projection=[0.0] * 15 + [float("inf")])]
BAD_DISPLAY = [dict(display_type=3), dict(visualization_skip_step=0)]


def test_errors_leave_the_outputs_untouched(fe, clouds):
    case = BY_NAME["fan_front_k8"]
    ids, shape = [NODE0 + k for k in case["nodes"]], (case["rp"]["height"], case["rp"]["width"])
    for bad in BAD_RENDER:
        got = raw(fe, ids, None, case["disp"], dict(case["rp"], **bad), shape=shape)
        assert got["status"] == INVALID_ARG and untouched(got), bad
    for bad in BAD_DISPLAY:
        got = raw(fe, ids, None, dict(case["disp"], **bad), case["rp"])
        assert got["status"] == INVALID_ARG and untouched(got), bad
    for null in ("rgba", "depth"):
        got = raw(fe, ids, None, case["disp"], case["rp"], null=(null,))
        assert got["status"] == INVALID_ARG and untouched(got), null
    got = raw(fe, ids + [9999], None, case["disp"], case["rp"])
    assert got["status"] == UNKNOWN_NODE and untouched(got)
    p, d = render_params(case["rp"]), display_params(case["disp"])
    out = np.zeros(4, np.uint8)
    assert fe._L.rgbdfe_render_nodes(fe._ctx, -1, None, None, C.byref(d), C.byref(p), out.ctypes.data, out.ctypes.data, None, None) == INVALID_ARG
    assert fe._L.rgbdfe_render_nodes(fe._ctx, 1, None, None, C.byref(d), C.byref(p), out.ctypes.data, out.ctypes.data, None, None) == INVALID_ARG
    assert fe._L.rgbdfe_render_nodes(fe._ctx, 0, None, None, None, C.byref(p), out.ctypes.data, out.ctypes.data, None, None) == INVALID_ARG
    assert fe._L.rgbdfe_render_nodes(fe._ctx, 0, None, None, C.byref(d), None, out.ctypes.data, out.ctypes.data, None, None) == INVALID_ARG
    # and the call still works afterwards
    same(run_case(fe, clouds, case), run_case(fe, clouds, case))


def test_default_params_and_the_helpers_are_the_oracles(fe):
    from rgbdslam_v2_amd import _lib
    from rgbdslam_v2_amd import frontend as F
    p = _lib.RgbdfeRenderParams()
    fe._L.rgbdfe_render_default_params(C.byref(p))
    want = ro.default_render_params()
    assert (p.width, p.height, p.gl_point_size, p.cull, tuple(p.clear_rgba), p.max_vertices_in_flight) == (640, 480, 1.0, 1, (3, 3, 3, 3), 0)
    assert list(p.view) == want["view"] and list(p.projection) == want["projection"]
    assert F.render_perspective().T.reshape(-1).tolist() == ro.perspective()
    assert F.render_viewer_view().T.reshape(-1).tolist() == ro.viewer_view()
    pose = np.eye(4)
    pose[:3, 3] = (1.0, 2.0, 3.0)
    v, pr = F.render_sensor_camera(525.0, 525.0, 319.5, 239.5, 640, 480, pose=pose)
    wv, wp = ro.sensor_camera(525.0, 525.0, 319.5, 239.5, 640, 480, pose=ro.column_major(pose))
    assert v.T.reshape(-1).tolist() == wv and pr.T.reshape(-1).tolist() == wp
    assert F.render_unproject(100.0, 50.0, 0.75, v, pr, 640, 480).tolist() == ro.unproject(100.0, 50.0, 0.75, wv, wp, 640, 480)
    assert F.render_unproject(1.0, 1.0, 0.5, np.zeros((4, 4)), pr, 8, 8) is None


def test_the_counting_kernels_draw_the_same_and_count_the_oracles_fragments(fe, clouds):
    """rgbdfe_render_fragment_stats (diagnostics): the fragments offered are the oracle's; those that lowered a word on arrival
    are at least the pixels drawn; the images are the same bytes; with counting off both figures are 0."""
    for name in ("mixed_forms", "perspective_form1_step1", "point_size_64"):
        case = BY_NAME[name]
        stream = do.display([clouds[k] for k in case["nodes"]], case["disp"], case["transforms"])
        want = ro.render_stream(stream, case["rp"])
        fe.render_fragment_stats(True)
        try:
            same(run_case(fe, clouds, case), want)
        finally:
            tested, won = fe.render_fragment_stats(False)
        assert tested == want["tested"] and int(np.sum(want["ids"] >= 0)) <= won <= tested
        same(run_case(fe, clouds, case), want)
        assert fe.render_fragment_stats() == (0, 0)
