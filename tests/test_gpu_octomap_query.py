"""-m gpu: the read side of the occupancy map (include/rgbdfe.h, "occupancy map: the read side"; csrc/octomap_query.hip and
the query entry points of csrc/api_octomap.hip) through the C ABI against tests/octomap_query_oracle.py.  Every comparison
is on bytes: search results, hit records, view clouds and status planes.  The cases are octomap_query_oracle.cases(), which
tests/test_emu_octomap_query_kernels.py runs through the kernel source on the CPU; what each planted ray must give is
written out by hand in tests/test_oracle_octomap_query.py."""

import numpy as np
import pytest

import octomap_oracle as oo
import octomap_query_oracle as qo

pytestmark = pytest.mark.gpu

INVALID_ARG, CAPACITY = -1, -5


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    yield f
    f.close()


@pytest.fixture(scope="module")
def maps(fe):
    """The map of a scene, built once through set_leaves and shared: no query changes it."""
    made = {}

    def get(scene):
        if id(scene) not in made:
            lv = scene["leaves"]
            m = fe.octomap(scene.get("capacity", 2 * len(lv) + 8), resolution=scene["resolution"],
                           occupancy_threshold=scene["occupancy_threshold"])
            m.set_leaves(lv)
            made[id(scene)] = m
        return made[id(scene)]
    yield get
    for m in made.values():
        m.close()


def rowmajor(T):
    return np.asarray(T, np.float32).reshape(4, 4).T


def ask(m, query, **kw):
    if query[0] == "search":
        return m.search(query[1], **kw)
    if query[0] == "cast":
        return m.cast_rays(*query[1:], **kw)
    _, T, fx, fy, cx, cy, rows, cols, ign, mr, occ = query
    return m.view_cloud(rowmajor(T), fx, fy, cx, cy, rows, cols, ign, mr, occ, with_status=True, **kw)


def same(got, ref, what=""):
    if isinstance(ref, tuple):
        assert len(got) == len(ref)
        for i, (g, r) in enumerate(zip(got, ref)):
            same(g, r, "%s[%d]" % (what, i))
        return
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    if got.tobytes() != ref.tobytes():
        rows = lambda x: np.ascontiguousarray(x).reshape(-1).view(np.uint8).reshape(max(len(x), 1), -1)
        bad = np.nonzero((rows(got) != rows(ref)).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ; the first at %d: got %s, want %s" %
                             (what, len(bad), len(got), bad[0], got[bad[0]], ref[bad[0]]))


@pytest.mark.parametrize("name", list(qo.CASES))
def test_every_case_gives_the_oracles_bytes(maps, name):
    scene, query = qo.CASES[name]
    m = maps(scene)
    before = m.leaves()
    same(ask(m, query, grow=False), qo.expected(name), name)
    assert m.last_query_launches == 1
    assert m.leaves().tobytes() == before.tobytes() == scene["leaves"].tobytes()


def test_the_hit_record_the_default_threshold_and_the_launch_count(fe, maps):
    assert fe._L.rgbdfe_sizeof_octomap_ray_hit() == qo.HIT_REC.itemsize == 36
    from rgbdslam_v2_amd import _lib
    assert _lib.OCTOMAP_RAY_HIT_DTYPE == qo.HIT_REC
    scene = qo.planted_scene()
    m = maps(qo.CASES["planted search"][0])
    assert np.float32(m.occupied_log_odds) == qo.oracle_of(scene).occupied_log_odds()
    # empty calls succeed and launch nothing
    m.search(scene["leaves"]["key"][:1].astype(np.float32))
    assert m.last_query_launches == 1
    found, leaves = m.search(np.zeros((0, 3), np.float32))
    assert len(found) == 0 and len(leaves) == 0 and m.last_query_launches == 0
    m.search(np.zeros((1, 3), np.float32))
    assert len(m.cast_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))) == 0 and m.last_query_launches == 0
    for rows, cols in ((0, 5), (5, 0), (0, 0)):
        m.search(np.zeros((1, 3), np.float32))
        cloud, status = m.view_cloud(np.eye(4), 5.0, 5.0, 2.0, 2.0, rows, cols, with_status=True)
        assert cloud.shape == (rows, cols, 4) and status.shape == (rows, cols) and m.last_query_launches == 0


def test_argument_errors(fe, maps):
    m = maps(qo.CASES["planted search"][0])
    L, h = fe._L, m._map
    p = np.zeros((4, 3), np.float32)
    found, leaves, hits = np.zeros(4, np.int32), np.zeros(4, qo.LEAF), np.zeros(4, qo.HIT_REC)
    a = lambda x: x.ctypes.data
    assert L.rgbdfe_octomap_search(h, None, 4, a(found), a(leaves)) == INVALID_ARG
    assert L.rgbdfe_octomap_search(h, a(p), 4, None, a(leaves)) == INVALID_ARG
    assert L.rgbdfe_octomap_search(h, a(p), 4, a(found), None) == INVALID_ARG
    assert L.rgbdfe_octomap_search(h, a(p), -1, a(found), a(leaves)) == INVALID_ARG
    assert L.rgbdfe_octomap_search(h, a(p), 1 << 31, a(found), a(leaves)) == CAPACITY
    assert L.rgbdfe_octomap_search(h, None, 0, None, None) == 0
    nan = float("nan")
    assert L.rgbdfe_octomap_cast_rays(h, None, a(p), 4, 0, -1.0, nan, a(hits)) == INVALID_ARG
    assert L.rgbdfe_octomap_cast_rays(h, a(p), None, 4, 0, -1.0, nan, a(hits)) == INVALID_ARG
    assert L.rgbdfe_octomap_cast_rays(h, a(p), a(p), 4, 0, -1.0, nan, None) == INVALID_ARG
    assert L.rgbdfe_octomap_cast_rays(h, a(p), a(p), 4, 0, nan, nan, a(hits)) == INVALID_ARG
    assert L.rgbdfe_octomap_cast_rays(h, a(p), a(p), -4, 0, -1.0, nan, a(hits)) == INVALID_ARG
    assert L.rgbdfe_octomap_cast_rays(h, a(p), a(p), 1 << 31, 0, -1.0, nan, a(hits)) == CAPACITY
    assert L.rgbdfe_octomap_cast_rays(h, None, None, 0, 0, -1.0, nan, None) == 0
    T = np.ascontiguousarray(np.eye(4, dtype=np.float32))
    out = np.zeros((2, 2, 4), np.float32)
    view = lambda T, rows, cols, mr, out: L.rgbdfe_octomap_view_cloud(h, T, 5.0, 5.0, 1.0, 1.0, rows, cols, 0, mr, nan, out, None)
    assert view(None, 2, 2, -1.0, a(out)) == INVALID_ARG
    assert view(a(T), 2, 2, -1.0, None) == INVALID_ARG
    assert view(a(T), -2, 2, -1.0, a(out)) == INVALID_ARG
    assert view(a(T), 2, -2, -1.0, a(out)) == INVALID_ARG
    assert view(a(T), 2, 2, nan, a(out)) == INVALID_ARG
    assert view(a(T), 1 << 16, 1 << 15, -1.0, a(out)) == CAPACITY
    assert view(a(T), 0, 2, -1.0, None) == 0
    assert view(a(T), 2, 2, -1.0, a(out)) == 0  # and without a status plane
    assert L.rgbdfe_octomap_view_cloud_device(h, a(T), 5.0, 5.0, 1.0, 1.0, 2, 2, 0, -1.0, nan, None, None, None) == INVALID_ARG
    assert L.rgbdfe_octomap_occupied_log_odds(h, None) == INVALID_ARG
    assert L.rgbdfe_octomap_search(None, a(p), 4, a(found), a(leaves)) == INVALID_ARG
    with pytest.raises(ValueError):
        m.cast_rays(p, p[:3])


def test_the_occupancy_threshold_is_checked_where_it_is_used(fe):
    from rgbdslam_v2_amd._lib import RgbdfeError
    cells = {(0, 0, 0): (-1.0, (1, 2, 3)), (2, 0, 0): (1.0, (4, 5, 6))}
    scene = dict(resolution=0.25, occupancy_threshold=0.5, leaves=qo.leaves_of(cells))
    o, d = np.array([qo.centre_of((0, 0, 0), 0.25)], np.float32), np.array([[1, 0, 0]], np.float32)
    for bad in (1.5, 0.0, 1.0, float("nan")):
        with fe.octomap(16, resolution=0.25, occupancy_threshold=bad) as m:  # create accepts what it accepted before
            m.set_leaves(scene["leaves"])
            with pytest.raises(RgbdfeError, match="occupancy_threshold"):
                m.occupied_log_odds
            with pytest.raises(RgbdfeError, match="occupancy_threshold"):
                m.cast_rays(o, d, ignore_unknown=True)
            with pytest.raises(RgbdfeError, match="occupancy_threshold"):
                m.view_cloud(np.eye(4), 2.0, 2.0, 0.0, 0.0, 1, 1)
            same(m.cast_rays(o, d, True, -1.0, 0.5), qo.oracle_of(scene).cast_rays(o, d, True, -1.0, 0.5))
            same(m.search(o), qo.oracle_of(scene).search(o))


def test_the_load_rule_at_three_quarters_and_the_wrappers_reserve(fe):
    from rgbdslam_v2_amd._lib import RgbdfeError
    lv13, queries = qo.load_rule_inputs()
    for lv, refused in ((lv13[:12], False), (lv13, True)):
        scene = dict(resolution=0.1, occupancy_threshold=0.5, leaves=lv)
        with fe.octomap(16, resolution=0.1) as m:
            m.set_leaves(lv)
            for q in queries:
                if refused:  # 4 * 13 > 3 * 16: nothing runs, the map stays as it is
                    with pytest.raises(RgbdfeError, match="reserve"):
                        ask(m, q, grow=False)
                    assert m.capacity == 16 and m.last_query_launches == 0
                else:        # 4 * 12 == 3 * 16: accepted
                    same(ask(m, q, grow=False), qo.run(scene, q), q[0])
            if refused:
                same(ask(m, queries[0]), qo.run(scene, queries[0]))
                assert m.capacity == 26 and m.leaves().tobytes() == lv.tobytes()
                for q in queries[1:]:
                    same(ask(m, q, grow=False), qo.run(scene, q), q[0])


def test_view_cloud_device_equals_view_cloud(fe, maps):
    import torch
    for name in ("view 9x7 tilted", "view 64x48 tilted", "view 8x8 inside an occupied cell"):
        scene, query = qo.CASES[name]
        _, T, fx, fy, cx, cy, rows, cols, ign, mr, occ = query
        m = maps(scene)
        ref_cloud, ref_status = qo.expected(name)
        out = torch.full((rows, cols, 4), 7.0, dtype=torch.float32, device="cuda:0")
        status = torch.full((rows, cols), 99, dtype=torch.uint8, device="cuda:0")
        m.view_cloud_device(out, rowmajor(T), fx, fy, cx, cy, ign, mr, occ, status=status)
        assert m.last_query_launches == 1
        same(out.cpu().numpy(), ref_cloud, name)
        same(status.cpu().numpy(), ref_status, name)
        out.fill_(7.0)
        s = torch.cuda.Stream(device="cuda:0")
        m.view_cloud_device(out, rowmajor(T), fx, fy, cx, cy, ign, mr, occ, stream=s.cuda_stream)  # no status plane, a stream
        same(out.cpu().numpy(), ref_cloud, name)


def test_an_insert_after_a_query_gives_the_leaves_it_gives_without(fe):
    a, b = oo.cloud(257, seed=7), oo.cloud(255, seed=8)
    T0, T1 = oo.translation(), oo.shifted(oo.translation(), 0.7)
    ref = oo.LiteralMap(resolution=0.1)
    ref.insert(a, T0, 2.8)
    first = ref.leaves()
    ref.insert(b, T1, 2.8)
    O, D = qo.random_rays(64, seed=3)
    with fe.octomap(4 * len(ref), resolution=0.1) as m:
        m.insert_cloud(a, rowmajor(T0), 2.8)
        q = qo.QueryOracle(first, resolution=0.1)
        same(m.cast_rays(O, D, True, 2.0), q.cast_rays(O, D, True, 2.0))
        same(m.search(O), q.search(O))
        same(m.view_cloud(rowmajor(T1), 20.0, 20.0, 4.0, 4.0, 9, 9, True, 3.0), q.view_cloud(T1, 20.0, 20.0, 4.0, 4.0, 9, 9, True, 3.0)[0])
        m.insert_cloud(b, rowmajor(T1), 2.8)
        assert m.leaves().tobytes() == ref.leaves().tobytes()


def test_the_map_of_a_cloud_seen_from_the_pose_it_was_inserted_from(fe):
    """End to end: the 64 x 48 raster inserted at 0.1 m, then viewed from the insertion pose with the raster's
    intrinsics.  The view is the oracle's cloud, and as a node's depth and colour planes it gives display_geometry
    (POINTS) one vertex per finite row."""
    w, h, fx = 64, 48, 52.5
    pts, T, scene, query, (ref_cloud, ref_status) = qo.raster_view()
    lv = scene["leaves"]
    with fe.octomap(2 * len(lv), resolution=scene["resolution"]) as m:
        m.insert_cloud(pts, rowmajor(T), -1.0)
        assert m.leaves().tobytes() == lv.tobytes()
        cloud, status = ask(m, query)
    same(cloud, ref_cloud, "view")
    same(status, ref_status, "status")
    finite = np.isfinite(cloud[:, :, :3]).all(axis=2)
    # a pixel whose point went in is hit again in at least 99 of 100 cases (tests/test_oracle_octomap_query.py, (c))
    assert (finite == (status == qo.HIT)).all() and finite.sum() * 100 >= 99 * np.isfinite(pts[:, :3]).all(axis=1).sum()
    words = cloud.view(np.uint32)[:, :, 3]
    rgb = np.stack([(words >> 16) & 255, (words >> 8) & 255, words & 255], axis=-1).astype(np.uint8)
    fe.upload_node_cloud(3, cloud[:, :, 2], fx, fx, w / 2 - 0.5, h / 2 - 0.5, rgb=rgb, cloud_skip=1)
    g = fe.display_geometry([3])
    assert len(g["vertices"]) == int(finite.sum())
    fe.release_node_cloud(3)
