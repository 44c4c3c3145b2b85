"""-m gpu: the occupancy map (include/rgbdfe.h, "occupancy map"; csrc/octomap.hip, csrc/api_octomap.hip) through the C ABI
against the scalar restatement in tests/octomap_oracle.py.  Every comparison is on the bytes of the sorted leaf records:
keys, log-odds bits, colours.  tests/test_oracle_octomap.py shows what such a comparison is known to see (the census)."""
import ctypes as C

import numpy as np
import pytest

import octomap_oracle as oo

pytestmark = pytest.mark.gpu

INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
CASES = oo.cases()
_ORACLE = {}


def want(case):
    """The oracle's leaves of a case, computed once."""
    if case[0] not in _ORACLE:
        _ORACLE[case[0]] = oo.run(case).leaves()
    return _ORACLE[case[0]]


def case_named(name):
    return [c for c in CASES if c[0] == name][0]


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    yield f
    f.close()


def rowmajor(T):
    return np.asarray(T, np.float32).reshape(4, 4).T


def same(got, ref):
    assert got.dtype == oo.LEAF and len(got) == len(ref), (len(got), len(ref))
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(got != ref)[0]
        raise AssertionError("%d of %d leaves differ; the first: got %s, want %s" % (len(bad), len(ref), got[bad[0]], ref[bad[0]]))


def build(fe, case, capacity):
    m = fe.octomap(capacity, **case[1])
    for pts, T, mr in case[2]:
        m.insert_cloud(pts, rowmajor(T), mr)
    return m


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_leaves_are_the_oracles_bytes(fe, case):
    ref = want(case)
    with build(fe, case, 2 * len(ref) + 64) as m:
        assert len(m) == len(ref)
        same(m.leaves(), ref)


def test_determinism_and_the_table_size_do_not_show(fe):
    """The 64 x 48 family three times into fresh maps: identical bytes, also when the table (and with it every slot) is
    another."""
    for name in ("n 3072 res 0.05 range -1", "n 3072 res 0.1 range 2.8"):
        case, ref = case_named(name), want(case_named(name))
        for cap in (2 * len(ref), 2 * len(ref), len(ref) + len(ref) // 3):
            with build(fe, case, cap) as m:
                same(m.leaves(), ref)


def upload(fe, node_id, rows, cols, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 3.2, (rows, cols)).astype(np.float32)
    d[rng.random((rows, cols)) < 0.1] = np.nan
    rgb = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    return fe.upload_node_cloud(node_id, d, 40.0, 40.0, cols / 2.0, rows / 2.0, rgb=rgb, min_depth=0.4, cloud_skip=1,
                                return_cloud=True)


SHAPES = ((7, 9), (25, 41), (16, 16), (24, 32), (1, 1), (13, 5))  # 63, 1025, 256, 768, 1, 65 points


@pytest.fixture(scope="module")
def nodes(fe):
    clouds = [upload(fe, k, r, c, 90 + k).reshape(-1, 4) for k, (r, c) in enumerate(SHAPES)]
    Ts = [rowmajor(oo.rigid(50 + k)) for k in range(len(clouds))]
    yield list(range(len(clouds))), clouds, Ts
    for k in range(len(clouds)):
        fe.release_node_cloud(k)


def oracle_of(clouds, Ts, mr, **prm):
    m = oo.LiteralMap(**prm)
    counts = []
    for c, T in zip(clouds, Ts):
        m.insert(c, np.ascontiguousarray(T.T).reshape(16), mr)
        counts.append(len(m))
    return m, counts


def test_six_nodes_in_one_call_six_calls_and_host_clouds(fe, nodes):
    ids, clouds, Ts = nodes
    ref, _ = oracle_of(clouds, Ts, 2.8, resolution=0.1)
    ref = ref.leaves()
    cap = 2 * len(ref)
    with fe.octomap(cap, resolution=0.1) as a, fe.octomap(cap, resolution=0.1) as b, fe.octomap(cap, resolution=0.1) as c:
        assert a.insert_nodes_status(ids, Ts, 2.8) == (0, 6)
        assert a.last_launches % 6 == 0  # the launches of a cloud do not depend on its size
        per_cloud = a.last_launches // 6
        for k in ids:
            assert b.insert_nodes_status([k], [Ts[k]], 2.8) == (0, 1)
            assert b.last_launches == per_cloud
            c.insert_cloud(fe.node_cloud(k), Ts[k], 2.8)
        for m in (a, b, c):
            same(m.leaves(), ref)


def test_a_repeated_id_twenty_times_in_one_call_and_as_twenty_calls(fe, nodes):
    ids, clouds, Ts = nodes
    ref, _ = oracle_of([clouds[3]] * 20, [Ts[3]] * 20, -1.0)
    ref = ref.leaves()
    assert ref["log_odds"].max() == oo.logodds(0.999) and ref["log_odds"].min() == oo.logodds(0.001)  # both clamps are reached
    with fe.octomap(2 * len(ref)) as a, fe.octomap(2 * len(ref)) as b:
        assert a.insert_nodes_status([3] * 20, [Ts[3]] * 20) == (0, 20)
        for _ in range(20):
            b.insert_nodes([3], [Ts[3]])
        same(a.leaves(), ref)
        same(b.leaves(), ref)


def test_a_reduced_node_is_an_ordinary_input(fe):
    upload(fe, 8, 25, 41, 77)
    try:
        n, flags = fe.reduce_node_cloud(8, 0.1)
        reduced = fe.node_cloud(8)
        assert flags == 0 and reduced.shape == (1, n, 4) and n > 100
        T = rowmajor(oo.rigid(61))
        ref, _ = oracle_of([reduced.reshape(-1, 4)], [T], 2.8)
        with fe.octomap(2 * len(ref)) as m:
            m.insert_nodes([8], [T], 2.8)
            same(m.leaves(), ref.leaves())
    finally:
        fe.release_node_cloud(8)


def test_an_unknown_id_changes_nothing(fe, nodes):
    ids, clouds, Ts = nodes
    ref, _ = oracle_of(clouds[:1], Ts[:1], -1.0)
    with fe.octomap(2 * len(ref)) as m:
        m.insert_nodes([0], Ts[:1])
        done = C.c_int32(-1)
        idv = np.array([1, 99, 2], np.int32)
        T = np.ascontiguousarray(np.stack(Ts[:3]).transpose(0, 2, 1))
        st = fe._L.rgbdfe_octomap_insert_nodes(m._map, 3, idv.ctypes.data, T.ctypes.data, -1.0, C.byref(done))
        assert (st, done.value) == (UNKNOWN_NODE, 0)
        same(m.leaves(), ref.leaves())
        assert fe._L.rgbdfe_octomap_insert_nodes(m._map, 1, idv.ctypes.data, T.ctypes.data, float("nan"), None) == INVALID_ARG
        assert fe._L.rgbdfe_octomap_insert_nodes(m._map, -1, idv.ctypes.data, T.ctypes.data, -1.0, None) == INVALID_ARG
        assert fe._L.rgbdfe_octomap_insert_nodes(m._map, 1, None, T.ctypes.data, -1.0, None) == INVALID_ARG
        assert fe._L.rgbdfe_octomap_insert_nodes(None, 1, idv.ctypes.data, T.ctypes.data, -1.0, None) == INVALID_ARG
        same(m.leaves(), ref.leaves())


def test_a_cloud_that_does_not_fit_then_reserve(fe, nodes):
    ids, clouds, Ts = nodes
    order = [1, 3, 2, 0, 5]
    cl, tr = [clouds[k] for k in order], [Ts[k] for k in order]
    ref, counts = oracle_of(cl, tr, 2.8)
    after_two, _ = oracle_of(cl[:2], tr[:2], 2.8)
    cap = (counts[1] + counts[2]) // 2
    assert counts[1] <= cap < counts[2]
    with fe.octomap(cap) as m:
        assert m.insert_nodes_status(order, tr, 2.8) == (CAPACITY, 2)
        assert len(m) == counts[1] and m.capacity == cap
        same(m.leaves(), after_two.leaves())
        assert m.insert_nodes_status(order[2:], tr[2:], 2.8) == (CAPACITY, 0)  # again, and still nothing is lost
        same(m.leaves(), after_two.leaves())
        from rgbdslam_v2_amd._lib import RgbdfeError
        with pytest.raises(RgbdfeError):
            m.reserve(counts[1] - 1)
        m.reserve(counts[4])  # exactly the cells the five clouds need: the table ends up full
        assert m.insert_nodes_status(order[2:], tr[2:], 2.8) == (0, 3)
        assert len(m) == m.capacity == counts[4]
        same(m.leaves(), ref.leaves())
    with fe.octomap(cap) as m:  # the same through the growing loop
        m.insert_nodes(order, tr, 2.8)
        assert m.capacity in (2 * cap, 4 * cap, 8 * cap)
        same(m.leaves(), ref.leaves())


def test_a_table_just_under_its_limit(fe):
    """One free slot: the probe sequences run through the end of the table and around."""
    case = case_named("n 1025 res 0.1 range 2.8")
    ref = want(case)
    with build(fe, case, len(ref) + 1) as m:
        same(m.leaves(), ref)
    with fe.octomap(len(ref) - 1, **case[1]) as m:
        pts, T, mr = case[2][0]
        T = np.ascontiguousarray(np.asarray(T, np.float32))
        pts = np.ascontiguousarray(pts)
        assert fe._L.rgbdfe_octomap_insert_cloud(m._map, pts.ctypes.data, len(pts), T.ctypes.data, mr) == CAPACITY
        assert len(m) == 0 and len(m.leaves()) == 0


def test_leaves_with_a_short_buffer_and_reset(fe):
    case = case_named("n 257 res 0.1 range -1")
    ref = want(case)
    with build(fe, case, 4 * len(ref)) as m:
        buf = np.full(len(ref), 0x5a, np.uint8).repeat(16).view(oo.LEAF)
        n = C.c_int64(-1)
        assert fe._L.rgbdfe_octomap_leaves(m._map, buf.ctypes.data, len(ref) - 1, C.byref(n)) == CAPACITY
        assert n.value == len(ref) and np.all(buf.view(np.uint8) == 0x5a)
        assert fe._L.rgbdfe_octomap_leaves(m._map, None, 0, C.byref(n)) == CAPACITY and n.value == len(ref)
        assert fe._L.rgbdfe_octomap_leaves(m._map, buf.ctypes.data, len(ref), None) == INVALID_ARG
        m.reset()
        assert len(m) == 0 and len(m.leaves()) == 0 and m.capacity == 4 * len(ref)
        other = case_named("n 255 res 0.1 range 2.8")
        for pts, T, mr in other[2]:
            m.insert_cloud(pts, rowmajor(T), mr)
        same(m.leaves(), want(other))


def test_refused_parameters(fe):
    from rgbdslam_v2_amd._lib import RgbdfeError
    for bad in (dict(resolution=0.0), dict(resolution=-0.05), dict(resolution=float("nan")), dict(resolution=float("inf")),
                dict(prob_hit=1.0), dict(prob_miss=0.0), dict(clamping_min=0.9, clamping_max=0.1)):
        with pytest.raises(RgbdfeError):
            fe.octomap(1024, **bad)
    for cap in (0, -1, 2**31):
        with pytest.raises(RgbdfeError):
            fe.octomap(cap)


def colour_passes(cap):
    """Host twin of insert_clouds (csrc/api_octomap.hip): the colour rows are sorted by slot, `cap` standing for "no leaf",
    in the 8-bit passes that cover 0 .. cap."""
    return -(-int(cap).bit_length() // 8)


def test_the_pass_counts_of_the_capacities_above():
    """2 * leaves + 64 slots give one, two and three passes of the colour sort, never four."""
    for name, passes in (("n 1 res 0.4 range 2.8", 1), ("n 1025 res 0.1 range 2.8", 2), ("n 3072 res 0.05 range 2.8", 3)):
        cap = 2 * len(want(case_named(name))) + 64
        print("%s: %d slots, %d passes" % (name, cap, colour_passes(cap)))
        assert colour_passes(cap) == passes


@pytest.mark.parametrize("cap,passes", [(255, 1), (256, 2), (70000, 3), (2**24, 4)])
def test_every_number_of_colour_sort_passes(fe, cap, passes):
    """Coloured families into tables of one, two, three and four passes: leaves and colours are the oracle's, the capacity
    does not show.  5000 samples of one cell and 400 of two are the rows the sort has to bring together."""
    assert colour_passes(cap) == passes
    names = ["5000 in one cell", "two cells alternating", "n 1025 res 0.4 range 2.8"]
    if cap >= 70000:
        names[2] = "n 3072 res 0.05 range 2.8"
    for name in names:
        case, ref = case_named(name), want(case_named(name))
        assert len(ref) <= cap
        with build(fe, case, cap) as m:
            assert m.capacity == cap and len(m) == len(ref)
            same(m.leaves(), ref)
