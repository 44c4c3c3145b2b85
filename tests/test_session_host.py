"""CPU: the pose graph's and the decision machine's byte strings (include/rgbdfe.h, "session files"; csrc/session_format.h)
through the library without a device.  Every comparison is on bytes.

The reader and the patcher below are written from the header's description of the strings, not from the C++ code.  Two kinds
of content have no setter in the C ABI and reach a graph only through a string: inactive edges (pruning runs on the device)
and non-finite estimates (rgbdfe_pose_graph_set_estimate refuses them) -- those are planted by patching a valid string and
sealing it with its CRC again: the pruning verdicts come from tests/pose_graph_eval_oracle.py's prune of the same graph."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import pose_graph_eval_oracle as pe
import slam_cases as sc
from rgbdslam_v2_amd import _lib
from rgbdslam_v2_amd.candidates import PoseGraph
from rgbdslam_v2_amd.frontend import RgbdfeError, Slam

INVALID_ARG = -1
ENVELOPE, NODE_BYTES, EDGE_BYTES = 24, 112, 400


# ---- a reader and a patcher from the format's description ----------------------------------------------------------------
def seal(b):
    b = bytearray(b)
    b[12:16] = struct.pack("<I", zlib.crc32(bytes(b[16:])))
    return bytes(b)


def read_graph(b):
    assert b[:8] == b"RGBDFEPG" and len(b) % 8 == 0
    version, crc, length = struct.unpack_from("<IIQ", b, 8)
    assert version == 1 and length == len(b) and crc == zlib.crc32(b[16:])
    strategy, earliest, n_nodes, n_edges, n_kf, n_links, n_extra, zero = struct.unpack_from("<iiIIIIII", b, ENVELOPE)
    assert zero == 0
    at = ENVELOPE + 32
    g = dict(strategy=strategy, earliest=earliest, nodes={}, edges=[], node_at={}, edge_at=[])
    for _ in range(n_nodes):
        i, v, matchable, fixed = struct.unpack_from("<iiBB", b, at)
        g["nodes"][i] = dict(vertex=v, matchable=matchable, fixed=fixed, est=b[at + 16:at + NODE_BYTES])
        g["node_at"][i] = at
        at += NODE_BYTES
    for _ in range(n_edges):
        i, j, active = struct.unpack_from("<iiB", b, at)
        g["edges"].append(dict(id1=i, id2=j, active=active, z=b[at + 16:at + 112], info=b[at + 112:at + EDGE_BYTES]))
        g["edge_at"].append(at)
        at += EDGE_BYTES
    g["keyframes"] = list(struct.unpack_from("<%di" % n_kf, b, at)); at += 4 * n_kf
    g["links"] = [struct.unpack_from("<ii", b, at + 8 * k) for k in range(n_links)]; at += 8 * n_links
    g["extra"] = list(struct.unpack_from("<%di" % n_extra, b, at)); at += 4 * n_extra
    assert len(b) - at < 8 and not any(b[at:])
    return g


def est_bytes(matrix_rc):
    """A 4x4 (row, column) matrix as the string's 12 doubles: rotation row-major, then translation."""
    m = np.asarray(matrix_rc, np.float64)
    return m[:3, :3].tobytes() + m[:3, 3].tobytes()


def library_graph(g, strategy="none", keyframes=(), not_matchable=(), links=()):
    """tests/pose_graph_eval_oracle.py's EvalGraph as a library graph."""
    out = PoseGraph()
    out.set_strategy(strategy)
    for v in range(g.n):
        out.add_node(v, matchable=v not in not_matchable, keyframe=v in keyframes)
        X = np.eye(4)
        X[:3, :3], X[:3, 3] = g.R[v], g.t[v]
        out.set_estimate(v, X)
        out.set_fixed(v, bool(g.fixed[v]))
    for e in range(len(g.ei)):
        out.add_edge_se3(g.ei[e], g.ej[e], g.edge(e)["transform"], g.Om[e])
    for a, b in links:
        out.add_edge(a, b)
    return out


def n_edges(g):
    k = 0
    while g._L.rgbdfe_pose_graph_get_edge(g._g, k, None, None, None, None, None) == 0:
        k += 1
    return k


def same_through_the_getters(a, b):
    assert a.node_ids().tolist() == b.node_ids().tolist() and a.node_count() == b.node_count()
    for i in a.node_ids():
        assert a.get_estimate(i).tobytes() == b.get_estimate(i).tobytes() and a.get_fixed(i) == b.get_fixed(i)
    assert n_edges(a) == n_edges(b)
    for k in range(n_edges(a)):
        ea, eb = a.edge(k), b.edge(k)
        assert (ea["id1"], ea["id2"], ea["active"]) == (eb["id1"], eb["id2"], eb["active"])
        assert ea["transform"].tobytes() == eb["transform"].tobytes() and ea["information"].tobytes() == eb["information"].tobytes()


TARGET_ARGS = [(2, 2, 2, 3, -1, False), (1, 3, 0, 2, -1, True), (0, 2, 3, 3, 2, False), (1, 1, 1, 1, -1, True)]


def same_targets(a, b):
    """rgbdfe_potential_edge_targets walks the adjacency, weighs by id and samples the keyframes: the same lists from the same
    generator state (the library's counter-based one, by seed)."""
    for seed in range(6):
        for seq, geo, smp, depth, pred, incl in TARGET_ARGS:
            kw = dict(geodesic_depth=depth, predecessor_id=pred, include_predecessor=incl, seed=seed)
            assert a.potential_edge_targets(seq, geo, smp, **kw).tolist() == b.potential_edge_targets(seq, geo, smp, **kw).tolist()


def round_trip(g):
    b = g.serialize()
    assert g.serialize() == b   # the same state, the same bytes
    h = PoseGraph()
    h.deserialize(b)
    assert h.serialize() == b
    same_through_the_getters(g, h)
    same_targets(g, h)
    return b, h


# ---- the pose graph ---------------------------------------------------------------------------------------------------
def test_an_empty_graph_and_nodes_without_an_edge():
    b, h = round_trip(PoseGraph())
    assert read_graph(b)["nodes"] == {} and h.node_count() == 0
    g = PoseGraph()
    g.set_strategy("previous")
    for i in (0, 3, 4):   # ids with a gap; vertex ids of their own
        g.add_node(i, vertex_id=10 + i, keyframe=(i == 3))
    b, h = round_trip(g)
    r = read_graph(b)
    assert r["strategy"] == _lib.POSE_RELATIVE_TO["previous"] and r["earliest"] == 4 and r["keyframes"] == [3]
    assert [r["nodes"][i]["vertex"] for i in (0, 3, 4)] == [10, 13, 14] and r["edges"] == [] and r["links"] == [] and r["extra"] == []


@pytest.mark.parametrize("strategy", list(pe.STRATEGIES))
def test_a_planted_graph_under_every_strategy(strategy):
    og = pe.planted(7, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (0, 6)], [(1, 5, 0.4)])
    g = library_graph(og, strategy, keyframes=(0, 3, 5), not_matchable=(2,), links=[(0, 4)])
    g.set_fixed(3, True)
    b, h = round_trip(g)
    r = read_graph(b)
    assert r["strategy"] == pe.STRATEGIES[strategy] and r["keyframes"] == [0, 3, 5]
    assert [i for i, n in r["nodes"].items() if not n["matchable"]] == [2]
    assert r["links"] == [(0, 4)]   # the edge without a measurement travels as a link; the measured ones are not repeated
    for v in range(og.n):
        X = np.eye(4)
        X[:3, :3], X[:3, 3] = og.R[v], og.t[v]
        assert r["nodes"][v]["est"] == est_bytes(X) and g.get_estimate(v).tobytes() == X.tobytes()
    for k, e in enumerate(r["edges"]):
        want = g.edge(k)
        assert (e["id1"], e["id2"], bool(e["active"])) == (want["id1"], want["id2"], want["active"])
        assert e["z"] == est_bytes(want["transform"]) and e["info"] == want["information"].tobytes()
    want_fixed = {v: g.get_fixed(v) for v in range(og.n)}   # (inaffected releases the flags of an edge's vertices)
    assert {i: bool(n["fixed"]) for i, n in r["nodes"].items()} == want_fixed and want_fixed[3] and want_fixed[0] == (strategy != "inaffected")
    # a graph that goes on growing behaves the same: the next node and edge give the same bytes on both sides
    for x in (g, h):
        x.add_node(7)
        x.add_edge_se3(6, 7, np.eye(4), 2.0, set_estimate=True)
        x.add_edge_se3(7, 1, np.eye(4), 3.0)
    assert g.serialize() == h.serialize() and read_graph(g.serialize())["earliest"] == (1 if strategy == "largest_loop" else 0 if strategy == "none" else 7)


@pytest.mark.parametrize("case", [c[0] for c in pe.VERDICT_CASES])
def test_inactive_edges_after_the_oracles_prune(case):
    """The oracle prunes its copy of the graph; its REMOVED verdicts are planted into the string (pruning itself runs on the
    device: tests/test_gpu_session.py prunes there), and the restored graph reports them, keeps their slots and serialises
    to the same bytes."""
    og, n_good, calls = pe.verdict_case(case)
    g = library_graph(og, "first")
    b = bytearray(g.serialize())
    r = read_graph(bytes(b))
    for thresh, _, _ in calls:
        pe.prune_edges(og, thresh)
    for e, active in enumerate(og.active):
        b[r["edge_at"][e] + 8] = int(active)
    for e in range(len(og.ei)):   # DISCOUNTED / ZERO_MOTION rewrite the information: the oracle's values, as bytes
        b[r["edge_at"][e] + 112:r["edge_at"][e] + EDGE_BYTES] = np.ascontiguousarray(og.Om[e], np.float64).tobytes()
    b = seal(b)
    h = PoseGraph()
    h.deserialize(b)
    assert h.serialize() == b
    assert [h.edge(e)["active"] for e in range(len(og.ei))] == [bool(a) for a in og.active]
    for e in range(len(og.ei)):
        assert h.edge(e)["information"].tobytes() == np.ascontiguousarray(og.Om[e], np.float64).tobytes()
    same_targets(g, h)   # an inactive edge stays in the adjacency, as after pruneEdgesWithErrorAbove
    k = PoseGraph()
    k.deserialize(h.serialize())
    same_through_the_getters(h, k)


def test_doubles_travel_as_their_bytes():
    g = PoseGraph()
    for i in range(3):
        g.add_node(i)
    tiny = np.eye(4)
    tiny[0, 3], tiny[1, 3], tiny[2, 3], tiny[0, 1] = -0.0, 5e-324, -2.2250738585072009e-308, -0.0   # -0.0, two denormals
    g.set_estimate(1, tiny)
    g.add_edge_se3(0, 1, tiny, np.full((6, 6), -0.0))
    b, h = round_trip(g)
    assert read_graph(b)["nodes"][1]["est"] == est_bytes(tiny) and h.get_estimate(1).tobytes() == tiny.tobytes()
    assert np.signbit(h.get_estimate(1)[0, 3]) and h.edge(0)["information"].tobytes() == np.full((6, 6), -0.0).tobytes()
    # NaNs with payloads: no setter takes them, a string does
    r = read_graph(b)
    nans = struct.pack("<3Q", 0x7FF8000000000001, 0xFFF0000000000123, 0x7FF4DEADBEEF0001)   # quiet, negative, signalling
    p = bytearray(b)
    p[r["node_at"][2] + 16 + 72:r["node_at"][2] + NODE_BYTES] = nans
    p[r["edge_at"][0] + 16:r["edge_at"][0] + 40] = nans
    p = seal(p)
    k = PoseGraph()
    k.deserialize(p)
    assert k.serialize() == p
    assert k.get_estimate(2)[:3, 3].tobytes() == nans and k.edge(0)["transform"][0, :3].tobytes() == nans


# ---- the decision machine ----------------------------------------------------------------------------------------------
STEP_FIELDS = [name for name, _ in _lib.SlamStep._fields_ if name != "seconds"]


def step_bytes(st):
    out = {}
    for name in STEP_FIELDS:
        v = getattr(st, name)
        out[name] = v if isinstance(v, (int, float)) else bytes(v)
    return out


def string_of(fn, obj):
    n = C.c_int64(0)
    assert fn(obj, None, 0, C.byref(n)) == -5
    buf = np.zeros(n.value, np.uint8)
    assert fn(obj, buf.ctypes.data, n.value, C.byref(n)) == 0
    return buf.tobytes()


def run_with_a_cut(lib, case, cut=None):
    """sc.run_case, with the graph and the machine serialised, destroyed, created again and deserialised after `cut` frames.
    -> (the step records as dicts of bytes, the final state, the two strings at the cut)."""
    def create():
        g = lib.rgbdfe_pose_graph_create()
        s = C.c_void_p()
        assert lib.rgbdfe_slam_create(None, g, C.byref(sc.params_of(lib, case)), C.byref(s)) == 0
        return g, s

    g, s = create()
    assert lib.rgbdfe_pose_graph_set_strategy(g, case.get("strategy", sc.NONE)) == 0
    steps, strings = [], None
    try:
        for k, fr in enumerate(case["frames"]):
            if k == cut:
                strings = (string_of(lib.rgbdfe_pose_graph_serialize, g), string_of(lib.rgbdfe_slam_serialize, s))
                lib.rgbdfe_slam_destroy(s)
                lib.rgbdfe_pose_graph_destroy(g)
                g, s = create()   # (the strategy comes with the graph's string)
                gb, sb = (np.frombuffer(x, np.uint8) for x in strings)
                assert lib.rgbdfe_pose_graph_deserialize(g, gb.ctypes.data, len(gb)) == 0
                assert lib.rgbdfe_slam_deserialize(s, sb.ctypes.data, len(sb)) == 0
                assert string_of(lib.rgbdfe_pose_graph_serialize, g) == strings[0] and string_of(lib.rgbdfe_slam_serialize, s) == strings[1]
            ids = np.zeros(_lib.SLAM_MAX_CANDIDATES, np.int32)
            n, st = C.c_int32(0), _lib.SlamStep()
            assert lib.rgbdfe_slam_begin(s, fr["slot"], fr["rows"], fr["t"][0], fr["t"][1], ids.ctypes.data, len(ids), C.byref(n), C.byref(st)) == 0
            while n.value > 0:
                rec, flags = sc.compact_records(fr, ids[:n.value])
                assert lib.rgbdfe_slam_feed(s, rec.ctypes.data, flags.ctypes.data, n.value, ids.ctypes.data, len(ids), C.byref(n), C.byref(st)) == 0
            steps.append(step_bytes(st))
        final = sc.final_state(lib, g, s)
        final["estimates"] = [x.tobytes() for x in final["estimates"]]
        final["strings"] = (string_of(lib.rgbdfe_pose_graph_serialize, g), string_of(lib.rgbdfe_slam_serialize, s))
    finally:
        lib.rgbdfe_slam_destroy(s)
        lib.rgbdfe_pose_graph_destroy(g)
    return steps, final, strings


def sampled_case():
    """More vertices than targets, so that candidate selection draws: geodesic neighbours by weight and keyframes uniformly,
    from the library's generator seeded with seed + the number of steps begun -- the draw counter a resume must carry.  Every
    candidate gives an edge, so the graph a draw walks depends on the draws before it."""
    frames = [sc.F(0, status=sc.FIRST)]
    for k in range(1, 12):
        res = {i: sc.R(tx=0.03 * (k - i), deg=0.0, n_inl=60 - (k - i)) for i in range(k)}
        if k in (4, 8):   # nothing but the predecessor... which is refused: a keyframe promotion
            res = {k - 1: sc.R()}
        frames.append(sc.F(k, k=k * sc.GAP, res=res))
    return dict(name="sampled candidates", strategy=sc.STRAT_FIRST, frames=frames,
                params=dict(predecessor_candidates=2, neighbor_candidates=1, min_sampled_candidates=2, seed=5, clear_non_keyframes=0))


ALL_CASES = sc.CASES + [sampled_case()]


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_a_resumed_machine_continues_as_the_uninterrupted_one(case):
    lib = _lib.load()
    want_steps, want_final, _ = run_with_a_cut(lib, case)
    for cut in range(len(case["frames"]) + 1):
        steps, final, _ = run_with_a_cut(lib, case, cut)
        assert steps == want_steps, (case["name"], cut)
        assert final == want_final, (case["name"], cut)


def test_the_sampled_case_draws():
    """(conditions on the script) some list holds an id beyond the sequential ones, the lists depend on the seed, and a
    machine resumed with its draw counter back at zero does not continue as the uninterrupted one -- the counter matters."""
    lib = _lib.load()
    case = sampled_case()
    steps, final, _ = run_with_a_cut(lib, case)
    lists = [list(struct.unpack("<%di" % s["n_candidates"], s["candidates"][:4 * s["n_candidates"]])) for s in steps]
    k_far = [k for k, l in enumerate(lists) if any(i < k - 3 for i in l)]
    assert k_far, lists
    other = dict(case, params=dict(case["params"], seed=6))
    assert [s["candidates"] for s in run_with_a_cut(lib, other)[0]] != [s["candidates"] for s in steps]
    assert len(read_graph(final["strings"][0])["keyframes"]) >= 3
    # the counter in the string: u32 at the envelope + 14 x 4 + 6 x 8 + 16 x 8 parameter bytes + 12
    cut = k_far[-1]
    _, _, (gb, sb) = run_with_a_cut(lib, case, cut)
    at = ENVELOPE + 56 + 48 + 128 + 12
    assert struct.unpack_from("<I", sb, at)[0] == cut   # one begin per frame so far


# ---- refusals: each leaves the target's own serialisation unchanged ------------------------------------------------------
def small_graph():
    g = PoseGraph()
    g.set_strategy("largest_loop")
    for i in range(3):
        g.add_node(i, keyframe=(i == 0))
    g.add_edge_se3(0, 1, np.eye(4), 1.0, set_estimate=True)
    g.add_edge(0, 2)
    return g


def refused(fn, *args, naming=None):
    with pytest.raises(RgbdfeError) as e:
        fn(*args)
    assert "invalid argument" in str(e.value)
    if naming:
        assert naming in str(e.value), str(e.value)


def test_serialising_between_begin_and_feed_is_refused():
    g = PoseGraph()
    s = Slam(None, g, min_translation_meter=0.01)
    assert s.begin(0, 100, (0, 0))[1] is not None
    before = s.serialize()
    ids, rec = s.begin(1, 100, (0, sc.FRAME_NS))
    assert ids == [0] and rec is None
    refused(s.serialize, naming="busy")
    while rec is None:   # the initial comparison, then the main list
        ids, rec = s.feed(sc.compact_records(sc.F(1, res={0: sc.R()}), ids)[0])
    assert s.serialize() != before   # and between two steps it works again
    s.close()


def test_deserialising_into_objects_that_are_not_empty_or_differ():
    g = small_graph()
    b = g.serialize()
    refused(g.deserialize, b, naming="empty")
    assert g.serialize() == b
    h = PoseGraph()
    h.add_node(0)
    hb = h.serialize()
    refused(h.deserialize, b, naming="empty")
    assert h.serialize() == hb
    s = Slam(None, g, min_matches=20)
    assert s.begin(0, 100, (0, 0))[1] is not None   # (resets nothing: the graph g has nodes of its own; the machine counts its own)
    sb = s.serialize()
    refused(s.deserialize, sb, naming="fresh")
    assert s.serialize() == sb
    for field, value in (("min_matches", 21), ("seed", 9), ("observability_threshold", 0.25), ("clear_non_keyframes", 1),
                         ("init_base_pose", np.diag([1.0, 1.0, 1.0, 1.0]) + np.eye(4, k=3) * 0.5)):
        t = Slam(None, PoseGraph(), **{"min_matches": 20, field: value})
        tb = t.serialize()
        refused(t.deserialize, sb, naming=field)
        assert t.serialize() == tb
        t.close()
    t = Slam(None, PoseGraph(), min_matches=20)
    t.deserialize(sb)
    assert t.serialize() == sb and t.slots() == s.slots() and t.keyframes() == s.keyframes() and t.valid_tf() == s.valid_tf()
    t.reset()
    t.deserialize(sb)   # reset makes it fresh again
    assert t.serialize() == sb


def test_every_prefix_and_every_flipped_byte_is_refused():
    g = small_graph()
    b = g.serialize()
    s = Slam(None, PoseGraph())
    assert s.begin(3, 100, (0, 0))[1] is not None
    sb = s.serialize()
    lib = _lib.load()
    empty_graph, fresh = PoseGraph(), Slam(None, PoseGraph())
    eb, fb = empty_graph.serialize(), fresh.serialize()

    def try_graph(data):
        buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
        return lib.rgbdfe_pose_graph_deserialize(empty_graph._g, buf.ctypes.data, len(data))

    def try_slam(data):
        buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
        return lib.rgbdfe_slam_deserialize(fresh._s, buf.ctypes.data, len(data))

    for data, attempt in ((b, try_graph), (sb, try_slam)):
        for k in range(len(data)):
            assert attempt(data[:k]) == INVALID_ARG, k
        assert attempt(data + bytes(8)) == INVALID_ARG
        for k in range(len(data)):
            flipped = bytearray(data)
            flipped[k] ^= 0x01 << (k % 8)
            assert attempt(bytes(flipped)) == INVALID_ARG, k
        assert lib.rgbdfe_last_error(None).decode() != ""
    assert empty_graph.serialize() == eb and fresh.serialize() == fb
    # a sealed string whose counts lie is refused by the counts, not by the CRC
    lying = bytearray(b)
    struct.pack_into("<I", lying, ENVELOPE + 12, 4)   # n_edges
    assert try_graph(seal(lying)) == INVALID_ARG and "counts" in lib.rgbdfe_last_error(None).decode()
    dangling = bytearray(b)
    struct.pack_into("<i", dangling, read_graph(b)["edge_at"][0] + 4, 17)   # an edge to a node that is not there
    assert try_graph(seal(dangling)) == INVALID_ARG and "edge" in lib.rgbdfe_last_error(None).decode()
    assert empty_graph.serialize() == eb
    assert try_graph(b) == 0 and try_slam(sb) == 0   # and the untouched strings go in
