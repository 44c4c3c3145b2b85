"""-m gpu: pose-graph optimisation (include/rgbdfe.h, "pose-graph optimisation"; csrc/pose_graph.hip,
csrc/api_pose_graph.hip) through the C ABI against the literal restatement in tests/pose_graph_oracle.py.  Every comparison
is on bytes: the linearisation (errors, weights, every block of H, b, chi2), the report of optimize / optimize_graph (trial
counts, PCG iteration counts, lambda, chi2) and the estimates.  tests/test_oracle_pose_graph.py holds the oracle against
independent arithmetic; tests/test_emu_pose_graph_kernels.py runs the kernel source on the CPU."""
import ctypes as C
import struct

import numpy as np
import pytest

import pose_graph_oracle as po

pytestmark = pytest.mark.gpu

INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
PLANTED = po.planted_graphs()
_ORACLE = {}


def node_id(v):
    return 2 * int(v) + 5   # ascending with the vertex, neither dense nor from 0


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=512, max_pairs_per_batch=64)
    yield f
    f.close()


def library_graph(g):
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg = PoseGraph()
    for v in range(g.n):
        pg.add_node(node_id(v), vertex_id=g.n - v)
        pg.set_estimate(node_id(v), g.estimate(v))
        pg.set_fixed(node_id(v), bool(g.fixed[v]))
    ei, ej, ZR, Zt, Om = g.arrays()
    for e in range(len(ei)):
        Z = np.eye(4)
        Z[:3, :3], Z[:3, 3] = ZR[e], Zt[e]
        pg.add_edge_se3(node_id(ei[e]), node_id(ej[e]), Z, Om[e])
    return pg


def oracle_run(name, what):
    """The oracle's result for a planted graph, computed once: (graph after, report / value)."""
    key = (name, what)
    if key not in _ORACLE:
        g = dict(PLANTED)[name]()
        if what == "linearize":
            _ORACLE[key] = (g, po.linearize(g))
        elif what[0] == "optimize":
            rep = po.new_report()
            po.optimize(g, what[1], rep)
            _ORACLE[key] = (g, rep)
        else:
            rep = po.new_report()
            po.optimize_graph(g, what[1], rep)
            _ORACLE[key] = (g, rep)
    return _ORACLE[key]


def bits(v):
    return struct.pack("<d", float(v))


def same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def check_report(got, want):
    assert got["iterations"] == want["iterations"]
    assert bits(got["chi2"]) == bits(want["chi2"]), (got["chi2"], float(want["chi2"]))
    assert len(got["its"]) == len(want["its"])
    for k, (a, b) in enumerate(zip(got["its"], want["its"])):
        assert a["trials"] == b["trials"] and a["pcg"] == [int(v) for v in b["pcg"]], (k, a, b)
        for f in ("chi2_before", "chi2_after", "lam"):
            assert bits(a[f]) == bits(b[f]), (k, f, a[f], float(b[f]))


def check_estimates(pg, g):
    for v in range(g.n):
        assert same(pg.get_estimate(node_id(v)), g.estimate(v)), v


@pytest.mark.parametrize("name", [n for n, _ in PLANTED])
def test_linearize_is_the_oracles_bytes(fe, name):
    g, lin = oracle_run(name, "linearize")
    pg = library_graph(g)
    got = pg.linearize(fe)
    plan = lin["plan"]
    assert same(got["e"], lin["e"]) and same(got["w"], lin["w"])
    assert [int(i) for i in got["free_ids"]] == [node_id(v) for v in plan.verts]
    assert [(int(r), int(c)) for r, c in zip(got["rows"], got["cols"])] == [(int(r), int(c)) for r, c in plan.blocks]
    assert same(got["Hd"], lin["Hd"]) and same(got["b"], lin["b"]) and same(got["B"], lin["B"])
    assert bits(got["chi2"]) == bits(lin["chi2"]) and bits(pg.chi2(fe)) == bits(lin["chi2"])
    check_estimates(pg, g)  # a linearisation changes nothing
    pg.close()


@pytest.mark.parametrize("name", [n for n, _ in PLANTED])
def test_optimize_is_the_oracles_bytes(fe, name):
    g, want = oracle_run(name, ("optimize", 10))
    pg = library_graph(dict(PLANTED)[name]())
    got = pg.optimize(fe, 10)
    check_report(got, want)
    check_estimates(pg, g)
    assert bits(pg.chi2(fe)) == bits(want["chi2"])
    pg.close()


@pytest.mark.parametrize("name", ["rejected trials a", "rejected trials b"])
def test_the_rejecting_graphs_reject(name):
    """The case cannot quietly stop covering a rejected trial (pop of the estimates, lambda *= ni)."""
    _, want = oracle_run(name, ("optimize", 10))
    assert max(r["trials"] for r in want["its"]) >= 3


def test_a_pcg_solve_runs_into_a_second_read_back_chunk(fe):
    _, want = oracle_run("second pcg chunk", ("optimize", 10))
    assert max(max(r["pcg"]) for r in want["its"]) > 2 * po.PCG_FIRST_CHUNK
    pg = library_graph(dict(PLANTED)["second pcg chunk"]())
    got = pg.optimize(fe, 1)
    assert got["its"][0]["trials"] == 1
    n = got["its"][0]["pcg"][0]
    chunks, size, left = 0, po.PCG_FIRST_CHUNK, n
    while True:   # the chunks double from 8 to 64
        chunks += 1
        left -= size
        if left <= 0:
            break
        size = min(2 * size, 64)
    assert chunks >= 2
    assert got["readbacks"] == 1 + chunks + 1 + 1   # the linearisation, the chunks, the final chi2, the estimates
    pg.close()


@pytest.mark.parametrize("name,criterion", [("general information", 0.01), ("rejected trials a", 0.01), ("no fixed vertex", 20.0),
                                            ("65 vertices, 129 edges", 3.0), ("huber boundary", 0.01)])
def test_optimize_graph_is_the_oracles_bytes(fe, name, criterion):
    g, want = oracle_run(name, ("optimize_graph", criterion))
    pg = library_graph(dict(PLANTED)[name]())
    got = pg.optimize_graph(fe, criterion)
    check_report(got, want)
    check_estimates(pg, g)
    pg.close()


def test_more_leaves_than_accumulators(fe):
    """4161 edges = 66 leaves of the reduction tree: the second level takes more than one leaf per accumulator.  (The same
    path over vertices needs more than 4096 free vertices: test_more_vertex_leaves_than_accumulators.)"""
    rng = np.random.default_rng(21)
    pairs = [(int(a), int(b)) for a, b in (rng.choice(5, 2, replace=False) for _ in range(4161))]
    g = po.make_graph(5, pairs, 21)
    lin = po.linearize(g)
    pg = library_graph(g)
    got = pg.linearize(fe)
    assert same(got["e"], lin["e"]) and same(got["Hd"], lin["Hd"]) and same(got["B"], lin["B"]) and same(got["b"], lin["b"])
    assert bits(got["chi2"]) == bits(lin["chi2"]) and bits(pg.chi2(fe)) == bits(lin["chi2"])
    want = po.new_report()
    po.optimize(g, 2, want)
    check_report(pg.optimize(fe, 2), want)
    check_estimates(pg, g)
    pg.close()


def test_more_vertex_leaves_than_accumulators(fe):
    """4097 free vertices = 65 leaves: pg_tree_finish over part_b (pg_pcg_start, pg_pcg_alpha, pg_pcg_beta, pg_trial_finish)
    takes a second leaf into accumulator 0.  Two fixed hubs, every other vertex on one of them, 40 edges between
    neighbours: the PCG solves stay short, and the first one is still read back in a second chunk."""
    star = [(v % 2, v) for v in range(2, 4099)]
    cross = [(v, v + 1) for v in range(2, 202, 5)]
    g = po.make_graph(4099, star + cross, 3, fixed=(0, 1))
    assert len(g.ei) == 4137 and g.n - int(np.sum(g.fixed)) == 4097 and -(-4097 // po.TILE) == 65 > po.TILE
    lin = po.linearize(g)
    pg = library_graph(g)
    got = pg.linearize(fe)
    assert same(got["e"], lin["e"]) and same(got["Hd"], lin["Hd"]) and same(got["B"], lin["B"]) and same(got["b"], lin["b"])
    assert bits(got["chi2"]) == bits(lin["chi2"]) and bits(pg.chi2(fe)) == bits(lin["chi2"])
    want = po.new_report()
    po.optimize(g, 2, want)
    counts = [int(c) for r in want["its"] for c in r["pcg"][:r["trials"]]]
    print("PCG iterations per solve:", counts)
    assert len(want["its"]) == 2 and max(counts) <= 20 and max(counts) > po.PCG_FIRST_CHUNK
    check_report(pg.optimize(fe, 2), want)
    check_estimates(pg, g)
    pg.close()


def test_huber_at_the_boundary(fe):
    """e'Oe = 1 exactly is not down-weighted; the next representable value is."""
    at = library_graph(po.huber_boundary(False)).linearize(fe)
    up = library_graph(po.huber_boundary(True)).linearize(fe)
    assert at["w"][0] == 1.0 and at["chi2"] == 1.0
    assert up["w"][0] < 1.0


def test_nothing_to_optimise(fe):
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg = PoseGraph()
    pg.add_node(0); pg.add_node(1)
    pg.add_edge(0, 1)   # no measurement: ignored
    rep = pg.optimize_graph(fe, 0.01)
    assert rep["iterations"] == 0 and rep["chi2"] == 0.0 and pg.chi2(fe) == 0.0
    T = np.eye(4); T[0, 3] = 0.5
    pg.set_estimate(1, T)
    pg.add_edge_se3(0, 1, np.eye(4), np.eye(6))
    pg.set_fixed(0); pg.set_fixed(1)   # no free vertex
    before = pg.chi2(fe)
    assert before == 0.25
    for rep in (pg.optimize(fe, 5), pg.optimize_graph(fe, 0.01), pg.optimize_graph(fe, 20)):
        assert rep["iterations"] == 0 and rep["chi2"] == before
    assert same(pg.get_estimate(1), T)
    pg.close()


def test_argument_errors(fe):
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg = PoseGraph()
    L, g = pg._L, pg._g
    pg.add_node(0); pg.add_node(1)
    T = np.ascontiguousarray(np.eye(4)); info = np.ascontiguousarray(np.eye(6)); out = np.zeros(16)
    bad = T.copy(); bad[1, 2] = np.nan
    bad_info = info.copy(); bad_info[3, 3] = np.inf
    assert L.rgbdfe_pose_graph_set_estimate(g, 7, T.ctypes.data) == UNKNOWN_NODE
    assert L.rgbdfe_pose_graph_set_estimate(g, 0, bad.ctypes.data) == INVALID_ARG
    assert L.rgbdfe_pose_graph_set_estimate(g, 0, None) == INVALID_ARG
    assert L.rgbdfe_pose_graph_get_estimate(g, 7, out.ctypes.data) == UNKNOWN_NODE
    assert L.rgbdfe_pose_graph_set_fixed(g, 7, 1) == UNKNOWN_NODE
    assert L.rgbdfe_pose_graph_add_edge_se3(g, 0, 7, T.ctypes.data, info.ctypes.data, 1) == UNKNOWN_NODE
    assert L.rgbdfe_pose_graph_add_edge_se3(g, 0, 0, T.ctypes.data, info.ctypes.data, 0) == INVALID_ARG
    assert L.rgbdfe_pose_graph_add_edge_se3(g, 0, 1, bad.ctypes.data, info.ctypes.data, 1) == INVALID_ARG
    assert L.rgbdfe_pose_graph_add_edge_se3(g, 0, 1, T.ctypes.data, bad_info.ctypes.data, 1) == INVALID_ARG
    assert same(pg.get_estimate(1), np.eye(4))   # nothing changed
    assert pg.chi2(fe) == 0.0                     # and no edge went in
    ids = np.array([0, 7], np.int32); tf = np.full(32, 9.0, np.float32)
    assert L.rgbdfe_pose_graph_transforms(g, 2, ids.ctypes.data, tf.ctypes.data) == UNKNOWN_NODE and (tf == 9.0).all()
    chi2 = C.c_double(0)
    assert L.rgbdfe_pose_graph_chi2(None, g, C.byref(chi2)) == INVALID_ARG
    assert L.rgbdfe_pose_graph_chi2(fe._ctx, None, C.byref(chi2)) == INVALID_ARG
    assert L.rgbdfe_pose_graph_optimize(fe._ctx, g, -1, None) == INVALID_ARG
    assert L.rgbdfe_pose_graph_optimize_graph(fe._ctx, g, float("nan"), None) == INVALID_ARG
    Z = np.eye(4); Z[0, 3] = 1.0
    pg.add_edge_se3(0, 1, Z, 4.0, set_estimate=True)
    assert same(pg.get_estimate(1), Z)            # X2 = X1 * Z
    ne, nf, nb = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert L.rgbdfe_pose_graph_linearize(fe._ctx, g, None, None, 0, C.byref(ne), None, None, None, 0, C.byref(nf), None, None, None,
                                         0, C.byref(nb), None) == CAPACITY
    assert (ne.value, nf.value, nb.value) == (1, 2, 1)
    assert L.rgbdfe_pose_graph_optimize(fe._ctx, g, 2, None) == 0   # a NULL report is fine
    pg.close()


def test_edges_to_poses_to_the_assembled_map(fe):
    """synthetic nodes -> match_node_pairs -> add_edge_se3 -> optimize_graph -> transforms -> assemble_map: the cloud from the
    optimised poses is the cloud from the oracle's poses.  No claim about ground truth."""
    from rgbdslam_v2_amd import synth
    from rgbdslam_v2_amd.candidates import PoseGraph
    n = 6
    seq = synth.make_sequence(n_frames=n, n_kp=500, n_world=2000, seed=7)
    rng = np.random.default_rng(5)
    pg, g = PoseGraph(), po.Graph(n)
    for f in range(n):
        fe.upload_node(f, seq["desc"][f], seq["xyz1"][f])
        fe.upload_node_cloud(f, rng.uniform(0.5, 4.0, (6, 8)).astype(np.float32), 40.0, 40.0, 4.0, 3.0,
                             rgb=rng.integers(0, 256, (6, 8, 3), dtype=np.uint8), encoding_bgr=False, depth_scaling=1.0)
        pg.add_node(f)
    pg.set_fixed(0)
    g.fixed[0] = True
    n_edges = 0
    for f in range(1, n):
        placed = False
        for rec in fe.match_node_pairs(f, list(range(max(0, f - 3), f))[::-1]):
            if rec["id1"] < 0 or not rec["info_scale"] > 0:
                continue
            Z = np.array(rec["trafo"], np.float64).reshape(4, 4).T
            first = not placed and int(rec["id2"]) == f
            pg.add_edge_se3(int(rec["id1"]), int(rec["id2"]), Z, float(rec["info_scale"]), set_estimate=first)
            g.add_edge(int(rec["id1"]), int(rec["id2"]), Z, np.eye(6) * float(rec["info_scale"]), set_estimate=first)
            placed = placed or first
            n_edges += 1
    assert n_edges >= n - 1
    want = po.new_report()
    po.optimize_graph(g, 0.01, want)
    got = pg.optimize_graph(fe, 0.01)
    check_report(got, want)
    assert got["iterations"] >= 1
    ids = np.arange(n, dtype=np.int32)
    T = pg.transforms(ids)
    T_oracle = np.stack([g.estimate(v).astype(np.float32) for v in range(n)])
    assert T.tobytes() == T_oracle.tobytes()
    cloud = fe.assemble_map(ids, T, 3.5)
    assert len(cloud) > 0 and cloud.tobytes() == fe.assemble_map(ids, T_oracle, 3.5).tobytes()
    for f in range(n):
        fe.release_node_cloud(f)
    pg.close()
