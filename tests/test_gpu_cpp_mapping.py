"""-m gpu: the mapping wrappers of include/rgbdfe.hpp end to end against the Python binding.

tests/cpp/mapping_session.cpp, built with plain g++ against the header and librgbdfe.so, runs one section per test as a child
process on inputs this module writes; the module then performs the same calls in the same order on a fresh FrontEnd of the
same configuration and requires the same bytes.  The binding carries the header's wrapper logic a second time
(rgbdslam_v2_amd/frontend.py, candidates.py) and is what the oracles pin, so equality with it needs no tolerance.  Every
condition a case is there for (an edge withdrawn, a table grown in the middle of the list, more corners than the header's
first buffer, ...) is asserted on the binding's result.

A child that ends by a signal or a time limit sets a flag: every later test of the module then fails at once and starts no
further process."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import icp_oracle as io
import octomap_oracle as oo
import pose_graph_eval_oracle as pe
from rgbdslam_v2_amd import _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 60
_BROKEN = []   # why no further child process is started
_TYPES = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float32): 3, np.dtype(np.float64): 4,
          np.dtype(np.uint16): 5}
EYE16 = np.eye(4, dtype=np.float32).reshape(16)
RAY_HIT = 1   # RGBDFE_OCTOMAP_RAY_HIT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, linked and rpath'ed as examples/cpp/Makefile does."""
    out = str(tmp_path_factory.mktemp("mapping_session") / "mapping_session")
    lib = os.path.join(ROOT, "rgbdslam_v2_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mapping_session.cpp"), "-o", out, "-L" + lib, "-lrgbdfe",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.fixture(autouse=True)
def not_broken():
    """After a child that ended by a signal or a time limit every test fails at once, before any work on the device."""
    if _BROKEN:
        pytest.fail("nothing is run: an earlier section ended by " + _BROKEN[0])


def write_container(path, arrays):
    with open(path, "wb") as f:
        f.write(b"RGBDFEC1" + struct.pack("<i", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            f.write(struct.pack("<i", len(name)) + name.encode())
            f.write(struct.pack("<ii", _TYPES[a.dtype], a.ndim) + struct.pack("<%dq" % a.ndim, *a.shape))
            f.write(a.tobytes())


class Session:
    """The files one run of the program left behind."""

    def __init__(self, directory):
        self.dir = directory
        with open(os.path.join(directory, "scalars.json")) as f:
            self.scalars = json.loads(f.read())

    def path(self, name):
        return os.path.join(self.dir, name)

    def bytes(self, name):
        with open(self.path(name + ".bin"), "rb") as f:
            return f.read()

    def array(self, name, dtype):
        return np.frombuffer(self.bytes(name), dtype)

    def __getitem__(self, name):
        return self.scalars[name]


def run_section(exe, section, arrays, tmp_path):
    if _BROKEN:
        pytest.fail("no process is started: an earlier section ended by " + _BROKEN[0])
    inp, out = str(tmp_path / "input.bin"), str(tmp_path / "out")
    os.makedirs(out)
    write_container(inp, arrays)
    try:
        p = subprocess.run([exe, section, inp, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _BROKEN.append("the time limit (section %s)" % section)
        pytest.fail("mapping_session %s did not end within %d s" % (section, TIMEOUT))
    if p.returncode < 0:
        _BROKEN.append("signal %d (section %s)" % (-p.returncode, section))
        pytest.fail("mapping_session %s ended by signal %d: %s" % (section, -p.returncode, p.stderr))
    assert p.returncode == 0, p.stderr
    return Session(out)


def front_end(max_nodes, max_keypoints, max_pairs):
    from rgbdslam_v2_amd.frontend import FrontEnd
    return FrontEnd(device_id=0, max_nodes=max_nodes, max_keypoints=max_keypoints, max_pairs_per_batch=max_pairs)


def same(got, want, what=""):
    """Bytes against an array of the binding's."""
    want = np.ascontiguousarray(want)
    assert len(got) == want.nbytes, (what, len(got), want.nbytes)
    assert np.array_equal(np.frombuffer(got, np.uint8), want.reshape(-1).view(np.uint8)), what


def colmajor(T):
    """n x 4 x 4 (row, column) matrices as n x 16 column-major values."""
    T = np.asarray(T)
    return np.ascontiguousarray(T.reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)


def rowmajor(T16):
    return np.asarray(T16).reshape(-1, 4, 4).transpose(0, 2, 1)


def small_features(n, m=8, seed=5):
    """Features for nodes whose matching is not the point: n nodes of m keypoints."""
    rng = np.random.default_rng(seed)
    xyz = np.ones((n, m, 4), np.float32)
    xyz[..., :3] = rng.uniform(-1, 1, (n, m, 3)).astype(np.float32) + np.float32([0, 0, 2])
    return dict(desc=rng.integers(0, 256, (n, m, 32), dtype=np.uint8), xyz1=xyz, counts=np.full(n, m, np.int32))


def upload_nodes(fe, feats, ids=None):
    for k in range(len(feats["counts"])):
        c = int(feats["counts"][k])
        fe.upload_node(k if ids is None else ids[k], feats["desc"][k][:c], feats["xyz1"][k][:c])


def random_depth(rows, cols, seed, lo=0.5, hi=3.2, holes=0.1):
    rng = np.random.default_rng(seed)
    d = rng.uniform(lo, hi, (rows, cols)).astype(np.float32)
    d[rng.random((rows, cols)) < holes] = np.nan
    return d, rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)


# ---- pairs --------------------------------------------------------------------------------------------------------------------
class Result:
    """rgbdslam::MatchingResult as the header fills it from one record of the binding."""

    def __init__(self, rec):
        n = int(rec["n_all"])
        bits = np.unpackbits(np.asarray(rec["inlier_mask"]).view(np.uint8), bitorder="little")[:n].astype(bool)
        pairs = np.stack([rec["all_q"][:n], rec["all_t"][:n]], 1).astype(np.int32)
        self.all, self.inliers = pairs, pairs[bits]
        self.ids = [int(rec["id1"]), int(rec["id2"])]
        self.ransac = np.array(rec["trafo"], np.float32)
        self.final, self.icp, self.rmse = self.ransac.copy(), EYE16.copy(), np.float32(rec["rmse"])
        self.edge_T, self.info = np.eye(4).reshape(16), 0.0
        if self.ids[0] >= 0:
            self.edge_T, self.info = self.ransac.astype(np.float64), float(rec["info_scale"])
        self.points = np.zeros(4, np.uint32)


def check_results(s, tag, results):
    same(s.bytes(tag + "_ids"), np.array([r.ids for r in results], np.int32), tag + " ids")
    same(s.bytes(tag + "_counts"), np.array([[len(r.all), len(r.inliers)] for r in results], np.int32), tag + " counts")
    same(s.bytes(tag + "_trafos"), np.array([np.concatenate([r.ransac, r.final, r.icp]) for r in results], np.float32), tag + " trafos")
    same(s.bytes(tag + "_rmse"), np.array([r.rmse for r in results], np.float32), tag + " rmse")
    same(s.bytes(tag + "_edge"), np.array([np.append(r.edge_T, r.info) for r in results], np.float64), tag + " edge")
    same(s.bytes(tag + "_points"), np.array([r.points for r in results], np.uint32), tag + " points")
    same(s.bytes(tag + "_matches"), np.concatenate([np.concatenate([r.all, r.inliers]).reshape(-1) for r in results]).astype(np.int32),
         tag + " matches")


EMM_SKIP_STEP, OBSERVABILITY_THRESHOLD = 8, 0.6   # tests/test_gpu_emm.py::test_pairwise_likelihood_gates_ransac_edges
MIN_DEPTH = 0.1


def test_pairs(exe, tmp_path):
    """Node 5 against 4 (adjacent, five features), 3 (an edge the measurement model keeps), 2 (five features, not adjacent),
    1 (an edge whose cloud contradicts it: withdrawn) and 0 (unrelated): nodeComparisons, pairwiseObservationLikelihood,
    icpFallback."""
    seq = synth.make_sequence(n_frames=6, n_kp=300, n_world=1200, seed=7)
    other = synth.make_sequence(n_frames=1, n_kp=300, n_world=1200, seed=99)
    desc, xyz = seq["desc"].copy(), seq["xyz1"].copy()
    desc[0], xyz[0] = other["desc"][0], other["xyz1"][0]
    feats = dict(desc=desc, xyz1=xyz, counts=np.array([300, 300, 5, 300, 5, 300], np.int32))
    poses = [seq["poses"][k].copy() for k in range(6)]
    poses[1] = poses[1] @ io.rigid([0, 0, 0], [0, 0, -0.6])   # the room as node 1 would see it from 0.6 m further back
    depth = np.stack([io.corner_depth(64, 48, p)[0] for p in poses])
    K = np.array(io.corner_depth(64, 48)[1], np.float64)
    cand = np.array([4, 3, 2, 1, 0], np.int32)
    s = run_section(exe, "pairs", dict(feats, depth=depth, K=K, min_depth=np.array([MIN_DEPTH]), candidates=cand,
                                       emm_skip_step=np.array([EMM_SKIP_STEP], np.int64),
                                       observability_threshold=np.array([OBSERVABILITY_THRESHOLD])), tmp_path)
    fe = front_end(16, 512, 64)
    upload_nodes(fe, feats)
    for k in range(6):
        fe.upload_node_cloud(k, depth[k], *K, min_depth=MIN_DEPTH, cloud_skip=1)
    rec = fe.match_node_pairs(5, cand)
    results = [Result(r) for r in rec]
    assert [r.ids[0] >= 0 for r in results] == [False, True, False, True, False]
    check_results(s, "compare", results)
    # pairwiseObservationLikelihood
    edges = [i for i, r in enumerate(results) if r.ids[0] >= 0]
    counts, met = fe.pairwise_observation_likelihood(rec[edges], OBSERVABILITY_THRESHOLD, EMM_SKIP_STEP)
    assert met.any() and not met.all(), (counts, met)
    for k, i in enumerate(edges):
        results[i].points = counts[k].astype(np.uint32)
        if not met[k]:
            rec[i]["id1"] = rec[i]["id2"] = -1
            results[i].ids = [-1, -1]
    check_results(s, "emm", results)
    # icpFallback
    had_edge = [int(r["id1"]) >= 0 for r in rec]
    out, served, T, rep = fe.icp_fallback(rec, 5, cand)
    assert list(served) == [0] and rep[0]["converged"], (served, rep)
    assert had_edge[1] and not had_edge[2] and 5 - int(cand[2]) > 1 and int(out[2]["id1"]) < 0
    for k, i in enumerate(served):
        if rep[k]["converged"]:
            t = colmajor(T[k])[0].astype(np.float32)
            results[i].final, results[i].icp, results[i].edge_T = t, t.copy(), t.astype(np.float64)
            results[i].ids = [int(cand[i]), 5]
        assert np.array_equal(np.array(out[i]["trafo"], np.float32).view(np.uint32), results[i].final.view(np.uint32))
    check_results(s, "icp", results)
    assert s["icp_edges"] == int(sum(bool(r["converged"]) for r in rep)) and s["icp_reports"] == len(rep)
    same(s.bytes("icp_reports"), rep, "icp reports")
    fe.close()


# ---- graph --------------------------------------------------------------------------------------------------------------------
(OP_NODE, OP_EDGE, OP_STRATEGY, OP_FIXED, OP_OPTIMIZE, OP_PRUNE, OP_SANITY, OP_EVALUATION, OP_TRAJECTORY, OP_TRANSFORMS, OP_CLOUDS,
 OP_ASSEMBLE) = range(12)
ID0 = 3   # the library's node id of a planted graph's node 0


class Script:
    """The operations of one graph run, for the program and for the binding."""

    def __init__(self):
        self.ops, self.opf, self.edges = [], [], []

    def add(self, kind, a=0, b=0, f=0.0):
        self.ops.append((kind, a, b, 0))
        self.opf.append((f, 0.0))

    def edge(self, i, j, Z, Om, set_estimate):
        scale = float(Om[0, 0])
        assert np.array_equal(Om, np.eye(6) * scale)   # scalar information: LoadedEdge3D::informationScale
        self.edges.append(np.concatenate([[ID0 + i, ID0 + j], colmajor(Z)[0], [scale]]))
        self.add(OP_EDGE, len(self.edges) - 1, int(bool(set_estimate)))

    def arrays(self, n_nodes):
        return dict(small_features(n_nodes), ops=np.array(self.ops, np.int32), opf=np.array(self.opf, np.float64),
                    edges=np.array(self.edges, np.float64))


BASE2POINTS, INIT_BASE_POSE = io.rigid([0.1, -0.2, 0.3], [0.05, 0.0, 1.2]), io.rigid([-0.3, 0.1, 0.2], [2.0, -1.0, 0.5])


def run_binding(fe, script, arrays, s):
    """The script on the binding, every result compared with the program's as it appears.  Returns what the binding gave."""
    from rgbdslam_v2_amd.candidates import PoseGraph
    pg, ids, seen = PoseGraph(), [], {}
    for at, ((kind, a, b, _), (f0, _)) in enumerate(zip(script.ops, script.opf)):
        tag = "_%d" % at
        if kind == OP_NODE:
            k = len(ids)
            fe.upload_node(a, arrays["desc"][k], arrays["xyz1"][k])
            pg.add_node(a, a, True, False)
            ids.append(a)
        elif kind == OP_EDGE:
            e = script.edges[a]
            pg.add_edge_se3(int(e[0]), int(e[1]), rowmajor(e[2:18])[0], float(e[18]), bool(b))
        elif kind == OP_STRATEGY:
            pg.set_strategy(a)
        elif kind == OP_FIXED:
            pg.set_fixed(a, bool(b))
        elif kind == OP_OPTIMIZE:
            rep = pg.optimize_graph(fe, f0)
            ri, rf = [rep["iterations"], rep["launches"], rep["readbacks"], len(rep["its"])], [rep["chi2"], rep["chi2"]]
            for it in rep["its"]:
                ri += [it["trials"]] + it["pcg"]
                rf += [it["chi2_before"], it["chi2_after"], it["lam"]]
            same(s.bytes("report_i" + tag), np.array(ri, np.int64), "report" + tag)
            same(s.bytes("report_f" + tag), np.array(rf, np.float64), "chi2" + tag)
            seen.setdefault("iterations", []).append(rep["iterations"])
        elif kind == OP_PRUNE:
            n, verdicts = pg.prune_edges(fe, np.float32(f0))
            assert s["pruned" + tag] == n
            same(s.bytes("verdicts" + tag), verdicts, "verdicts" + tag)
            seen["verdicts"] = verdicts
        elif kind == OP_SANITY:
            seen["sanity"] = pg.sanity_check(np.float32(f0))
            assert s["sanity" + tag] == seen["sanity"]
        elif kind == OP_EVALUATION:
            rounds, est = pg.evaluate(fe, f0)
            same(s.bytes("evaluation_chi2" + tag), np.array([r["chi2"] for r in rounds]), "evaluation chi2")
            same(s.bytes("evaluation_counts" + tag),
                 np.array([[r["iterations"], r["pruned"], r["launches"], r["readbacks"]] for r in rounds], np.int64), "evaluation counts")
            same(s.bytes("estimates" + tag), colmajor(est.reshape(-1, 4, 4)), "estimates")
            seen["rounds"] = rounds
        elif kind == OP_TRAJECTORY:
            mine = s.path("binding_trajectory" + tag + ".txt")
            stamps = 1000.0 + 0.5 * np.arange(len(ids))
            if a == 2:   # unequal lists: refused by both, and no file
                with pytest.raises(ValueError):
                    pg.write_trajectory(mine, ids, stamps[:-1])
                assert s["trajectory" + tag] == 0 and not os.path.exists(s.path("trajectory" + tag + ".txt"))
                continue
            if a == 1:
                pg.write_trajectory(mine, ids, stamps, BASE2POINTS, INIT_BASE_POSE, "/map", "/camera")
            else:
                pg.write_trajectory(mine, ids, stamps)
            with open(mine, "rb") as f, open(s.path("trajectory" + tag + ".txt"), "rb") as g:
                text = f.read()
                assert text == g.read() and text.count(b"\n") >= len(ids)
            seen.setdefault("trajectories", []).append(text)
        elif kind == OP_TRANSFORMS:
            if a == 1:   # an unknown id: refused by the binding, empty from the header
                with pytest.raises(_lib.RgbdfeError):
                    pg.transforms(ids + [9999])
                assert s.bytes("transforms" + tag) == b""
                continue
            same(s.bytes("transforms" + tag), colmajor(pg.transforms(ids)).astype(np.float32), "transforms")
        elif kind == OP_CLOUDS:
            for k in range(a):
                fe.upload_node_cloud(ids[k], arrays["depth"][k], *arrays["K"], rgb=arrays["rgb"][k], min_depth=MIN_DEPTH, cloud_skip=1)
        elif kind == OP_ASSEMBLE:
            cloud, offsets = fe.assemble_map(ids[:a], pg.transforms(ids[:a]), f0, False, return_offsets=True)
            same(s.bytes("assembled" + tag), cloud, "assembled")
            same(s.bytes("assembled_offsets" + tag), offsets, "assembled offsets")
            seen["assembled"] = (cloud, offsets)
    pg.close()
    return seen


@pytest.mark.parametrize("strategy", ["previous", "largest_loop", "none"])
def test_graph_online(exe, tmp_path, strategy):
    """The 12-node online case (tests/pose_graph_eval_oracle.py): nodeAdded, addEdgeToG2O with and without set_estimate,
    optimizeGraph after every node under a strategy (or setFixed under _NONE), then transforms, saveTrajectory in its forms,
    the estimates as the world2cam of assembleAllClouds, sanityCheck, pruneEdgesWithErrorAbove."""
    sc = Script()
    sc.add(OP_STRATEGY, pe.STRATEGIES[strategy])
    for v, edges in enumerate(pe.online_sequence()):
        sc.add(OP_NODE, ID0 + v)
        if strategy == "none" and v == 0:
            sc.add(OP_FIXED, ID0, 1)
        for k, (i, j, Z, Om) in enumerate(edges):
            sc.edge(i, j, Z, Om, k == 0)
        if edges:
            sc.add(OP_OPTIMIZE, f=0.01)
    sc.add(OP_TRANSFORMS, 0)
    sc.add(OP_TRANSFORMS, 1)
    sc.add(OP_TRAJECTORY, 0)
    sc.add(OP_TRAJECTORY, 2)
    sc.add(OP_TRAJECTORY, 1)
    sc.add(OP_CLOUDS, 12)
    sc.add(OP_ASSEMBLE, 12, f=2.5)
    sc.add(OP_SANITY, f=2.0)
    sc.add(OP_PRUNE, f=1.0)
    sc.add(OP_OPTIMIZE, f=0.01)
    sc.add(OP_TRANSFORMS, 0)
    arrays = sc.arrays(12)
    clouds = [random_depth(48, 64, 300 + k) for k in range(12)]
    arrays.update(depth=np.stack([c[0] for c in clouds]), rgb=np.stack([c[1] for c in clouds]), K=np.array([40.0, 40.0, 32.0, 24.0]),
                  min_depth=np.array([MIN_DEPTH]), base2points=colmajor(BASE2POINTS)[0], init_base_pose=colmajor(INIT_BASE_POSE)[0])
    s = run_section(exe, "graph", arrays, tmp_path)
    fe = front_end(80, 64, 16)
    seen = run_binding(fe, sc, arrays, s)
    fe.close()
    assert len(seen["iterations"]) == 12 and sum(seen["iterations"]) > 12
    assert seen["trajectories"][0] != seen["trajectories"][1]
    cloud, offsets = seen["assembled"]
    assert 0 < len(cloud) < 12 * 48 * 64 and np.all(np.diff(offsets) > 0)   # every node gives points, the range clips some


def test_graph_ring(exe, tmp_path):
    """The ring of 64 with planted false loop edges: built through addEdgeToG2O under _INAFFECTED, optimizeGraph,
    pruneEdgesWithErrorAbove with verdicts, sanityCheck, evaluation with estimates, saveTrajectory, transforms."""
    g, _, false_slots = pe.ring()
    sc = Script()
    sc.add(OP_STRATEGY, pe.INAFFECTED)
    sc.add(OP_NODE, ID0)
    added = 1
    for e in range(len(g.ei)):
        ed = g.edge(e)
        v = max(ed["id1"], ed["id2"])
        first = v == added
        if first:
            sc.add(OP_NODE, ID0 + v)
            added += 1
        sc.edge(ed["id1"], ed["id2"], ed["transform"], ed["information"], first)
    assert added == pe.RING_N
    sc.add(OP_OPTIMIZE, f=0.01)
    sc.add(OP_PRUNE, f=5.0)
    sc.add(OP_SANITY, f=1.0)
    sc.add(OP_EVALUATION, f=0.01)
    sc.add(OP_TRAJECTORY, 1)
    sc.add(OP_TRANSFORMS, 0)
    arrays = sc.arrays(pe.RING_N)
    arrays.update(base2points=colmajor(BASE2POINTS)[0], init_base_pose=colmajor(INIT_BASE_POSE)[0])
    s = run_section(exe, "graph", arrays, tmp_path)
    fe = front_end(80, 64, 16)
    seen = run_binding(fe, sc, arrays, s)
    fe.close()
    verdicts = seen["verdicts"]
    assert len(verdicts) == len(g.ei) and (verdicts != pe.KEPT).any() and (verdicts == pe.KEPT).any()
    assert all(verdicts[e] != pe.KEPT for e in false_slots)
    assert seen["sanity"] > 0 and len(seen["rounds"]) == 5


# ---- clouds -------------------------------------------------------------------------------------------------------------------
DISPLAY_FORMS = [(_lib.DISPLAY_POINTS, 1, 0.0009, np.inf), (_lib.DISPLAY_TRIANGLES, 1, 0.0009, np.inf),
                 (_lib.DISPLAY_TRIANGLE_STRIP, 1, 0.0009, np.inf), (_lib.DISPLAY_TRIANGLE_STRIP, 2, 0.0009, np.inf),
                 (_lib.DISPLAY_TRIANGLES, 1, -1.0, np.inf), (_lib.DISPLAY_POINTS, 1, 0.0009, 1.2)]


def surface_depth(rows, cols, seed):
    """A slanted plane with NaN holes and two depth jumps (what tests/display_cases.py plants in its host clouds, as a depth
    image: the header has no call that takes a host cloud)."""
    rng = np.random.default_rng(seed)
    d = (1.0 + 0.001 * np.arange(cols)[None, :] + rng.uniform(0, 0.002, (rows, cols))).astype(np.float32)
    d[:, cols // 2:] += np.float32(0.5)
    d[rows // 3:, :] += np.float32(0.25)
    d[rng.random((rows, cols)) < 0.1] = np.nan
    return d, rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def check_cloud(s, name, cloud):
    same(s.bytes(name), cloud, name)
    assert (s[name + "_rows"], s[name + "_cols"]) == cloud.shape[:2], name


def check_display(s, name, got):
    same(s.bytes(name + "_vertices"), got["vertices"], name)
    same(s.bytes(name + "_strips"), got["strips"], name)
    same(s.bytes(name + "_offsets"), got["node_offsets"], name)
    same(s.bytes(name + "_strip_offsets"), got["node_strip_offsets"], name)
    same(s.bytes(name + "_types"), got["node_types"], name)


def test_clouds(exe, tmp_path):
    """pointCloud, reducePointCloud, assembleAllClouds and displayGeometry over five nodes: two 48 x 64 surfaces, a cloud of one
    row, a cloud without a valid point, and a copy of the first for the leaf that is too small."""
    surfaces = [surface_depth(48, 64, 400 + k) for k in range(5)]
    depth, rgb = np.stack([c[0] for c in surfaces]), np.stack([c[1] for c in surfaces])
    depth[3] = np.nan
    depth[4], rgb[4] = depth[0], rgb[0]
    depth_row, rgb_row = depth[:1, 7:8].copy(), rgb[:1, 7:8].copy()
    K = np.array([200.0, 200.0, 32.0, 24.0])
    world2cam = np.stack([oo.rigid(50 + k) for k in range(5)]).astype(np.float32)
    maximum_depth, vfs, tiny, min_depth = 1.45, 0.05, 1e-9, 0.4
    arrays = dict(small_features(5), depth=depth, rgb=rgb, depth_row=depth_row, rgb_row=rgb_row, K=K, min_depth=np.array([min_depth]),
                  world2cam=world2cam, maximum_depth=np.array([maximum_depth]), voxelfilter_size=np.array([vfs]),
                  tiny_leaf=np.array([tiny]), display_forms=np.array([f[:2] for f in DISPLAY_FORMS], np.int32),
                  display_f=np.array([f[2:] for f in DISPLAY_FORMS], np.float64))
    s = run_section(exe, "clouds", arrays, tmp_path)
    fe = front_end(16, 64, 16)
    upload_nodes(fe, arrays)
    for k in (0, 1, 3, 4):
        fe.upload_node_cloud(k, depth[k], *K, rgb=rgb[k], min_depth=min_depth, cloud_skip=1)
    fe.upload_node_cloud(2, depth_row[0], *K, rgb=rgb_row[0], min_depth=min_depth, cloud_skip=1)
    for k in range(5):
        check_cloud(s, "cloud_%d" % k, fe.node_cloud(k))
    assert fe.node_cloud(2).shape == (1, 64, 4) and np.isnan(fe.node_cloud(3)[..., 2]).all()
    T = rowmajor(world2cam)
    listed = [0, 1, 2, 0, 3]
    compact, off = fe.assemble_map(listed, T[listed], maximum_depth, False, return_offsets=True)
    same(s.bytes("assembled_compact"), compact, "compact")
    same(s.bytes("assembled_compact_offsets"), off, "compact offsets")
    raster, roff = fe.assemble_map(listed, T[listed], maximum_depth, True, return_offsets=True)
    same(s.bytes("assembled_raster"), raster, "raster")
    same(s.bytes("assembled_raster_offsets"), roff, "raster offsets")
    assert 0 < len(compact) < len(raster) == 3 * 48 * 64 + 64 + 48 * 64 and off[4] == off[5]   # clipped; the last cloud has no point
    assert s.bytes("assembled_empty") == b""
    same(s.bytes("assembled_empty_offsets"), np.zeros(1, np.int64), "empty offsets")
    filtered = fe.voxel_filter(compact, vfs)
    assert 0 < len(filtered) < len(compact)
    same(s.bytes("assembled_filtered"), filtered, "filtered")
    same(s.bytes("assembled_filtered_offsets"), off, "filtered offsets")   # they still describe the unfiltered cloud
    assert s["assemble_bad_length"] == 0 and s["assemble_bad_untouched"] == 1 and s["display_bad_length"] == 0
    shown = [0, 1, 2]
    for k, (kind, step, thr, far) in enumerate(DISPLAY_FORMS):
        prm = dict(display_type=kind, visualization_skip_step=step, squared_meshing_threshold=thr, maximum_depth=far)
        node, world = fe.display_geometry(shown, None, **prm), fe.display_geometry(shown, T[shown], **prm)
        check_display(s, "display_node_%d" % k, node)
        check_display(s, "display_world_%d" % k, world)
        assert len(node["vertices"]) > 0 and node["vertices"].tobytes() != world["vertices"].tobytes()
        assert node["node_types"][2] == _lib.DISPLAY_POINTS   # the cloud of one row
        assert node["node_types"][0] == (_lib.DISPLAY_POINTS if thr < 0 else kind)
        assert (len(node["strips"]) > 0) == (kind == _lib.DISPLAY_TRIANGLE_STRIP)
    # reducePointCloud
    before = fe.node_cloud(1)
    with pytest.warns(UserWarning):
        assert fe.reduce_node_cloud(1, 0.0) is None and fe.reduce_node_cloud(1, -1.0) is None
    assert s["reduce_zero"] == 0 and s["reduce_negative"] == 0
    check_cloud(s, "cloud_1_after_invalid", before)
    points, flags = fe.reduce_node_cloud(1, vfs)
    assert (s["reduce_points"], s["reduce_flags"]) == (points, flags) and flags == 0 and 0 < points < 48 * 64
    assert fe.node_cloud(1).shape == (1, points, 4)
    check_cloud(s, "cloud_1_reduced", fe.node_cloud(1))
    points, flags = fe.reduce_node_cloud(4, tiny)
    assert (s["tiny_points"], s["tiny_flags"]) == (points, flags) and flags == 1   # RGBDFE_VOXEL_LEAF_TOO_SMALL
    assert fe.node_cloud(4).tobytes() == fe.node_cloud(0).tobytes()   # the cloud stays as it is
    check_cloud(s, "cloud_4_after_tiny", fe.node_cloud(4))
    # a cloud without a valid point reduces to a cloud of no rows: the C ABI calls that a cloud too (include/rgbdfe.h,
    # rgbdfe_reduce_node_cloud), so pointCloud succeeds with 1 row and 0 columns, as node_cloud does
    points, flags = fe.reduce_node_cloud(3, vfs)
    assert (s["empty_points"], s["empty_flags"]) == (points, flags) == (0, 0)
    assert fe.node_cloud(3).shape == (1, 0, 4)
    check_cloud(s, "cloud_3_reduced", fe.node_cloud(3))
    after = [0, 1, 3]
    cloud, off = fe.assemble_map(after, T[after], maximum_depth, False, return_offsets=True)
    same(s.bytes("assembled_after"), cloud, "after")
    same(s.bytes("assembled_after_offsets"), off, "after offsets")
    got = fe.display_geometry(after, T[after], display_type=_lib.DISPLAY_TRIANGLE_STRIP)
    check_display(s, "display_after", got)
    assert list(got["node_types"]) == [_lib.DISPLAY_TRIANGLE_STRIP, _lib.DISPLAY_POINTS, _lib.DISPLAY_POINTS]
    fe.close()


# ---- octomap ------------------------------------------------------------------------------------------------------------------
def test_octomap(exe, tmp_path):
    """All of class OctoMap: insertClouds from a table that must double twice (once before any cloud fits, once in the middle
    of the list), the tree and depth queries, write / read / setLeaves, the read side on a table loaded to 1, a map that
    failed to create."""
    clouds = [random_depth(48, 64, 90 + k) for k in range(6)]
    depth, rgb = np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds])
    K = np.array([40.0, 40.0, 32.0, 24.0])
    world2cam = np.stack([oo.rigid(50 + k) for k in range(6)]).astype(np.float32)
    T, ids = rowmajor(world2cam), list(range(6))
    resolution, max_range, min_depth = 0.1, 2.8, 0.4
    feats = small_features(6)
    fe = front_end(16, 64, 16)
    upload_nodes(fe, feats)
    for k in ids:
        fe.upload_node_cloud(k, depth[k], *K, rgb=rgb[k], min_depth=min_depth, cloud_skip=1)
    # the leaves after every cloud, on a map that never grows
    roomy = fe.octomap(1 << 18, resolution=resolution)
    sizes = []
    for k in ids:
        assert roomy.insert_nodes_status([k], T[k:k + 1], max_range) == (0, 1)
        sizes.append(len(roomy))
    leaves = roomy.leaves()
    assert len(leaves) == sizes[-1] < 1 << 17
    # the starting capacity: too small for the first cloud (the first pass applies none: done == 0), and twice it holds some
    # clouds but not all.  The trace of the growth loop on the binding says what was planted.
    capacity = min((sizes[2] + 1) // 2, sizes[0] - 1)
    trace, at = [], 0
    with fe.octomap(capacity, resolution=resolution) as grown:
        while True:
            st, done = grown.insert_nodes_status(ids[at:], T[at:], max_range)
            if st == 0:
                break
            trace.append((at, done))
            at += done
            grown.reserve(2 * grown.capacity)
        final_capacity = grown.capacity
        assert grown.leaves().tobytes() == leaves.tobytes()
    assert len(trace) >= 2 and trace[0] == (0, 0) and any(0 < a < 6 and d > 0 for a, d in trace[1:]), trace
    assert final_capacity == capacity << len(trace)
    # what the read side is asked
    rng = np.random.default_rng(17)
    centres = ((leaves["key"].astype(np.float64) - 32768 + 0.5) * resolution).astype(np.float32)
    points = np.concatenate([centres[:: max(len(centres) // 40, 1)], rng.uniform(-30, 30, (20, 3)).astype(np.float32),
                             np.array([[np.nan, 0, 0], [0, 0, 1e9]], np.float32)])
    origins = np.repeat(world2cam[:, 12:15], 8, axis=0)
    directions = (centres[rng.integers(0, len(centres), len(origins))] - origins).astype(np.float32)
    directions[::5] = rng.normal(size=(len(directions[::5]), 3)).astype(np.float32)
    view = np.array([20.0, 20.0, 16.0, 12.0, 24, 32], np.float64)
    s = run_section(exe, "octomap", dict(feats, depth=depth, rgb=rgb, K=K, min_depth=np.array([min_depth]), world2cam=world2cam,
                                         resolution=np.array([resolution]), max_range=np.array([max_range]),
                                         depth_threshold=np.zeros(1, np.float32), capacity=np.array([capacity], np.int64),
                                         points=points, origins=origins, directions=directions, ray_range=np.array([4.0]),
                                         cam2world=world2cam[0], view=view), tmp_path)
    # a map that failed to create: valid() false, every member false or -1
    assert list(s.array("invalid_map", np.int32)) == [0, 0, 0, 0, 0, -1, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert not os.path.exists(s.path("never.ot"))
    assert s["empty_tree"] == 0 and s["empty_level"] == 0
    # growth
    assert s["size"] == len(leaves) and s["capacity_after_insert"] == final_capacity
    same(s.bytes("leaves"), leaves, "leaves")
    # a view refused for its size on a table reserved to a load of 1/3: false, and no re-housing to 2 n
    assert s["oversized_view"] == 0 and s["capacity_after_oversized_view"] == 3 * len(leaves)
    # the tree, depth queries, files
    same(s.bytes("tree"), roomy.tree(), "tree")
    for d in (16, 14):
        some, every = roomy.nodes_at_depth(d, 0.0), roomy.nodes_at_depth(d)
        assert 0 < len(some) < len(every)
        same(s.bytes("level_threshold_%d" % d), some, "level")
        same(s.bytes("level_all_%d" % d), every, "level")
    mine = s.path("binding.ot")
    roomy.write(mine)
    with open(mine, "rb") as f, open(s.path("map.ot"), "rb") as g:
        assert f.read() == g.read()
    same(s.bytes("leaves_read"), leaves, "read")
    with fe.octomap(len(leaves), resolution=resolution) as half:
        half.set_leaves(leaves[::-1][:len(leaves) // 2])
        same(s.bytes("leaves_set"), half.leaves(), "set_leaves")
    # the read side: the program's table was loaded to 1 and re-housed once; the binding's is roomy
    assert s["capacity_full"] == len(leaves) and 4 * len(leaves) <= 3 * roomy.capacity
    assert s["capacity_after_search"] == s["capacity_after_rays"] == s["capacity_after_view"] == 2 * len(leaves)
    same(s.bytes("occupied_log_odds"), np.array([roomy.occupied_log_odds], np.float32), "occupied")
    found, at_points = roomy.search(points)
    assert set(found.tolist()) == {0, 1, 2}
    same(s.bytes("found"), found, "found")
    same(s.bytes("found_leaves"), at_points, "found leaves")
    hits = roomy.cast_rays(origins, directions, False, 4.0)
    assert len(set(hits["status"].tolist())) >= 2 and (hits["status"] == RAY_HIT).any()
    same(s.bytes("hits"), hits, "hits")
    cloud, status = roomy.view_cloud(T[0], *view[:4], int(view[4]), int(view[5]), ignore_unknown=True, with_status=True)
    assert (status == RAY_HIT).any()
    same(s.bytes("view"), cloud, "view")
    same(s.bytes("view_status"), status, "view status")
    same(s.bytes("leaves_after_queries"), leaves, "leaves after the queries")
    roomy.close()
    fe.close()


# ---- front --------------------------------------------------------------------------------------------------------------------
def padded(a, extra):
    """(the rows of a 2-D array in a buffer whose rows are `extra` elements longer, that buffer)."""
    buf = np.zeros((a.shape[0], a.shape[1] + extra), a.dtype)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]], buf


def check_node(s, name, fe, node_id, got):
    kp, desc, xyz = got
    assert len(kp) > 50, name
    same(s.bytes(name + "_keypoints"), kp, name)
    same(s.bytes(name + "_descriptors"), desc, name)
    same(s.bytes(name + "_xyz"), xyz, name)
    fe.upload_node(node_id, desc, xyz)
    assert s[name + "_features"] == len(kp) and s[name + "_matchable"] == 1 and s[name + "_resident"] == fe.node_count(node_id) == len(kp)


def test_front(exe, tmp_path):
    """setDetectorType, fastDetect with more corners than its first buffer holds, and the sensor-frame Node constructor on
    rgb8 + 16UC1 and mono8 + 32FC1 frames with padded rows and a depth image of half the size."""
    rng = np.random.default_rng(23)
    noise, flat = rng.integers(0, 256, (480, 640), dtype=np.uint8), np.full((480, 640), 90, np.uint8)
    threshold, max_keypoints = 20, 300
    img = synth.make_image_sequence(n_frames=2, seed=1)
    K = np.array([float(img[k]) for k in ("fx", "fy", "cx", "cy")])
    gray = [np.ascontiguousarray(g, np.uint8) for g in img["gray"]]
    rows, cols = gray[0].shape
    colour = np.stack([gray[0], np.roll(gray[0], 1, axis=1), 255 - gray[0]], axis=2)
    rgb_rows, rgb_buf = padded(colour.reshape(rows, cols * 3), 13)
    rgb_view = np.lib.stride_tricks.as_strided(rgb_buf, (rows, cols, 3), (rgb_buf.strides[0], 3, 1))
    assert np.array_equal(rgb_view, colour)
    half = [np.ascontiguousarray(d[::2, ::2], np.float32) for d in img["depth"]]
    mm = np.where(np.isnan(half[0]), 0, np.round(half[0] * 1000.0)).astype(np.uint16)
    d16_view, d16_buf = padded(mm, 5)
    mono_view, mono_buf = padded(gray[1], 7)
    d32_view, d32_buf = padded(half[1], 3)
    s = run_section(exe, "front", dict(noise=noise, flat=flat, fast_threshold=np.array([threshold], np.int64),
                                       max_keypoints=np.array([max_keypoints], np.int64), rgb8=rgb_buf, depth16=d16_buf,
                                       mono8=mono_buf, depth32=d32_buf, K=K,
                                       shapes=np.array([rows, cols, rows // 2, cols // 2], np.int64)), tmp_path)
    fe = front_end(4, 2048, 8)
    fe.set_detector_type("FAST")
    fe.set_detector_type("ORB")
    with pytest.raises(ValueError):
        fe.set_detector_type("SURF")
    assert s["unknown_detector_throws"] == 1
    corners = fe.fast_detect(noise, None, threshold)
    assert len(corners) > 4096   # more than fastDetect's first buffer
    same(s.bytes("fast_noise"), corners, "fast noise")
    assert len(fe.fast_detect(flat, None, threshold)) == 0 and s.bytes("fast_flat") == b""
    fe.detector_configure(max_keypoints=max_keypoints)
    check_node(s, "colour", fe, 0, fe.sensor_detect_describe(rgb_view, d16_view, *K, visual_encoding="rgb8"))
    check_node(s, "grey", fe, 1, fe.sensor_detect_describe(mono_view, d32_view, *K))
    fe.close()
