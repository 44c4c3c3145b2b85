"""Candidate selection for loop closure: the host-side mirror of
``GraphManager::getPotentialEdgeTargetsWithDijkstra`` (graph_manager.cpp:204-324) over the C ABI
(``rgbdfe_pose_graph_*`` / ``rgbdfe_potential_edge_targets`` in include/rgbdfe.h).  Its output is the list of
earlier nodes a new node is compared with, i.e. the ``tids`` of ``FrontEnd.match_node_pairs``."""
import ctypes as C

import numpy as np

from . import _lib


class PoseGraph:
    """What the reference's candidate selection reads from GraphManager: graph_ (id_, vertex_id_, matchable_),
    camera_vertices, the optimizer's edges and keyframe_ids_."""

    def __init__(self):
        self._L = _lib.load()
        self._g = self._L.rgbdfe_pose_graph_create()
        if not self._g:
            raise _lib.RgbdfeError("rgbdfe_pose_graph_create failed")
        self._ids = set()

    def close(self):
        if self._g:
            self._L.rgbdfe_pose_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise _lib.RgbdfeError(self._L.rgbdfe_status_string(rc).decode())

    def add_node(self, node_id, vertex_id=None, matchable=True, keyframe=False):
        """A Node entering graph_ (GraphManager::addNode, graph_manager.cpp:681; firstNode :326)."""
        self._check(self._L.rgbdfe_pose_graph_add_node(self._g, int(node_id), int(node_id if vertex_id is None else vertex_id),
                                                       int(bool(matchable)), int(bool(keyframe))))
        self._ids.add(int(node_id))

    def add_edge(self, id1, id2):
        """An edge entering the optimizer (GraphManager::addEdgeToG2O, graph_manager.cpp:811)."""
        self._check(self._L.rgbdfe_pose_graph_add_edge(self._g, int(id1), int(id2)))

    # ---- the optimiser (include/rgbdfe.h, "pose-graph optimisation") ----
    @staticmethod
    def _ctx(front_end):
        return getattr(front_end, "_ctx", front_end)

    @staticmethod
    def _report(rep):
        its = [dict(trials=int(r.trials), pcg=[int(v) for v in r.pcg_iterations[:r.trials]], chi2_before=float(r.chi2_before),
                    chi2_after=float(r.chi2_after), lam=float(r.lam)) for r in rep.it[:rep.recorded]]
        return dict(iterations=int(rep.iterations), chi2=float(rep.chi2), its=its, launches=int(rep.launches),
                    readbacks=int(rep.readbacks), upload_seconds=float(rep.upload_seconds),
                    total_seconds=float(rep.total_seconds))

    def set_estimate(self, node_id, transform):
        """The vertex's estimate: a 4x4 (row, column) array."""
        t = np.ascontiguousarray(np.asarray(transform, np.float64).reshape(4, 4).T)
        self._check(self._L.rgbdfe_pose_graph_set_estimate(self._g, int(node_id), t.ctypes.data))

    def get_estimate(self, node_id):
        t = np.zeros((4, 4), np.float64)
        self._check(self._L.rgbdfe_pose_graph_get_estimate(self._g, int(node_id), t.ctypes.data))
        return t.T.copy()

    def set_fixed(self, node_id, fixed=True):
        self._check(self._L.rgbdfe_pose_graph_set_fixed(self._g, int(node_id), int(bool(fixed))))

    def add_edge_se3(self, id1, id2, transform, information, set_estimate=False):
        """An edge with its measurement entering the optimizer (GraphManager::addEdgeToG2O, graph_manager.cpp:811-909):
        transform 4x4, information 6x6 (or a scalar: I * information, matchNodePair's)."""
        t = np.ascontiguousarray(np.asarray(transform, np.float64).reshape(4, 4).T)
        info = np.asarray(information, np.float64)
        info = np.ascontiguousarray(np.eye(6) * float(info) if info.ndim == 0 else info.reshape(6, 6))
        self._check(self._L.rgbdfe_pose_graph_add_edge_se3(self._g, int(id1), int(id2), t.ctypes.data, info.ctypes.data,
                                                           int(bool(set_estimate))))

    def chi2(self, front_end):
        out = C.c_double(0)
        self._check(self._L.rgbdfe_pose_graph_chi2(self._ctx(front_end), self._g, C.byref(out)))
        return out.value

    def linearize(self, front_end):
        """One linearisation: dict(e[E,6], w[E], free_ids, Hd[nf,6,6], b[nf,6], rows, cols, B[nb,6,6], chi2)."""
        ne, nf, nb = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        chi2 = C.c_double(0)
        rc = self._L.rgbdfe_pose_graph_linearize(self._ctx(front_end), self._g, None, None, 0, C.byref(ne), None, None, None, 0,
                                                 C.byref(nf), None, None, None, 0, C.byref(nb), C.byref(chi2))
        if rc not in (0, -5):  # RGBDFE_ERR_CAPACITY: the counts are set
            self._check(rc)
        e, w = np.zeros((ne.value, 6)), np.zeros(ne.value)
        ids, Hd, b = np.zeros(nf.value, np.int32), np.zeros((nf.value, 6, 6)), np.zeros((nf.value, 6))
        rows, cols, B = np.zeros(nb.value, np.int32), np.zeros(nb.value, np.int32), np.zeros((nb.value, 6, 6))
        self._check(self._L.rgbdfe_pose_graph_linearize(
            self._ctx(front_end), self._g, e.ctypes.data, w.ctypes.data, ne.value, C.byref(ne), ids.ctypes.data, Hd.ctypes.data,
            b.ctypes.data, nf.value, C.byref(nf), rows.ctypes.data, cols.ctypes.data, B.ctypes.data, nb.value, C.byref(nb),
            C.byref(chi2)))
        return dict(e=e, w=w, free_ids=ids, Hd=Hd, b=b, rows=rows, cols=cols, B=B, chi2=chi2.value)

    def optimize(self, front_end, iterations):
        """SparseOptimizer::optimize(iterations); the report as a dict."""
        rep = _lib.PoseGraphReport()
        self._check(self._L.rgbdfe_pose_graph_optimize(self._ctx(front_end), self._g, int(iterations), C.byref(rep)))
        return self._report(rep)

    def optimize_graph(self, front_end, break_criterion=0.01):
        """The loop of GraphManager::optimizeGraphImpl (optimizer_iterations = 0.01 by default); the report as a dict."""
        rep = _lib.PoseGraphReport()
        self._check(self._L.rgbdfe_pose_graph_optimize_graph(self._ctx(front_end), self._g, float(break_criterion), C.byref(rep)))
        return self._report(rep)

    # ---- fixation strategies, pruning and the evaluation rounds (include/rgbdfe.h) ----
    def set_strategy(self, strategy):
        """pose_relative_to: "none" (the default: set_fixed's flags as they stand), "first", "previous", "largest_loop",
        "inaffected", or the RGBDFE_POSE_RELATIVE_TO_* number."""
        s = _lib.POSE_RELATIVE_TO[strategy] if isinstance(strategy, str) else int(strategy)
        self._check(self._L.rgbdfe_pose_graph_set_strategy(self._g, s))

    def get_fixed(self, node_id):
        out = C.c_int32(0)
        self._check(self._L.rgbdfe_pose_graph_get_fixed(self._g, int(node_id), C.byref(out)))
        return bool(out.value)

    def edge(self, index):
        """A measured edge by insertion index: dict(id1, id2, transform[4,4], information[6,6], active)."""
        i1, i2, act = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        t, info = np.zeros((4, 4)), np.zeros((6, 6))
        self._check(self._L.rgbdfe_pose_graph_get_edge(self._g, int(index), C.byref(i1), C.byref(i2), t.ctypes.data,
                                                       info.ctypes.data, C.byref(act)))
        return dict(id1=i1.value, id2=i2.value, transform=t.T.copy(), information=info, active=bool(act.value))

    def sanity_check(self, thresh):
        """GraphManager::sanityCheck: the number of edges whose information became 0.000001 I."""
        n = self._L.rgbdfe_pose_graph_sanity_check(self._g, float(thresh))
        if n < 0:
            self._check(n)
        return n

    def edge_errors(self, front_end):
        """Per measured edge: dict(chi2[E] (before Huber), err_sq[E], active[E])."""
        ne = C.c_int32(0)
        rc = self._L.rgbdfe_pose_graph_edge_errors(self._ctx(front_end), self._g, None, None, None, 0, C.byref(ne))
        if rc not in (0, -5):  # RGBDFE_ERR_CAPACITY: the count is set
            self._check(rc)
        chi2, sq, act = np.zeros(ne.value), np.zeros(ne.value), np.zeros(ne.value, np.int32)
        self._check(self._L.rgbdfe_pose_graph_edge_errors(self._ctx(front_end), self._g, chi2.ctypes.data, sq.ctypes.data,
                                                          act.ctypes.data, ne.value, C.byref(ne)))
        return dict(chi2=chi2, err_sq=sq, active=act.astype(bool))

    def prune_edges(self, front_end, thresh, n_edges=None):
        """GraphManager::pruneEdgesWithErrorAbove: (edges pruned, a verdict per edge: RGBDFE_PRUNE_* as uint8)."""
        if n_edges is None:
            ne = C.c_int32(0)
            rc = self._L.rgbdfe_pose_graph_edge_errors(self._ctx(front_end), self._g, None, None, None, 0, C.byref(ne))
            if rc not in (0, -5):
                self._check(rc)
            n_edges = ne.value
        verdicts = np.zeros(max(int(n_edges), 1), np.uint8)
        n = C.c_int32(0)
        self._check(self._L.rgbdfe_pose_graph_prune_edges(self._ctx(front_end), self._g, float(thresh), verdicts.ctypes.data,
                                                          int(n_edges), C.byref(n)))
        return n.value, verdicts[:int(n_edges)].copy()

    def evaluate(self, front_end, optimizer_iterations=0.01):
        """OpenNIListener::evaluation's five rounds: (rounds: a list of dicts, estimates[5, n, 4, 4] in ascending node id)."""
        ev = _lib.PoseGraphEvaluation()
        n_nodes = self.node_count()
        est = np.zeros((_lib.POSE_GRAPH_EVALUATION_ROUNDS, n_nodes, 16))
        self._check(self._L.rgbdfe_pose_graph_evaluate(self._ctx(front_end), self._g, float(optimizer_iterations), C.byref(ev),
                                                       est.ctypes.data, n_nodes))
        rounds = [dict(chi2=float(r.chi2), iterations=int(r.iterations), pruned=int(r.pruned), launches=int(r.launches),
                       readbacks=int(r.readbacks), upload_seconds=float(r.upload_seconds), seconds=float(r.seconds))
                  for r in ev.round]
        return rounds, est.reshape(-1, n_nodes, 4, 4).transpose(0, 1, 3, 2).copy()

    def node_count(self):
        return len(self._ids)

    def write_trajectory(self, path, node_ids, timestamps, base2points=None, init_base_pose=None, frame_id=None,
                         child_frame_id=None):
        """GraphManager::saveTrajectory's estimate file (TUM format: stamp tx ty tz qx qy qz qw)."""
        ids = np.ascontiguousarray(node_ids, np.int32).reshape(-1)
        ts = np.ascontiguousarray(timestamps, np.float64).reshape(-1)
        if len(ids) != len(ts):
            raise ValueError("one time stamp per node")
        mat = lambda m: None if m is None else np.ascontiguousarray(np.asarray(m, np.float64).reshape(4, 4).T)
        b2p, init = mat(base2points), mat(init_base_pose)
        enc = lambda v: None if v is None else str(v).encode()
        self._check(self._L.rgbdfe_pose_graph_write_trajectory(
            self._g, str(path).encode(), len(ids), ids.ctypes.data, ts.ctypes.data, None if b2p is None else b2p.ctypes.data,
            None if init is None else init.ctypes.data, enc(frame_id), enc(child_frame_id)))

    def transforms(self, node_ids):
        """The estimates as n x 4 x 4 float32 (row, column) matrices: the `transforms` of FrontEnd.assemble_map and
        OctoMap.insert_nodes."""
        ids = np.ascontiguousarray(node_ids, np.int32).reshape(-1)
        out = np.zeros((len(ids), 16), np.float32)  # column-major rows, as the C ABI gives them
        self._check(self._L.rgbdfe_pose_graph_transforms(self._g, len(ids), ids.ctypes.data, out.ctypes.data))
        return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()

    # ---- the graph as a byte string (include/rgbdfe.h, "session files") ----
    def _check_string(self, rc):
        if rc != 0:
            raise _lib.RgbdfeError("%s: %s" % (self._L.rgbdfe_status_string(rc).decode(), self._L.rgbdfe_last_error(None).decode()))

    def serialize(self) -> bytes:
        """Everything in the graph -- nodes with their estimates and flags, edges with their pruning gates, keyframes,
        strategy, earliest_loop_closure_node -- as one byte string; the same graph gives the same bytes."""
        n = C.c_int64(0)
        rc = self._L.rgbdfe_pose_graph_serialize(self._g, None, 0, C.byref(n))
        if rc not in (0, -5):  # RGBDFE_ERR_CAPACITY: the length is set
            self._check_string(rc)
        buf = np.zeros(max(n.value, 1), np.uint8)
        self._check_string(self._L.rgbdfe_pose_graph_serialize(self._g, buf.ctypes.data, n.value, C.byref(n)))
        return buf[: n.value].tobytes()

    def deserialize(self, data: bytes):
        """Into an empty graph (a new one, or after clear): refused otherwise, and for any string that is not exactly what
        serialize returned."""
        buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        self._check_string(self._L.rgbdfe_pose_graph_deserialize(self._g, buf.ctypes.data, len(data)))
        self._sync_ids()

    def node_ids(self):
        n = C.c_int32(0)
        rc = self._L.rgbdfe_pose_graph_node_ids(self._g, None, 0, C.byref(n))
        if rc not in (0, -5):
            self._check(rc)
        ids = np.zeros(max(n.value, 1), np.int32)
        self._check(self._L.rgbdfe_pose_graph_node_ids(self._g, ids.ctypes.data, n.value, C.byref(n)))
        return ids[: n.value].copy()

    def _sync_ids(self):
        """After the C side filled the graph (deserialize, FrontEnd.load_session)."""
        self._ids = set(int(i) for i in self.node_ids())

    def set_matchable(self, node_id, matchable):
        self._check(self._L.rgbdfe_pose_graph_set_matchable(self._g, int(node_id), int(bool(matchable))))

    def potential_edge_targets(self, sequential_targets, geodesic_targets, sampled_targets, geodesic_depth=3,
                               predecessor_id=-1, include_predecessor=False, rand=None, seed=0):
        """ids to compare the next node with.  rand: a callable returning the next rand() value (e.g. libc's rand for
        the reference's stream); None = the library's counter-based generator seeded with `seed`."""
        cap = int(sequential_targets + geodesic_targets + sampled_targets + 1)
        out = np.zeros(max(cap, 1), np.int32)
        n = C.c_int32(0)
        cb = self._L.rgbdfe_rand_fn((lambda _state: int(rand())) if rand is not None else 0)
        self._check(self._L.rgbdfe_potential_edge_targets(
            self._g, int(sequential_targets), int(geodesic_targets), int(sampled_targets), int(geodesic_depth),
            int(predecessor_id), int(bool(include_predecessor)), cb, None, int(seed) & 0xFFFFFFFF,
            out.ctypes.data, out.size, C.byref(n)))
        return out[: n.value].copy()
