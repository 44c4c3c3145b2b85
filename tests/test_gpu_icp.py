"""-m gpu: the ICP fallback (include/rgbdfe.h, "ICP fallback"; csrc/icp.hip, csrc/api_icp.hip) through the C ABI against the
literal restatement in tests/icp_oracle.py.  Every comparison is on bytes: the transforms, the reports, j(i) and d2 of the
last iteration, filterCloud's indices and rows.  tests/test_oracle_icp.py holds the oracle against independent arithmetic;
tests/test_emu_icp_kernels.py runs the kernel source on the CPU."""
import ctypes as C

import numpy as np
import pytest

import icp_oracle as io

pytestmark = pytest.mark.gpu

INVALID_ARG, UNKNOWN_NODE, CAPACITY = -1, -4, -5
CASES = io.planted_cases()


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=512, max_pairs_per_batch=64)
    yield f
    f.close()


def same(a, b, dtype):
    return np.asarray(a, dtype).tobytes() == np.asarray(b, dtype).tobytes()


def record_reads(k, max_iterations):
    """(record reads, iterations enqueued) of a call whose last job stops at iteration k: chunks of 2, 4, 8, 16, 16 ..."""
    done, chunk, reads = 0, 2, 0
    while done < k:
        done = min(done + chunk, max_iterations)
        reads += 1
        chunk = min(2 * chunk, 16)
    return reads, done


def check_report(rep, ref):
    assert (int(rep["converged"]), int(rep["state"]), int(rep["iterations"]), int(rep["correspondences"])) == \
        (ref["converged"], ref["state"], ref["iterations"], ref["c"])
    assert same(rep["mse"], ref["mse"], np.float64)
    assert (int(rep["n_source"]), int(rep["n_target"])) == (ref["n_source"], ref["n_target"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_planted_case_gives_the_oracles_bytes(fe, name):
    case = CASES[name]
    ref = io.reference(name)
    assert (ref["state"], ref["iterations"]) == case["expect"]
    T, rep, nn_j, nn_d2 = fe.icp_align_clouds(case["source"], case["target"], case["G"], fe.icp_params(**case["params"]), debug=True)
    check_report(rep, ref)
    assert same(T, ref["T"], np.float32)
    assert same(nn_j, ref["nn_j"], np.int32) and same(nn_d2, ref["nn_d2"], np.float32)
    reads, enqueued = record_reads(ref["iterations"], case["params"]["max_iterations"])
    gather = 1 if max(ref["n_source"], ref["n_target"]) else 0
    assert int(rep["launches"]) == 2 + gather + enqueued * (2 if ref["n_source"] else 1)
    assert int(rep["readbacks"]) == 1 + reads + 1   # the valid counts, the records per chunk, the debug arrays


def test_the_guess_comes_back_untouched_when_nothing_converges(fe):
    case = CASES["target 10 m away"]
    G = np.array(case["G"], np.float32)
    G[3] = [1e-3, -2.0, 0.5, 7.0]   # the last row is not used, and returned as given
    T, rep = fe.icp_align_clouds(case["source"], case["target"], G, fe.icp_params())
    assert int(rep["converged"]) == 0 and int(rep["state"]) == io.NO_CORRESPONDENCES and same(T, G, np.float32)


def test_the_kept_pairs_at_the_threshold(fe):
    case = CASES["d2 at the threshold and one float above"]
    _, rep, nn_j, nn_d2 = fe.icp_align_clouds(case["source"], case["target"], None, fe.icp_params(**case["params"]), debug=True)
    thr = np.float32(0.0625)
    assert nn_d2[0] == thr and nn_d2[1] == np.nextafter(thr, np.float32(1)) and list(nn_j) == [0, 1, 2, 3, 4]
    assert int(rep["correspondences"]) == 4   # row 0 kept, row 1 dropped


def test_duplicated_target_rows_answer_with_the_lowest_index(fe):
    case = CASES["duplicated target rows"]
    _, _, nn_j, _ = fe.icp_align_clouds(case["source"], case["target"], None, fe.icp_params(**case["params"]), debug=True)
    assert nn_j.min() >= 0 and nn_j.max() < len(case["target"]) // 2


@pytest.mark.parametrize("n_valid,desired,count", [(3072, 100, 101), (2999, 7, 8), (3072, 3072, 3072), (3072, 5000, 3072),
                                                   (1, 10, 1), (257, 256, 256), (513, 2, 2), (65, 64, 64)])
def test_filter_cloud(fe, n_valid, desired, count):
    cloud = io.room_corner(holes=3072 - n_valid, seed=n_valid)
    idx, rows = fe.filter_cloud(cloud, desired)
    ref_idx, ref_rows = io.filter_cloud(cloud, desired)
    assert len(idx) == count == len(ref_idx)
    assert np.array_equal(idx, ref_idx) and same(rows, ref_rows, np.float32)


def test_filter_cloud_edges(fe):
    nan = io.room_corner()
    nan[:, 2] = np.nan
    idx, rows = fe.filter_cloud(nan, 100)
    assert len(idx) == 0 and len(rows) == 0
    idx, rows = fe.filter_cloud(np.zeros((0, 4), np.float32), 100)
    assert len(idx) == 0
    bad = io.room_corner()
    bad[3, 0], bad[4, 1] = np.inf, np.nan   # filterCloud itself looks at z alone
    idx, rows = fe.filter_cloud(bad, 5000)
    assert len(idx) == 3072 and same(rows, bad, np.float32)
    cloud = io.room_corner()
    n_out = C.c_int64(0)
    out = np.zeros((50, 4), np.float32)
    st = fe._L.rgbdfe_filter_cloud(fe._ctx, cloud.ctypes.data, len(cloud), 100, None, out.ctypes.data, 50, C.byref(n_out))
    assert st == CAPACITY and n_out.value == 101
    for desired in (0, -3):
        assert fe._L.rgbdfe_filter_cloud(fe._ctx, cloud.ctypes.data, len(cloud), desired, None, out.ctypes.data, 50,
                                         C.byref(n_out)) == INVALID_ARG


def test_argument_errors(fe):
    from rgbdslam_v2_amd.frontend import RgbdfeError
    c = io.room_corner(16, 12)
    for kw in (dict(max_iterations=0), dict(max_iterations=1001), dict(max_correspondence_distance=-0.01),
               dict(max_correspondence_distance=float("nan")), dict(transformation_epsilon=float("nan")),
               dict(euclidean_fitness_epsilon=float("nan")), dict(desired_size=0), dict(desired_size=-1)):
        with pytest.raises(RgbdfeError):
            fe.icp_align_clouds(c, c, None, fe.icp_params(**kw))
    for kw in (dict(max_iterations=1), dict(max_iterations=1000), dict(max_correspondence_distance=0.0),
               dict(max_correspondence_distance=float("inf"))):
        fe.icp_align_clouds(c, c, None, fe.icp_params(**kw))
    prm = fe.icp_params()
    T = np.zeros(16, np.float32)
    L = fe._L
    assert L.rgbdfe_icp_align_nodes(fe._ctx, 0, None, None, None, C.byref(prm), None, None) == 0
    ids = np.array([987654], np.int32)
    assert L.rgbdfe_icp_align_nodes(fe._ctx, 1, ids.ctypes.data, ids.ctypes.data, None, C.byref(prm), T.ctypes.data, None) == UNKNOWN_NODE
    assert L.rgbdfe_icp_align_nodes(fe._ctx, -1, ids.ctypes.data, ids.ctypes.data, None, C.byref(prm), T.ctypes.data, None) == INVALID_ARG
    assert L.rgbdfe_icp_align_nodes(fe._ctx, 1, ids.ctypes.data, ids.ctypes.data, None, None, T.ctypes.data, None) == INVALID_ARG
    nn = np.zeros(10, np.int32)
    assert L.rgbdfe_icp_align_clouds(fe._ctx, c.ctypes.data, len(c), c.ctypes.data, len(c), None, C.byref(prm), T.ctypes.data, None,
                                     nn.ctypes.data, None, 10) == CAPACITY
    assert L.rgbdfe_icp_align_clouds(fe._ctx, None, 5, c.ctypes.data, len(c), None, C.byref(prm), T.ctypes.data, None, None, None,
                                     0) == INVALID_ARG


@pytest.fixture(scope="module")
def batch(fe):
    """The resident clouds of io.BATCH_NODES, as the library built them from the depth images."""
    clouds = {}
    for nid, (cols, rows, mv) in io.BATCH_NODES.items():
        depth, (fx, fy, cx, cy) = io.corner_depth(cols, rows, None if mv is None else io._pose(mv))
        clouds[nid] = fe.upload_node_cloud(nid, depth, fx, fy, cx, cy, cloud_skip=1, return_cloud=True).reshape(-1, 4).copy()
    yield clouds
    for nid in io.BATCH_NODES:
        fe.release_node_cloud(nid)


def test_one_batch_of_mixed_jobs_over_resident_clouds(fe, batch):
    src = [j[0] for j in io.BATCH_JOBS]
    tgt = [j[1] for j in io.BATCH_JOBS]
    G = np.stack([np.eye(4, dtype=np.float32) if j[2] is None else np.linalg.inv(io._pose(j[2])).astype(np.float32)
                  for j in io.BATCH_JOBS])
    T, rep = fe.icp_align_nodes(src, tgt, G, fe.icp_params(**io.BATCH_PARAMS))
    refs = [io.align_clouds(batch[s], batch[t], g, **io.BATCH_PARAMS) for s, t, g in zip(src, tgt, G)]
    ends = set()
    for k, ref in enumerate(refs):
        check_report(rep[k], ref)
        assert same(T[k], ref["T"], np.float32)
        ends.add(record_reads(ref["iterations"], io.BATCH_PARAMS["max_iterations"])[0])
    # the jobs end in different read-back chunks, one of them at the iteration limit; a repeated job repeats its bytes
    assert len(ends) >= 3 and any(r["state"] == io.ITERATIONS for r in refs)
    assert same(T[3], T[8], np.float32)
    last = max(r["iterations"] for r in refs)
    reads, enqueued = record_reads(last, io.BATCH_PARAMS["max_iterations"])
    assert all(int(r["launches"]) == 2 + 1 + 2 * enqueued and int(r["readbacks"]) == 1 + reads for r in rep)


def test_guesses_may_be_null_and_a_job_alone_equals_the_batch(fe, batch):
    prm = fe.icp_params(**io.BATCH_PARAMS)
    T, rep = fe.icp_align_nodes([30, 11], [31, 11], None, prm)
    one, rep1 = fe.icp_align_nodes([30], [31], None, prm)
    assert same(T[0], one[0], np.float32) and int(rep[0]["iterations"]) == int(rep1[0]["iterations"])
    host, rep2 = fe.icp_align_clouds(batch[30], batch[31], None, prm)
    assert same(host, one[0], np.float32)


def test_icp_fallback_serves_the_adjacent_pair_without_an_edge(fe, batch):
    """A new node 12 against candidates 11 (adjacent, five features: RANSAC has nothing to work with), 9 (RANSAC finds its
    edge) and 5 (five features again, but not adjacent): icp_fallback gives 11, and only 11, an edge."""
    from rgbdslam_v2_amd import synth
    seq = synth.make_sequence(n_frames=4, n_kp=500, n_world=2000, seed=7)
    fe.upload_node(12, seq["desc"][3], seq["xyz1"][3])
    fe.upload_node(11, seq["desc"][2][:5], seq["xyz1"][2][:5])
    fe.upload_node(9, seq["desc"][1], seq["xyz1"][1])
    fe.upload_node(5, seq["desc"][0][:5], seq["xyz1"][0][:5])
    cand = np.array([11, 9, 5], np.int32)
    results = fe.match_pair_list(np.full(3, 12, np.int32), cand)
    assert [int(r["id1"]) >= 0 for r in results] == [False, True, False]
    out, served, trafos, rep = fe.icp_fallback(results, 12, cand)
    assert list(served) == [0]
    ref = io.align_clouds(batch[11], batch[12], None)   # the older cloud is the source; the reference's defaults
    assert ref["converged"] and (ref["state"], ref["iterations"]) == (io.REL_MSE, 2)
    check_report(rep[0], ref)
    assert same(trafos[0], ref["T"], np.float32)
    assert (int(out[0]["id1"]), int(out[0]["id2"])) == (11, 12)
    assert same(np.array(out[0]["trafo"], np.float32).reshape(4, 4).T, ref["T"], np.float32)
    for name in out.dtype.names:   # nothing else changes, in any record
        if name not in ("id1", "id2", "trafo"):
            assert np.array_equal(out[name], results[name])
    assert out[1].tobytes() == results[1].tobytes() and out[2].tobytes() == results[2].tobytes()
    for nid in (9, 5):   # 12 and 11 go with the fixture's clouds
        fe.release_node(nid)


def test_profiling_times_the_nearest_neighbour_launches_and_changes_nothing(fe):
    from rgbdslam_v2_amd import _lib
    case = CASES["full loop, abs mse in the second chunk"]
    prm = fe.icp_params(**case["params"])
    plain, rep0 = fe.icp_align_clouds(case["source"], case["target"], None, prm)
    fe.set_profiling(True)
    fe.reset_kernel_time()
    try:
        timed, rep1 = fe.icp_align_clouds(case["source"], case["target"], None, prm)
        ms, launches, jobs = fe.kernel_time(_lib.KERNEL_ICP_NN)
    finally:
        fe.set_profiling(False)
    assert same(timed, plain, np.float32) and rep1.tobytes() == rep0.tobytes()
    enqueued = record_reads(int(rep0["iterations"]), case["params"]["max_iterations"])[1]
    assert launches == enqueued == jobs and ms > 0


# ---- the later trips of icp_scan_kernel (csrc/icp.hip): 256 tiles of 256 rows a trip, then icp_gather_kernel's search over them
SCAN_TILE, SCAN_TRIP = 256, 256 * 256  # kIcpScanTile; the rows of one trip


def empty_tiles(cloud):
    """No depth in the rows of tiles 0 .. 3 and 100 .. 102: runs of equal entries in tile_first."""
    cloud[:4 * SCAN_TILE, 2] = np.nan
    cloud[100 * SCAN_TILE:103 * SCAN_TILE, 2] = np.nan
    return cloud


@pytest.fixture(scope="module")
def quarter_vga():
    """320 x 240 = 76 800 rows = 300 tiles: a second trip of 44 tiles."""
    return empty_tiles(io.room_corner(320, 240, holes=5000, seed=9))


def check_filter(fe, cloud, desired):
    idx, rows = fe.filter_cloud(cloud, desired)
    ref_idx, ref_rows = io.filter_cloud(cloud, desired)
    assert len(idx) == len(ref_idx) and np.array_equal(idx, ref_idx) and same(rows, ref_rows, np.float32)
    return ref_idx


@pytest.mark.parametrize("desired", [7, 5000, 76800])
def test_filter_cloud_over_more_tiles_than_one_trip(fe, quarter_vga, desired):
    valid = ~np.isnan(quarter_vga[:, 2])
    assert len(quarter_vga) == 300 * SCAN_TILE and valid[SCAN_TRIP:].sum() > 10000 and not valid[:4 * SCAN_TILE].any()
    ref_idx = check_filter(fe, quarter_vga, desired)
    assert ref_idx.max() >= SCAN_TRIP and ref_idx.min() >= 4 * SCAN_TILE  # samples whose tile lies in the second trip
    assert desired < 76800 or len(ref_idx) == valid.sum()


@pytest.mark.parametrize("n,n_trips", [(65536, 1), (65537, 2), (640 * 480, 5)])
def test_filter_cloud_at_one_full_trip_one_row_more_and_five_trips(fe, n, n_trips):
    cols, rows = (640, 480) if n > 320 * 240 else (320, 240)
    cloud = empty_tiles(io.room_corner(cols, rows, holes=n // 16, seed=n % 1000))[:n].copy()
    cloud[n - 1, 2] = np.float32(2.0)  # the last row is valid: at 65 537 rows it is tile 256, the second trip, alone
    assert -(-(-(-n // SCAN_TILE)) // SCAN_TILE) == n_trips
    check_filter(fe, cloud, 1000)
    ref_idx = check_filter(fe, cloud, n)  # every valid row comes back, the last one too
    assert ref_idx[-1] == n - 1 and len(ref_idx) == (~np.isnan(cloud[:, 2])).sum()


def test_a_resident_pair_of_more_tiles_than_one_trip(fe):
    """Two 320 x 240 resident clouds (300 tiles each, the first five without depth) aligned by icp_align_nodes: the
    samples come from both trips of the scan."""
    prm = dict(max_correspondence_distance=0.25, max_iterations=12, desired_size=1000, **io.FULL_LOOP)
    clouds = {}
    try:
        for nid, mv in ((50, None), (51, 2.0)):
            depth, (fx, fy, cx, cy) = io.corner_depth(320, 240, None if mv is None else io._pose(mv), holes=3000, seed=nid)
            depth[:4, :] = np.nan  # 1280 rows: tiles 0 .. 4
            clouds[nid] = fe.upload_node_cloud(nid, depth, fx, fy, cx, cy, cloud_skip=1, return_cloud=True).reshape(-1, 4).copy()
            idx, _ = io.filter_cloud(clouds[nid], prm["desired_size"])
            assert len(clouds[nid]) == 300 * SCAN_TILE and np.isnan(clouds[nid][:5 * SCAN_TILE, 2]).all()
            assert (idx >= SCAN_TRIP).sum() > 100 and (idx < SCAN_TRIP).sum() > 100
        T, rep = fe.icp_align_nodes([50, 51], [51, 50], None, fe.icp_params(**prm))
        for k, (s, t) in enumerate(((50, 51), (51, 50))):
            ref = io.align_clouds(clouds[s], clouds[t], None, **prm)
            assert ref["c"] > 100 and ref["iterations"] >= 2
            check_report(rep[k], ref)
            assert same(T[k], ref["T"], np.float32)
    finally:
        for nid in clouds:
            fe.release_node_cloud(nid)
