"""-m gpu: the SIFT matcher's five dot kernels, mixed float-key / integer-key batches, the 4096-row cap, the ends of the dot
value and planted second-best dot products (tests/sift_match_reference.py) against the oracle.  Every comparison is exact:
index lists, n_all, L2 distances, inlier sets and pose bits with np.array_equal against po.sift_match /
po.match_sift_node_pair; against sift_match_reference.match the index lists."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po

import sift_match_reference as sr

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sift_variant_worker.py")


def _front_end(**kw):
    from rgbdslam_v2_amd.frontend import FrontEnd
    return FrontEnd(device_id=0, **kw)


def _match_nodes(fe, d1, x1, d2, x2):
    fe.upload_sift_node(1, d1, x1)
    fe.upload_sift_node(2, d2, x2)
    try:
        return fe.sift_match_nodes(1, 2)
    finally:
        fe.release_node(1)
        fe.release_node(2)


def _assert_record(rec, dd, ref, what):
    from rgbdslam_v2_amd.frontend import inlier_indices
    n = ref["n_all"]
    assert rec["n_all"] == n, what
    assert np.array_equal(rec["all_q"][:n], ref["all_q"]) and np.array_equal(rec["all_t"][:n], ref["all_t"]), what
    assert np.array_equal(np.asarray(dd)[:n], ref["all_dist"]), what
    assert (rec["id1"], rec["id2"], rec["n_inl"]) == (ref["id1"], ref["id2"], ref["n_inl"]), what
    assert rec["real_iterations"] == ref["real_iterations"], what
    assert np.array_equal(inlier_indices(rec), ref["inl_idx"]), what
    assert np.array_equal(np.array(rec["trafo"], np.float32).reshape(4, 4).T, ref["T"]), what


# ---- the oracle's answers: once per module -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_answers():
    """{case name: (q, t, dist)} of the oracle for sift_match_reference.worker_cases()."""
    return {c["name"]: po.sift_match(c["d1"], c["d2"]) for c in sr.worker_cases()}


@pytest.fixture(scope="module")
def mixed():
    """The mixed batch's nodes, pair list and the oracle's record of every pair."""
    nodes, pq, pt = sr.mixed_batch_nodes()
    prm = po.default_params()
    refs = [po.match_sift_node_pair(nodes[q][0], nodes[q][1], int(q), nodes[t][0], nodes[t][1], int(t), prm)
            for q, t in zip(pq, pt)]
    fast = np.array([sr.fast_key_node(nodes[q][0]) and sr.fast_key_node(nodes[t][0]) for q, t in zip(pq, pt)])
    return nodes, pq, pt, refs, fast


# ---- a. planted second best, default library -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fe_planted():
    f = _front_end(max_nodes=4, max_keypoints=1152, max_pairs_per_batch=4)
    yield f
    f.close()


@pytest.mark.parametrize("n1,n2", sr.PLANTED_SIZES)
def test_planted_second_best(fe_planted, n1, n2):
    """Rows and columns that only their second-best dot product rejects, the second placed in every relation to the best
    that the kernels treat differently (sift_match_reference.row_classes / col_classes; the census is asserted by
    tests/test_oracle_sift_reference.py): a second lost in a lane's insert, the 32-lane butterfly, across LDS tiles or in
    the finish kernel's merge of row blocks makes a match appear.  Once as planted and once with the nodes exchanged, so that
    the row-side triples meet the column side and the other way round."""
    d1, d2, planted = sr.planted_case(n1, n2, 1000 * n1 + n2)
    rng = np.random.default_rng(n1 + n2)
    x1, x2 = sr.xyz(rng, n1), sr.xyz(rng, n2)
    for a, xa, b, xb in ((d1, x1, d2, x2), (d2, x2, d1, x1)):
        mq, mt, md = _match_nodes(fe_planted, a, xa, b, xb)
        oq, ot, od = po.sift_match(a, b)
        rq, rt = sr.match(a, b)
        assert np.array_equal(mq, rq) and np.array_equal(mt, rt)
        assert np.array_equal(mq, oq) and np.array_equal(mt, ot) and np.array_equal(md, od)
    assert len(mq) >= len(planted["plain"])


# ---- b. every kernel variant -----------------------------------------------------------------------------------------------------
ENVS = [{}, {"RGBDFE_SIFT_ONEPASS": "0"}, {"RGBDFE_SIFT_ONEPASS": "0", "RGBDFE_SIFT_ROWS64": "0"},
        {"RGBDFE_SIFT_ONEPASS": "0", "RGBDFE_SIFT_ROWS64": "1"}, {"RGBDFE_SIFT_FAST_KEYS": "0"}]
_SWITCHES = ("RGBDFE_SIFT_ONEPASS", "RGBDFE_SIFT_ROWS64", "RGBDFE_SIFT_FAST_KEYS")
_dead_child = []     # set once a worker died (signal, foreign exit status, timeout): no further child is started


def _env_id(env):
    return "-".join("%s=%s" % (k[len("RGBDFE_SIFT_"):], v) for k, v in env.items()) or "default"


@pytest.mark.parametrize("env", ENVS, ids=_env_id)
def test_kernel_variants(env, case_answers, mixed, tmp_path):
    """Every switch of launch_sift_dot (sift_match.hip) in a process of its own -- the switches are read once per process --
    over the planted cases, test_sift_block_shapes' sizes, test_sift_key_paths' cases and the mixed batch.  Which kernel
    a pair reaches:

      default                float-key pairs (both nodes <= 1024 rows, squared norms < 2^19): sift_top2_onepass_kernel, 256-row
                             blocks, column partials merged by sift_finish_kernel; every other pair: sift_row_top2_kernel
                             <false> and <true> (integer keys, 128-row blocks)
      ONEPASS=0              float-key pairs: two passes, rows then columns; a pass whose larger side in the batch is <= 128
                             rows runs sift_top2_fast_kernel<SWAP> (128-row blocks), above that sift_top2_fast64_kernel<SWAP>
                             (256-row blocks): (31, 128) runs fast / fast, (129, 64) fast64 / fast, (64, 129) fast / fast64;
                             integer-key pairs as by default
      ONEPASS=0 ROWS64=0     float-key pairs: sift_top2_fast_kernel<SWAP> at every size (up to 8 row blocks)
      ONEPASS=0 ROWS64=1     float-key pairs: sift_top2_fast64_kernel<SWAP> at every size (down to one row)
      FAST_KEYS=0            every pair: sift_row_top2_kernel, also the inputs that otherwise take float keys

    In the mixed batch the float-key kernel(s) and the integer-key kernel run over the same pair list and each leaves
    the other kind's pairs alone.  A worker that dies stops the remaining environments: they fail without being started."""
    if _dead_child:
        pytest.fail("not started: the worker of [%s] died (%s)" % _dead_child[0])
    out = str(tmp_path / "variant.npz")
    child_env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    child_env.update(env)
    try:
        p = subprocess.run([sys.executable, WORKER, out], env=child_env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _dead_child.append((_env_id(env), "timeout"))
        pytest.fail("the worker of [%s] ran into the timeout" % _env_id(env))
    if p.returncode not in (0, 3):
        _dead_child.append((_env_id(env), "exit status %d" % p.returncode))
        pytest.fail("the worker of [%s] died with status %d: %s" % (_env_id(env), p.returncode, p.stderr[-2000:]))
    assert p.returncode == 0 and "worker ok" in p.stdout, (p.stdout[-1000:], p.stderr[-2000:])
    got = np.load(out)
    for name, (oq, ot, od) in case_answers.items():
        assert np.array_equal(got[name + "/q"], oq) and np.array_equal(got[name + "/t"], ot), name
        assert np.array_equal(got[name + "/d"], od), name
    from rgbdslam_v2_amd._lib import RESULT_DTYPE
    nodes, pq, pt, refs, _ = mixed
    recs = np.frombuffer(got["mixed/records"].tobytes(), RESULT_DTYPE)
    assert len(recs) == len(pq)
    for rec, dd, ref, q, t in zip(recs, got["mixed/dist"], refs, pq, pt):
        _assert_record(rec, dd, ref, "pair (%d, %d)" % (q, t))


# ---- c. mixed batches through match_sift_pair_list ---------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1 << 20], ids=["one_wave_per_pair", "record_replay"])
def fe_mixed(request, mixed):
    f = _front_end(max_nodes=12, max_keypoints=1536, max_pairs_per_batch=64)
    f.set_latency_mode(request.param, 0)
    for k, (d, x) in enumerate(mixed[0]):
        f.upload_sift_node(k, d, x)
    yield f
    f.close()


def test_mixed_key_kinds_in_one_batch(fe_mixed, mixed):
    """All 64 ordered pairs of eight nodes in ONE call: 1025 and 1536 rows and a x 1.6 norm make integer-key pairs, the
    others float-key pairs, so both kernels run over the same pair list and the one-pass grid is sized by a 1536-row
    node that is not its own.  Every record equals the oracle's; a pair's record does not depend on its company."""
    nodes, pq, pt, refs, fast = mixed
    assert fast.sum() >= 10 and (~fast).sum() >= 10
    out, dist = fe_mixed.match_sift_pair_list(pq, pt)
    for rec, dd, ref, q, t in zip(out, dist, refs, pq, pt):
        _assert_record(rec, dd, ref, "pair (%d, %d)" % (q, t))
    assert sum(r["id1"] >= 0 for r in refs) >= 10           # edges among them, not only rejected pairs
    perm = np.random.default_rng(64).permutation(len(pq))
    out_p, dist_p = fe_mixed.match_sift_pair_list(pq[perm], pt[perm])
    assert out_p.tobytes() == out[perm].tobytes() and np.array_equal(np.asarray(dist_p), np.asarray(dist)[perm])
    for kind in (fast, ~fast):
        out_k, dist_k = fe_mixed.match_sift_pair_list(pq[kind], pt[kind])
        assert out_k.tobytes() == out[kind].tobytes() and np.array_equal(np.asarray(dist_k), np.asarray(dist)[kind])


# ---- d. the 4096-row cap -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fe_cap():
    f = _front_end(max_nodes=4, max_keypoints=5120, max_pairs_per_batch=4)
    yield f
    f.close()


@pytest.fixture(scope="module")
def cap_inputs():
    return sr.cap_nodes()


@pytest.mark.parametrize("n1,n2", sr.CAP_SIZES)
def test_row_cap_match_nodes(fe_cap, cap_inputs, n1, n2):
    """Nodes at and above the matcher's 4096 rows (sift_gpu_wrapper.cpp:231): rows beyond the cap never enter, and the
    integer key's 7 sequence bits are used to their end (sequence 127 = columns 4064 .. 4095)."""
    noisy, base, xn, xb = cap_inputs
    d1, d2 = noisy[:n1], base[:n2]
    mq, mt, md = _match_nodes(fe_cap, d1, xn[:n1], d2, xb[:n2])
    oq, ot, od = po.sift_match(d1, d2)
    assert len(oq) > 500 and oq.max() < 4096 and ot.max() < 4096
    if n2 >= 4096:
        assert (ot >= 4064).any()
    if n1 >= 4096:
        assert (oq >= 4064).any()
    assert np.array_equal(mq, oq) and np.array_equal(mt, ot) and np.array_equal(md, od)


def test_row_cap_pair_op(fe_cap, cap_inputs):
    noisy, base, xn, xb = cap_inputs
    fe_cap.upload_sift_node(1, noisy[:4097], xn[:4097])
    fe_cap.upload_sift_node(2, base[:5000], xb[:5000])
    try:
        out, dist = fe_cap.match_sift_pair_list([1], [2])
    finally:
        fe_cap.release_node(1)
        fe_cap.release_node(2)
    prm = po.default_params(seed=fe_cap.params.seed, depth_cov=fe_cap.params.depth_cov)
    ref = po.match_sift_node_pair(noisy[:4097], xn[:4097], 1, base[:5000], xb[:5000], 2, prm)
    assert ref["n_all"] == 300
    _assert_record(out[0], dist[0], ref, "(4097, 5000)")


# ---- e. the ends of the dot value --------------------------------------------------------------------------------------------------
def test_dot_value_extremes(fe_planted):
    """Dot 8 323 200 (all-255 rows: the largest value an integer key holds; the angle clips to 0 and the match stands) and dot
    0 (all-zero rows: the index sentinel), some of them at rows 0 and n - 1 and in the ragged last tile: through
    sift_match_nodes and inside one batch of four pairs."""
    cases = sr.extreme_cases()
    fe = fe_planted
    for c in cases:
        mq, mt, md = _match_nodes(fe, c["d1"], c["xyz1"], c["d2"], c["xyz2"])
        oq, ot, od = po.sift_match(c["d1"], c["d2"])
        assert np.array_equal(mq, oq) and np.array_equal(mt, ot) and np.array_equal(md, od), c["name"]
        if c["name"] == "saturated":
            assert (77, 133) in set(zip(oq.tolist(), ot.tolist()))
        else:
            assert len(oq) > 100
    sat, zero = cases[0], cases[1]
    nodes = [(sat["d1"], sat["xyz1"]), (sat["d2"], sat["xyz2"]), (zero["d1"], zero["xyz1"]), (zero["d2"], zero["xyz2"])]
    for k, (d, x) in enumerate(nodes):
        fe.upload_sift_node(k, d, x)
    kw = dict(max_matches=300, min_matches=5, ransac_iterations=200)
    fe.set_params(**kw)
    try:
        pq, pt = [0, 2, 1, 3], [1, 3, 0, 2]
        out, dist = fe.match_sift_pair_list(pq, pt)
        prm = po.default_params(seed=fe.params.seed, depth_cov=fe.params.depth_cov, **kw)
        for rec, dd, q, t in zip(out, dist, pq, pt):
            ref = po.match_sift_node_pair(nodes[q][0], nodes[q][1], q, nodes[t][0], nodes[t][1], t, prm)
            _assert_record(rec, dd, ref, "pair (%d, %d)" % (q, t))
    finally:
        fe.set_params(max_matches=300, min_matches=20, ransac_iterations=200)
        for k in range(4):
            fe.release_node(k)
