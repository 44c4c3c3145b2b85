"""-m gpu: the hypothesis kernel's split pre-screen.  The pair's last wave with iterations, when at most half
full, spreads each hypothesis' pre-screen over 8, 4 or 2 lanes; the count must be the integer the one-lane forms give, so
that the viable masks, the recorded iterations and the order buckets stay bit for bit.

Count equality: tests/cpp/prescreen_split.hip, built here with the Makefile's flags, evaluates prescreen_may_pass,
prescreen_may_pass_s4 and prescreen_may_pass_s4_split on the same hypotheses (identity, random, and ones with records
planted within one ulp of the threshold on either side) and records (n_all from 4 to 300, one NaN and one zero-depth record),
for every number of active lanes and group count of the list below.

End to end: batches of 3, 20 and 300 pairs at iteration counts that leave the partial wave 1, 7, 8, 9, 40 and 44 lanes, none
(64), or make it the first wave as well, against the CPU oracle and against the one-wave schedule."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from rgbdslam_v2_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbdslam_v2_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

N_ALL = [4, 5, 21, 63, 64, 65, 299, 300]
LANES = [1, 7, 8, 9, 16, 17, 32]
GROUPS = [8, 4, 2]


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    flags = (var["FLAGS"] + " " + var["FLAGS_ransac_split"]).replace("$(ARCH)", var["ARCH"])
    assert "$(" not in flags, flags
    return flags.split()


@pytest.fixture(scope="module")
def count_cases(tmp_path_factory):
    """The program's `case` lines, keyed by (n_all, active lanes, groups)."""
    exe = str(tmp_path_factory.mktemp("prescreen_split") / "prescreen_split")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc"] + makefile_flags() + ["-I.", "-o", exe,
                   os.path.join(ROOT, "tests", "cpp", "prescreen_split.hip")], cwd=CSRC, check=True, capture_output=True, timeout=600)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stderr + p.stdout[-2000:]
    cases = {}
    for line in p.stdout.splitlines():
        if line.startswith("case "):
            f = {k: int(v) for k, v in (kv.split("=") for kv in line.split()[1:])}
            cases[(f["n_all"], f["a"], f["G"])] = f
    return cases


def test_split_count_equals_one_lane_count(count_cases):
    want = {(n, a, g) for n in N_ALL for g in GROUPS for a in LANES if a <= 64 // g}   # G lanes per hypothesis
    assert set(count_cases) == want
    for key, f in sorted(count_cases.items()):
        assert f["mismatches"] == 0, (key, f)
        assert f["hypotheses"] == 48, (key, f)
        assert f["host_differs"] == 0, (key, f)          # the planted records sit at the device's threshold
        assert f["count_min"] >= 1, (key, f)             # the NaN record counts under every hypothesis
        assert f["planted"] >= (1 if key[0] >= 5 else 0), (key, f)
        assert key[0] < 21 or f["count_max"] > f["count_min"], (key, f)   # the hypotheses differ in what they let pass
    assert count_cases[(300, 8, 8)]["planted"] == 16


# ---- end to end
ITERATIONS = [1, 7, 8, 9, 63, 64, 65, 72, 200, 264, 300]
MAX_MATCHES = [5, 21, 64, 300]
# with the default 20 the 21 or 64 best matches of this scene give no hypothesis that survives its scoring, and the count
# would decide nothing; with 4 those batches hold accepted pairs, rejected pairs and iterations of both kinds
MIN_MATCHES = {5: 4, 21: 4, 64: 4, 300: 20}
BATCHES = [3, 20, 300]
F = 20


@pytest.fixture(scope="module")
def scene():
    from rgbdslam_v2_amd.frontend import FrontEnd
    seq = synth.make_sequence(n_frames=F, n_kp=400, n_world=1500, seed=13)
    pq, pt = synth.candidate_pairs(F, per_frame=20, seed=13)
    assert len(pq) >= max(BATCHES)
    fe = FrontEnd(device_id=0, max_nodes=F, max_keypoints=512, max_pairs_per_batch=max(BATCHES))
    for f in range(F):
        fe.upload_node(f, seq["desc"][f], seq["xyz1"][f])
    yield fe, seq, pq[:max(BATCHES)], pt[:max(BATCHES)]
    fe.close()


def check_against_oracle(rec, ref):
    from rgbdslam_v2_amd.frontend import inlier_indices
    n = ref["n_all"]
    assert rec["n_all"] == n
    assert np.array_equal(rec["all_q"][:n], ref["all_q"]) and np.array_equal(rec["all_t"][:n], ref["all_t"])
    assert np.array_equal(rec["all_hd"][:n], ref["all_hd"])
    assert (rec["id1"], rec["id2"]) == (ref["id1"], ref["id2"])
    assert rec["real_iterations"] == ref["real_iterations"] and rec["valid_iterations"] == ref["valid_iterations"]
    assert rec["n_inl"] == ref["n_inl"]
    assert np.array_equal(inlier_indices(rec), ref["inl_idx"])
    T = np.array(rec["trafo"], np.float32).reshape(4, 4).T
    assert np.array_equal(T, ref["T"]), "pose bits differ from the oracle"
    assert np.float32(rec["rmse"]) == ref["rmse"] and rec["info_scale"] == ref["info_scale"]


@pytest.mark.parametrize("max_matches", MAX_MATCHES)
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_batches_equal_oracle_and_one_wave_schedule(scene, iterations, max_matches):
    fe, seq, pq, pt = scene
    kw = dict(ransac_iterations=iterations, max_matches=max_matches, min_matches=MIN_MATCHES[max_matches])
    fe.set_params(**kw)
    try:
        prm = po.default_params(seed=fe.params.seed, depth_cov=fe.params.depth_cov, **kw)
        refs = [po.result_to_dict(r) for r in po.match_pairs_mt(list(seq["desc"]), list(seq["xyz1"]), np.arange(F), pq, pt, prm)]
        assert sum(r["real_iterations"] > 0 for r in refs) > len(refs) // 2     # RANSAC really ran
        assert iterations == 1 or sum(r["valid_iterations"] for r in refs) > 0  # ... and some hypotheses passed the pre-screen
        for n in BATCHES:
            fe.set_latency_mode((1 << 31) - 1, 0)            # record / replay: the hypothesis kernel
            got = fe.match_pair_list(pq[:n], pt[:n])
            for rec, ref in zip(got, refs[:n]):
                check_against_oracle(rec, ref)
            fe.set_latency_mode(0, 0)                        # one wave per pair
            assert fe.match_pair_list(pq[:n], pt[:n]).tobytes() == got.tobytes(), (n, kw)
    finally:
        fe.set_latency_mode((1 << 31) - 1, 0)
        fe.set_params(ransac_iterations=200, max_matches=300, min_matches=20)
