"""-m gpu: a plain `bench.py --gpus 1 --steps K --warmup W` (no --full) times exactly K steps once and prints the head of the
line only; --dump-outputs writes the records of the last timed step, whose sums are the oracle's constants for the workload
(tests/golden/bench_expected.json) -- on the N = 1 path and on the one-rank RCCL gather path alike."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"}
FULL_ONLY = {"repeats", "roofline", "timing", "parity_check", "match_roofline", "issue_roofline", "cpu_baseline", "sift",
             "detect", "sift_extract", "front_end", "host_io", "loop_closure", "ransac_heavy"}


def _line(out):
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def _check_against_oracle(dump):
    import bench
    exp = bench.expected("orb", 0.01, 1)
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20 and len(dump["id1"]) == 4000
    got = {"edges": int((dump["id1"] >= 0).sum()), "real_iterations": int(dump["real_iterations"].sum()),
           "inliers": int(dump["n_inl"].sum())}
    assert got == exp


def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                          "--dump-outputs", str(tmp_path / "n1")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    d = _line(out)
    assert HEAD <= set(d) and not (FULL_ONLY & set(d))
    assert d["steps"] == 6 and d["warmup"] == 2 and d["value"] > 0
    assert abs(d["ms_per_step"] - 4000 / d["value"] * 1e3) <= 1e-3 * d["ms_per_step"] + 1e-4   # one region of K steps
    dump = _load(tmp_path / "n1")
    _check_against_oracle(dump)
    assert dump["all_q"].shape == (4000, 320) and np.all(dump["inlier_mask"].sum(1) == dump["n_inl"])
    # the one-rank RCCL gather path (inlier streams) dumps what rank 0 received: the same records as the N = 1 path
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, RGBDFE_BENCH_FORCE_GATHER="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RGBDFE_BENCH_BACKEND", None)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
         "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--dump-outputs", str(tmp_path / "gather")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    g = _line(out)
    assert g["gather"]["gathers_in_timed_regions"] == 3 and not (FULL_ONLY & set(g))
    gd = _load(tmp_path / "gather")
    _check_against_oracle(gd)
    for k in ("id1", "id2", "n_all", "n_inl", "rmse", "trafo", "info_scale", "real_iterations"):
        assert np.array_equal(gd[k], dump[k], equal_nan=True), k
    for i in range(0, 4000, 97):
        want = dump["all_q"][i][dump["inlier_mask"][i] > 0]
        assert np.array_equal(gd["inlier_q_row"][i, :len(want)], want)
