"""-m gpu: small match+RANSAC batches beside context churn -- the setting in which round 4's streaming refinement kernel fell back
about twice per 10^4 launches (tools/stress_small_batches.py: 41 give-ups in 2*10^5).  The refinement kernel has
no waits to bound any more; this is the short form of that harness for the test suite: a few thousand launches of 5 .. 60
pairs from two threads while three side threads create and destroy contexts, upload and release nodes and allocate / free
device memory.  Every record byte for byte, no call that fails to return (the harness aborts after 20 s without progress),
and the library exports no give-up counter."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_small_batches_beside_context_churn():
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stress_small_batches.py"), "6000", "2", "single", "20", "3"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and line, (out.stdout[-1500:], out.stderr[-1500:])
    r = json.loads(line[-1])
    assert r["stress_small_batches"] == "ok" and r["launches"] == 6000 and r["wrong"] == 0
    assert r["churn_rounds"] > 20 and r["churn_errors"] == []
    assert r["bounded_wait_give_ups"] is None      # (round 4's counter: the symbol is gone with the waits)
