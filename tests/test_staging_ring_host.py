"""CPU: the batch pipelines' staging helper (csrc/staging_ring.h) as a stand-alone program (tests/emu/staging_ring_main.cpp)
built with the thread sanitizer: more items than buffers with a slow consumer, a slow stager, destruction with the helper
blocked or staging (the error path, before all items are consumed), one item, none.  The program checks that no item is staged
before its buffer's previous user was consumed and that every item is staged exactly once; the sanitizer reports any
unsynchronised access to a buffer; the run has to end."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["slow consumer", "slow stager", "destroyed with the helper blocked", "destroyed while staging", "one item",
             "no item, no thread", "fewer items than buffers"]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("staging_ring")
    exe = os.path.join(d, "staging_ring_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
           os.path.join(ROOT, "tests", "emu", "staging_ring_main.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=thread"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtime: the plain program still checks the ring's rule
        subprocess.run(cmd, check=True)
    return exe


def test_the_ring_keeps_its_rule_and_every_run_ends(prog):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines() == ["ok " + s for s in SCENARIOS]
    assert "ThreadSanitizer" not in r.stderr
