"""GPU: rgbdslam::GraphManager::addNode of include/rgbdfe.hpp (tests/cpp/slam_session.cpp, plain g++ against the header and
librgbdfe.so, a child process) on the main planted sequence of tests/slam_sequence.py against the binding's
GraphManager.addNode on a fresh FrontEnd of the same configuration: every step record without its times, the keyframes,
the slot table and valid_tf, text for text.  (The binding gives the oracle's bytes: tests/test_gpu_slam_step.py.)"""
import os
import struct
import subprocess

import pytest

import slam_cases as sc
import slam_sequence as sq
from rgbdslam_v2_amd import _lib
from rgbdslam_v2_amd.candidates import PoseGraph
from rgbdslam_v2_amd.frontend import FrontEnd, GraphManager, Node

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, linked and rpath'ed as examples/cpp/Makefile does."""
    out = str(tmp_path_factory.mktemp("cpp_slam") / "slam_session")
    lib = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "slam_session.cpp"), "-o", out, "-L" + lib, "-lrgbdfe",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("strategy,skip", [("first", 0), ("largest_loop", 3)])
def test_the_headers_add_node_prints_the_bindings_records(exe, tmp_path, strategy, skip):
    frames = sq.main_sequence()
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(frames)))
        for fr in frames:
            f.write(struct.pack("<iqi", len(fr["desc"]), fr["stamp"][0], fr["stamp"][1]))
            f.write(fr["desc"].tobytes() + fr["xyz1"].tobytes())
    p = sq.SPARSE
    r = subprocess.run([exe, str(path), str(_lib.POSE_RELATIVE_TO[strategy]), str(skip), str(p["clear_non_keyframes"]),
                        str(p["predecessor_candidates"]), str(p["neighbor_candidates"]), str(p["min_sampled_candidates"])],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    fe = FrontEnd(device_id=0, max_nodes=24, max_keypoints=130, max_pairs_per_batch=16)
    try:
        gm = GraphManager(fe, PoseGraph())
        gm.set_pose_relative_to(strategy)
        slam = gm.slam(optimizer_skip_step=skip, **{k: v for k, v in p.items() if k != "create_cloud_every_nth_node"})
        want = [sc.step_line(gm.addNode(Node(fe, k, fr["desc"], fr["xyz1"]), fr["stamp"]).raw) for k, fr in enumerate(frames)]
        want += ["K " + " ".join(map(str, slam.keyframes())), "T " + " ".join(map(str, slam.slots())),
                 "V " + " ".join(map(str, slam.valid_tf()))]
        assert len(slam.keyframes()) >= 3 and -1 in slam.slots()   # (conditions on the run: keyframes, a cleared node)
        slam.close()
    finally:
        fe.close()
    assert [l.rstrip() for l in r.stdout.splitlines()] == want
