"""CPU: the decision machine of csrc/slam_machine.h as a stand-alone program (tests/emu/slam_machine_main.cpp with
csrc/candidates.cpp) built with the address and undefined-behaviour sanitizers, over the scripts of tests/slam_cases.py: what
it prints -- every step record without its times, the keyframes, slots, flags, edges and estimates -- against the scripts'
hand-written records and, text for text, against the library's rgbdfe_slam_begin / rgbdfe_slam_feed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import slam_cases as sc
from rgbdslam_v2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("slam_machine")
    exe = os.path.join(d, "slam_machine_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(ROOT, "rgbdslam_v2_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "slam_machine_main.cpp"),
           os.path.join(ROOT, "rgbdslam_v2_amd", "csrc", "candidates.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the answers
        print("slam_machine_main: the sanitizer build failed, running the PLAIN build:\n" + san.stderr.decode()[-1500:])
        subprocess.run(cmd, check=True)
    else:
        print("slam_machine_main: built with -fsanitize=address,undefined")
    return exe


def test_the_program_under_test_is_the_sanitizer_build(prog):
    """Where the compiler has the sanitizer runtimes (g++ links a trivial program with them), the stand-alone program must be
    the sanitizer build: the coverage may not vanish behind the fallback."""
    probe = subprocess.run(["g++", "-x", "c++", "-", "-fsanitize=address,undefined", "-o", os.devnull], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("this compiler cannot link the sanitizer runtimes")
    syms = subprocess.run(["nm", "-D", prog], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms


class TextStep:
    """A printed step record read back into the fields check_case looks at."""
    def __init__(self, line):
        head, motion, broadcast = line.split(" | ")
        v = [int(x) for x in head.split()]
        self.status, self.id, self.found, self.initial_id, self.initial_verdict, self.n_candidates = v[:6]
        n = self.n_candidates
        self.candidates, self.verdicts = v[6:6 + n], v[6 + n:6 + 2 * n]
        (self.best_id1, self.best_id2, self.best_n_inl, self.predecessor_matched, self.edge_to_keyframe, self.keyframe_added,
         self.cleared_first, self.cleared_last, self.released_slot, self.constant_position, self.cloud_released,
         self.has_broadcast_pose, self.optimize_due, self.sequential_edges, self.loop_closure_edges) = v[6 + 2 * n:]
        as_doubles = lambda s: [C.c_double.from_buffer_copy(bytes.fromhex(h)[::-1]).value for h in s.split()]
        self.motion_estimate, self.broadcast_pose = as_doubles(motion), as_doubles(broadcast)


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_the_program_prints_the_scripts_records(prog, frontend_lib, tmp_path, case):
    script = tmp_path / "script.txt"
    script.write_text(sc.script_text(case))
    r = subprocess.run([prog, str(script)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l.rstrip() for l in r.stdout.splitlines()]
    n = len(case["frames"])
    steps = [TextStep(l) for l in lines[:n]]
    state = {l[0]: l[1:].split() for l in lines[n:] if l[0] in "KTVXE"}
    final = dict(keyframes=[int(v) for v in state["K"]], slots=[int(v) for v in state["T"]], valid_tf=[int(v) for v in state["V"]],
                 fixed=[int(v) for v in state["X"]],
                 edges=[tuple(int(i) for i in e.split(":")[0].split("-")) for e in state["E"]],
                 info00=[C.c_double.from_buffer_copy(bytes.fromhex(e.split(":")[1])[::-1]).value for e in state["E"]])
    sc.check_case(case, steps, final)
    # ... and the library says the same, text for text
    lib_steps, lib_final = sc.run_case(frontend_lib, case)
    assert lines == [sc.step_line(st) for st in lib_steps] + [l.rstrip() for l in sc.final_lines(lib_final)]
