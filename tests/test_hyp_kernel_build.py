"""CPU (hipcc cross-compiles): the resources of the two kernels of ransac_split.hip as the compiler reports them in the kernel
metadata, built with the Makefile's flags.  The hypothesis kernel shares a CU with the next batch's Hamming blocks and runs
seven waves per SIMD: at most 72 VGPRs, nothing in scratch, and the LDS of its two record copies (16 644 B) plus at most a
few words.  The refinement kernel keeps its 128 VGPRs without scratch.  Reads the resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbdslam_v2_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def makefile_flags():
    """FLAGS and FLAGS_ransac_split of csrc/Makefile (continuation lines joined, make variables substituted)."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    flags = (var["FLAGS"] + " " + var["FLAGS_ransac_split"]).replace("$(ARCH)", var["ARCH"])
    assert "$(" not in flags, flags
    return flags.split()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "ransac_split.s"
    flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc"] + flags + ["-S", "--cuda-device-only", "-o", str(out),
                   "ransac_split.hip"], cwd=CSRC, check=True, capture_output=True, timeout=900)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    found = {}
    for block in re.split(r"\n  - \.", meta):
        name = re.search(r"\.name:\s+_ZN6rgbdfe\d+(ransac_\w+?_kernel)E", block)
        if not name:
            continue
        found[name.group(1)] = {
            k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
            for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return found


def test_both_kernels_found(kernels):
    assert sorted(kernels) == ["ransac_hyp_kernel", "ransac_refine_kernel"]


def test_hypothesis_kernel_seven_waves_per_simd_no_scratch_same_lds(kernels):
    k = kernels["ransac_hyp_kernel"]
    print(k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k   # no scratch
    assert k["vgpr_count"] <= 72, k                                                 # 512 / 72: seven waves per SIMD
    assert k["group_segment_fixed_size"] <= 16644 + 64, k                           # the records, their transposed copy, a counter


def test_refinement_kernel_unchanged(kernels):
    k = kernels["ransac_refine_kernel"]
    print(k)
    assert k["vgpr_count"] == 128, k
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
