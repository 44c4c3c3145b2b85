"""CPU (hipcc cross-compiles): the resources of the 16x16x128 form of the 512-query Hamming kernel, with and without train
splits, as the compiler reports them in the kernel metadata, built with the Makefile's flags.  It shares the chip with its
siblings' terms: three waves per SIMD and three blocks per CU -- at most 168 VGPRs, nothing in scratch, 48 KB of LDS.
Reads the resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbdslam_v2_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def makefile_flags():
    """FLAGS and FLAGS_hamming_mfma of csrc/Makefile (continuation lines joined, make variables substituted)."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    flags = (var["FLAGS"] + " " + var["FLAGS_hamming_mfma"]).replace("$(ARCH)", var["ARCH"])
    assert "$(" not in flags, flags
    return flags.split()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "hamming_mfma.s"
    flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc"] + flags + ["-S", "--cuda-device-only", "-o", str(out),
                   "hamming_mfma.hip"], cwd=CSRC, check=True, capture_output=True, timeout=900)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    found = {}
    for block in re.split(r"\n  - \.", meta):
        name = re.search(r"\.name:\s+\S*hamming_mfma_x16_kernelILb(\d)E", block)
        if not name:
            continue
        found[int(name.group(1))] = {
            k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
            for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return found


def test_built_with_and_without_train_splits(kernels):
    assert sorted(kernels) == [0, 1]


@pytest.mark.parametrize("split", [0, 1])
def test_three_waves_per_simd_no_scratch_48k_lds(kernels, split):
    k = kernels[split]
    print(split, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k   # no scratch
    assert k["group_segment_fixed_size"] == 49152, k                                # three stage buffers of 16 KB
    assert k["vgpr_count"] <= 168, k                                                # three waves per SIMD
