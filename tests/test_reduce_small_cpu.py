"""Register / scratch budget of reduce_apply_small_kernel, from the compiler's own resource report, as
tests/test_kernel_resources.py reads it for the step's other kernels (hipcc cross-compiles gfx950 without a GPU).  The kernel
exists to launch fewer waves than reduce_apply_kernel and none with a scratch allocation: a run-time subscript into one of its
by-value arguments, or a register allocation past its budget, would bring the scratch back without failing a parity test."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbtt-embedding_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]  # as __graft_entry__.build() compiles the product


@pytest.fixture(scope="module")
def small():
    """the resource report of reduce_apply_small_kernel (device code of ttx_tt.hip only)"""
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "--cuda-device-only",
                          "-Wno-unused-function", *PRELOAD, "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
                          os.path.join(CSRC, "ttx_tt.hip")], capture_output=True, text=True, timeout=900).stderr
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    hits = [v for k, v in res.items() if "reduce_apply_small_kernel" in k]
    assert len(hits) == 1, f"{len(hits)} kernels match"
    return hits[0]


def test_no_scratch(small):
    assert small["ScratchSize"] == 0, small


def test_three_work_groups_per_cu(small):
    """512-thread work-groups, three per CU as reduce_apply_kernel's: six waves per SIMD, at most 80 of the 512 registers each"""
    assert small["VGPRs"] <= 80 and small["Occupancy"] >= 6, small
    assert small["LDS Size"] * 3 <= 160 * 1024, small
