"""Register, scratch and LDS budgets of the soft-cancellation kernel, read from hipcc's gfx950 assembly (CPU).

DESIGN.md section 18 rests on these: every scan_kernel<LOG_N, FM> instantiation (n = 2 ... 2048, min-sum and
exact f) keeps its messages in registers and LDS -- no scratch, no VGPR spills -- and its LDS is the formula
stated there, within the 160 KiB of a CU.  Only the kernel metadata fields are read.
"""
import os
import re
import subprocess
import tempfile

import pytest

from polar_amd import build as _build

HIPCC = os.path.join(_build.ROCM, "bin", "hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

EXACT_TABLES = 8 * (256 + 512)  # csrc/exactf.h Tabs (lean): e[256], cl[512] fp64
LDS_PER_CU = 163840


def lds_bytes(log_n, fm):
    """DESIGN.md section 18.  n <= 64: the codeword is one register block, no message is in LDS.  n >= 128, one
    codeword a work-group, in floats: the L path 2 n - 64 (L[S], then the current node of stages S-1 ... 6), R[s][n]
    for s = 6 ... S, 5 n / 2 for the R of the right children inside the 64-position blocks, n for L[0] -- in all
    (S + 1/2) n - 64 -- and 2 n / 32 words of packed decisions for the early stop; plus the exact f's tables."""
    n = 1 << log_n
    floats = 0 if n <= 64 else (2 * n - 64) + (log_n - 5) * n + 5 * n // 2 + n
    assert n <= 64 or 2 * floats == (2 * log_n + 1) * n - 128
    words = 0 if n <= 64 else 2 * (n // 32)
    return 4 * (floats + words) + (EXACT_TABLES if fm else 0)


@pytest.fixture(scope="module")
def meta():
    src = os.path.join(_build.CSRC, "scan_kernel.hip")
    assert "scan_kernel.hip" in _build.SOURCES
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, f"--offload-arch={_build.ARCH}", *[f for f in _build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    res = {}
    for block in asm.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*scan_kernelILi(\d+)ELi(\d+)E", block)
        if not m:
            continue
        fields = {}
        for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            fields[key] = int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        res[(int(m.group(1)), int(m.group(2)))] = fields
    return res


def test_every_instantiation_is_built(meta):
    assert sorted(meta) == [(log_n, fm) for log_n in range(1, 12) for fm in (0, 1)]


@pytest.mark.parametrize("log_n", list(range(1, 12)))
@pytest.mark.parametrize("fm", [0, 1])
def test_no_scratch_and_budgets(meta, log_n, fm):
    m = meta[(log_n, fm)]
    print((log_n, fm), m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == lds_bytes(log_n, fm), m
    assert m["group_segment_fixed_size"] <= LDS_PER_CU, m


def test_n2048_is_smaller_than_bp_at_1024():
    """What the schedule buys: a codeword of n = 2048 needs about as much LDS as the BP kernel's (2 S + 1) n fp32
    at n = 1024, and n = 1024 leaves room for three work-groups a CU."""
    assert lds_bytes(11, 1) <= 100 * 1024 and 3 * lds_bytes(10, 1) <= LDS_PER_CU
