"""Register, scratch and LDS budgets of the genie-aided SC kernel, read from hipcc's gfx950 assembly (CPU).

DESIGN.md section 13 rests on these: every genie_kernel<LOG_N, FM> instantiation (n = 2 ... 2048, min-sum
and exact f) keeps its codewords, partial sums and error counts in registers -- no scratch, no VGPR
spills -- within the 256 VGPRs of the two waves per SIMD it declares, and its LDS is the n counters (plus
the exact f's 6 KiB tables).  Only the kernel metadata fields are read.
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
VGPR_BUDGET = 512 // 2  # two waves per SIMD (the kernel's __launch_bounds__)


def lds_bytes(log_n, fm):
    """The kernel's static LDS: one uint32 counter per position, and the exact f's tables."""
    return 4 * (1 << log_n) + (EXACT_TABLES if fm else 0)


@pytest.fixture(scope="module")
def meta():
    src = os.path.join(_build.CSRC, "genie_kernel.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, f"--offload-arch={_build.ARCH}", *[f for f in _build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    res = {}
    for block in asm.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*genie_kernelILi(\d+)ELi(\d+)E", block)
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
    assert m["vgpr_count"] <= VGPR_BUDGET, m
    assert m["group_segment_fixed_size"] == lds_bytes(log_n, fm), m
