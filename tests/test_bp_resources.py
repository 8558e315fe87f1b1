"""Register, scratch and LDS budgets of the belief-propagation kernel, read from hipcc's gfx950 assembly (CPU).

DESIGN.md section 14 rests on these: every bp_kernel<LOG_N, FM> instantiation (n = 2 ... 1024, min-sum and
exact f) keeps the messages of its codewords in LDS -- no scratch, no VGPR spills -- and its LDS is the
formula stated there, within the 160 KiB of a CU.  Only the kernel metadata fields are read.
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
    """a work-group of max(256, n/2) threads holds C = threads / (n/2) codewords, each
    (2 S + 1) n floats of messages (one float of padding for n <= 32) and 2 W + 1 words for the early stop
    (W = n / 32 packed words for n >= 128, else 1), one more word for the group, and the exact f's tables."""
    n = 1 << log_n
    c = max(256, n // 2) // (n // 2)
    w = n // 32 if n >= 128 else 1
    per_cw = (2 * log_n + 1) * n + (1 if n <= 32 else 0) + 2 * w + 1
    return 4 * (c * per_cw + 1) + (EXACT_TABLES if fm else 0)


@pytest.fixture(scope="module")
def meta():
    src = os.path.join(_build.CSRC, "bp_kernel.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, f"--offload-arch={_build.ARCH}", *[f for f in _build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    res = {}
    for block in asm.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*bp_kernelILi(\d+)ELi(\d+)E", block)
        if not m:
            continue
        fields = {}
        for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            fields[key] = int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        res[(int(m.group(1)), int(m.group(2)))] = fields
    return res


def test_every_instantiation_is_built(meta):
    assert sorted(meta) == [(log_n, fm) for log_n in range(1, 11) for fm in (0, 1)]


@pytest.mark.parametrize("log_n", list(range(1, 11)))
@pytest.mark.parametrize("fm", [0, 1])
def test_no_scratch_and_budgets(meta, log_n, fm):
    m = meta[(log_n, fm)]
    print((log_n, fm), m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == lds_bytes(log_n, fm), m
    assert m["group_segment_fixed_size"] <= LDS_PER_CU, m
