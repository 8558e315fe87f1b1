"""Register, scratch and LDS budgets of the automorphism-ensemble kernel, read from hipcc's gfx950 assembly (CPU).

DESIGN.md section 17 rests on these: every ae_kernel<LOG_N, FM> instantiation (n = 2 ... 1024, min-sum and
exact f) is built; the min-sum ones use no scratch and spill no VGPR; the exact-f ones stay within the budget
stated there (none either, and at most 512 registers, arch and accumulation VGPRs together, which is one wave
per SIMD); and the LDS of a work-group is the formula stated there, far inside the 160 KiB of a CU.
Only the kernel metadata fields are read.
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
MINSUM_VGPR_BUDGET = 512  # the file's __launch_bounds__(64) allows one wave per SIMD the whole register file
EXACT_VGPR_BUDGET = 512


def lds_bytes(log_n, fm):
    """a work-group is one wave and one row at a time.  n floats of LLRs, n bytes of the
    best candidate's codeword (at least 4), and the exact f's tables."""
    n = 1 << log_n
    return 4 * n + max(n, 4) + (EXACT_TABLES if fm else 0)


@pytest.fixture(scope="module")
def meta():
    src = os.path.join(_build.CSRC, "ae_kernel.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, f"--offload-arch={_build.ARCH}", *[f for f in _build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    res = {}
    for block in asm.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*ae_kernelILi(\d+)ELi(\d+)E", block)
        if not m:
            continue
        fields = {"agpr_count": int(re.match(r":\s+(\d+)", block).group(1))}
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
    assert m["vgpr_count"] <= (EXACT_VGPR_BUDGET if fm else MINSUM_VGPR_BUDGET), m
    assert m["group_segment_fixed_size"] == lds_bytes(log_n, fm), m
    assert m["group_segment_fixed_size"] <= LDS_PER_CU, m
