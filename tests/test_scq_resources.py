"""Register and scratch budgets of the fixed-point SC kernel, read from hipcc's gfx950 assembly (CPU).

DESIGN.md section 16 rests on these: every scq_decode_kernel<LOG_N, OUTK> instantiation (n = 2 ... 2048, both
output kinds) is built, none uses scratch or spills a VGPR, n <= 1024 fits 256 registers (arch and accumulation
VGPRs together: two waves per SIMD, as the generic float kernel), and n = 2048 fits the 512 of one wave.
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

REGISTER_FILE = 512  # registers a SIMD lane holds for its waves


def register_budget(log_n):
    """two waves per SIMD up to n = 1024, one at n = 2048."""
    return REGISTER_FILE // (2 if log_n <= 10 else 1)


@pytest.fixture(scope="module")
def meta():
    src = os.path.join(_build.CSRC, "scq_kernel.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, f"--offload-arch={_build.ARCH}", *[f for f in _build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    res = {}
    for block in asm.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*(scq_decode_kernelILi(\d+)ELi(\d+)E|llr_quantize_kernel)", block)
        if not m:
            continue
        fields = {"agpr_count": int(re.match(r":\s+(\d+)", block).group(1))}
        for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            fields[key] = int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        res[(int(m.group(2)), int(m.group(3))) if m.group(2) else "quantize"] = fields
    return res


def test_every_instantiation_is_built(meta):
    assert sorted(k for k in meta if k != "quantize") == [(log_n, kind) for log_n in range(1, 12) for kind in (0, 1)]
    assert "quantize" in meta


@pytest.mark.parametrize("log_n", list(range(1, 12)))
@pytest.mark.parametrize("kind", [0, 1])
def test_no_scratch_and_occupancy(meta, log_n, kind):
    m = meta[(log_n, kind)]
    print((log_n, kind), m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    # vgpr_count is the unified allocation (the accumulation registers follow the arch ones)
    assert max(m["vgpr_count"], m["agpr_count"]) <= register_budget(log_n), m
    n = 1 << log_n
    words = (n // max(1, n // 128) + 31) // 32
    assert m["group_segment_fixed_size"] == 4 * 4 * 64 * words, m  # the u words of 4 waves


def test_quantiser_is_small(meta):
    m = meta["quantize"]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["vgpr_count"] <= 32, m
