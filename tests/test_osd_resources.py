"""Register, scratch and LDS budgets of the ordered-statistics kernel, read from hipcc's gfx950 assembly (CPU).

DESIGN.md section 12 rests on these: every osd_kernel<NW, RPL> instantiation (NW words per basis row,
RPL rows per lane) keeps a codeword's state in registers and LDS -- no scratch, no VGPR spills -- and its
LDS, one 64-thread block per codeword, leaves room for at least 8 blocks per CU (two waves per SIMD) at
the largest instantiation (n <= 256), 16 at NW = 4 (n <= 128) and 31 or more at NW <= 2 (n <= 64).
"""
import os
import re
import subprocess
import tempfile

import pytest

from polar_amd import build as _build

HIPCC = os.path.join(_build.ROCM, "bin", "hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

LDS_PER_CU = 160 * 1024  # gfx950


def lds_bytes(nw, rpl):
    """The kernel's static LDS layout: |llr| bits, llr, sorted llr / a (4 B x 32 NW each), the order and
    the pivots (2 B), the sorted columns (16 B x 32 NW), the basis rows (4 NW B x 64 RPL), the nibble
    tables (8 B x 16 x 8 NW)."""
    np_, kp = 32 * nw, 64 * rpl
    return 3 * 4 * np_ + 2 * np_ + 16 * np_ + 4 * nw * kp + 2 * kp + 8 * 16 * 8 * nw


@pytest.fixture(scope="module")
def meta():
    src = os.path.join(_build.CSRC, "osd_kernel.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, f"--offload-arch={_build.ARCH}", *[f for f in _build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    res = {}
    for block in asm.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*osd_kernelILi(\d+)ELi(\d+)E", block)
        if not m:
            continue
        fields = {}
        for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            fields[key] = int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        res[(int(m.group(1)), int(m.group(2)))] = fields
    assert "scratch_" not in asm
    return res


def test_every_instantiation_is_built(meta):
    assert sorted(meta) == [(nw, rpl) for nw in (1, 2, 4, 8) for rpl in (1, 2)]


@pytest.mark.parametrize("nw", [1, 2, 4, 8])
@pytest.mark.parametrize("rpl", [1, 2])
def test_no_scratch_and_lds_fits_the_claimed_occupancy(meta, nw, rpl):
    m = meta[(nw, rpl)]
    print((nw, rpl), m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= 64, m  # 8 waves per SIMD by registers: LDS and block slots decide
    assert m["group_segment_fixed_size"] == lds_bytes(nw, rpl), m
    blocks = LDS_PER_CU // m["group_segment_fixed_size"]
    assert blocks >= {8: 8, 4: 16, 2: 31, 1: 32}[nw], (blocks, m)
