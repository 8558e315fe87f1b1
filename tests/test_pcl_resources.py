"""Register, scratch and LDS budgets of the parity-constrained list decoder, read from hipcc's gfx950 assembly (CPU).

DESIGN.md section 20 rests on these: every pcl_decode_kernel<LOG_N, LOG_L> instantiation (n = 2 ... 1024,
L = 1 ... 32) keeps its state in registers and LDS -- no scratch, no VGPR spills -- and a
decoder's LDS is the formula stated there, within the 160 KiB of a CU.  Only the kernel metadata fields are read.
"""
import os
import re
import subprocess
import tempfile

import pytest

from polar_amd import build as _build

HIPCC = os.path.join(_build.ROCM, "bin", "hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

LDS_PER_CU = 163840
FIELDS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def lds_bytes(log_n, log_l):
    """DESIGN.md section 20, one codeword a work-group: L n floats of stage buffers, n of channel, 2 L W packed
    words of partial sums and decisions (W = max(n / 32, 1)), the 2 L words of the fork table, and L log2 n bytes
    of stage owners rounded up to a word."""
    n, L = 1 << log_n, 1 << log_l
    w = max(n // 32, 1)
    return 4 * (L * n + n + 2 * L * w + 2 * L) + (L * log_n + 3) // 4 * 4


@pytest.fixture(scope="module")
def meta():
    src = os.path.join(_build.CSRC, "pcl_kernel.hip")
    assert "pcl_kernel.hip" in _build.SOURCES
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, f"--offload-arch={_build.ARCH}", *[f for f in _build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(out).read()
    res = {}
    for block in asm.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*pcl_decode_kernelILi(\d+)ELi(\d+)E", block)
        key = (int(m.group(1)), int(m.group(2))) if m else None
        if key is None:
            continue
        res[key] = {f: int(re.search(r"\." + f + r":\s+(\d+)", block).group(1)) for f in FIELDS}
    return res


def test_every_instantiation_is_built(meta):
    assert sorted(meta) == [(log_n, log_l) for log_n in range(1, 11) for log_l in range(6)]


@pytest.mark.parametrize("log_n", list(range(1, 11)))
@pytest.mark.parametrize("log_l", list(range(6)))
def test_no_scratch_and_budgets(meta, log_n, log_l):
    m = meta[(log_n, log_l)]
    print((log_n, log_l), m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == lds_bytes(log_n, log_l), m
    assert m["group_segment_fixed_size"] <= LDS_PER_CU, m


def test_the_largest_case_fits_and_small_codes_fill_a_cu():
    """n = 1024 with L = 32 is the LDS maximum (about 140 KB); at n = 128 a CU's 32 wave slots, not its LDS,
    bound the codewords in flight up to L = 8, and L = 32 still keeps 8 a CU."""
    assert 140000 < lds_bytes(10, 5) <= LDS_PER_CU
    assert LDS_PER_CU // lds_bytes(7, 3) >= 32 and LDS_PER_CU // lds_bytes(7, 5) == 8
