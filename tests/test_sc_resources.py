"""Register and scratch budgets of the generic SC kernel, read from hipcc's gfx950 assembly (CPU).

sc_decode_kernel<LOG_N, FM, OUTK> (csrc/sc_kernel.hip) has the tightest register state of the register-tree
kernels: two waves per SIMD (256 registers) at every n, which min-sum holds without scratch up to n = 1024 and
the exact f only up to n = 64.  Every instantiation (n = 2 ... 2048, both f modes, both output kinds) is built;
its LDS is the u words of 4 waves, plus the exact f's 6144 bytes of tables; and its VGPR spills and private
bytes stay within what the kernel had when this table was taken (_SC_BUDGET, as _SCL_EXACT_BUDGET in
tests/test_kernel_resources.py): a change of the tree walk that costs the kernel registers shows up here.
Only the kernel metadata fields are read (tests/test_kernel_resources.py compiles and parses).
"""
import os
import re
import tempfile

import pytest
from test_kernel_resources import _compile_asm, _kernel_meta

from polar_amd import build as _build

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(_build.ROCM, "bin", "hipcc")),
                                reason="hipcc not available")

REGISTER_BUDGET = 256  # two waves per SIMD (__launch_bounds__(256, 2))
EXACTF_TABLE_BYTES = 6144

# (log_n, f mode, output kind) -> (spilled VGPRs, private bytes); every instantiation not listed has neither
_SC_BUDGET = {
    (7, 1, 0): (43, 176), (7, 1, 1): (43, 176),
    (8, 1, 0): (44, 192), (8, 1, 1): (44, 192),
    (9, 1, 0): (51, 208), (9, 1, 1): (53, 208),
    (10, 1, 0): (59, 240), (10, 1, 1): (57, 240),
    (11, 0, 0): (118, 468), (11, 0, 1): (116, 468),
    (11, 1, 0): (201, 816), (11, 1, 1): (201, 816),
}
_ALL = [(log_n, fm, kind) for log_n in range(1, 12) for fm in (0, 1) for kind in (0, 1)]
_NAME = re.compile(r"sc_decode_kernelILi(\d+)ELi(\d+)ELi(\d+)E")


@pytest.fixture(scope="module")
def meta():
    with tempfile.TemporaryDirectory() as td:
        asm = _compile_asm(os.path.join(_build.CSRC, "sc_kernel.hip"), [], td)
    found = _kernel_meta(asm, lambda name: _NAME.search(name) is not None)
    return {tuple(int(g) for g in _NAME.search(name).groups()): fields for name, fields in found.items()}


def test_every_instantiation_is_built(meta):
    assert sorted(meta) == _ALL


@pytest.mark.parametrize("log_n,fm,kind", _ALL)
def test_registers_scratch_and_lds(meta, log_n, fm, kind):
    m = meta[(log_n, fm, kind)]
    print((log_n, fm, kind), m)
    spills, private = _SC_BUDGET.get((log_n, fm, kind), (0, 0))
    assert m["vgpr_spill_count"] <= spills and m["private_segment_fixed_size"] <= private, m
    assert m["vgpr_count"] <= REGISTER_BUDGET, m  # the unified allocation: accumulation registers included
    n = 1 << log_n
    words = (n // max(1, n // 128) + 31) // 32
    assert m["group_segment_fixed_size"] == 4 * 4 * 64 * words + (EXACTF_TABLE_BYTES if fm else 0), m
