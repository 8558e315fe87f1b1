"""The exact-boxplus SC kernels held to csrc/exactf.h's contract on the device: fp32 with the
reference's roundings and CORRECTLY ROUNDED exp / log, to the last ulp.

pl_sc_decode on very small codes is a direct probe of one or two f evaluations, on inputs built so
that the decided bit follows the last ulp of each (tests/golden/exactf_probes.py; that they do,
is checked on the CPU by tests/test_exactf_ulp.py: a libm with every 8th result one ulp off
changes 4.7-41 % of the rows of each case).  The decided bits must equal the plain-numpy correctly
rounded restatement (tests/golden/exactf_cr.py) on EVERY row but the fragile ones -- rows with an
exp / log argument within 2^-27 fp32-ulp of a rounding midpoint, where the device's fp64
evaluation may round the other way (none at all in the inputs as generated).

  * n = 2 and 4, every frozen pattern with k >= 1, llr_max 7.5 / 30 / 43 (the fast forms, 43 the
    last) and 60 / 80 (the full-range forms): ~2^16 rows at mixed scales plus edge rows (+-0,
    subnormals, +-llr_max and neighbours, far beyond the clip, +-FLT_MAX, xc + yc = +-86);
  * n = 8 ... 1024 with position 1 the only information bit: the in-lane f loops (f_exact2), the
    cross-lane stages and the n = 1024 channel half, llr_max 30 and 60;
  * the (128, 256) and (512, 1024) reference codes on AWGN logits at 1-3 dB.
Both SC kernels, the specialised ones pre-built (polar_amd.build.reference_codes()).  The list
decoders' f and penalty (csrc/softplus.h), which make no correct-rounding claim, are pinned to a few
ulp by tests/test_pm_ulp_gpu.py; NaN / Inf inputs remain unpinned everywhere.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import exactf_probes as P  # noqa: E402

KINDS = ("specialized", "generic")


@pytest.fixture(scope="module")
def pa():
    import polar_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return polar_amd


def _plan(mask, lmax, kind):
    from polar_amd import _lib
    # specialised: only pre-built code objects, never a compile on the GPU box
    flags = _lib.PL_PLAN_GENERIC if kind == "generic" else _lib.PL_PLAN_CACHE_ONLY
    plan = _lib.Plan(len(mask), np.ascontiguousarray(mask, dtype=np.uint8), 1, _lib.PL_F_EXACT, lmax, flags=flags)
    assert plan.kernel()[0] == kind, plan.kernel()
    return plan


def _mismatch(pa, plan, logits, want, fragile):
    """Rows (indices) whose decided bits differ from the reference, fragile rows left out."""
    got = pa.ops.sc_decode(plan, logits).cpu().numpy()
    assert got.shape == want.shape
    return np.flatnonzero((got != want).any(axis=1) & ~fragile)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lmax", P.TINY_LMAX)
@pytest.mark.parametrize("n", [2, 4])
def test_tiny_codes_decide_as_correctly_rounded_f(pa, n, lmax, kind):
    llr = P.tiny_llr(n, lmax)
    logits = torch.from_numpy(-llr).cuda()
    for code in range(1, 1 << n):  # every frozen pattern with k >= 1
        want, fragile = P.tiny_reference(n, lmax, code)
        bad = _mismatch(pa, _plan(P.tiny_mask(n, code), lmax, kind), logits, want, fragile)
        assert bad.size == 0, (f"information pattern {code:0{n}b}: {bad.size} of {len(llr)} rows differ from the "
                               f"correctly rounded reference; first LLR rows {llr[bad[:4]].tolist()}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,lmax", P.LONG_CASES)
def test_position_one_sums_two_f_trees_correctly_rounded(pa, n, lmax, kind):
    llr = P.long_llr(n, lmax)
    mask = np.ones(n, dtype=np.uint8)
    mask[1] = 0
    want, fragile = P.long_reference(n, lmax)
    bad = _mismatch(pa, _plan(mask, lmax, kind), torch.from_numpy(-llr).cuda(), want, fragile)
    assert bad.size == 0, f"{bad.size} of {len(llr)} rows differ from the correctly rounded reference; first {bad[:8].tolist()}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,n,rows,ebno", P.WHOLE_CASES)
def test_whole_codes_decode_as_correctly_rounded_f(pa, k, n, rows, ebno, kind):
    logits = P.whole_logits(k, n, rows, ebno)
    want, fragile = P.whole_reference(k, n, rows, ebno)
    bad = _mismatch(pa, _plan(pa.frozen_mask(P.whole_frozen(k, n), n), P.WHOLE_LMAX, kind),
                    torch.from_numpy(np.array(logits)).cuda(), want, fragile)
    assert bad.size == 0, f"{bad.size} of {rows} rows differ from the correctly rounded reference; first {bad[:8].tolist()}"
