"""The list decoders' fp64 penalty softplus_pm and exact f f_exact_pm_n (csrc/softplus.h) held to
their accuracy claims on the device, a few ulp per evaluation.

pl_scl_decode returns its path metrics as fp64; on a tiny code a metric is one or two
evaluations of those functions.  Every returned metric must lie within its tolerance of the
mpmath value of tests/golden/pm_probes.npz (reference and budgets: tests/golden/pm_ref.py, rows:
tests/golden/make_golden_pm.py; tests/test_pm_ref.py shows on the CPU that the budgets are met by
glibc and by a transcription of the header, and reject a 2^-40 table error, a 9th-digit
coefficient error and an exp 8 ulp off) -- elementwise on the sorted 2L metrics of EVERY row,
which must also be finite with a clear sign bit.

  * n = 2 and 4, generic kernel, every frozen pattern (k = 0 included), list sizes at which no
    real path is pruned, both f modes, llr_max 7.5 / 30 / 300 / 700;
  * n = 8 ... 2048, both kernels (subtree for 32 <= n <= 1024), L = 2 and 8, both f modes, llr_max
    30 and 700, all-frozen and position-1-only codes, without and with fast-SCL (rate-0 and
    repetition nodes summed in numpy's pairwise order).
Rows with NaN or Inf are not part of any contract and are not probed.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import pm_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def pa():
    import polar_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return polar_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "pm_probes.npz"))


def _check(pa, plan, logits, want, tol, what):
    """want, tol: [rows, L] -- the L survivors, each twice among the 2L sorted rows."""
    _, pm = pa.ops.scl_decode(plan, torch.from_numpy(np.ascontiguousarray(logits)).cuda(), return_pm=True)
    assert bool(torch.isfinite(pm).all()), what
    assert bool((pm.view(torch.int64) >= 0).all()), f"{what}: a metric with the sign bit set"
    pm = pm.cpu().numpy()
    want, tol = np.repeat(want, 2, axis=1), np.repeat(tol.astype(np.float64), 2, axis=1)
    assert pm.shape == want.shape, what
    dev = np.abs(pm - want) / tol
    r, c = np.unravel_index(np.argmax(dev), dev.shape)
    print(f"{what}: worst {dev[r, c]:.3f} of its tolerance ({tol[r, c]:.3g}) at row {r}, logits {logits[r][:8].tolist()}, "
          f"got {pm[r, c]!r} want {want[r, c]!r}")
    assert dev[r, c] <= 1.0, (f"{what}: row {r} metric {c} is {dev[r, c]:.2f} x its tolerance {tol[r, c]:.3g} off: got "
                              f"{pm[r].tolist()} want {want[r].tolist()} for logits {logits[r].tolist()}")
    return dev[r, c]


@pytest.mark.parametrize("f_mode", [0, 1])
@pytest.mark.parametrize("li", range(len(R.TINY_LMAX)), ids=[f"llr_max{v:g}" for v in R.TINY_LMAX])
@pytest.mark.parametrize("n", [2, 4])
def test_tiny_code_metrics_within_budget(pa, fx, n, li, f_mode):
    from polar_amd import _lib
    lmax = R.TINY_LMAX[li]
    logits, code = fx[f"t{n}_{li}_logits"], fx[f"t{n}_{li}_code"]
    pm, tol = fx[f"t{n}_{li}_f{f_mode}_pm"], fx[f"t{n}_{li}_f{f_mode}_tol"]
    o = 0
    assert len(logits) >= (1000 if n == 2 else 400) and set(code.tolist()) == set(range(1 << n))
    for c in range(1 << n):  # every frozen pattern, k = 0 included
        rows = np.flatnonzero(code == c)
        L = R.tiny_L(n, c)
        plan = _lib.Plan(n, R.tiny_mask(n, c), L, f_mode, lmax, flags=_lib.PL_PLAN_GENERIC)
        assert plan.kernel()[0] == "generic", plan.kernel()
        m = len(rows) * L
        _check(pa, plan, logits[rows], pm[o:o + m].reshape(-1, L), tol[o:o + m].reshape(-1, L),
               f"n={n} llr_max={lmax} f_mode={f_mode} information pattern {c:0{n}b} L={L}")
        o += m
    assert o == len(pm)


# the subtree kernel takes 32 <= n <= 1024; the generic one every n
DEEP = [(n, kernel) for n in R.DEEP_N for kernel in ("subtree", "generic") if kernel == "generic" or 32 <= n <= 1024]


@pytest.mark.parametrize("fast", [0, 1], ids=["plain", "fast_scl"])
@pytest.mark.parametrize("f_mode", [0, 1])
@pytest.mark.parametrize("n,kernel", DEEP)
def test_deep_tree_metrics_within_budget(pa, fx, n, kernel, f_mode, fast):
    """Rows of a case that the generator left out (a selection too close to call, see
    make_golden_pm.py) are listed per case in the fixture; every row it kept is checked."""
    from polar_amd import _lib
    logits = R.deep_logits(n)
    checked = 0
    for L in R.DEEP_L:
        for lmax in R.DEEP_LMAX:
            for fset in (0, 1):
                flags = (_lib.PL_PLAN_FAST_SCL if fast else 0) | (_lib.PL_PLAN_GENERIC if kernel == "generic" else 0)
                plan = _lib.Plan(n, R.deep_mask(n, fset), L, f_mode, lmax, flags=flags)
                assert plan.kernel()[0] == ("scl_subtree" if kernel == "subtree" else "generic"), plan.kernel()
                key = R.deep_key(n, L, f_mode, lmax, fset, fast)
                rows = fx[key + "_rows"].astype(np.int64)
                if len(rows):
                    _check(pa, plan, logits[rows], fx[key + "_pm"], fx[key + "_tol"], f"{key} {kernel}")
                checked += len(rows)
    assert checked >= 4 * len(logits)
