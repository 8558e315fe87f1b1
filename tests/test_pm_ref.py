"""CPU checks of the path-metric fixture tests/golden/pm_probes.npz (tests/golden/pm_ref.py,
make_golden_pm.py) that tests/test_pm_ulp_gpu.py holds the list decoders' softplus and exact f to.

  1. a sample of rows recomputed with the mpmath reference gives the stored values;
  2. an independent numpy.longdouble evaluation of the stable forms (sign (m + log1p(-t)),
     z + log1p(exp -z)) agrees with the stored values to 1e-17 relative plus the fp64 rounding
     of the stored value: a slip in the generator would show;
  3. the budgets are honest without the device: the C oracle (glibc, fp64) meets the tolerance
     of EVERY min-sum row.  The oracle's exact f evaluates the reference's cancelling expression
     (up to 8.8e-15 off) and is not expected to meet the exact-f tolerances: nothing is asserted
     about it;
  4. the gate has teeth: an fp64 transcription of csrc/softplus.h meets every sampled tolerance,
     and each damaged copy -- one 2^(j/64) entry off by 2^-40, one atanh coefficient changed in
     its 9th digit, the penalty's exp 8 ulp off -- puts some row outside its tolerance.
"""
import os
import sys

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import pm_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "pm_probes.npz"))


def _tiny(fx, step, f_modes=(0, 1), ns=(2, 4)):
    """(n, lmax, code, L, f_mode, logits row, pm [L], tol [L]) of every step-th stored tiny row."""
    for n in ns:
        for li, lmax in enumerate(R.TINY_LMAX):
            logits, code = fx[f"t{n}_{li}_logits"], fx[f"t{n}_{li}_code"]
            Ls = np.array([R.tiny_L(n, int(c)) for c in code])
            off = np.concatenate([[0], np.cumsum(Ls)])
            for fm in f_modes:
                pm, tol = fx[f"t{n}_{li}_f{fm}_pm"], fx[f"t{n}_{li}_f{fm}_tol"].astype(np.float64)
                assert len(pm) == off[-1] == len(tol)
                for r in range((n + li + fm) % step, len(logits), step):
                    yield n, lmax, int(code[r]), int(Ls[r]), fm, logits[r], pm[off[r]:off[r + 1]], tol[off[r]:off[r + 1]]


def test_fixture_shape_and_budgets(fx):
    assert np.array_equal(fx["tiny_lmax"], R.TINY_LMAX)
    for n in (2, 4):
        for li in range(4):
            x = fx[f"t{n}_{li}_logits"]
            assert np.isfinite(x).all() and x.dtype == np.float32
            assert set(fx[f"t{n}_{li}_code"].tolist()) == set(range(1 << n))
            for fm in (0, 1):
                pm, tol = fx[f"t{n}_{li}_f{fm}_pm"], fx[f"t{n}_{li}_f{fm}_tol"]
                assert np.isfinite(pm).all() and (pm >= 0).all()
                # a handful of operations on values up to 4 llr_max (g of g): never more than 64 ulp of those
                assert (tol >= 2.0 ** -52).all() and (tol <= 64 * np.spacing(np.maximum(pm, 4 * R.TINY_LMAX[li]))).all()
    assert os.path.getsize(os.path.join(GOLDEN, "pm_probes.npz")) < 1 << 20


def test_sampled_rows_recompute_in_mpmath(fx):
    k = 0
    for n, lmax, code, L, fm, x, pm, tol in _tiny(fx, 23):
        v, t, fragile = R.reference(x, R.tiny_mask(n, code), L, fm, lmax)
        assert not fragile and np.array_equal(v, pm) and (t <= tol).all() and (tol <= t * (1 + 2.0 ** -22)).all()
        k += 1
    assert k > 500
    for n in (8, 64):  # deep rows, without and with fast-SCL
        x = R.deep_logits(n)
        for L, fm, lmax, fset, fast in R.deep_cases()[::5]:
            key = R.deep_key(n, L, fm, lmax, fset, fast)
            r = int(fx[key + "_rows"][-1])
            v, t, fragile = R.reference(x[r], R.deep_mask(n, fset), L, fm, lmax, fast=bool(fast))
            assert not fragile and np.array_equal(v, fx[key + "_pm"][-1])


def test_longdouble_stable_forms_agree(fx):
    if np.finfo(np.longdouble).nmant < 63:
        pytest.fail("numpy.longdouble has no 64-bit mantissa here")
    worst = 0.0
    for n, lmax, code, L, fm, x, pm, tol in _tiny(fx, 7):
        v, _, _ = R.decode(R.make_root(R.LdArith(), x, fm, lmax), R.tiny_mask(n, code), L)
        v = np.array(v, dtype=np.longdouble)
        want = pm.astype(np.longdouble)
        # the stored value is the mpmath one rounded to fp64: half an ulp of it is the storage's, not a slip
        err = np.abs(v - want) - 0.5 * np.spacing(pm).astype(np.longdouble)
        worst = max(worst, float(np.max(err / want.clip(np.finfo(np.float64).tiny))))
    assert worst <= 1e-17, worst


def test_minsum_oracle_meets_every_tolerance(fx):
    """glibc's exp / log through the C oracle: the reference side alone stays inside the gate."""
    worst = 0.0
    for n in (2, 4):
        for li, lmax in enumerate(R.TINY_LMAX):
            logits, code = fx[f"t{n}_{li}_logits"], fx[f"t{n}_{li}_code"]
            pm, tol = fx[f"t{n}_{li}_f0_pm"], fx[f"t{n}_{li}_f0_tol"].astype(np.float64)
            o = 0
            for c in range(1 << n):
                rows, L = np.flatnonzero(code == c), R.tiny_L(n, c)
                _, got = oracle.scl_decode_mysn(logits[rows], np.flatnonzero(R.tiny_mask(n, c)), L, fast_scl=False,
                                                exact_f=False, llr_max=lmax)
                m = len(rows) * L
                dev = np.abs(got - np.repeat(pm[o:o + m].reshape(-1, L), 2, axis=1)) / np.repeat(tol[o:o + m].reshape(-1, L), 2, axis=1)
                assert dev.max() <= 1.0, (n, lmax, c, float(dev.max()), logits[rows][np.argmax(dev.max(axis=1))].tolist())
                worst = max(worst, float(dev.max()))
                o += m
    for n in R.DEEP_N[:4]:
        x = R.deep_logits(n)
        for L, fm, lmax, fset, fast in R.deep_cases():
            if fm == 0:
                key = R.deep_key(n, L, fm, lmax, fset, fast)
                rows = fx[key + "_rows"].astype(np.int64)
                _, got = oracle.scl_decode_mysn(x[rows], np.flatnonzero(R.deep_mask(n, fset)), L, fast_scl=bool(fast),
                                                exact_f=False, llr_max=lmax)
                dev = np.abs(got - np.repeat(fx[key + "_pm"], 2, axis=1)) / np.repeat(fx[key + "_tol"].astype(np.float64), 2, axis=1)
                assert dev.max() <= 1.0, (key, float(dev.max()))
    print("worst min-sum oracle deviation, in tolerances:", worst)


def _worst(fx, ar, step, f_modes):
    worst = 0.0
    for n, lmax, code, L, fm, x, pm, tol in _tiny(fx, step, f_modes):
        v, _, _ = R.decode(R.make_root(ar, x, fm, lmax), R.tiny_mask(n, code), L)
        worst = max(worst, float(np.max(np.abs(np.array(v) - pm) / tol)))
    return worst


def test_fixture_accepts_the_header_and_rejects_each_mutant(fx):
    good = _worst(fx, R.DevArith(), 3, (0, 1))
    assert good <= 1.0, good
    for name, ar, fms in (("2^(37/64) off by 2^-40", R.DevArith(tab_mut=(37, 2.0 ** -40)), (1,)),
                          ("kS[1] changed in its 9th digit", R.DevArith(ks_mut=(1, 1e-9)), (1,)),
                          ("exp 8 ulp off", R.DevArith(exp_ulps=8), (0, 1))):
        bad = _worst(fx, ar, 3, fms)
        assert bad > 1.0, f"mutant '{name}' passes the fixture: worst deviation {bad:.3f} tolerances (intact: {good:.3f})"
