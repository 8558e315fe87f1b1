"""The correctly rounded reference of the exact-boxplus f (tests/golden/exactf_cr.py) and the probe
inputs of tests/test_exactf_ulp_gpu.py, checked on the CPU.

  * exp_cr / log_cr against mpmath at 70 digits rounded once to fp32, full range: |x| <= 87,
    subnormal and overflowing results, +-160, subnormal and huge log arguments, 0 and +inf;
  * the fragile mask on values built next to a midpoint;
  * sc_decode_cr against the C oracle (glibc) where the last ulp cannot matter;
  * the probe inputs meet their conditions, on the reference alone: (a) fragile rows <= 1e-4 of a
    case (1e-3 at n = 1024, 1 % for whole codes), (b) every exp and log table cell of the device
    forms is hit in every llr_max group, (c) a libm with every 8th exp / log result one ulp up
    changes >= 50 rows of every probe case, (d) rows that decide by the tie rule (probed LLR
    exactly 0) are present and under half of a case.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import exactf_cr as C  # noqa: E402
import exactf_probes as P  # noqa: E402

F32 = np.float32
FLT_MAX = np.finfo(F32).max


def _round_f32(v):
    """An mpmath value rounded once to fp32 (nearest-even; inf counts as 2^128), exactly."""
    import mpmath
    if v == mpmath.inf:
        return F32(np.inf)
    if v == -mpmath.inf:
        return F32(-np.inf)
    sign, man, exp, _ = v._mpf_
    q = Fraction(int(man)) * (Fraction(2) ** int(exp)) * (-1 if sign else 1)
    with np.errstate(over="ignore"):
        c = F32(min(max(float(q), -3.5e38), 3.5e38))
    cands = {c, np.nextafter(c, F32(-np.inf)), np.nextafter(c, F32(np.inf))}

    def frac(f):
        return Fraction(2) ** 128 * (1 if f > 0 else -1) if np.isinf(f) else Fraction(float(f))
    best = sorted(cands, key=lambda f: (abs(frac(f) - q), int(np.array(f, dtype=F32).view(np.uint32)) & 1))[0]
    return F32(best)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_exp_cr_equals_mpmath():
    import mpmath
    mpmath.mp.dps = 70
    g = np.random.default_rng(1)
    x = np.concatenate([
        g.uniform(-87.0, 87.0, 1500), g.standard_normal(500) * 0.01, g.uniform(-104.5, -87.0, 400),  # subnormal results
        g.uniform(88.0, 89.5, 300), g.uniform(-160.0, 160.0, 300),
        [0.0, -0.0, 87.0, -87.0, 86.0, -86.0, 160.0, -160.0, 200.0, -200.0, 88.72283, 88.72284, 88.7229,
         -103.27, -103.97, -103.98, -104.0, -105.0, 1e-45, -1e-45, 1e-30, 6e-8, -6e-8],
    ]).astype(F32)
    got, _ = C.exp_cr(x)
    want = np.array([_round_f32(mpmath.exp(mpmath.mpf(float(v)))) for v in x], dtype=F32)
    assert np.isinf(want).any() and (want == 0).any() and ((want > 0) & (want < np.finfo(F32).tiny)).any()
    assert np.array_equal(_bits(got), _bits(want)), x[_bits(got) != _bits(want)][:10]


def test_log_cr_equals_mpmath():
    import mpmath
    mpmath.mp.dps = 70
    g = np.random.default_rng(2)
    x = np.concatenate([
        g.integers(1, 0x7F800000, 2000, dtype=np.int64).astype(np.uint32).view(F32),  # every exponent, subnormals too
        g.integers(1, 0x00800000, 300, dtype=np.int64).astype(np.uint32).view(F32),  # subnormal arguments
        (1.0 + g.standard_normal(500) * 1e-3).astype(F32), g.uniform(0.5, 2.0, 500).astype(F32),
        np.array([1.0, np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), FLT_MAX, np.finfo(F32).tiny, 1e-45,
                  2.0, 0.5, 0.70710677, 0.7071068, 1.4142135, 1.4142137], dtype=F32),
    ]).astype(F32)
    got, _ = C.log_cr(x)
    want = np.array([_round_f32(mpmath.log(mpmath.mpf(float(v)))) for v in x], dtype=F32)
    assert np.array_equal(_bits(got), _bits(want)), x[_bits(got) != _bits(want)][:10]
    ends, _ = C.log_cr(np.array([np.inf, 0.0], dtype=F32))
    assert ends[0] == np.inf and ends[1] == -np.inf


def test_fragile_mask_marks_values_next_to_a_midpoint():
    LD = np.longdouble
    r = np.array([1.0, 1.5, 3.0e-40, 0.7, 1e30, 0.99999994], dtype=F32)
    up = np.nextafter(r, F32(np.inf))
    mid = (r.astype(LD) + up.astype(LD)) / 2
    gap = up.astype(LD) - r.astype(LD)
    for off, want in ((2.0 ** -29, True), (-2.0 ** -29, True), (2.0 ** -25, False), (-2.0 ** -25, False), (0.25, False)):
        v = mid + LD(off) * gap
        assert (C._near_midpoint(v, v.astype(F32), 2.0 ** -27) == want).all(), off
    # the overflow threshold: FLT_MAX + half its ulp
    v = np.array([LD(float(FLT_MAX)) + LD(2.0 ** 103) * (1 + LD(2.0 ** -30)), LD(2.0 ** 127)], dtype=LD)
    with np.errstate(over="ignore"):
        assert C._near_midpoint(v, v.astype(F32), 2.0 ** -27).tolist() == [True, False]
    # and nothing exact is fragile: exp(0), log(1)
    assert not C.exp_cr(np.zeros(3, dtype=F32))[1].any() and not C.log_cr(np.ones(3, dtype=F32))[1].any()


@pytest.mark.parametrize("lmax", [30.0, 60.0])
@pytest.mark.parametrize("n", [2, 4])
def test_sc_decode_cr_equals_the_oracle_away_from_ties(n, lmax):
    """Magnitudes 5-30 (no clipping, no overflow): every f is at least ~4 from zero and glibc's
    last ulp cannot reach a decision."""
    g = np.random.default_rng([n, int(lmax)])
    x = (g.uniform(5.0, 30.0, (4099, n)) * g.choice([-1.0, 1.0], (4099, n))).astype(F32)
    for code in range(1, 1 << n):
        fp = np.flatnonzero(P.tiny_mask(n, code))
        got, fragile = C.sc_decode_cr(x, fp, n, lmax)
        assert not fragile.any()
        assert np.array_equal(got, oracle.sc_decode(x, fp, f_mode=1, llr_max=lmax)), code


def _probe(tag, llr, fp, n, lmax, leaf, trace, fragile_max):
    """Conditions (a), (c), (d) of one probe case; returns the shares it prints."""
    rows = len(llr)
    seen = {}
    want, fragile = C.sc_decode_cr(-llr, fp, n, lmax, trace=trace, root_llr=seen)
    mut, _ = C.sc_decode_cr(-llr, fp, n, lmax, mutate=C.Mutate())
    flipped = int((mut != want).any(axis=1).sum())
    ties = int((seen[leaf] == 0).sum())
    print(f"{tag}: {rows} rows, fragile {int(fragile.sum())} ({fragile.mean():.1e}), one-ulp libm flips {flipped} "
          f"({flipped / rows:.1%}), tie rows {ties} ({ties / rows:.1%})")
    assert fragile.sum() <= fragile_max * rows, tag
    assert flipped >= 50, tag
    assert 0 < ties < rows / 2, tag


@pytest.mark.parametrize("lmax", P.TINY_LMAX)
def test_tiny_code_probes_meet_their_conditions(lmax):
    trace = C.Trace()
    for n in (2, 4):
        llr = P.tiny_llr(n, lmax)
        assert abs(len(llr) - 2 ** 16) < 2 ** 12 and len(llr) % 64
        for code in range(1, 1 << n):  # (a) for every frozen pattern
            _, fragile = P.tiny_reference(n, lmax, code)
            assert fragile.sum() <= 1e-4 * len(llr), (n, code, int(fragile.sum()))
        code = P.TINY_PROBE[n]
        _probe(f"n={n} llr_max={lmax}", llr, np.flatnonzero(P.tiny_mask(n, code)), n, lmax,
               {2: 0, 4: 1}[n], trace, 1e-4)
    print(f"llr_max={lmax}: exp cells hit >= {trace.exp_cells.min()} times, log cells >= {trace.log_cells.min()}")
    assert trace.exp_cells.min() >= 1 and trace.log_cells.min() >= 1  # (b)


def test_tiny_code_edge_rows_are_there():
    """+-0, subnormals, +-llr_max and both neighbours, +-FLT_MAX, and xc + yc = +-86 at llr_max 43."""
    for lmax in P.TINY_LMAX:
        for n in (2, 4):
            x = P.tiny_llr(n, lmax)
            lm = F32(lmax)
            for v in (lm, np.nextafter(lm, F32(0)), np.nextafter(lm, F32(np.inf)), FLT_MAX, F32(1e-45), F32(1e30)):
                assert (x == v).any() and (x == -v).any(), (lmax, n, v)
            assert (_bits(x) == 0x80000000).any() and (_bits(x) == 0).any()
    x = P.tiny_llr(2, 43.0)
    assert ((x[:, 0] == 43) & (x[:, 1] == 43)).any() and ((x[:, 0] == -43) & (x[:, 1] == -43)).any()
    x = P.tiny_llr(4, 43.0)
    assert ((x[:, 0] == 43) & (x[:, 2] == 43)).any() and ((x[:, 1] == -43) & (x[:, 3] == -43)).any()


@pytest.mark.parametrize("n,lmax", P.LONG_CASES)
def test_long_code_probes_meet_their_conditions(n, lmax):
    llr = P.long_llr(n, lmax)
    assert abs(len(llr) - 2 ** 14) < 2 ** 10 and len(llr) % 64
    _probe(f"n={n} llr_max={lmax}", llr, P.long_frozen(n), n, lmax, 1, None, 1e-3 if n == 1024 else 1e-4)


@pytest.mark.parametrize("k,n,rows,ebno", P.WHOLE_CASES)
def test_whole_code_references_are_hardly_fragile(k, n, rows, ebno):
    bits, fragile = P.whole_reference(k, n, rows, ebno)
    print(f"({k},{n}) {ebno} dB: {rows} rows, fragile {int(fragile.sum())}")
    assert bits.shape == (rows, k) and fragile.sum() <= 0.01 * rows
