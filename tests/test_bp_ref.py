"""The numpy restatement of belief-propagation decoding (tests/golden/bp_ref.py) against what can be known
without a GPU: a closed form at n = 2, noiseless rows, the sign symmetry of min-sum (which checks the
wiring against the encoder), early stop against the full run, and the fragile-row count of the exact-f
inputs tests/test_bp_gpu.py compares on.  CPU only.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import bp_ref  # noqa: E402

F32 = np.float32

from bp_ref import EXACT_CASES, EXACT_ROWS, FRAGILE_CAP, exact_case_inputs  # noqa: E402


def test_n2_closed_form():
    """n = 2, position 0 frozen, llr_max 19.3, a = -logits = (a0, a1): R[0] = (lmax, 0), so
    L[0][1] = clip(f(a0, lmax) + a1), R[1][0] = clip(f(lmax, a1 + 0)), R[1][1] = clip(f(lmax, a0) + 0);
    with min-sum f(v, lmax) = clip(v).  No message depends on an earlier iteration."""
    lm = float(F32(19.3))
    logits = np.array([[-1.5, 0.25], [2.0, -3.0], [25.0, 1.0], [-0.5, -30.0], [0.0, 0.0]], dtype=F32)
    want_soft = np.array([[-1.25], [-1.0], [lm], [-lm], [0.0]], dtype=F32)  # -clip(clip(a0) + a1)
    want_ext = np.array([[0.25, -1.5], [-3.0, 2.0], [1.0, lm], [-lm, -0.5], [0.0, 0.0]], dtype=F32)
    for it in (1, 4):
        for es in (False, True):
            r = bp_ref.bp_decode(logits, [0], 2, it, 19.3, early_stop=es)
            assert np.array_equal(r["soft_u"], want_soft), r["soft_u"]
            assert np.array_equal(r["ext_x"], want_ext), r["ext_x"]
            assert np.array_equal(r["bits"], (~(-want_soft > 0)).astype(np.uint8))
    # scaled min-sum: the magnitude of f is scaled (one rounding), the sum is not
    r = bp_ref.bp_decode(logits[:1], [0], 2, 1, 19.3, scale=0.9375)
    assert np.array_equal(r["soft_u"], np.array([[-(F32(1.5) * F32(0.9375)) + F32(0.25)]], dtype=F32))
    # both positions information: R[0] = 0, f(., 0) = 0: soft_u[0] = -f(a0, a1), soft_u[1] = -a1, ext = 0
    r = bp_ref.bp_decode(logits[:2], [], 2, 2, 19.3)
    assert np.array_equal(r["soft_u"], np.array([[0.25, 0.25], [2.0, -3.0]], dtype=F32))
    assert np.array_equal(r["ext_x"], np.zeros((2, 2), dtype=F32))


def test_n2_closed_form_exact():
    """The same unit with the exact f, against the boxplus evaluated in float64."""
    logits = np.array([[-1.5, 0.25], [2.0, -3.0]], dtype=F32)
    r = bp_ref.bp_decode(logits, [], 2, 1, 19.3, exact=True)
    a = -logits.astype(np.float64)
    box = np.log1p(np.exp(a[:, 0] + a[:, 1])) - np.log(np.exp(a[:, 0]) + np.exp(a[:, 1]))
    assert np.allclose(-r["soft_u"][:, 0], box, rtol=0, atol=1e-6)
    assert np.array_equal(r["soft_u"][:, 1], logits[:, 1])


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n", [2, 4, 16, 64, 256])
def test_noiseless_rows_decode_in_one_iteration(n, exact):
    for seed in range(3):
        rng = np.random.default_rng(10 * n + seed)
        k = int(rng.integers(1, n + 1))
        fp = bp_ref.rate_half_frozen(n, 50 + seed, k)
        u, _ = bp_ref.awgn_logits(rng, fp, n, 6)
        x = bp_ref.noiseless_logits(u)
        r = bp_ref.bp_decode(x, fp, n, 5, 19.3, exact=exact, early_stop=True)
        info = np.setdiff1d(np.arange(n), fp)
        assert np.array_equal(r["bits"], u[:, info])
        assert np.array_equal(r["iters"], np.ones(6, dtype=np.int32))
        one = bp_ref.bp_decode(x, fp, n, 1, 19.3, exact=exact)
        assert np.array_equal(one["bits"], u[:, info]) and np.array_equal(one["soft_u"], r["soft_u"])


@pytest.mark.parametrize("n", [4, 8, 32, 128])
def test_minsum_sign_symmetry(n):
    """For a codeword x = u G (frozen bits 0), decoding logits (1 - 2x) gives soft_u (1 - 2u) and
    ext_x (1 - 2x) exactly: min-sum commutes with sign flips along a codeword, whatever the wiring's
    order of operations -- but only if the wiring is the encoder's."""
    fp = bp_ref.rate_half_frozen(n, 300 + n)
    info = np.setdiff1d(np.arange(n), fp)
    rng = np.random.default_rng(n)
    _, base = bp_ref.awgn_logits(rng, fp, n, 8)
    u, _ = bp_ref.awgn_logits(rng, fp, n, 8)
    sx = (1.0 - 2.0 * bp_ref.encode(u)).astype(F32)
    su = (1.0 - 2.0 * u[:, info]).astype(F32)
    for scale in (1.0, 0.9375):
        a = bp_ref.bp_decode(base, fp, n, 3, 19.3, scale=scale)
        b = bp_ref.bp_decode(base * sx, fp, n, 3, 19.3, scale=scale)
        assert np.array_equal(b["soft_u"], a["soft_u"] * su)
        assert np.array_equal(b["ext_x"], a["ext_x"] * sx)
    assert np.abs(a["soft_u"]).max() > 0 and np.abs(a["ext_x"]).max() > 0


@pytest.mark.parametrize("exact", [False, True])
def test_early_stop_against_the_full_run(exact):
    n, num_iter = 64, 6
    fp = bp_ref.rate_half_frozen(n, 1)
    _, x = bp_ref.make_inputs(5, n, fp, 40, 19.3, ebno_db=1.0)
    full = bp_ref.bp_decode(x, fp, n, num_iter, 19.3, exact=exact)
    es = bp_ref.bp_decode(x, fp, n, num_iter, 19.3, exact=exact, early_stop=True)
    assert np.array_equal(full["iters"], np.full(40, num_iter, dtype=np.int32))
    assert es["iters"].min() >= 1 and es["iters"].max() <= num_iter
    never = es["iters"] == num_iter
    assert never.any() and (~never).any()
    # a row that stops in the last iteration has run them all as well: it is equal too
    for key in ("bits", "soft_u", "ext_x"):
        assert np.array_equal(full[key][never], es[key][never])
    # a stopped row holds the messages of the iteration it stopped in
    for i in np.flatnonzero(~never)[:4]:
        short = bp_ref.bp_decode(x[i:i + 1], fp, n, int(es["iters"][i]), 19.3, exact=exact)
        for key in ("bits", "soft_u", "ext_x"):
            assert np.array_equal(short[key][0], es[key][i])


@pytest.mark.parametrize("n", bp_ref.EARLY_STOP_SIZES + (64,))
def test_early_stop_gpu_inputs_show_every_class(n):
    """The inputs of tests/test_bp_gpu.py's early-stop cases: rows that stop after 1 iteration, after 2 ... 9 and
    never, plain and (n = 64, 256) scaled; at n = 2 only the first class exists."""
    fp = bp_ref.rate_half_frozen(n, bp_ref.EARLY_STOP_FROZEN_SEED)
    x = bp_ref.early_stop_inputs(n, fp)
    for scale in (1.0, 0.9375) if n in (64, 256) else (1.0,):
        if n == 64 and scale == 1.0:
            continue
        it = bp_ref.bp_decode(x, fp, n, bp_ref.EARLY_STOP_ITERS, 19.3, scale=scale, early_stop=True)["iters"]
        print(f"n={n} scale={scale}: iters histogram {np.bincount(it, minlength=11).tolist()}")
        assert (it == 1).any()
        assert n == 2 or (((it > 1) & (it < 10)).any() and (it == 10).any())


def test_past_grid_early_stop_inputs():
    fp, x = bp_ref.past_grid_early_stop_inputs()
    assert x.shape == (64 * 1024 * 2 + 5, 8)
    it = bp_ref.bp_decode(x, fp, 8, 6, 19.3, early_stop=True)["iters"]
    assert (it == 1).any() and ((it > 1) & (it < 6)).any() and (it == 6).any()
    for g in (0, 1024, 2047):  # a work-group of the first stride, of the second, and the last full one
        assert len(set(it[64 * g: 64 * g + 64])) >= 2
    assert len(x) - 64 * 2048 == 5


@pytest.mark.parametrize("n,num_iter,llr_max", EXACT_CASES)
def test_fragile_rows_of_the_gpu_inputs_are_few(n, num_iter, llr_max):
    """A row at n = 1024 over 3 iterations evaluates about 6e4 f, each with five roundings and a 2^-27-ulp
    window: about 0.6 rows in 128 are expected to be fragile.  The GPU test leaves those rows out, so their
    number is capped here (another seed, never a higher cap)."""
    fp, x = exact_case_inputs(n, num_iter, llr_max)
    r = bp_ref.bp_decode(x, fp, n, num_iter, llr_max, exact=True)
    print(f"n={n} iters={num_iter} llr_max={llr_max}: fragile rows {int(r['fragile'].sum())} of {EXACT_ROWS}")
    assert r["fragile"].sum() <= FRAGILE_CAP
    assert not np.isnan(r["soft_u"]).any() and not np.isnan(r["ext_x"]).any()


def test_entry_point_is_exported():
    import polar_amd
    from polar_amd import _lib
    assert "pl_bp_decode" in _lib.EXPORTED_SYMBOLS
    assert "BP_Dec" in polar_amd.__all__ and callable(polar_amd.ops.bp_decode)
    with pytest.raises(ValueError):
        polar_amd.BP_Dec(np.arange(1024), 2048)
