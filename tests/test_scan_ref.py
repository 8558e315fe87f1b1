"""The numpy restatement of soft-cancellation decoding (tests/golden/scan_ref.py) against what can be known
without a GPU: a closed form at n = 2, the first SC leaf, noiseless rows, the sign symmetry of min-sum (which
checks the wiring against the encoder), BP as the other schedule of the same units, the block error rate the
decoder exists for, and what tests/test_scan_gpu.py assumes of its inputs (iteration classes of the early-stop
rows, fragile rows of the exact-f cases).  CPU only.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import bp_ref  # noqa: E402
import scan_ref  # noqa: E402

F32 = np.float32


def test_n2_closed_form():
    """n = 2, position 0 frozen, a = -logits = (a0, a1): R[0] = (lmax, 0), so L[0][1] = clip(f(a0, lmax) + a1),
    R[1][0] = clip(f(lmax, a1 + 0)), R[1][1] = clip(f(lmax, a0) + 0); with min-sum f(v, lmax) = clip(v).  No
    message depends on an earlier iteration: one iteration suffices, a second changes nothing."""
    lm = float(F32(19.3))
    logits = np.array([[-1.5, 0.25], [2.0, -3.0], [25.0, 1.0], [-0.5, -30.0], [0.0, 0.0]], dtype=F32)
    want_soft = np.array([[-1.25], [-1.0], [lm], [-lm], [0.0]], dtype=F32)  # -clip(clip(a0) + a1)
    want_ext = np.array([[0.25, -1.5], [-3.0, 2.0], [1.0, lm], [-lm, -0.5], [0.0, 0.0]], dtype=F32)
    for it in (1, 2, 4):
        for es in (False, True):
            r = scan_ref.scan_decode(logits, [0], 2, it, 19.3, early_stop=es)
            assert np.array_equal(r["soft_u"], want_soft), r["soft_u"]
            assert np.array_equal(r["ext_x"], want_ext), r["ext_x"]
            assert np.array_equal(r["bits"], (~(-want_soft > 0)).astype(np.uint8))
            assert np.array_equal(r["iters"], np.full(5, 1 if es else it, dtype=np.int32))
    r = scan_ref.scan_decode(logits[:1], [0], 2, 1, 19.3, scale=0.9375)
    assert np.array_equal(r["soft_u"], np.array([[-(F32(1.5) * F32(0.9375)) + F32(0.25)]], dtype=F32))
    # both positions information: soft_u[0] = -f(a0, a1); the leaf R are 0, so L[0][1] = a1 and ext = 0
    r = scan_ref.scan_decode(logits[:2], [], 2, 2, 19.3)
    assert np.array_equal(r["soft_u"], np.array([[0.25, 0.25], [2.0, -3.0]], dtype=F32))
    assert np.array_equal(r["ext_x"], np.zeros((2, 2), dtype=F32))
    # at n = 2 the two schedules are the same
    b = bp_ref.bp_decode(logits, [0], 2, 1, 19.3)
    assert all(np.array_equal(r2, b[k]) for k, r2 in scan_ref.scan_decode(logits, [0], 2, 1, 19.3).items())


@pytest.mark.parametrize("n", [4, 32, 256])
def test_first_leaf_of_iteration_one_is_the_sc_leaf(n):
    """Positions 0 and 1 information: every R on the path to leaf 0 is 0 in the first iteration, so L[0][0] is
    the f-only chain of SC over the clipped channel row."""
    fp = np.arange(2, 2 + n // 4)
    rng = np.random.default_rng(n)
    _, x = bp_ref.awgn_logits(rng, fp, n, 16, 1.0)
    a = bp_ref.clip(-x, 19.3)
    while a.shape[1] > 1:
        h = a.shape[1] // 2
        a = bp_ref.clip(bp_ref.f_minsum(np.ascontiguousarray(a[:, :h]), np.ascontiguousarray(a[:, h:]), 19.3), 19.3)
    r = scan_ref.scan_decode(x, fp, n, 1, 19.3)
    assert np.array_equal(r["soft_u"][:, 0], -a[:, 0])
    assert np.abs(a).max() > 0


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n", [2, 4, 16, 64, 256])
def test_noiseless_rows_decode_in_one_iteration(n, exact):
    for seed in range(3):
        rng = np.random.default_rng(10 * n + seed)
        k = int(rng.integers(1, n + 1))
        fp = bp_ref.rate_half_frozen(n, 50 + seed, k)
        u, _ = bp_ref.awgn_logits(rng, fp, n, 6)
        x = bp_ref.noiseless_logits(u)
        r = scan_ref.scan_decode(x, fp, n, 5, 19.3, exact=exact, early_stop=True)
        info = np.setdiff1d(np.arange(n), fp)
        assert np.array_equal(r["bits"], u[:, info])
        assert np.array_equal(r["iters"], np.ones(6, dtype=np.int32))
        one = scan_ref.scan_decode(x, fp, n, 1, 19.3, exact=exact)
        assert np.array_equal(one["bits"], u[:, info]) and np.array_equal(one["soft_u"], r["soft_u"])


@pytest.mark.parametrize("n", [4, 8, 32, 128])
def test_minsum_sign_symmetry(n):
    """For a codeword x = u G (frozen bits 0), decoding logits (1 - 2x) gives soft_u (1 - 2u) and ext_x (1 - 2x)
    exactly: min-sum commutes with sign flips along a codeword -- but only if the wiring is the encoder's."""
    fp = bp_ref.rate_half_frozen(n, 300 + n)
    info = np.setdiff1d(np.arange(n), fp)
    rng = np.random.default_rng(n)
    _, base = bp_ref.awgn_logits(rng, fp, n, 8)
    u, _ = bp_ref.awgn_logits(rng, fp, n, 8)
    sx = (1.0 - 2.0 * bp_ref.encode(u)).astype(F32)
    su = (1.0 - 2.0 * u[:, info]).astype(F32)
    for scale in (1.0, 0.9375):
        a = scan_ref.scan_decode(base, fp, n, 3, 19.3, scale=scale)
        b = scan_ref.scan_decode(base * sx, fp, n, 3, 19.3, scale=scale)
        assert np.array_equal(b["soft_u"], a["soft_u"] * su)
        assert np.array_equal(b["ext_x"], a["ext_x"] * sx)
    assert np.abs(a["soft_u"]).max() > 0 and np.abs(a["ext_x"]).max() > 0


def test_scan_is_another_schedule_than_bp():
    n = 64
    fp = bp_ref.rate_half_frozen(n, 1)
    _, x = bp_ref.awgn_logits(np.random.default_rng(3), fp, n, 32, 1.0)
    s, b = scan_ref.scan_decode(x, fp, n, 1, 19.3), bp_ref.bp_decode(x, fp, n, 1, 19.3)
    assert (s["soft_u"] != b["soft_u"]).any(axis=1).all() and (s["ext_x"] != b["ext_x"]).any(axis=1).all()
    # a second iteration uses the first one's R
    assert not np.array_equal(scan_ref.scan_decode(x, fp, n, 2, 19.3)["soft_u"], s["soft_u"])


def test_two_scan_iterations_beat_twenty_of_bp():
    """(64,128), the package's reference frozen set, 3 dB, 2000 rows of default_rng(5), min-sum: 0.100 against
    0.178."""
    import polar_amd
    n, k = 128, 64
    fp = polar_amd.reference_frozen_pos(k, n).numpy()
    u, x = bp_ref.awgn_logits(np.random.default_rng(5), fp, n, 2000, 3.0)
    info = np.setdiff1d(np.arange(n), fp)
    scan = (scan_ref.scan_decode(x, fp, n, 2, 19.3)["bits"] != u[:, info]).any(axis=1).mean()
    bp = (bp_ref.bp_decode(x, fp, n, 20, 19.3)["bits"] != u[:, info]).any(axis=1).mean()
    print(f"BLER: SCAN-2 {scan:.4f}, BP-20 {bp:.4f}")
    assert scan <= bp


@pytest.mark.parametrize("exact", [False, True])
def test_early_stop_against_the_full_run(exact):
    n, num_iter = 64, 4
    fp = bp_ref.rate_half_frozen(n, 1)
    _, x = bp_ref.make_inputs(5, n, fp, 40, 19.3, ebno_db=1.0)
    full = scan_ref.scan_decode(x, fp, n, num_iter, 19.3, exact=exact)
    es = scan_ref.scan_decode(x, fp, n, num_iter, 19.3, exact=exact, early_stop=True)
    assert np.array_equal(full["iters"], np.full(40, num_iter, dtype=np.int32))
    never = es["iters"] == num_iter
    assert never.any() and (~never).any()
    for key in ("bits", "soft_u", "ext_x"):
        assert np.array_equal(full[key][never], es[key][never])
    for i in np.flatnonzero(~never)[:4]:  # a stopped row holds the messages of the iteration it stopped in
        short = scan_ref.scan_decode(x[i:i + 1], fp, n, int(es["iters"][i]), 19.3, exact=exact)
        for key in ("bits", "soft_u", "ext_x"):
            assert np.array_equal(short[key][0], es[key][i])


@pytest.mark.parametrize("n", scan_ref.EARLY_STOP_SIZES)
def test_early_stop_gpu_inputs_show_their_classes(n):
    fp = bp_ref.rate_half_frozen(n, scan_ref.EARLY_STOP_FROZEN_SEED)
    x = bp_ref.early_stop_inputs(n, fp)
    iters = scan_ref.EARLY_STOP_ITERS
    it = scan_ref.scan_decode(x, fp, n, iters, 19.3, early_stop=True)["iters"]
    print(f"n={n}: iters histogram {np.bincount(it, minlength=iters + 1).tolist()}")
    one, few, never = scan_ref.early_stop_classes(n)
    assert (it == 1).any() == one and ((it > 1) & (it < iters)).any() == few and (it == iters).any() == never


def test_past_grid_rows_stop_at_several_iterations():
    fp = bp_ref.rate_half_frozen(8, 3)
    _, x = bp_ref.awgn_logits(np.random.default_rng(11), fp, 8, 70001)
    it = scan_ref.scan_decode(x, fp, 8, 4, 19.3, early_stop=True)["iters"]
    assert len(set(it.tolist())) >= 3 and len(set(it[-17:].tolist())) >= 2  # the ragged last work-group too


@pytest.mark.parametrize("n,num_iter,llr_max", scan_ref.SCAN_EXACT_CASES)
def test_fragile_rows_of_the_gpu_inputs_are_few(n, num_iter, llr_max):
    fp, x = scan_ref.exact_case_inputs(n, num_iter, llr_max)
    assert len(x) == (32 if n == 2048 else 128)
    r = scan_ref.scan_decode(x, fp, n, num_iter, llr_max, exact=True)
    print(f"n={n} iters={num_iter} llr_max={llr_max}: fragile rows {int(r['fragile'].sum())} of {len(x)}")
    assert r["fragile"].sum() <= scan_ref.FRAGILE_CAP
    assert not np.isnan(r["soft_u"]).any() and not np.isnan(r["ext_x"]).any()


@pytest.mark.parametrize("n", [64, 256])
def test_fragile_rows_of_the_exact_early_stop_inputs_are_few(n):
    fp = bp_ref.rate_half_frozen(n, scan_ref.EARLY_STOP_FROZEN_SEED)
    x = bp_ref.early_stop_inputs(n, fp)
    r = scan_ref.scan_decode(x, fp, n, scan_ref.EARLY_STOP_ITERS, 19.3, exact=True, early_stop=True)
    assert r["fragile"].sum() <= scan_ref.FRAGILE_CAP and len(set(r["iters"].tolist())) >= 3


def test_entry_point_is_exported():
    import polar_amd
    from polar_amd import _lib
    assert "pl_scan_decode" in _lib.EXPORTED_SYMBOLS and _lib.PL_SCAN_EARLY_STOP == 1
    assert "SCAN_Dec" in polar_amd.__all__ and callable(polar_amd.ops.scan_decode)
    assert polar_amd.SCAN_Dec(np.arange(1024), 2048).k == 1024
    with pytest.raises(ValueError):
        polar_amd.SCAN_Dec(np.arange(2048), 4096)
