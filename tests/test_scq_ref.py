"""The numpy restatement of fixed-point SC decoding (tests/golden/scq_ref.py) against the float oracle where
nothing can saturate, its clamp where something does, its quantiser at the awkward inputs, and the argument
checks of pl_llr_quantize / pl_scq_decode that need no GPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import scq_ref  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "polar_mi355x.h")


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32])
def test_reference_equals_float_minsum_where_nothing_saturates(n):
    """Inputs in [-3, 3], q_internal = 8: every node value is bounded by 3 n <= 96 < 127, so no clamp acts and the
    integer decoder is the float min-sum decoder on integer-valued floats, row for row."""
    import oracle
    rng = np.random.default_rng(100 + n)
    rows = 0
    for trial in range(8):
        k = int(rng.integers(1, n + 1))
        fp = scq_ref.random_frozen(n, k, 1000 * n + trial)
        q = rng.integers(-3, 4, size=(256, n)).astype(np.int8)
        bits, st = scq_ref.sc_decode(q, fp, 8, return_stats=True)
        assert st["g_clamped"] == 0 and st["load_clamped"] == 0
        want = oracle.sc_decode(q.astype(np.float32), fp, llr_max=127.0)
        assert np.array_equal(bits, want.astype(np.uint8)), (n, trial)
        rows += len(q)
    assert rows == 2048


def test_reference_clamp_is_live():
    """n = 64, full-range inputs, q_internal = 6: the clamps act, and the result differs from unclamped float
    min-sum decoding of the same integers on some rows."""
    import oracle
    n, k = 64, 32
    fp = scq_ref.rm_frozen(n)
    assert fp is not None and len(fp) == n - k
    rng = np.random.default_rng(7)
    q = rng.integers(-128, 128, size=(512, n)).astype(np.int8)
    bits, st = scq_ref.sc_decode(q, fp, 6, return_stats=True)
    assert st["load_clamped"] > 0 and st["g_clamped"] > 0
    want = oracle.sc_decode(q.astype(np.float32), fp, llr_max=127.0).astype(np.uint8)
    differ = int((bits != want).any(axis=1).sum())
    print("rows differing from the float result:", differ, "of", len(q), st)
    assert differ > 0


def test_reference_small_cases_by_hand():
    # n = 2, both information: u0 = HD(f(a0, a1)), u1 = HD(g(a0, a1, u0)); a = -q
    q = np.array([[3, -2], [0, 0], [-1, -1], [127, -128]], dtype=np.int8)
    # row 0: a = (-3, 2): f = -2 -> u0 = 1; g = 2 + 3 = 5 -> clamp 3 at q_internal 3 -> u1 = 0
    # row 1: zeros decide 1, 1; g = 0 - 0 = 0 -> 1
    # row 2: a = (1, 1): f = 1 -> 0; g = 2 -> 0
    # row 3: a = (-3, 3) after the load clamp: f = -3 -> 1; g = 3 + 3 = 6 -> 3 -> 0
    bits, st = scq_ref.sc_decode(q, [], 3, return_stats=True)
    assert bits.tolist() == [[1, 0], [1, 1], [0, 0], [1, 0]]
    assert st == {"load_clamped": 2, "g_clamped": 2, "g_total": 4}
    assert scq_ref.sc_decode(q, [0], 3).tolist() == [[1], [1], [0], [1]]  # u0 frozen: g = a1 + a0
    assert scq_ref.sc_decode(q, [0, 1], 3).shape == (4, 0)


def test_quantize_reference_at_the_awkward_inputs():
    x, inv, qc, want = scq_ref.quantizer_vectors()
    got = scq_ref.quantize(x, inv, qc)
    assert got.dtype == np.int8 and np.array_equal(got, want), np.flatnonzero(got != want)
    # the narrowest and the widest channel
    assert scq_ref.quantize(np.array([-9, -0.6, -0.5, 0.5, 0.6, 1.5, 9], np.float32), 1.0, 2).tolist() == \
        [-1, -1, 0, 0, 1, 1, 1]
    assert scq_ref.quantize(np.array([-1000, -127.5, -126.5, 126.5, 127.49, 1000], np.float32), 1.0, 8).tolist() == \
        [-127, -127, -126, 126, 127, 127]


def test_abi_argument_checks_without_gpu():
    """Every check but the stream's device runs before any HIP call."""
    from polar_amd import _lib
    assert "pl_llr_quantize" in _lib.EXPORTED_SYMBOLS and "pl_scq_decode" in _lib.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert "int pl_llr_quantize(const float* llr_logits" in text and "int pl_scq_decode(const pl_plan* plan" in text
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def err():
        return L.pl_last_error_string().decode()

    for qc in (1, 9, 0, -3):
        assert L.pl_llr_quantize(p, 4, 1.0, qc, p, None) == _lib.PL_EINVAL and "q_channel" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.pl_llr_quantize(p, 4, bad, 6, p, None) == _lib.PL_EINVAL and "inv_step" in err()
    assert L.pl_llr_quantize(p, -1, 1.0, 6, p, None) == _lib.PL_EINVAL and "count" in err()
    assert L.pl_llr_quantize(None, 4, 1.0, 6, p, None) == _lib.PL_EINVAL and "llr_logits" in err()
    assert L.pl_llr_quantize(p, 4, 1.0, 6, None, None) == _lib.PL_EINVAL and "out_q" in err()
    assert L.pl_llr_quantize(None, 0, 1.0, 6, None, None) == _lib.PL_OK  # count == 0: nothing to do, no HIP call
    rc = L.pl_scq_decode(None, p, 1, 6, p, _lib.PL_OUT_U8, None)
    assert rc == _lib.PL_EINVAL and "plan" in err()
    with pytest.raises(_lib.PolarArgumentError, match="plan"):
        _lib.check(rc, "pl_scq_decode")


def test_python_surface_argument_errors():
    import torch
    import polar_amd
    from polar_amd import cli, ops
    from polar_amd.quant import SCQ_Dec
    assert polar_amd.SCQ_Dec is SCQ_Dec
    fp = np.arange(16)
    d = SCQ_Dec(fp, 32, q_channel=5, q_internal=6, llr_max=30.0)
    assert (d.k, d.cmax, d.imax) == (16, 15, 31) and d.step == 2.0 and d.inv_step == 0.5
    for kw in ({"q_channel": 1}, {"q_internal": 9}, {"q_channel": 7, "q_internal": 6}, {"q_channel": 4.0},
               {"llr_max": 0.0}, {"llr_max": float("inf")}, {"output_dtype": torch.int32}):
        with pytest.raises(ValueError):
            SCQ_Dec(fp, 32, **kw)
    with pytest.raises(ValueError):
        SCQ_Dec(fp, 48)
    with pytest.raises(ValueError):
        SCQ_Dec(fp, 4096)
    with pytest.raises(ValueError):
        d.forward_q(torch.zeros((2, 32)))  # not int8
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.llr_quantize(torch.zeros(4), 1.0, 6)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.scq_decode(None, torch.zeros((1, 4), dtype=torch.int8), 6)
    c = cli.parse(["--k", "32", "--n", "64", "--algos", "[scq]", "--scq_qc", "4", "--scq_qi", "5"])
    assert c.algos == ["scq"] and (c.scq_qc, c.scq_qi, c.scq_llr_max) == (4, 5, 30.0)
    for argv in (["--algos", "[scq]", "--code", "5g"], ["--algos", "[scq]", "--scq_qc", "7", "--scq_qi", "6"],
                 ["--algos", "[scq]", "--scq_qi", "9"], ["--algos", "[scq]", "--scq_llr_max", "0"]):
        with pytest.raises(SystemExit):
            cli.parse(argv)
