"""pl_scq_decode / pl_llr_quantize / SCQ_Dec on the GPU against the numpy restatement (tests/golden/scq_ref.py,
itself checked by tests/test_scq_ref.py).  The arithmetic is integer: every comparison is bit equality.
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import scq_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 3, 67, 257)  # never a multiple of the codewords per wave (64 / G) or per work-group
WIDTHS = (2, 5, 6, 8)


def _plan(n, fp, **kw):
    import polar_amd
    from polar_amd import _lib
    return _lib.Plan(n, polar_amd.frozen_mask(np.asarray(fp, dtype=np.int64), n), 1, _lib.PL_F_MINSUM,
                     flags=_lib.PL_PLAN_GENERIC, device=DEV, **kw)


def _decode(plan, q, qi, out_dtype=torch.uint8):
    from polar_amd import ops
    out = ops.scq_decode(plan, torch.as_tensor(np.ascontiguousarray(q), device=DEV), qi, out_dtype=out_dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_rows(got, want, what):
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1)) if want.size else []
    print(f"{what}: rows differing {len(bad)} of {len(want)}")
    assert got.shape == want.shape and np.array_equal(got, want), (what, list(bad[:8]))


def _all_inputs(values, n):
    return np.array(list(itertools.product(values, repeat=n)), dtype=np.int8)


@pytest.mark.parametrize("n", [2, 4])
def test_exhaustive_small_codes(n):
    """Every frozen pattern of n = 2 and n = 4 on every input of [-3, 3]^n at q_internal = 3 (where +-3 is
    Imax, so g saturates); the n = 4 patterns again at q_internal = 2 on inputs out to +-127 and -128, for
    the clamp at the load."""
    runs = [(3, _all_inputs(range(-3, 4), n))]
    if n == 4:
        runs.append((2, _all_inputs([-128, -127, -2, -1, 0, 1, 127], n)))
    for qi, q in runs:
        clamped = 0
        for pattern in range(1 << n):
            fp = [i for i in range(n) if (pattern >> i) & 1]
            want, st = scq_ref.sc_decode(q, fp, qi, return_stats=True)
            clamped += st["g_clamped"]
            assert qi == 3 or st["load_clamped"] > 0
            _assert_rows(_decode(_plan(n, fp), q, qi), want, f"n={n} frozen={fp} q_internal={qi}")
        assert clamped > 0


def _frozen_sets(n):
    """(name, frozen positions): the pinned RM-weight set where there is one, and a seeded random set whose k
    is 1 at n = 8 and n = 1024, n at n = 16 and n = 512."""
    k = {8: 1, 1024: 1, 16: 16, 512: 512}.get(n, int(np.random.default_rng(n).integers(2, n)))
    sets = [(f"random_k{k}", scq_ref.random_frozen(n, k, 17 * n + 1))]
    rm = scq_ref.rm_frozen(n)
    if rm is not None:
        sets.insert(0, (f"rm_k{n - len(rm)}", rm))
    return sets


@pytest.mark.parametrize("n", [8, 16, 32, 64, 128, 256, 512, 1024, 2048])
def test_every_length_width_and_batch(n):
    """Uniform int8 inputs over the whole range including -128; the reference's counters show that the load
    and g clamped on each input."""
    rng = np.random.default_rng(9000 + n)
    q_all = rng.integers(-128, 128, size=(max(BATCHES), n)).astype(np.int8)
    q_all[0, 0] = -128
    for name, fp in _frozen_sets(n):
        plan = _plan(n, fp)
        for qi in WIDTHS:
            for bs in BATCHES:
                q = q_all[:bs]
                want, st = scq_ref.sc_decode(q, fp, qi, return_stats=True)
                assert st["g_clamped"] > 0 and (qi == 8 or st["load_clamped"] > 0), (name, qi, bs, st)
                _assert_rows(_decode(plan, q, qi), want, f"n={n} {name} q_internal={qi} bs={bs}")


@pytest.mark.parametrize("n", [4, 64, 256, 2048])
def test_constant_rows(n):
    """Rows of zeros decide 1 at every information position (f(0, 0) = 0, g = 0, HD(0) = 1); rows of all +Imax
    and all -Imax, and of +-127 / -128 beyond it."""
    fp = scq_ref.rm_frozen(n)
    fp = scq_ref.random_frozen(n, n // 2, 5) if fp is None else fp
    plan = _plan(n, fp)
    for qi in (3, 6, 8):
        im = scq_ref.imax(qi)
        q = np.stack([np.full(n, v, np.int8) for v in (0, im, -im, 127, -127, -128)])
        want = scq_ref.sc_decode(q, fp, qi)
        assert want[0].all()
        _assert_rows(_decode(plan, q, qi), want, f"n={n} q_internal={qi} constant rows")


def test_output_kinds_agree_and_empty_batch():
    n, fp = 256, scq_ref.rm_frozen(256)
    plan = _plan(n, fp)
    q = np.random.default_rng(3).integers(-128, 128, size=(131, n)).astype(np.int8)
    u8, f32 = _decode(plan, q, 6, torch.uint8), _decode(plan, q, 6, torch.float32)
    assert f32.dtype == np.float32 and np.array_equal(f32, u8.astype(np.float32))
    _assert_rows(u8, scq_ref.sc_decode(q, fp, 6), "u8")
    assert _decode(plan, q[:0], 6).shape == (0, n - len(fp))


def test_plan_f_mode_and_llr_max_are_ignored():
    from polar_amd import _lib
    n, fp = 128, scq_ref.random_frozen(128, 50, 11)
    q = np.random.default_rng(4).integers(-128, 128, size=(67, n)).astype(np.int8)
    want = scq_ref.sc_decode(q, fp, 5)
    import polar_amd
    exact = _lib.Plan(n, polar_amd.frozen_mask(fp, n), 1, _lib.PL_F_EXACT, 2.0, flags=_lib.PL_PLAN_GENERIC, device=DEV)
    _assert_rows(_decode(exact, q, 5), want, "exact-f plan, llr_max 2")
    _assert_rows(_decode(_plan(n, fp), q, 5), want, "min-sum plan")


def test_argument_errors_with_a_plan():
    from polar_amd import _lib, ops
    n, fp = 32, scq_ref.random_frozen(32, 16, 2)
    plan = _plan(n, fp)
    q = torch.zeros((4, n), dtype=torch.int8, device=DEV)
    for qi in (1, 9):
        with pytest.raises(ValueError, match="q_internal"):
            ops.scq_decode(plan, q, qi)
    with pytest.raises(ValueError):
        ops.scq_decode(plan, q.to(torch.float32), 6)
    with pytest.raises(ValueError):
        ops.scq_decode(plan, q[:, :16], 6)
    L = _lib.lib()
    out = torch.empty((4, 16), dtype=torch.uint8, device=DEV)
    args = (plan.handle, q.data_ptr(), 4, 6, out.data_ptr())
    assert L.pl_scq_decode(*args[:3], 9, args[4], 1, None) == _lib.PL_EINVAL and b"q_internal" in L.pl_last_error_string()
    assert L.pl_scq_decode(args[0], args[1], -1, 6, args[4], 1, None) == _lib.PL_EINVAL and b"bs" in L.pl_last_error_string()
    assert L.pl_scq_decode(*args, 7, None) == _lib.PL_EINVAL and b"out_kind" in L.pl_last_error_string()
    assert L.pl_scq_decode(args[0], None, 4, 6, args[4], 1, None) == _lib.PL_EINVAL and b"llr_q" in L.pl_last_error_string()
    assert L.pl_scq_decode(args[0], args[1], 4, 6, None, 1, None) == _lib.PL_EINVAL and b"out_bits" in L.pl_last_error_string()
    assert L.pl_scq_decode(args[0], args[1] + 1, 3, 6, args[4], 1, None) == _lib.PL_EINVAL \
        and b"aligned" in L.pl_last_error_string()
    import polar_amd
    lst = _lib.Plan(n, polar_amd.frozen_mask(fp, n), 4, _lib.PL_F_MINSUM, device=DEV)
    assert L.pl_scq_decode(lst.handle, *args[1:], 1, None) == _lib.PL_EINVAL and b"list-size-1" in L.pl_last_error_string()
    # a row view that is not 16-byte aligned is copied by ops, not refused
    qq = torch.as_tensor(np.random.default_rng(1).integers(-128, 128, size=(5, n + 1)).astype(np.int8), device=DEV)
    got = ops.scq_decode(plan, qq[:, 1:], 6, out_dtype=torch.uint8).cpu().numpy()
    _assert_rows(got, scq_ref.sc_decode(qq[:, 1:].cpu().numpy().copy(), fp, 6), "unaligned view")


def test_graph_replay_equals_eager():
    from polar_amd import ops
    n, fp = 512, scq_ref.rm_frozen(512)
    plan = _plan(n, fp)
    rng = np.random.default_rng(5)
    logits = torch.as_tensor((rng.standard_normal((131, n)) * 6).astype(np.float32), device=DEV)
    q = torch.empty((131, n), dtype=torch.int8, device=DEV)
    out = torch.empty((131, n - len(fp)), dtype=torch.uint8, device=DEV)

    def fn():
        ops.llr_quantize(logits, 1.0, 5, out=q)
        ops.scq_decode(plan, q, 6, out=out)
    fn()
    torch.cuda.synchronize()
    eager = out.cpu().numpy().copy()
    graph = ops.LaunchGraph(fn, 1, device=DEV)
    logits.copy_(torch.as_tensor((rng.standard_normal((131, n)) * 6).astype(np.float32), device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    qn = scq_ref.quantize(logits.cpu().numpy(), 1.0, 5)
    assert np.array_equal(q.cpu().numpy(), qn)
    _assert_rows(out.cpu().numpy(), scq_ref.sc_decode(qn, fp, 6), "replayed on refilled logits")
    assert not np.array_equal(out.cpu().numpy(), eager)
    logits.zero_()
    fn()
    graph.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().all()


def test_quantiser_vectors_and_tails():
    from polar_amd import ops
    x, inv, qc, want = scq_ref.quantizer_vectors()
    got = ops.llr_quantize(torch.as_tensor(x, device=DEV), inv, qc).cpu().numpy()
    assert got.dtype == np.int8 and np.array_equal(got, want), np.flatnonzero(got != want)
    rng = np.random.default_rng(6)
    for count in (0, 1, 5, 4099):
        for qc in (2, 6, 8):
            cmax = scq_ref.imax(qc)
            inv = float(np.float32(cmax / 30.0))
            v = (rng.standard_normal(count) * 20).astype(np.float32)
            v[::7] = np.float32(0.5) / np.float32(inv) * np.float32(3.0)  # near ties too
            t = torch.as_tensor(v, device=DEV)
            got = ops.llr_quantize(t, inv, qc).cpu().numpy()
            assert np.array_equal(got, scq_ref.quantize(v, inv, qc)), (count, qc)
            if count > 1:  # a view whose first element is not 16-byte aligned takes the element-wise path
                got = ops.llr_quantize(t[1:], inv, qc).cpu().numpy()
                assert np.array_equal(got, scq_ref.quantize(v[1:], inv, qc)), (count, qc, "offset")
    m = torch.as_tensor((rng.standard_normal((3, 5, 64)) * 9).astype(np.float32), device=DEV)
    assert np.array_equal(ops.llr_quantize(m, 0.5, 6).cpu().numpy(), scq_ref.quantize(m.cpu().numpy(), 0.5, 6))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="inv_step"):
            ops.llr_quantize(m, bad, 6)
    with pytest.raises(ValueError, match="q_channel"):
        ops.llr_quantize(m, 1.0, 9)


def test_module_forward():
    import polar_amd
    from polar_amd import _lib, ops
    n, k = 32, 16
    fp = polar_amd.reference_frozen_pos(k, n).numpy()
    rng = np.random.default_rng(8)
    # (k, n) = (16, 32), q_channel 3, q_internal 8, integer logits in [-3, 3], llr_max 3: the step is 1, nothing
    # saturates (3 n < 127), and the float min-sum kernel on a plan with llr_max = 127 decides the same bits
    dec = polar_amd.SCQ_Dec(fp, n, q_channel=3, q_internal=8, llr_max=3., device=DEV)
    assert dec.step == 1.0 and dec.inv_step == 1.0 and dec.k == k
    x = rng.integers(-3, 4, size=(5, 41, n)).astype(np.float32)
    got = dec(torch.as_tensor(x))  # a CPU tensor, 3-D
    assert got.shape == (5, 41, k) and got.dtype == torch.float32 and got.device.type == "cpu"
    plan = _lib.Plan(n, polar_amd.frozen_mask(fp, n), 1, _lib.PL_F_MINSUM, 127.0, flags=_lib.PL_PLAN_GENERIC,
                     device=DEV)
    want = ops.sc_decode(plan, torch.as_tensor(x.reshape(-1, n), device=DEV)).cpu().numpy().reshape(5, 41, k)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(got.numpy().reshape(-1, k), scq_ref.sc_decode(x.reshape(-1, n).astype(np.int8), fp, 8))
    # forward == forward_q o quantize, on GPU tensors, at the default widths
    dec6 = polar_amd.SCQ_Dec(fp, n, device=DEV, output_dtype=torch.float64)
    y = torch.as_tensor((rng.standard_normal((3, 7, n)) * 12).astype(np.float32), device=DEV)
    out = dec6(y)
    q = dec6.quantize(y)
    assert out.device.type == "cuda" and out.dtype == torch.float64 and q.dtype == torch.int8 and q.shape == y.shape
    assert torch.equal(out, dec6.forward_q(q))
    qn = scq_ref.quantize(y.cpu().numpy(), dec6.inv_step, 6)
    assert np.array_equal(q.cpu().numpy(), qn)
    assert np.array_equal(out.cpu().numpy().reshape(-1, k), scq_ref.sc_decode(qn.reshape(-1, n), fp, 6))


def test_cli_scq_leg():
    from polar_amd import cli
    res = cli.main(["--k", "32", "--n", "64", "--algos", "[scq]", "--bs", "100", "--mc_iter", "1", "--snr_end", "1.5",
                    "--target_block_errs", "100000"])
    assert "SC" in res and "SCQ (6,6)" in res
    bler_sc, bler_q = res["SC"][1], res["SCQ (6,6)"][1]
    print("BLER SC", bler_sc, "SCQ", bler_q)
    assert bler_q.shape == bler_sc.shape == (3,) and ((bler_q >= 0) & (bler_q <= 1)).all()
