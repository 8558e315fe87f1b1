"""pl_bp_decode / ops.bp_decode / BP_Dec on the GPU against the numpy restatement (tests/golden/bp_ref.py,
itself checked by tests/test_bp_ref.py): bits, soft_u, ext_x and iters value for value (np.array_equal:
+0 and -0 compare equal, nothing else may differ); with the exact f, rows flagged fragile by the
correctly rounded restatement are left out, and their number is capped before the comparison.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import bp_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("bits", "soft_u", "ext_x", "iters")


def _plan(n, fp, f_mode=0, llr_max=19.3, list_size=1):
    import polar_amd
    from polar_amd import _lib
    return _lib.Plan(n, polar_amd.frozen_mask(fp, n), list_size, f_mode, llr_max, flags=_lib.PL_PLAN_GENERIC, device=DEV)


def _run(plan, logits, num_iter, **kw):
    from polar_amd import ops
    x = torch.as_tensor(np.ascontiguousarray(logits, dtype=np.float32), device=DEV)
    r = ops.bp_decode(plan, x, num_iter, out_dtype=torch.uint8, soft=True, ext=True, iters=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_equal(got, ref, keep=None, what=""):
    for key in KEYS:
        g, r = got[key], ref[key]
        if keep is not None:
            g, r = g[keep], r[keep]
        bad = np.flatnonzero((g != r).reshape(g.shape[0], -1).any(axis=1)) if g.size else []
        print(f"{what} {key}: rows differing {len(bad)} of {g.shape[0]}")
        assert np.array_equal(g, r), (what, key, list(bad[:8]))


MINSUM_CODES = [(n, None) for n in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)] + [(64, 64), (64, 1)]


@pytest.mark.parametrize("n,k", MINSUM_CODES)
def test_minsum_equals_the_restatement(n, k):
    """67 rows (a wave or work-group ends in a partial set of codewords), a seeded rate-1/2 frozen set
    (at n = 64 also k = n and k = 1), 1, 2 and 5 iterations."""
    fp = bp_ref.rate_half_frozen(n, 40 + n, k)
    _, x = bp_ref.make_inputs(60 + n + (k or 0), n, fp, 67)
    plan = _plan(n, fp)
    for num_iter in (1, 2, 5):
        ref = bp_ref.bp_decode(x, fp, n, num_iter, 19.3)
        _assert_equal(_run(plan, x, num_iter), ref, what=f"n={n} k={k} iters={num_iter}")


@pytest.mark.parametrize("n", [8, 256])
def test_scaled_minsum(n):
    fp = bp_ref.rate_half_frozen(n, 40 + n)
    _, x = bp_ref.make_inputs(80 + n, n, fp, 67)
    ref = bp_ref.bp_decode(x, fp, n, 3, 19.3, scale=0.9375)
    assert not np.array_equal(ref["soft_u"], bp_ref.bp_decode(x, fp, n, 3, 19.3)["soft_u"])
    _assert_equal(_run(_plan(n, fp), x, 3, scale=0.9375), ref, what=f"n={n} scale=0.9375")


@pytest.mark.parametrize("n,num_iter,llr_max", bp_ref.EXACT_CASES)
def test_exact_f_equals_the_restatement(n, num_iter, llr_max):
    """128 rows; llr_max 60 (n = 4) takes the full-range forms of the exact f.  Every non-fragile row is equal."""
    fp, x = bp_ref.exact_case_inputs(n, num_iter, llr_max)
    ref = bp_ref.bp_decode(x, fp, n, num_iter, llr_max, exact=True)
    print(f"n={n} iters={num_iter} llr_max={llr_max}: fragile rows {int(ref['fragile'].sum())}")
    assert ref["fragile"].sum() <= bp_ref.FRAGILE_CAP
    got = _run(_plan(n, fp, 1, llr_max), x, num_iter)
    _assert_equal(got, ref, keep=~ref["fragile"], what=f"exact n={n} iters={num_iter} llr_max={llr_max}")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n", [64, 1024])
def test_early_stop(n, exact):
    """Noiseless, noisy and pure-noise rows, 10 iterations: rows stop after 1, after a few and never."""
    import polar_amd
    fp = polar_amd.reference_frozen_pos(n // 2, n).numpy()
    x = bp_ref.early_stop_inputs(n, fp)
    ref = bp_ref.bp_decode(x, fp, n, 10, 19.3, exact=exact, early_stop=True)
    it = ref["iters"]
    print(f"n={n} exact={exact}: iters {it.tolist()}, fragile rows {int(ref['fragile'].sum())}")
    assert (it == 1).any() and ((it > 1) & (it < 10)).any() and (it == 10).any()
    assert ref["fragile"].sum() <= bp_ref.FRAGILE_CAP
    got = _run(_plan(n, fp, int(exact)), x, 10, early_stop=True)
    _assert_equal(got, ref, keep=~ref["fragile"], what=f"early stop n={n} exact={exact}")
    # the flag off: every row runs them all
    off = _run(_plan(n, fp, int(exact)), x, 10)
    assert np.array_equal(off["iters"], np.full(len(x), 10, dtype=np.int32))


@pytest.mark.parametrize("n", bp_ref.EARLY_STOP_SIZES)
def test_early_stop_every_size(n):
    """Min-sum early stop at the sizes of both stop paths that test_early_stop leaves out: n = 2 ... 32 (2 to 32
    codewords in one wave) and n = 128, 256, 512.  Rows stop after 1 iteration, after a few and never; at n = 2 no
    message depends on an earlier iteration and every row of these inputs stops after the first, so only that
    class is asserted there."""
    fp = bp_ref.rate_half_frozen(n, bp_ref.EARLY_STOP_FROZEN_SEED)
    x = bp_ref.early_stop_inputs(n, fp)
    ref = bp_ref.bp_decode(x, fp, n, bp_ref.EARLY_STOP_ITERS, 19.3, early_stop=True)
    it = ref["iters"]
    print(f"n={n}: iters {it.tolist()}")
    assert (it == 1).any()
    assert n == 2 or (((it > 1) & (it < 10)).any() and (it == 10).any())
    _assert_equal(_run(_plan(n, fp), x, bp_ref.EARLY_STOP_ITERS, early_stop=True), ref, what=f"early stop n={n}")


@pytest.mark.parametrize("n", [64, 256])
def test_early_stop_scaled_minsum(n):
    fp = bp_ref.rate_half_frozen(n, bp_ref.EARLY_STOP_FROZEN_SEED)
    x = bp_ref.early_stop_inputs(n, fp)
    ref = bp_ref.bp_decode(x, fp, n, 10, 19.3, scale=0.9375, early_stop=True)
    it = ref["iters"]
    print(f"n={n} scale=0.9375: iters {it.tolist()}")
    assert (it == 1).any() and ((it > 1) & (it < 10)).any() and (it == 10).any()
    assert not np.array_equal(it, bp_ref.bp_decode(x, fp, n, 10, 19.3, early_stop=True)["iters"])
    _assert_equal(_run(_plan(n, fp), x, 10, scale=0.9375, early_stop=True), ref, what=f"early stop scaled n={n}")


def test_early_stop_ragged_and_past_the_grid():
    """n = 8, bs = 64 * 1024 * 2 + 5: every work-group starts a second stride with fresh `act` and `done`, and
    the last one holds 5 valid codewords; noiseless, noisy and noise rows in every group."""
    fp, x = bp_ref.past_grid_early_stop_inputs()
    assert len(x) == 64 * 1024 * 2 + 5
    ref = bp_ref.bp_decode(x, fp, 8, 6, 19.3, early_stop=True)
    it = ref["iters"]
    print("iters histogram:", np.bincount(it, minlength=7).tolist(), "last five:", it[-5:].tolist())
    assert (it == 1).any() and ((it > 1) & (it < 6)).any() and (it == 6).any()
    _assert_equal(_run(_plan(8, fp), x, 6, early_stop=True), ref, what="early stop past the grid")


def test_batch_edges_and_optional_outputs():
    from polar_amd import ops
    n = 8
    fp = bp_ref.rate_half_frozen(n, 3)
    plan = _plan(n, fp)
    rng = np.random.default_rng(11)
    _, x = bp_ref.awgn_logits(rng, fp, n, 70001)  # 64 codewords a work-group: 1094 groups, past the 1024-block cap
    ref = bp_ref.bp_decode(x, fp, n, 1, 19.3)
    _assert_equal(_run(plan, x, 1), ref, what="bs=70001")
    one = _run(plan, x[5:6], 1)
    _assert_equal(one, {k: ref[k][5:6] for k in KEYS}, what="bs=1")
    empty = _run(plan, x[:0], 1)
    assert empty["bits"].shape == (0, 4) and empty["ext_x"].shape == (0, 8) and empty["iters"].shape == (0,)
    # each output alone equals its value in the full call
    xt = torch.as_tensor(x[:300], device=DEV)
    for key, kw in (("bits", dict(hard=True)), ("soft_u", dict(hard=False, soft=True)),
                    ("ext_x", dict(hard=False, ext=True)), ("iters", dict(hard=False, iters=True))):
        r = ops.bp_decode(plan, xt, 1, out_dtype=torch.uint8, **kw)
        assert list(r) == [key] and np.array_equal(r[key].cpu().numpy(), ref[key][:300]), key
    f32 = ops.bp_decode(plan, xt, 1)["bits"]
    assert f32.dtype == torch.float32 and np.array_equal(f32.cpu().numpy(), ref["bits"][:300].astype(np.float32))


def _call(plan, x, bs=None, num_iter=1, scale=1.0, flags=0, outs=(True, True, True, True), stream=None, dev=DEV):
    from polar_amd import _lib
    bs = x.shape[0] if bs is None else bs
    rows = max(x.shape[0], 1)
    bits = torch.empty((rows, max(plan.k, 1)), device=dev)
    soft = torch.empty((rows, max(plan.k, 1)), device=dev)
    ext = torch.empty((rows, plan.n), device=dev)
    its = torch.empty((rows,), dtype=torch.int32, device=dev)
    ptrs = [ctypes.c_void_p(t.data_ptr()) if on else None for t, on in zip((bits, soft, ext, its), outs)]
    st = stream if stream is not None else _lib.current_stream_ptr(torch.device(dev))
    rc = _lib.lib().pl_bp_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), bs, num_iter, scale, flags, ptrs[0],
                                 _lib.PL_OUT_F32, ptrs[1], ptrs[2], ptrs[3], st)
    torch.cuda.synchronize()
    return rc, _lib.lib().pl_last_error_string().decode()


def test_argument_checks():
    from polar_amd import _lib
    fp = bp_ref.rate_half_frozen(64, 1)
    ms, ex = _plan(64, fp), _plan(64, fp, 1)
    x = torch.zeros((4, 64), device=DEV)
    assert _call(ms, x)[0] == _lib.PL_OK
    assert _call(ms, x, bs=0)[0] == _lib.PL_OK
    assert _call(ms, x, scale=0.5, flags=_lib.PL_BP_EARLY_STOP)[0] == _lib.PL_OK
    for kw, word in ((dict(num_iter=0), "num_iter"), (dict(scale=0.0), "scale"), (dict(scale=1.5), "scale"),
                     (dict(scale=float("nan")), "scale"), (dict(outs=(False,) * 4), "NULL"), (dict(bs=-1), "bs")):
        rc, msg = _call(ms, x, **kw)
        assert rc == _lib.PL_EINVAL and word in msg, (kw, rc, msg)
    rc, msg = _call(ex, x, scale=0.5)
    assert rc == _lib.PL_EINVAL and "scale" in msg, msg
    rc, msg = _call(_plan(64, fp, list_size=2), x)
    assert rc == _lib.PL_EINVAL and "plan" in msg, msg
    fp2k = bp_ref.rate_half_frozen(2048, 1)
    rc, msg = _call(_plan(2048, fp2k), torch.zeros((2, 2048), device=DEV))
    assert rc == _lib.PL_ENOTSUP and "2048" in msg, msg


def test_other_devices_stream_is_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from polar_amd import _lib
    plan = _plan(64, bp_ref.rate_half_frozen(64, 1))
    x = torch.zeros((4, 64), device="cuda:1")
    with torch.cuda.device(1):
        rc, msg = _call(plan, x, stream=_lib.current_stream_ptr(torch.device("cuda:1")), dev="cuda:1")
    assert rc == _lib.PL_EINVAL and "device" in msg, msg


def test_module():
    import polar_amd
    n = 64
    fp = polar_amd.reference_frozen_pos(32, n)
    x = bp_ref.early_stop_inputs(n, fp.numpy())[:40].reshape(2, 20, n)
    ref = bp_ref.bp_decode(x.reshape(-1, n), fp.numpy(), n, 10, 19.3, early_stop=True)
    dec = polar_amd.BP_Dec(fp, n, num_iter=10, f="minsum", early_stop=True, return_ext=True)
    xc = torch.as_tensor(x)  # a CPU tensor goes in and comes out
    bits = dec(xc)
    assert bits.shape == (2, 20, 32) and bits.device.type == "cpu" and bits.dtype == torch.float32
    assert np.array_equal(bits.numpy().reshape(-1, 32), ref["bits"].astype(np.float32))
    assert dec.last_iters.shape == (2, 20) and np.array_equal(dec.last_iters.numpy().reshape(-1), ref["iters"])
    assert dec.last_ext.shape == (2, 20, n) and np.array_equal(dec.last_ext.numpy().reshape(-1, n), ref["ext_x"])
    soft = polar_amd.BP_Dec(fp, n, num_iter=10, hard_out=False, f="minsum", early_stop=True, device=DEV)
    s = soft(xc.to(DEV))
    assert s.device.type == "cuda" and soft.last_ext is None
    assert np.array_equal(s.cpu().numpy().reshape(-1, 32), ref["soft_u"])
    assert np.array_equal((~(-s.cpu().numpy() > 0)).astype(np.float32), bits.numpy())
    # the default f is the exact one: its hard decisions on the noiseless rows are the sent bits
    exact = polar_amd.BP_Dec(fp, n, num_iter=2)
    assert np.array_equal(exact(xc[:1, :6]).numpy(), bits.numpy()[:1, :6])
    with pytest.raises(ValueError):
        polar_amd.BP_Dec(np.arange(1024), 2048)
    with pytest.raises(ValueError):
        polar_amd.BP_Dec(fp, n, f="exact", scale=0.5)
