"""pl_scan_decode / ops.scan_decode / SCAN_Dec on the GPU against the numpy restatement (tests/golden/scan_ref.py,
itself checked by tests/test_scan_ref.py): bits, soft_u, ext_x and iters value for value (np.array_equal:
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
import scan_ref  # noqa: E402

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
    r = ops.scan_decode(plan, x, num_iter, out_dtype=torch.uint8, soft=True, ext=True, iters=True, **kw)
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


@pytest.mark.parametrize("n,k", scan_ref.MINSUM_CODES)
def test_minsum_equals_the_restatement(n, k):
    """67 rows (a wave or work-group ends in a partial set of codewords; the first four are all-zero, +-lmax,
    beyond lmax and noiseless), a seeded rate-1/2 frozen set (at n = 64 also k = n and k = 1), 1, 2 and 3
    iterations: every size of both kernels (n <= 64 in registers, n >= 128 over LDS)."""
    fp = scan_ref.rate_half_frozen(n, 40 + n, k)
    _, x = scan_ref.make_inputs(60 + n + (k or 0), n, fp, scan_ref.MINSUM_ROWS)
    plan = _plan(n, fp)
    for num_iter in scan_ref.MINSUM_ITERS:
        ref = scan_ref.scan_decode(x, fp, n, num_iter, 19.3)
        _assert_equal(_run(plan, x, num_iter), ref, what=f"n={n} k={k} iters={num_iter}")


@pytest.mark.parametrize("n", scan_ref.SCALED_SIZES)
def test_scaled_minsum(n):
    fp = scan_ref.rate_half_frozen(n, 40 + n)
    _, x = scan_ref.make_inputs(80 + n, n, fp, 67)
    ref = scan_ref.scan_decode(x, fp, n, 3, 19.3, scale=scan_ref.SCALE)
    assert not np.array_equal(ref["soft_u"], scan_ref.scan_decode(x, fp, n, 3, 19.3)["soft_u"])
    _assert_equal(_run(_plan(n, fp), x, 3, scale=scan_ref.SCALE), ref, what=f"n={n} scale={scan_ref.SCALE}")


@pytest.mark.parametrize("n,num_iter,llr_max", scan_ref.SCAN_EXACT_CASES)
def test_exact_f_equals_the_restatement(n, num_iter, llr_max):
    """128 rows (32 at n = 2048); llr_max 60 (n = 4) takes the full-range forms of the exact f.  Every
    non-fragile row is equal."""
    fp, x = scan_ref.exact_case_inputs(n, num_iter, llr_max)
    ref = scan_ref.scan_decode(x, fp, n, num_iter, llr_max, exact=True)
    print(f"n={n} iters={num_iter} llr_max={llr_max}: fragile rows {int(ref['fragile'].sum())}")
    assert ref["fragile"].sum() <= scan_ref.FRAGILE_CAP
    got = _run(_plan(n, fp, 1, llr_max), x, num_iter)
    _assert_equal(got, ref, keep=~ref["fragile"], what=f"exact n={n} iters={num_iter} llr_max={llr_max}")


@pytest.mark.parametrize("n", scan_ref.EARLY_STOP_SIZES)
def test_early_stop(n):
    """Noiseless, noisy and pure-noise rows, 6 iterations: rows stop after 1, after 2 ... 5 and never (n = 2: all
    after 1; n = 1024, 2048: after 1 and never), asserted before the comparison."""
    fp = scan_ref.rate_half_frozen(n, scan_ref.EARLY_STOP_FROZEN_SEED)
    x = scan_ref.early_stop_inputs(n, fp)
    iters = scan_ref.EARLY_STOP_ITERS
    ref = scan_ref.scan_decode(x, fp, n, iters, 19.3, early_stop=True)
    it = ref["iters"]
    print(f"n={n}: iters {it.tolist()}")
    one, few, never = scan_ref.early_stop_classes(n)
    assert (it == 1).any() == one and ((it > 1) & (it < iters)).any() == few and (it == iters).any() == never
    _assert_equal(_run(_plan(n, fp), x, iters, early_stop=True), ref, what=f"early stop n={n}")
    off = _run(_plan(n, fp), x, iters)  # the flag off: every row runs them all
    assert np.array_equal(off["iters"], np.full(len(x), iters, dtype=np.int32))


@pytest.mark.parametrize("n", [64, 256])
def test_early_stop_exact(n):
    fp = scan_ref.rate_half_frozen(n, scan_ref.EARLY_STOP_FROZEN_SEED)
    x = scan_ref.early_stop_inputs(n, fp)
    ref = scan_ref.scan_decode(x, fp, n, scan_ref.EARLY_STOP_ITERS, 19.3, exact=True, early_stop=True)
    print(f"n={n} exact: iters {ref['iters'].tolist()}, fragile rows {int(ref['fragile'].sum())}")
    assert ref["fragile"].sum() <= scan_ref.FRAGILE_CAP
    got = _run(_plan(n, fp, 1), x, scan_ref.EARLY_STOP_ITERS, early_stop=True)
    _assert_equal(got, ref, keep=~ref["fragile"], what=f"early stop exact n={n}")


def test_batch_edges_and_optional_outputs():
    from polar_amd import ops
    n = 8
    fp = scan_ref.rate_half_frozen(n, 3)
    plan = _plan(n, fp)
    rng = np.random.default_rng(11)
    _, x = scan_ref.awgn_logits(rng, fp, n, 70001)  # 32 codewords a work-group: 2188 groups, past the 1024-block cap
    ref = scan_ref.scan_decode(x, fp, n, 2, 19.3)
    _assert_equal(_run(plan, x, 2), ref, what="bs=70001")
    es = scan_ref.scan_decode(x, fp, n, 4, 19.3, early_stop=True)
    assert len(set(es["iters"].tolist())) >= 3
    _assert_equal(_run(plan, x, 4, early_stop=True), es, what="bs=70001 early stop")
    one = _run(plan, x[5:6], 2)
    _assert_equal(one, {k: ref[k][5:6] for k in KEYS}, what="bs=1")
    empty = _run(plan, x[:0], 2)
    assert empty["bits"].shape == (0, 4) and empty["ext_x"].shape == (0, 8) and empty["iters"].shape == (0,)
    # each output alone equals its value in the full call
    xt = torch.as_tensor(x[:300], device=DEV)
    for key, kw in (("bits", dict(hard=True)), ("soft_u", dict(hard=False, soft=True)),
                    ("ext_x", dict(hard=False, ext=True)), ("iters", dict(hard=False, iters=True))):
        r = ops.scan_decode(plan, xt, 2, out_dtype=torch.uint8, **kw)
        assert list(r) == [key] and np.array_equal(r[key].cpu().numpy(), ref[key][:300]), key
    f32 = ops.scan_decode(plan, xt, 2)["bits"]
    assert f32.dtype == torch.float32 and np.array_equal(f32.cpu().numpy(), ref["bits"][:300].astype(np.float32))
    # one codeword a work-group (n >= 128): each output alone
    n = 128
    fp = scan_ref.rate_half_frozen(n, 3)
    _, x = scan_ref.awgn_logits(rng, fp, n, 9)
    ref = scan_ref.scan_decode(x, fp, n, 2, 19.3)
    xt = torch.as_tensor(x, device=DEV)
    for key, kw in (("bits", dict(hard=True)), ("soft_u", dict(hard=False, soft=True)),
                    ("ext_x", dict(hard=False, ext=True)), ("iters", dict(hard=False, iters=True))):
        r = ops.scan_decode(_plan(n, fp), xt, 2, out_dtype=torch.uint8, **kw)
        assert list(r) == [key] and np.array_equal(r[key].cpu().numpy(), ref[key]), key


def test_one_wave_groups_past_the_grid():
    """n = 128 (one codeword a work-group, as many work-groups as the device holds at once -- at most a few thousand):
    8209 rows send every work-group round the grid stride more than once, the last round ragged; with early stop, so
    the rows of a work-group end after different numbers of iterations."""
    n, rows = 128, 8209
    fp = scan_ref.rate_half_frozen(n, scan_ref.EARLY_STOP_FROZEN_SEED)
    base = scan_ref.early_stop_inputs(n, fp)
    x = base[np.random.default_rng(128).integers(0, len(base), rows)]
    ref = scan_ref.scan_decode(x, fp, n, 3, 19.3, early_stop=True)
    print("iters histogram:", np.bincount(ref["iters"], minlength=4).tolist())
    assert len(set(ref["iters"].tolist())) == 3
    _assert_equal(_run(_plan(n, fp), x, 3, early_stop=True), ref, what="n=128 past the grid")


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
    rc = _lib.lib().pl_scan_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), bs, num_iter, scale, flags, ptrs[0],
                                   _lib.PL_OUT_F32, ptrs[1], ptrs[2], ptrs[3], st)
    torch.cuda.synchronize()
    return rc, _lib.lib().pl_last_error_string().decode()


def test_argument_checks():
    from polar_amd import _lib
    fp = scan_ref.rate_half_frozen(64, 1)
    ms, ex = _plan(64, fp), _plan(64, fp, 1)
    x = torch.zeros((4, 64), device=DEV)
    assert _call(ms, x)[0] == _lib.PL_OK
    assert _call(ms, x, bs=0)[0] == _lib.PL_OK
    assert _call(ms, x, scale=0.5, flags=_lib.PL_SCAN_EARLY_STOP)[0] == _lib.PL_OK
    for kw, word in ((dict(num_iter=0), "num_iter"), (dict(scale=0.0), "scale"), (dict(scale=1.5), "scale"),
                     (dict(scale=float("nan")), "scale"), (dict(outs=(False,) * 4), "NULL"), (dict(bs=-1), "bs"),
                     (dict(flags=2), "flags")):
        rc, msg = _call(ms, x, **kw)
        assert rc == _lib.PL_EINVAL and word in msg, (kw, rc, msg)
    rc, msg = _call(ex, x, scale=0.5)
    assert rc == _lib.PL_EINVAL and "scale" in msg, msg
    rc, msg = _call(_plan(64, fp, list_size=2), x)
    assert rc == _lib.PL_EINVAL and "plan" in msg, msg
    fp2k = scan_ref.rate_half_frozen(2048, 1)
    rc, msg = _call(_plan(2048, fp2k), torch.zeros((2, 2048), device=DEV))
    assert rc == _lib.PL_OK, msg


def test_other_devices_stream_is_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from polar_amd import _lib
    plan = _plan(64, scan_ref.rate_half_frozen(64, 1))
    x = torch.zeros((4, 64), device="cuda:1")
    with torch.cuda.device(1):
        rc, msg = _call(plan, x, stream=_lib.current_stream_ptr(torch.device("cuda:1")), dev="cuda:1")
    assert rc == _lib.PL_EINVAL and "device" in msg, msg


def test_graph_capture():
    """One capture on a single stream at n = 64, replayed twice (the second time on other inputs), equals eager."""
    from polar_amd import ops
    n = 64
    fp = scan_ref.rate_half_frozen(n, scan_ref.EARLY_STOP_FROZEN_SEED)
    xa = scan_ref.early_stop_inputs(n, fp)
    xb = np.ascontiguousarray(xa[::-1])
    plan = _plan(n, fp)
    x = torch.as_tensor(xa, device=DEV)
    kw = dict(num_iter=3, early_stop=True, out_dtype=torch.uint8, soft=True, ext=True, iters=True)
    eager = {k: v.cpu().numpy() for k, v in ops.scan_decode(plan, x, **kw).items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.scan_decode(plan, x, **kw)
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.cpu().numpy() for k, v in out.items()}, eager, what="graph replay 1")
    x.copy_(torch.as_tensor(xb, device=DEV))
    g.replay()
    torch.cuda.synchronize()
    ref = scan_ref.scan_decode(xb, fp, n, 3, 19.3, early_stop=True)
    _assert_equal({k: v.cpu().numpy() for k, v in out.items()}, ref, what="graph replay 2")


def test_module():
    import polar_amd
    n = 64
    fp = polar_amd.reference_frozen_pos(32, n)
    x = scan_ref.early_stop_inputs(n, fp.numpy())[:40].reshape(2, 20, n)
    ref = scan_ref.scan_decode(x.reshape(-1, n), fp.numpy(), n, 4, 19.3, early_stop=True)
    dec = polar_amd.SCAN_Dec(fp, n, num_iter=4, f="minsum", early_stop=True, return_ext=True)
    xc = torch.as_tensor(x)  # a CPU tensor goes in and comes out
    bits = dec(xc)
    assert bits.shape == (2, 20, 32) and bits.device.type == "cpu" and bits.dtype == torch.float32
    assert np.array_equal(bits.numpy().reshape(-1, 32), ref["bits"].astype(np.float32))
    assert dec.last_iters.shape == (2, 20) and np.array_equal(dec.last_iters.numpy().reshape(-1), ref["iters"])
    assert dec.last_ext.shape == (2, 20, n) and np.array_equal(dec.last_ext.numpy().reshape(-1, n), ref["ext_x"])
    soft = polar_amd.SCAN_Dec(fp, n, num_iter=4, hard_out=False, f="minsum", early_stop=True, device=DEV)
    s = soft(xc.to(DEV))
    assert s.device.type == "cuda" and soft.last_ext is None
    assert np.array_equal(s.cpu().numpy().reshape(-1, 32), ref["soft_u"])
    assert np.array_equal((~(-s.cpu().numpy() > 0)).astype(np.float32), bits.numpy())
    # the default is two iterations of the exact f: its hard decisions on the noiseless rows are the sent bits
    exact = polar_amd.SCAN_Dec(fp, n)
    assert exact.num_iter == 2 and exact.f == "exact"
    assert np.array_equal(exact(xc[:1, :6]).numpy(), bits.numpy()[:1, :6])
    big = polar_amd.SCAN_Dec(np.arange(1024), 2048, f="minsum")  # n = 2048 constructs and decodes
    assert big(torch.full((1, 2048), -8.0)).shape == (1, 1024)
    with pytest.raises(ValueError):
        polar_amd.SCAN_Dec(np.arange(2048), 4096)
    with pytest.raises(ValueError):
        polar_amd.SCAN_Dec(fp, n, f="exact", scale=0.5)
    with pytest.raises(ValueError):
        polar_amd.SCAN_Dec(fp, n, num_iter=0)
    with pytest.raises(ValueError):
        polar_amd.SCAN_Dec(fp, n, f="bp")
