"""pl_ae_decode / ops.ae_decode / AE_Dec on the GPU against the numpy restatement (tests/golden/ae_ref.py,
itself checked by tests/test_ae_ref.py).

On the exact grid every f, g and metric sum is exact in fp32 in any order, so bits, best_idx (with the
lowest-index tie rule) and best_metric must equal the restatement exactly.  On AWGN rows the device's fp32
metric is a sum of n non-negative terms in an order of its own: its relative error is at most n 2^-24, so
the candidate it picks may differ from the fp64 minimum only among candidates within (1 + 3 n 2^-24) of it
(two sums off by n 2^-24 each way, with a second-order margin), and the bits must be that candidate's.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import ae_ref  # noqa: E402
import genie_ref  # noqa: E402
import scf_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _plan(n, fp, f_mode=0, llr_max=30.0, list_size=1):
    import polar_amd
    from polar_amd import _lib
    return _lib.Plan(n, polar_amd.frozen_mask(fp, n), list_size, f_mode, llr_max, flags=_lib.PL_PLAN_GENERIC, device=DEV)


def _run(plan, logits, table, out_dtype=torch.uint8):
    from polar_amd import ops
    x = torch.as_tensor(np.ascontiguousarray(logits, dtype=np.float32), device=DEV)
    bits, idx, met = ops.ae_decode(plan, x, ops.ae_perm_table(table, DEV), out_dtype=out_dtype, return_info=True)
    torch.cuda.synchronize()
    return {"bits": bits.cpu().numpy(), "best_idx": idx.cpu().numpy(), "best_metric": met.cpu().numpy()}


def _assert_exact(got, ref, what):
    bits, metric = ae_ref.winner(ref)
    for key, g, r in (("best_idx", got["best_idx"], ref["best_idx"]),
                      ("best_metric", got["best_metric"].view(np.uint32), metric.astype(np.float32).view(np.uint32)),
                      ("bits", got["bits"], bits.astype(got["bits"].dtype))):
        bad = np.flatnonzero((g != r).reshape(g.shape[0], -1).any(axis=1))
        print(f"{what} {key}: rows differing {len(bad)} of {g.shape[0]}")
        assert np.array_equal(g, r), (what, key, list(bad[:8]))


def _assert_within_rounding(got, ref, n, what, keep=None):
    rows = np.arange(len(got["best_idx"]))
    keep = np.ones(len(rows), dtype=bool) if keep is None else keep
    idx = got["best_idx"]
    assert ((idx >= 0) & (idx < ref["metric"].shape[0])).all(), what
    mine = ref["metric"][idx, rows]
    best = ref["metric"].min(axis=0)
    eps = n * 2.0 ** -24
    same_bits = (got["bits"] == ref["bits"][idx, rows]).all(axis=1)
    rel = np.abs(got["best_metric"].astype(np.float64) - mine) / np.maximum(mine, np.finfo(np.float64).tiny)
    print(f"{what}: rows {int(keep.sum())}, winner differs from the fp64 one in {int((idx != ref['best_idx'])[keep].sum())}, "
          f"max metric excess {float((mine / np.maximum(best, 1e-300))[keep].max() - 1):.3g} (bound {3 * eps:.3g}), "
          f"max best_metric error {float(rel[keep].max()):.3g} (bound {eps:.3g})")
    assert same_bits[keep].all(), (what, list(np.flatnonzero(~same_bits & keep)[:8]))
    assert (mine <= (1.0 + 3.0 * eps) * best)[keep].all(), what
    assert (np.abs(got["best_metric"].astype(np.float64) - mine) <= eps * mine)[keep].all(), what


@pytest.mark.parametrize("case", ae_ref.GRID_CASES, ids=lambda c: c[0])
def test_grid_cases_equal_the_restatement_exactly(case):
    fp, table, x = ae_ref.case_inputs(case)
    ref = ae_ref.ae_decode(x, fp, case[1], table)
    _assert_exact(_run(_plan(case[1], fp), x, table), ref, case[0])


def test_more_rows_than_the_grid():
    """n = 8, M = 3, 4136 rows of grid logits on a 4096-block grid: the second stride reuses s_a and s_x."""
    case, rows = ae_ref.PAST_GRID_CASE
    fp, table, x = ae_ref.case_inputs(case, rows)
    assert len(x) == rows > 4096
    ref = ae_ref.ae_decode(x, fp, case[1], table)
    _assert_exact(_run(_plan(case[1], fp), x, table), ref, case[0])


@pytest.mark.parametrize("case", ae_ref.AWGN_CASES, ids=lambda c: c[0])
def test_awgn_cases_within_the_rounding_of_the_metric(case):
    fp, table, x = ae_ref.case_inputs(case)
    ref = ae_ref.ae_decode(x, fp, case[1], table)
    _assert_within_rounding(_run(_plan(case[1], fp), x, table), ref, case[1], case[0])


@pytest.mark.parametrize("case", ae_ref.EXACT_CASES, ids=lambda c: c[0])
def test_exact_f_cases(case):
    fp, table, x = ae_ref.case_inputs(case)
    n, lmax = case[1], case[6]
    ref = ae_ref.ae_decode(x, fp, n, table, llr_max=lmax, exact=True)
    print(case[0], "fragile rows:", int(ref["fragile"].sum()))
    assert ref["fragile"].sum() <= ae_ref.FRAGILE_CAP
    _assert_within_rounding(_run(_plan(n, fp, 1, lmax), x, table), ref, n, case[0], keep=~ref["fragile"])


@pytest.mark.parametrize("spec", [(1024, "pin:512"), (256, "rand:5")], ids=["pinned_512_1024", "random_256"])
def test_one_identity_candidate_is_sc_dec(spec):
    """M = 1 with the identity is plain SC: bit for bit SC_Dec (min-sum) on 67 AWGN rows and the awkward rows
    (zeros, -0, integer ties, a saturated row)."""
    import polar_amd
    n, code = spec
    fp = ae_ref.frozen_of(code, n)
    _, x = ae_ref.awgn_rows(n + 1, fp, n, 67, 2.5)
    x = np.concatenate([x, genie_ref.special_llrs(np.random.default_rng(n), 12, n)])
    want = polar_amd.SC_Dec(torch.as_tensor(fp), n, device=DEV)(torch.as_tensor(x, device=DEV)).cpu().numpy()
    got = _run(_plan(n, fp), x, np.arange(n)[None, :])
    assert (got["best_idx"] == 0).all()
    bad = np.flatnonzero((got["bits"] != want).any(axis=1))
    print(spec, "rows differing from SC_Dec:", len(bad))
    assert np.array_equal(got["bits"], want.astype(np.uint8)), list(bad[:8])
    u, _, _ = scf_ref.sc_flip(x, fp, n, np.full(len(x), -1))
    assert np.array_equal(got["bits"], u[:, np.setdiff1d(np.arange(n), fp)])


def test_a_table_that_is_no_automorphism():
    """The contract is total: candidate 0 goes through a random permutation of the (32,64) code."""
    case = ae_ref.NON_AUTOMORPHISM_CASE
    fp, table, x = ae_ref.case_inputs(case)
    ref = ae_ref.ae_decode(x, fp, case[1], table)
    print("winners:", np.bincount(ref["best_idx"], minlength=2))
    _assert_exact(_run(_plan(case[1], fp), x, table), ref, case[0])


def _call(plan, x, table, m_tot=None, bs=None, kind=None, outs=(True, True), bufs=None):
    from polar_amd import _lib
    L = _lib.lib()
    kind = _lib.PL_OUT_U8 if kind is None else kind
    bs = x.shape[0] if bs is None else bs
    rows = max(x.shape[0], 1)
    if bufs is None:
        bufs = (torch.zeros((rows, max(plan.k, 1)), dtype=torch.uint8 if kind == _lib.PL_OUT_U8 else torch.float32,
                            device=DEV),
                torch.full((rows,), 7, dtype=torch.int32, device=DEV), torch.full((rows,), 7.0, device=DEV))
    bits, idx, met = bufs
    ptrs = [ctypes.c_void_p(t.data_ptr()) if on else None for t, on in zip((idx, met), outs)]
    rc = L.pl_ae_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), bs, ctypes.c_void_p(table.data_ptr()),
                        table.shape[0] if m_tot is None else m_tot, ctypes.c_void_p(bits.data_ptr()), kind, ptrs[0],
                        ptrs[1], _lib.current_stream_ptr(torch.device(DEV)))
    return rc, L.pl_last_error_string().decode(), bufs


def test_abi_optional_outputs_output_kinds_and_argument_checks():
    from polar_amd import _lib, ops
    case = next(c for c in ae_ref.GRID_CASES if c[0] == "g32")  # n = 32
    fp, table, x = ae_ref.case_inputs(case)
    n = case[1]
    ref = ae_ref.ae_decode(x, fp, n, table)
    bits, metric = ae_ref.winner(ref)
    plan = _plan(n, fp)
    xt, tt = torch.as_tensor(x, device=DEV), ops.ae_perm_table(table, DEV)
    for outs in ((True, True), (False, True), (True, False), (False, False)):  # best_idx / best_metric NULL
        rc, msg, (b, idx, met) = _call(plan, xt, tt, outs=outs)
        torch.cuda.synchronize()
        assert rc == _lib.PL_OK, msg
        assert np.array_equal(b.cpu().numpy(), bits)
        assert np.array_equal(idx.cpu().numpy(), ref["best_idx"] if outs[0] else np.full(len(x), 7))
        assert np.array_equal(met.cpu().numpy(), metric.astype(np.float32) if outs[1] else np.full(len(x), 7.0))
    f32 = _run(plan, x, table, out_dtype=torch.float32)
    assert f32["bits"].dtype == np.float32
    _assert_exact(f32, ref, "PL_OUT_F32")
    out = torch.full((len(x), plan.k), 9, dtype=torch.uint8, device=DEV)
    back = ops.ae_decode(plan, xt, tt, out=out)
    torch.cuda.synchronize()
    assert back is out and np.array_equal(out.cpu().numpy(), bits)
    empty = _run(plan, x[:0], table)  # bs = 0
    assert empty["bits"].shape == (0, plan.k) and empty["best_idx"].shape == (0,)
    assert _call(plan, xt, tt, bs=0)[0] == _lib.PL_OK
    for kw, word in ((dict(m_tot=0), "num_perms"), (dict(m_tot=65), "num_perms"), (dict(bs=-1), "bs"),
                     (dict(kind=5), "out_kind")):
        rc, msg, _ = _call(plan, xt, tt, **kw)
        assert rc == _lib.PL_EINVAL and word in msg, (kw, rc, msg)
    rc, msg, _ = _call(_plan(n, fp, list_size=2), xt, tt)
    assert rc == _lib.PL_EINVAL and "plan" in msg, msg
    fp2k = scf_ref.rate_half_frozen(2048, 1)
    t2k = torch.zeros((1, 2048), dtype=torch.int16, device=DEV)
    rc, msg, _ = _call(_plan(2048, fp2k), torch.zeros((2, 2048), device=DEV), t2k)
    assert rc == _lib.PL_ENOTSUP and "2048" in msg, msg
    torch.cuda.synchronize()


def test_hip_graph_capture_and_replay():
    """One call captured into a HIP graph on a single stream and replayed once on inputs written into the same
    buffers afterwards: the replay equals the eager call."""
    from polar_amd import _lib, ops
    case = next(c for c in ae_ref.GRID_CASES if c[0] == "g256_m33")  # n = 256, M = 33: two passes
    fp, table, x = ae_ref.case_inputs(case)
    n = case[1]
    plan = _plan(n, fp)
    xt, tt = torch.zeros((len(x), n), device=DEV), ops.ae_perm_table(table, DEV)
    _, _, bufs = _call(plan, xt, tt)
    rcs = []
    graph = ops.LaunchGraph(lambda: rcs.append(_call(plan, xt, tt, bufs=bufs)[0]), 1, device=DEV)
    assert rcs and all(rc == _lib.PL_OK for rc in rcs)
    xt.copy_(torch.as_tensor(x))
    bufs[0].fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    got = {"bits": bufs[0].cpu().numpy(), "best_idx": bufs[1].cpu().numpy(), "best_metric": bufs[2].cpu().numpy()}
    eager = _run(plan, x, table)
    for key in got:
        assert np.array_equal(got[key], eager[key]), key
    _assert_exact(got, ae_ref.ae_decode(x, fp, n, table), "replay")


def test_module():
    import polar_amd
    case = next(c for c in ae_ref.GRID_CASES if c[0] == "g32")  # n = 32, RM(2,5), M = 8
    fp, table, x = ae_ref.case_inputs(case)
    n = case[1]
    x = x[:15].reshape(3, 5, n)
    ref = ae_ref.ae_decode(x.reshape(-1, n), fp, n, table)
    bits, metric = ae_ref.winner(ref)
    dec = polar_amd.AE_Dec(torch.as_tensor(fp), n, perms=table, return_metric=True)
    xc = torch.as_tensor(x)  # a CPU tensor goes in and comes out
    u_hat, met = dec(xc)
    assert u_hat.shape == (3, 5, 16) and u_hat.device.type == "cpu" and u_hat.dtype == torch.float32
    assert np.array_equal(u_hat.numpy().reshape(-1, 16), bits.astype(np.float32))
    assert met.shape == (3, 5) and np.array_equal(met.numpy().reshape(-1), metric.astype(np.float32))
    assert dec.last_best_idx.shape == (3, 5) and np.array_equal(dec.last_best_idx.numpy().reshape(-1), ref["best_idx"])
    assert dec.last_metric is met
    gpu = polar_amd.AE_Dec(fp, n, num_perms=8, kind="stage", device=DEV)  # its own tables
    b2 = gpu(xc.to(DEV))
    assert b2.device.type == "cuda" and b2.shape == (3, 5, 16) and gpu.last_best_idx.device.type == "cuda"
    own = ae_ref.ae_decode(x.reshape(-1, n), fp, n, gpu.perms)
    assert np.array_equal(b2.cpu().numpy().reshape(-1, 16), ae_ref.winner(own)[0].astype(np.float32))
    lin = polar_amd.AE_Dec(fp, n, num_perms=8, kind="linear", f="exact", device=DEV)
    assert lin(xc).shape == (3, 5, 16)


def test_end_to_end_rm_3_7_gains_a_decade_over_sc():
    """RM(3,7) = (64,128), seeded AWGN at 3 dB, 4096 rows: AE-32 (stage permutations, min-sum) makes at most a
    tenth of SC_Dec's block errors on the same rows (a CPU probe with the restatement gives about a hundredth)."""
    import polar_amd
    n = 128
    k, fp = polar_amd.automorphism.rm_code(3, 7)
    sent, x = ae_ref.awgn_rows(2024, fp, n, 4096, 3.0)
    xt = torch.as_tensor(x, device=DEV)
    sc = polar_amd.SC_Dec(torch.as_tensor(fp), n, device=DEV)(xt).cpu().numpy()
    ae = polar_amd.AE_Dec(fp, n, num_perms=32, kind="stage", f="minsum", device=DEV)(xt).cpu().numpy()
    err_sc = int((sc != sent).any(axis=1).sum())
    err_ae = int((ae != sent).any(axis=1).sum())
    print("block errors of 4096: SC", err_sc, "AE-32", err_ae)
    assert err_sc >= 100
    assert 10 * err_ae <= err_sc
