"""pl_scf_decode / ops.scf_decode / SCF_Dec on the GPU against the numpy restatement (tests/golden/scf_ref.py,
itself checked by tests/test_scf_ref.py): bits, crc_ok, flip_pos and attempts value for value; with the
exact f, rows flagged fragile by the correctly rounded restatement are left out, and their number is
capped before the comparison.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import genie_ref  # noqa: E402
import scf_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _case(name):
    return next(c for c in scf_ref.MINSUM_CASES if c[0] == name)
DEV = "cuda:0"
KEYS = ("bits", "crc_ok", "flip_pos", "attempts")


def _plan(n, fp, crc, f_mode=0, llr_max=30.0, list_size=1, flags=None):
    import polar_amd
    from polar_amd import _lib
    flags = _lib.PL_PLAN_GENERIC if flags is None else flags
    p = _lib.Plan(n, polar_amd.frozen_mask(fp, n), list_size, f_mode, llr_max, flags=flags, device=DEV)
    if crc is not None:
        p.set_crc(*crc)
    return p


def _run(plan, logits, max_flips, out_dtype=torch.uint8):
    from polar_amd import ops
    x = torch.as_tensor(np.ascontiguousarray(logits, dtype=np.float32), device=DEV)
    bits, ok, pos, att = ops.scf_decode(plan, x, max_flips, out_dtype=out_dtype, return_info=True)
    torch.cuda.synchronize()
    return {"bits": bits.cpu().numpy(), "crc_ok": ok.cpu().numpy(), "flip_pos": pos.cpu().numpy(),
            "attempts": att.cpu().numpy()}


def _assert_equal(got, ref, keep=None, what=""):
    for key in KEYS:
        g, r = got[key], ref[key]
        if keep is not None:
            g, r = g[keep], r[keep]
        bad = np.flatnonzero((g != r).reshape(g.shape[0], -1).any(axis=1)) if g.size else []
        print(f"{what} {key}: rows differing {len(bad)} of {g.shape[0]}")
        assert np.array_equal(g, r), (what, key, list(bad[:8]))


@pytest.mark.parametrize("case", scf_ref.MINSUM_CASES, ids=[c[0] for c in scf_ref.MINSUM_CASES])
def test_minsum_equals_the_restatement(case):
    """n = 8 ... 1024, 67 rows (the last four the awkward ones: zeros, -0, integer ties, a saturated row)."""
    fp, crc, x = scf_ref.case_inputs(case)
    n, T = case[1], case[4]
    ref = scf_ref.scf_decode(x, fp, n, crc, T)
    _assert_equal(_run(_plan(n, fp, crc), x, T), ref, what=case[0])


@pytest.mark.parametrize("case", scf_ref.EXACT_CASES, ids=[c[0] for c in scf_ref.EXACT_CASES])
def test_exact_f_equals_the_restatement(case):
    fp, crc, x = scf_ref.case_inputs(case)
    n, T, lmax = case[1], case[4], case[6]
    ref = scf_ref.scf_decode(x, fp, n, crc, T, llr_max=lmax, exact=True)
    print(case[0], "fragile rows:", int(ref["fragile"].sum()))
    assert ref["fragile"].sum() <= scf_ref.FRAGILE_CAP
    _assert_equal(_run(_plan(n, fp, crc, 1, lmax), x, T), ref, keep=~ref["fragile"], what=case[0])


@pytest.mark.parametrize("n", [2, 4])
def test_n2_and_n4_every_frozen_pattern(n):
    """The two shortest lengths of the flip kernel (n = 2 is its bottom-only root).  pl_plan_set_crc takes no
    degree above k, so the smallest pinned CRC (CRC6) is refused for every pattern: that is checked by return
    code and message, and the patterns run on x + 1 and, from k = 3, x^3 + x + 1, with T = k, on every row of a
    small integer grid (zeros and ties in (|alpha|, i) in most rows)."""
    import polar_amd
    from polar_amd import _lib
    x = scf_ref.tiny_rows(n)
    cases = scf_ref.tiny_cases(n)
    assert len(cases) >= (1 << n) - 1
    for name, fp, crc_name, T in cases:
        plan = _plan(n, fp, None)
        rc = _lib.lib().pl_plan_set_crc(plan.handle, *scf_ref.crc_params("CRC6"))
        assert rc == _lib.PL_EINVAL and b"pl_plan_set_crc" in _lib.lib().pl_last_error_string(), name
        crc = scf_ref.crc_params(crc_name)
        ref = scf_ref.scf_decode(x, fp, n, crc, T)
        assert (ref["attempts"] > 1).any() and (ref["flip_pos"] >= 0).any(), name
        _assert_equal(_run(_plan(n, fp, crc), x, T), ref, what=name)


@pytest.mark.parametrize("case", scf_ref.CRC_TABLE_CASES, ids=[c[0] for c in scf_ref.CRC_TABLE_CASES])
def test_in_kernel_crc_table(case):
    """k = 1024 (the maximum), k just above a power of two, and k = 63 where the doubling loop must not run: 8
    rows whose only wrong decision is u_0 (rank 0, the one reader of the table's last entry; u_0 = 1 in four of
    them) and which the first flip must rescue through a CRC over all k bits, and 8 rows of noise."""
    fp, crc, x, sent = scf_ref.crc_table_inputs(case)
    n, T = case[1], scf_ref.CRC_TABLE_FLIPS
    ref = scf_ref.scf_decode(x, fp, n, crc, T)
    won = ref["flip_pos"] >= 0
    assert (ref["attempts"] > 1).all() and won[:8].all() and np.array_equal(ref["bits"][:8], sent)
    assert (ref["bits"][won, 0] == 1).any() and (ref["bits"][won, 0] == 0).any() and (~ref["crc_ok"]).any()
    _assert_equal(_run(_plan(n, fp, crc), x, T), ref, what=case[0])


def test_awkward_llrs():
    """Rows of zeros, -0, integer ties and a saturated row only: the (|alpha|, i) order and HD(+-0)."""
    for n, spec, crc_name, T in ((16, "half:16", "CRC6", 8), (64, "ref", "CRC11", 16), (256, "ref", "CRC24C", 64)):
        fp, crc = scf_ref.frozen_of(spec, n), scf_ref.crc_params(crc_name)
        x = genie_ref.special_llrs(np.random.default_rng(n), 48, n)
        ref = scf_ref.scf_decode(x, fp, n, crc, T)
        print(n, "rescued", int((ref["flip_pos"] >= 0).sum()), "never", int((~ref["crc_ok"]).sum()))
        _assert_equal(_run(_plan(n, fp, crc), x, T), ref, what=f"special n={n}")


def test_max_flips_0_is_sc_plus_crc_status_and_first_pass_rows_are_sc_rows():
    from polar_amd import _lib, ops
    case = _case("n32")  # n = 32, the reference set: its specialised min-sum kernel is pre-built
    fp, crc, x = scf_ref.case_inputs(case)
    xt = torch.as_tensor(x, device=DEV)
    for flags in (_lib.PL_PLAN_GENERIC, _lib.PL_PLAN_CACHE_ONLY):
        plan = _plan(32, fp, crc, flags=flags)
        print("kernel:", plan.kernel()[0])
        sc = ops.sc_decode(plan, xt, out_dtype=torch.uint8)
        ok = ops.crc_status(plan, sc)
        r0 = _run(plan, x, 0)
        assert np.array_equal(r0["bits"], sc.cpu().numpy()) and np.array_equal(r0["crc_ok"], ok.cpu().numpy())
        assert (r0["flip_pos"] == -1).all() and (r0["attempts"] == 1).all()
        r = _run(plan, x, case[4])
        first = r["attempts"] == 1
        assert first.any() and np.array_equal(first, ok.cpu().numpy())
        assert np.array_equal(r["bits"][first], sc.cpu().numpy()[first])
        _assert_equal(r, scf_ref.scf_decode(x, fp, 32, crc, case[4]), what=f"flags={flags}")
    assert plan.kernel()[0] == "specialized"


def test_flip_positions_first_last_and_position_0():
    """n = 16, k = 12, CRC6, every information position a candidate, 4000 rows of pure noise: a random attempt
    passes one time in 64, so the winning flips spread over all positions -- the first and the last information
    position among them.  And a k = n code whose only wrong decision is at position 0."""
    n, T = 16, 12
    fp, crc = scf_ref.rate_half_frozen(n, 3, k=12), scf_ref.crc_params("CRC6")
    info = np.setdiff1d(np.arange(n), fp)
    x = (np.random.default_rng(11).standard_normal((4000, n)) * 3).astype(np.float32)
    ref = scf_ref.scf_decode(x, fp, n, crc, T)
    assert (ref["flip_pos"] == info[0]).any() and (ref["flip_pos"] == info[-1]).any()
    _assert_equal(_run(_plan(n, fp, crc), x, T), ref, what="noise n=16")
    # k = n = 64: a codeword at +-8 with channel position 0 weakly wrong -> only u_0 is wrong, and it is the
    # least reliable decision
    n, crc = 64, scf_ref.crc_params("CRC11")
    bits, _ = scf_ref.awgn_rows(5, np.zeros(0, dtype=np.int64), n, crc, 6, 3.0)
    cw = scf_ref.encode(bits)
    x = ((2.0 * cw - 1.0) * 8.0).astype(np.float32)
    x[:, 0] = -x[:, 0] / 16.0
    ref = scf_ref.scf_decode(x, np.zeros(0, dtype=np.int64), n, crc, 1)
    assert (ref["flip_pos"] == 0).all() and np.array_equal(ref["bits"], bits)
    _assert_equal(_run(_plan(n, [], crc), x, 1), ref, what="position 0")


def test_batch_edges():
    n, T = 256, 16
    fp, crc = scf_ref.frozen_of("ref", n), scf_ref.crc_params("CRC24C")
    plan = _plan(n, fp, crc)
    noise = (np.random.default_rng(1).standard_normal((300, n)) * 2).astype(np.float32)
    ref = scf_ref.scf_decode(noise, fp, n, crc, T)
    assert not ref["crc_ok"].any() and (ref["attempts"] == 1 + T).all()  # every row fails
    _assert_equal(_run(plan, noise, T), ref, what="all fail")
    bits, _ = scf_ref.awgn_rows(2, fp, n, crc, 70, 3.0)
    u = np.zeros((70, n), dtype=np.uint8)
    u[:, np.setdiff1d(np.arange(n), fp)] = bits
    clean = ((2.0 * scf_ref.encode(u) - 1.0) * 8.0).astype(np.float32)
    got = _run(plan, clean, T)  # no row fails
    assert np.array_equal(got["bits"], bits) and got["crc_ok"].all() and (got["attempts"] == 1).all()
    assert (got["flip_pos"] == -1).all()
    one = _run(plan, noise[:1], T)  # bs = 1
    _assert_equal(one, {k: ref[k][:1] for k in KEYS}, what="bs=1")
    empty = _run(plan, noise[:0], T)  # bs = 0
    assert empty["bits"].shape == (0, n // 2) and empty["attempts"].shape == (0,)


def test_batch_past_the_grid_cap():
    """bs = 70001 at n = 8: more rows than any grid of the two stages, about a quarter of them failing."""
    n, T, bs = 8, 3, 70001
    fp, crc = np.zeros(0, dtype=np.int64), scf_ref.crc_params("CRC6")
    _, x = scf_ref.awgn_rows(8, fp, n, crc, bs, 4.0)
    ref = scf_ref.scf_decode(x, fp, n, crc, T)
    print("fail at 0:", int((ref["attempts"] > 1).sum()), "rescued:", int((ref["flip_pos"] >= 0).sum()))
    assert (ref["attempts"] > 1).sum() > 4096
    _assert_equal(_run(_plan(n, fp, crc), x, T), ref, what="bs=70001")


def _call(plan, x, max_flips, bs=None, kind=None, outs=(True, True, True), bufs=None, ws="ok", llr=True, out=True):
    from polar_amd import _lib
    L = _lib.lib()
    kind = _lib.PL_OUT_U8 if kind is None else kind
    bs = x.shape[0] if bs is None else bs
    rows = max(x.shape[0], 1)
    if bufs is None:
        bufs = (torch.zeros((rows, max(plan.k, 1)), dtype=torch.uint8 if kind == _lib.PL_OUT_U8 else torch.float32,
                            device=DEV),
                torch.full((rows,), 7, dtype=torch.uint8, device=DEV),
                torch.full((rows,), 7, dtype=torch.int32, device=DEV),
                torch.full((rows,), 7, dtype=torch.int32, device=DEV),
                torch.empty((max(int(L.pl_scf_workspace_size(plan.handle, rows, 0)), 1),), dtype=torch.uint8, device=DEV))
    bits, ok, pos, att, wsb = bufs
    need = int(L.pl_scf_workspace_size(plan.handle, max(bs, 0), 0))
    ws_ptr, ws_bytes = {"ok": (ctypes.c_void_p(wsb.data_ptr()), wsb.numel()), "null": (None, need),
                        "short": (ctypes.c_void_p(wsb.data_ptr()), max(need - 1, 0))}[ws]
    ptrs = [ctypes.c_void_p(t.data_ptr()) if on else None for t, on in zip((ok, pos, att), outs)]
    rc = L.pl_scf_decode(plan.handle, ctypes.c_void_p(x.data_ptr()) if llr else None, bs, max_flips,
                         ctypes.c_void_p(bits.data_ptr()) if out else None, kind, ptrs[0], ptrs[1], ptrs[2], ws_ptr,
                         ws_bytes, _lib.current_stream_ptr(torch.device(DEV)))
    return rc, L.pl_last_error_string().decode(), bufs


def test_optional_outputs_output_kinds_and_out_reuse():
    from polar_amd import _lib, ops
    case = _case("n64")  # n = 64
    fp, crc, x = scf_ref.case_inputs(case)
    n, T = 64, case[4]
    ref = scf_ref.scf_decode(x, fp, n, crc, T)
    plan = _plan(n, fp, crc)
    xt = torch.as_tensor(x, device=DEV)
    for skip in range(3):
        outs = tuple(i != skip for i in range(3))
        rc, msg, (bits, ok, pos, att, _) = _call(plan, xt, T, outs=outs)
        torch.cuda.synchronize()
        assert rc == _lib.PL_OK, msg
        assert np.array_equal(bits.cpu().numpy(), ref["bits"])
        for name, t, on in zip(("crc_ok", "flip_pos", "attempts"), (ok, pos, att), outs):
            want = ref[name].astype(t.cpu().numpy().dtype) if on else np.full(len(x), 7)
            assert np.array_equal(t.cpu().numpy(), want), (skip, name)
    f32 = _run(plan, x, T, out_dtype=torch.float32)
    assert f32["bits"].dtype == np.float32
    _assert_equal(f32, dict(ref, bits=ref["bits"].astype(np.float32)), what="PL_OUT_F32")
    out = torch.full((len(x), 32), 9, dtype=torch.uint8, device=DEV)
    back = ops.scf_decode(plan, xt, T, out=out)
    torch.cuda.synchronize()
    assert back is out and np.array_equal(out.cpu().numpy(), ref["bits"])


def test_argument_checks():
    from polar_amd import _lib
    fp = scf_ref.frozen_of("ref", 64)
    crc = scf_ref.crc_params("CRC11")
    plan = _plan(64, fp, crc)
    x = torch.zeros((4, 64), device=DEV)
    assert _call(plan, x, 4)[0] == _lib.PL_OK
    assert _call(plan, x, 4, bs=0)[0] == _lib.PL_OK
    assert _call(plan, x, 64)[0] == _lib.PL_OK  # above k = 32: behaves as k
    for kw, word in ((dict(max_flips=-1), "max_flips"), (dict(max_flips=65), "max_flips"), (dict(bs=-1), "bs"),
                     (dict(llr=False), "llr_logits"), (dict(out=False), "out_bits"), (dict(ws="null"), "workspace"),
                     (dict(ws="short"), "ws_bytes"), (dict(kind=5), "out_kind")):
        kw = dict(kw)
        rc, msg, _ = _call(plan, x, kw.pop("max_flips", 4), **kw)
        assert rc == _lib.PL_EINVAL and word in msg, (kw, rc, msg)
    rc, msg, _ = _call(_plan(64, fp, crc, list_size=2), x, 4)
    assert rc == _lib.PL_EINVAL and "plan" in msg, msg
    rc, msg, _ = _call(_plan(64, fp, None), x, 4)
    assert rc == _lib.PL_ENOTSUP and "CRC" in msg, msg
    fp2k = scf_ref.rate_half_frozen(2048, 1)
    rc, msg, _ = _call(_plan(2048, fp2k, crc), torch.zeros((2, 2048), device=DEV), 4)
    assert rc == _lib.PL_ENOTSUP and "2048" in msg, msg
    torch.cuda.synchronize()


def test_hip_graph_capture_and_replay():
    """The whole call -- SC, CRC flags, compaction, the flip kernel -- is captured into a HIP graph (a stream
    synchronisation inside it would fail the capture) and replayed on inputs written into the same buffers
    afterwards: the failing rows and their number are new, and the replay equals the eager call."""
    from polar_amd import _lib, ops
    case = _case("n256")  # n = 256, T = 16
    fp, crc, x = scf_ref.case_inputs(case)
    n, T = case[1], case[4]
    plan = _plan(n, fp, crc)
    xt = torch.zeros((len(x), n), device=DEV)
    _, _, bufs = _call(plan, xt, T)
    rcs = []
    graph = ops.LaunchGraph(lambda: rcs.append(_call(plan, xt, T, bufs=bufs)[0]), 1, device=DEV)
    assert rcs and all(rc == _lib.PL_OK for rc in rcs)
    _, x2 = scf_ref.awgn_rows(77, fp, n, crc, len(x), 2.0)
    for fresh in (x, x2):
        xt.copy_(torch.as_tensor(fresh))
        for t in bufs[:4]:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        got = {"bits": bufs[0].cpu().numpy(), "crc_ok": bufs[1].cpu().numpy() != 0, "flip_pos": bufs[2].cpu().numpy(),
               "attempts": bufs[3].cpu().numpy()}
        eager = _run(plan, fresh, T)
        _assert_equal(got, eager, what="replay vs eager")
        _assert_equal(got, scf_ref.scf_decode(fresh, fp, n, crc, T), what="replay vs restatement")


def test_module():
    import polar_amd
    n = 64
    fp = polar_amd.reference_frozen_pos(32, n)
    case = _case("n64")
    _, crc, x = scf_ref.case_inputs(case)
    x = x[:60].reshape(3, 20, n)
    ref = scf_ref.scf_decode(x.reshape(-1, n), fp.numpy(), n, crc, 16)
    dec = polar_amd.SCF_Dec(fp, n, "CRC11", max_flips=16, f="minsum", return_crc_status=True)
    xc = torch.as_tensor(x)  # a CPU tensor goes in and comes out
    bits, ok = dec(xc)
    assert bits.shape == (3, 20, 32) and bits.device.type == "cpu" and bits.dtype == torch.float32
    assert np.array_equal(bits.numpy().reshape(-1, 32), ref["bits"].astype(np.float32))
    assert ok.shape == (3, 20) and ok.dtype == torch.bool and np.array_equal(ok.numpy().reshape(-1), ref["crc_ok"])
    assert dec.last_attempts.shape == (3, 20) and np.array_equal(dec.last_attempts.numpy().reshape(-1), ref["attempts"])
    assert np.array_equal(dec.last_flip_pos.numpy().reshape(-1), ref["flip_pos"])
    gpu = polar_amd.SCF_Dec(fp, n, "CRC11", max_flips=16, f="minsum", device=DEV)
    b2 = gpu(xc.to(DEV))
    assert b2.device.type == "cuda" and np.array_equal(b2.cpu().numpy(), bits.numpy())
    assert gpu.last_attempts.device.type == "cuda"


def test_polar5g_decoder_scf():
    """Polar5GDecoder(dec_type="SCF") on the (k_target 40, E 128) uplink code against the restatement fed the
    mother-code LLRs the decoder's own rate recovery produces (exact f, llr_max 30; fragile rows left out)."""
    from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
    enc = Polar5GEncoder(40, 128)
    dec = Polar5GDecoder(enc, dec_type="SCF", list_size=16, return_crc_status=True)
    g = torch.Generator().manual_seed(3)
    u = (torch.rand((64, 40), generator=g) < 0.5).float()
    c = enc(u.to(DEV)).cpu()
    sigma = 0.9
    y = (1.0 - 2.0 * c) + sigma * torch.randn(c.shape, generator=g)
    llr_ch = (-2.0 * y / sigma ** 2).float()
    u_hat, ok = dec(llr_ch.to(DEV))
    mother = dec.rate_recover(llr_ch.to(DEV)).cpu().numpy()
    fp = np.sort(np.asarray(enc._frozen_pos, dtype=np.int64))
    ref = scf_ref.scf_decode(mother, fp, dec.n_polar, scf_ref.crc_params(enc.enc_crc.crc_degree), 16, exact=True)
    keep = ~ref["fragile"]
    print("classes:", int((ref["attempts"] == 1).sum()), int((ref["flip_pos"] >= 0).sum()), int((~ref["crc_ok"]).sum()),
          "fragile:", int(ref["fragile"].sum()))
    assert ref["fragile"].sum() <= scf_ref.FRAGILE_CAP and (ref["flip_pos"] >= 0).any()
    assert np.array_equal(u_hat.cpu().numpy()[keep], ref["bits"][keep, :40].astype(np.float32))
    assert np.array_equal(ok.cpu().numpy()[keep], ref["crc_ok"][keep])
    assert np.array_equal(dec.polar_dec.last_attempts.cpu().numpy()[keep], ref["attempts"][keep])


def test_cli_scf_leg():
    from polar_amd import cli
    res = cli.main(["--code", "5g", "--k", "40", "--n", "128", "--algos", "[scf]", "--scf_flips", "8", "--bs", "256",
                    "--mc_iter", "1", "--snr_end", "1.5", "--target_block_errs", "100000"])
    name = [k for k in res if k.startswith("SCF-8")]
    assert len(name) == 1 and "SC" in res
    bler_sc, bler_scf = res["SC"][1], res[name[0]][1]
    print("BLER SC", bler_sc, "SCF", bler_scf)
    assert bler_scf.shape == bler_sc.shape == (3,)
    assert (bler_scf <= bler_sc).all() and (bler_scf < bler_sc).any()
