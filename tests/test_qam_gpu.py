"""GPU tests of 16/64/256-QAM in the fused link producers (pl_awgn_qam_llr, pl_nr_awgn_qam_llr,
csrc/channel_kernel.hip) and of num_bits_per_symbol in FusedAWGN / FusedAWGN5G:
  * m = 2 through the new entry points is the QPSK entry points bit for bit;
  * the information bits are channel.fused_info_bits for the key, whatever m;
  * mapper: y_out minus the op-by-op Mapper's symbols of the rebuilt code word is noise of variance
    no / 2 per component, I and Q uncorrelated, independent of the transmitted symbol; at a vanishing
    no, y_out is the Mapper's output exactly;
  * demapper: the logits against the reference's formula in float64 on the dumped y_out, within
    test_qam.DEMAP_BOUND (4x the op-by-op fp32 Demapper's measured error), also far outside the
    constellation and at a tiny no;
  * NR: the mother-code logits are Polar5GDecoder.rate_recover of the channel logits, bit for bit;
  * nullable outputs, batch edges, repeatability; BLER of FusedAWGN at 16-QAM against the reference's.
Shapes: plain n = 32 (one lane per row), 64, 1024 (two rows per wave) x m = 4, 8; NR one puncturing,
one shortening and one repetition code per m, with odd symbol counts and a several-pass case among them.
"""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

from test_qam import DEMAP_BOUND, GOLDEN, demap_f64, rel_err

pytestmark = pytest.mark.gpu

BS, ROW0, SEED, IT = 301, 1000, 7, 3      # 301: no multiple of any rows-per-wave count
PLAIN = [(n, m) for n in (32, 64, 1024) for m in (4, 8)]
# (k, E, m): a puncturing (P), a shortening (S) and a repetition (R) code per m.  Odd symbol counts:
# (100, 180, 4) 45, (12, 20, 4) 5, (12, 36, 4) 9, (20, 90, 6) 15, (64, 200, 8) 25, (100, 184, 8) 23, (12, 72, 8) 9.
# Several passes over the LDS stage (rows per pass < rows per wave): (30, 1088) 2 of 4, (12, 600) 3 of 8,
# (12, 36) 60 of 64, (12, 72) 30 of 32.  n_polar = 32 (64 rows per wave): (12, 20), (12, 36); 64: (12, 72).
NR = [(64, 200, 4), (100, 180, 4), (30, 1088, 4), (12, 20, 4), (12, 36, 4),          # P S R S R
      (24, 300, 6), (100, 180, 6), (12, 600, 6), (20, 90, 6), (12, 72, 6),          # P S R P R
      (64, 200, 8), (100, 184, 8), (30, 1088, 8), (12, 72, 8)]                       # P S R R


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _plain(n):
    """(plan, frozen positions, dense encoder on the CPU) of the reference's (n/2, n) code."""
    import polar_amd
    from polar_amd import _lib, channel, frozen
    k = n // 2
    fp = polar_amd.reference_frozen_pos(k, n)
    G, _, _ = frozen.get_Kern_frozen_bits(n, n - k, frozen.F2)
    plan = _lib.Plan(n, polar_amd.frozen_mask(fp, n), 1, flags=_lib.PL_PLAN_GENERIC, device=_dev())
    return plan, fp, channel.DenseEncoder(fp, n, G)


@functools.lru_cache(maxsize=None)
def _pair(k, e, dec_type="SC", hybrid_sc=False):
    from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
    with contextlib.redirect_stdout(io.StringIO()):
        enc = Polar5GEncoder(k, e)
        dec = Polar5GDecoder(enc, dec_type=dec_type, list_size=8, hybrid_sc=hybrid_sc)
    return enc, dec


def _plain_run(n, m, no, bs=BS, it=IT, row0=ROW0, seed=SEED, **kw):
    from polar_amd import ops
    kw = {"with_u": True, "with_ubits": True, "with_y": m != 2, **kw}
    return ops.awgn_qam_llr(_plain(n)[0], m, bs, no, seed, it, row0, **kw)


def _nr_run(k, e, m, no, bs=BS, it=IT, row0=ROW0, seed=SEED, **kw):
    from polar_amd import ops
    enc, dec = _pair(k, e)
    g, idx = enc.tables(_dev())
    a, b, f = dec.tables(_dev())
    kw = {"with_u": True, "with_ubits": True, "with_ch": True, "with_y": m != 2, **kw}
    return ops.nr_awgn_qam_llr(enc.plan(_dev()), m, k, g, enc.crc_length, idx, a, b, f, bs, no, seed, it, row0, **kw)


def _points(m):
    from polar_amd import channel
    return channel.QamConstellation(m).points.numpy()


def _symbols(cw, m):
    """The op-by-op Mapper's symbols (complex64 numpy) and their indices for 0/1 code rows cw [bs, len]."""
    from polar_amd import channel
    cw = cw.cpu().float()
    x = channel.Mapper(channel.QamConstellation(m))(cw).numpy()
    idx = (cw.reshape(cw.shape[0], -1, m).long() * (2 ** torch.arange(m - 1, -1, -1))).sum(-1).numpy()
    return x, idx


def _check_noise(y, x, idx, no, what):
    """y - x is N(0, no/2) per component, I and Q uncorrelated, no dependence on the symbol sent."""
    z = (y.astype(np.complex128) - x.astype(np.complex128)).reshape(-1)
    zs = np.stack([z.real, z.imag]) / np.sqrt(no / 2)              # standardised: N(0, 1)
    cnt = zs.shape[1]
    se = 1 / np.sqrt(cnt)
    print(what, "symbols", cnt, "mean", zs.mean(axis=1), "var", zs.var(axis=1), "corr", np.mean(zs[0] * zs[1]))
    assert np.all(np.abs(zs.mean(axis=1)) < 5 * se), what
    assert np.all(np.abs(zs.var(axis=1) - 1) < 5 * np.sqrt(2) * se), what       # Var of a chi^2 mean: 2 / cnt
    assert abs(np.mean(zs[0] * zs[1])) < 5 * se, what
    flat = idx.reshape(-1)
    for s in np.unique(flat):
        sel = zs[:, flat == s]
        # a wrong Gray label or an axis swap moves a group's mean by at least a level spacing over sigma
        assert np.all(np.abs(sel.mean(axis=1)) < 5.5 / np.sqrt(sel.shape[1])), (what, int(s), sel.mean(axis=1))


def _check_demap(y, llr, m, no, what, max_rows=24):
    """llr against the float64 formula on the dumped symbols (a prefix of the rows: float64 over 2^m points)."""
    r = min(max_rows, y.shape[0])
    yc = y[:r, :, 0].astype(np.float64) + 1j * y[:r, :, 1].astype(np.float64)
    want = demap_f64(yc, _points(m), float(np.float32(no)))
    got = llr[:r]
    assert np.isfinite(got).all(), what
    err = rel_err(got, want)
    print(what, f"no={no}: demapper error {err:.3e} (bound {DEMAP_BOUND:.3e}), max |llr| {np.abs(want).max():.4g}, "
                f"max |y| {np.abs(yc).max():.3g}")
    assert err <= DEMAP_BOUND, (what, err)


# ---- 1. m = 2 is the QPSK entry points -------------------------------------------------------------

@pytest.mark.parametrize("n", [32, 64, 1024])
def test_plain_m2_is_the_qpsk_kernel(n):
    from polar_amd import ops
    plan = _plain(n)[0]
    u, ubits, y, llr = _plain_run(n, 2, 0.7)
    u0, llr0 = ops.awgn_qpsk_llr(plan, BS, 0.7, SEED, IT, ROW0)
    ub1, llr1 = ops.awgn_qpsk_llr_bits(plan, BS, 0.7, SEED, IT, ROW0)
    assert y is None
    assert torch.equal(u, u0) and torch.equal(llr, llr0) and torch.equal(llr, llr1) and torch.equal(ubits, ub1)
    with pytest.raises(ValueError, match="with_y"):
        _plain_run(n, 2, 0.7, with_y=True)


@pytest.mark.parametrize("k,e", [(12, 20), (64, 200), (300, 1088)])
def test_nr_m2_is_the_qpsk_kernel(k, e):
    from polar_amd import ops
    enc, dec = _pair(k, e)
    g, idx = enc.tables(_dev())
    a, b, f = dec.tables(_dev())
    u, ubits, ch, y, llr = _nr_run(k, e, 2, 0.7)
    u0, ub0, ch0, llr0 = ops.nr_awgn_qpsk_llr(enc.plan(_dev()), k, g, enc.crc_length, idx, a, b, f, BS, 0.7, SEED, IT,
                                             ROW0, with_ch=True)
    assert y is None
    assert torch.equal(u, u0) and torch.equal(ubits, ub0) and torch.equal(ch, ch0) and torch.equal(llr, llr0)


# ---- 2.-4., 6. plain ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", PLAIN)
def test_plain_bits_mapper_noise_demapper(n, m):
    from polar_amd import ops
    from polar_amd.channel import fused_info_bits
    _, _, enc = _plain(n)
    k, no = n // 2, 0.1
    u, ubits, y, llr = _plain_run(n, m, no)
    assert u.shape == (BS, k) and y.shape == (BS, n // m, 2) and llr.shape == (BS, n)
    want = fused_info_bits(SEED, IT, np.arange(ROW0, ROW0 + BS), k)
    assert np.array_equal(u.cpu().numpy(), want)
    assert torch.equal(ubits, ops.pack_bits(torch.from_numpy(want).cuda()))
    x, idx = _symbols(enc(u.cpu()), m)
    yn = y.cpu().numpy()
    _check_noise(yn[..., 0] + 1j * yn[..., 1], x, idx, no, f"plain n={n} m={m}")
    _check_demap(yn, llr.cpu().numpy(), m, no, f"plain n={n} m={m}")
    # the same key twice, another iteration
    u2, ub2, y2, llr2 = _plain_run(n, m, no)
    assert torch.equal(u, u2) and torch.equal(ubits, ub2) and torch.equal(y, y2) and torch.equal(llr, llr2)
    u3, _, y3, _ = _plain_run(n, m, no, it=IT + 1)
    assert not torch.equal(y, y3) and not torch.equal(u, u3)
    # a vanishing no: the received symbols are the Mapper's output exactly (the host's PAM levels are
    # the reference's points), and the logits stay finite with the code bits as their signs
    _, _, y0, llr0 = _plain_run(n, m, 1e-20)
    y0 = y0.cpu().numpy()
    assert np.array_equal(y0[..., 0], x.real) and np.array_equal(y0[..., 1], x.imag)
    assert torch.isfinite(llr0).all() and torch.equal((llr0 > 0).float().cpu(), enc(u.cpu()))


@pytest.mark.parametrize("n,m", [(32, 8), (64, 4), (1024, 8), (1024, 4)])
@pytest.mark.parametrize("no", [50.0, 1e-3])
def test_plain_demapper_far_out_and_tiny_no(n, m, no):
    """no = 50: |y| reaches 10 and beyond; no = 1e-3: exponents of -1e3 and below, where a demapper
    without per-set maximum subtraction underflows to log(0)."""
    _, _, y, llr = _plain_run(n, m, no, with_u=False, with_ubits=False)
    yn = y.cpu().numpy()
    if no > 1:
        assert np.abs(yn).max() > 10
    _check_demap(yn, llr.cpu().numpy(), m, no, f"plain n={n} m={m}", max_rows=BS if n < 1024 else 24)


@pytest.mark.parametrize("n,m", [(32, 4), (64, 8), (1024, 4)])
def test_plain_nullable_outputs_and_batch_edges(n, m):
    no = 0.2
    u, ubits, y, llr = _plain_run(n, m, no)
    for wu, wb, wy in [(False, False, False), (True, False, False), (False, True, False), (False, False, True)]:
        u2, b2, y2, llr2 = _plain_run(n, m, no, with_u=wu, with_ubits=wb, with_y=wy)
        assert (u2 is None) == (not wu) and (b2 is None) == (not wb) and (y2 is None) == (not wy)
        assert torch.equal(llr2, llr)
        assert u2 is None or torch.equal(u2, u)
        assert b2 is None or torch.equal(b2, ubits)
        assert y2 is None or torch.equal(y2, y)
    cpw = 64 // max(1, n // 32)
    for bs in sorted({0, 1, cpw - 1, cpw + 1}):
        u2, b2, y2, llr2 = _plain_run(n, m, no, bs=bs)
        assert llr2.shape == (bs, n) and y2.shape == (bs, n // m, 2)
        assert torch.equal(llr2, llr[:bs]) and torch.equal(u2, u[:bs]) and torch.equal(b2, ubits[:bs])
        assert torch.equal(y2, y[:bs])


def test_plain_refuses_an_m_that_does_not_divide_n():
    from polar_amd import _lib
    import ctypes
    plan = _plain(64)[0]
    out = torch.empty(4 * 64, device="cuda")
    rc = _lib.lib().pl_awgn_qam_llr(plan.handle, 6, 1, 0, 0, 4, 0.5, None, None, None,
                                    ctypes.c_void_p(out.data_ptr()), None)
    assert rc == _lib.PL_EINVAL and b"bits_per_symbol" in _lib.lib().pl_last_error_string()
    with pytest.raises(ValueError, match="num_bits_per_symbol"):
        _plain_run(64, 6, 0.5)


# ---- 2.-6. NR -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,e,m", NR)
def test_nr_bits_mapper_noise_demapper_rate_recovery(k, e, m):
    from polar_amd import ops
    from polar_amd.channel import fused_info_bits
    enc, dec = _pair(k, e)
    no = 0.15
    u, ubits, ch, y, llr = _nr_run(k, e, m, no)
    assert u.shape == (BS, k) and ch.shape == (BS, e) and y.shape == (BS, e // m, 2) and llr.shape == (BS, enc.n_polar)
    want = fused_info_bits(SEED, IT, np.arange(ROW0, ROW0 + BS), k)
    assert np.array_equal(u.cpu().numpy(), want)
    assert torch.equal(ubits, ops.pack_bits(torch.from_numpy(want).cuda()))
    # Polar5GEncoder.forward: CRC attach, polar encode, rate matching -> the transmitted bits
    x, idx = _symbols(enc(u), m)
    yn = y.cpu().numpy()
    _check_noise(yn[..., 0] + 1j * yn[..., 1], x, idx, no, f"nr ({k},{e}) m={m}")
    _check_demap(yn, ch.cpu().numpy(), m, no, f"nr ({k},{e}) m={m}")
    assert torch.equal(llr, dec.rate_recover(ch))
    u2, ub2, ch2, y2, llr2 = _nr_run(k, e, m, no)
    assert torch.equal(u, u2) and torch.equal(ch, ch2) and torch.equal(y, y2) and torch.equal(llr, llr2)
    _, _, _, y3, _ = _nr_run(k, e, m, no, it=IT + 1)
    assert not torch.equal(y, y3)
    _, _, ch0, y0, llr0 = _nr_run(k, e, m, 1e-20)
    y0 = y0.cpu().numpy()
    assert np.array_equal(y0[..., 0], x.real) and np.array_equal(y0[..., 1], x.imag)
    assert torch.isfinite(ch0).all() and torch.equal((ch0 > 0).float(), enc(u))
    assert torch.equal(llr0, dec.rate_recover(ch0))


@pytest.mark.parametrize("k,e,m", [(100, 180, 4), (20, 90, 6), (100, 184, 8), (30, 1088, 8)])
@pytest.mark.parametrize("no", [50.0, 1e-3])
def test_nr_demapper_far_out_and_tiny_no(k, e, m, no):
    _, dec = _pair(k, e)
    _, _, ch, y, llr = _nr_run(k, e, m, no, with_u=False, with_ubits=False)
    yn = y.cpu().numpy()
    if no > 1:
        assert np.abs(yn).max() > 10
    _check_demap(yn, ch.cpu().numpy(), m, no, f"nr ({k},{e}) m={m}", max_rows=BS if e < 600 else 24)
    assert torch.equal(llr, dec.rate_recover(ch))


@pytest.mark.parametrize("k,e,m", [(12, 20, 4), (20, 90, 6), (12, 72, 8), (30, 1088, 4)])
def test_nr_nullable_outputs_and_batch_edges(k, e, m):
    enc, _ = _pair(k, e)
    no = 0.2
    u, ubits, ch, y, llr = _nr_run(k, e, m, no)
    for wu, wb, wc, wy in [(False, False, False, False), (True, False, False, False), (False, True, False, False),
                           (False, False, True, False), (False, False, False, True), (True, True, True, True)]:
        u2, b2, c2, y2, llr2 = _nr_run(k, e, m, no, with_u=wu, with_ubits=wb, with_ch=wc, with_y=wy)
        assert (u2 is None) == (not wu) and (b2 is None) == (not wb) and (c2 is None) == (not wc)
        assert (y2 is None) == (not wy) and torch.equal(llr2, llr)
        assert u2 is None or torch.equal(u2, u)
        assert b2 is None or torch.equal(b2, ubits)
        assert c2 is None or torch.equal(c2, ch)
        assert y2 is None or torch.equal(y2, y)
    cpw = 64 // (enc.n_polar // 32)
    for bs in sorted({0, 1, cpw - 1, cpw + 1}):
        u2, b2, c2, y2, llr2 = _nr_run(k, e, m, no, bs=bs)
        assert llr2.shape == (bs, enc.n_polar) and c2.shape == (bs, e) and y2.shape == (bs, e // m, 2)
        assert torch.equal(llr2, llr[:bs]) and torch.equal(u2, u[:bs]) and torch.equal(b2, ubits[:bs])
        assert torch.equal(c2, ch[:bs]) and torch.equal(y2, y[:bs])


# ---- 7. end to end ------------------------------------------------------------------------------------

def test_fused_awgn_16qam_bler_matches_the_reference():
    import polar_amd
    from polar_amd import channel, sim
    with np.load(GOLDEN) as d:
        k, n, m, ebno = int(d["bler_k"]), int(d["bler_n"]), int(d["bler_m"]), float(d["bler_ebno_db"])
        p, ref_rows = float(d["bler_bler"]), int(d["bler_rows"])
    fp = polar_amd.reference_frozen_pos(k, n)
    model = channel.FusedAWGN(n, k, fp, polar_amd.SC_Dec(fp, n, device="cuda"), seed=5, num_bits_per_symbol=m)
    assert model.n_bits_per_sym == 4
    bs = 8192
    b, bh = model(bs, ebno, stream=(0, 0))
    bler = float(sim.count_block_errors(b, bh)) / bs
    sd = (p * (1 - p) / ref_rows + p * (1 - p) / bs) ** 0.5
    print("16-QAM (128,256) SC BLER fused", bler, "reference", p, "sd", sd)
    assert abs(bler - p) < 4 * sd, (bler, p, sd)
    # error_counts: the two-kernel path on the same draw as forward()
    counts = model.error_counts(bs, ebno, stream=(0, 0))
    assert counts is not None
    assert counts.tolist() == [int(sim.count_errors(b, bh)), int(sim.count_block_errors(b, bh))]
    assert model.sim_kernel is True     # the QPSK in-kernel iteration was not tried
    ber, bl, cnt = sim.sim_ber(model, [ebno - 1.0, ebno + 1.0], 2048, 2, target_block_errs=100, verbose=False,
                               device="cuda", return_counts=True)
    assert bl[0] > bl[1] > 0 and (cnt[:, 3] % 2048 == 0).all() and model.epoch == 1


@pytest.mark.parametrize("kind", ["SC", "hybrid"])
def test_fused_awgn5g_16qam(kind):
    from polar_amd import channel, sim
    k, e, bs, ebno = 64, 128, 2048, 3.0
    enc, dec = _pair(k, e, "SC" if kind == "SC" else "SCL", hybrid_sc=kind == "hybrid")
    model = channel.FusedAWGN5G(enc, dec, seed=3, num_bits_per_symbol=4)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    want = [0, 0]
    for key in [(0, 0), (1, 4)]:
        assert model.error_counts(bs, ebno, counts=counts, stream=key) is counts
        b, bh = model(bs, ebno, stream=key)
        assert b.shape == bh.shape == (bs, k)
        want[0] += int(sim.count_errors(b, bh))
        want[1] += int(sim.count_block_errors(b, bh))
    assert want[1] > 0 and counts.tolist() == want
    qpsk = channel.FusedAWGN5G(enc, dec, seed=3)
    c2 = torch.zeros(2, dtype=torch.int64, device="cuda")
    for key in [(0, 0), (1, 4)]:
        qpsk.error_counts(bs, ebno, counts=c2, stream=key)
    print(kind, "block errors of", 2 * bs, "at", ebno, "dB: 16-QAM", want[1], "QPSK", int(c2[1]))
    assert want[1] > int(c2[1])   # the same Eb/N0 buys less at 16-QAM
