"""GPU tests of the fused 5G NR link producer (pl_nr_awgn_qpsk_llr), the packed error counter
(pl_count_errors_packed), channel.FusedAWGN5G and the CLI's --code 5g:

  * information bits bit-exact against the numpy Philox restatement, and their packing;
  * at very high SNR the channel logits' signs are exactly Polar5GEncoder.forward's codewords (CRC
    attach, encoder, rate matching, Gray mapping exact);
  * the mother-code logits are exactly Polar5GDecoder.rate_recover of the channel logits;
  * the channel logits have the demapper's distribution at 2 dB and neighbours are uncorrelated;
  * nullable outputs, batch edges and argument errors;
  * pl_count_errors_packed equals numpy's counts;
  * FusedAWGN5G: error-free at 12 dB, error_counts == forward() + count, sim_ber's stop rules;
  * BLER of the fused link against the op-by-op chain (System5G_AWGN_model) within binomial bounds;
  * the CLI sweep.
The codes are uplink cases of tests/golden/make_golden_5g.py that reach every branch of the kernel
(n_polar = 32 ... 1024, i.e. 64 ... 2 rows per wave; interleaving only, repetition, puncturing,
shortening; CRC6 and CRC11), plus (12, 600): E > 2 n_polar, where the third copy is dropped.
"""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CODES = [(12, 20), (64, 128), (64, 200), (24, 300), (100, 180), (250, 300), (16, 64), (300, 1088), (512, 700)]
EXTRA_CODES = [(12, 600)]  # n_polar = 256, E > 2 n_polar
BS, ROW0, SEED, IT = 301, 1000, 7, 3  # 301: no multiple of any rows-per-wave count


@functools.lru_cache(maxsize=None)
def _pair(k, e, dec_type="SC", list_size=8, hybrid_sc=False):
    from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
    assert torch.cuda.is_available()
    with contextlib.redirect_stdout(io.StringIO()):  # the CRC6 / SC warnings
        enc = Polar5GEncoder(k, e)
        dec = Polar5GDecoder(enc, dec_type=dec_type, list_size=list_size, hybrid_sc=hybrid_sc)
    return enc, dec


def _produce(k, e, no, bs=BS, it=IT, row0=ROW0, seed=SEED, **outputs):
    from polar_amd import ops
    enc, dec = _pair(k, e)
    dev = torch.device("cuda", torch.cuda.current_device())
    g, idx = enc.tables(dev)
    a, b, f = dec.tables(dev)
    outputs = {"with_u": True, "with_ubits": True, "with_ch": True, **outputs}
    return ops.nr_awgn_qpsk_llr(enc.plan(dev), k, g, enc.crc_length, idx, a, b, f, bs, no, seed, it, row0, **outputs)


@functools.lru_cache(maxsize=None)
def _high_snr(k, e):
    return _produce(k, e, 1e-7)


def _no(ebno_db, k, e):
    from polar_amd.channel import ebnodb2no
    return float(ebnodb2no(ebno_db, 2, k / e))


@pytest.mark.parametrize("k,e", CODES + EXTRA_CODES)
def test_bits(k, e):
    from polar_amd import ops
    from polar_amd.channel import fused_info_bits
    u, ubits, _, _ = _high_snr(k, e)
    want = fused_info_bits(SEED, IT, np.arange(ROW0, ROW0 + BS), k)
    assert np.array_equal(u.cpu().numpy(), want)
    assert ubits.shape == (BS, (k + 31) // 32) and ubits.dtype == torch.int32
    assert torch.equal(ubits, ops.pack_bits(torch.from_numpy(want).cuda()))  # bits past k_target are zero


@pytest.mark.parametrize("k,e", CODES + EXTRA_CODES)
def test_encoder_chain_exact(k, e):
    enc, _ = _pair(k, e)
    u, _, ch, llr = _high_snr(k, e)
    assert ch.shape == (BS, e) and llr.shape == (BS, enc.n_polar)
    assert torch.equal((ch > 0).float(), enc(u))  # logits > 0 <=> bit 1
    _, _, ch2, llr2 = _produce(k, e, 1e-7)
    assert torch.equal(ch, ch2) and torch.equal(llr, llr2)  # same key -> same draw
    _, _, ch3, _ = _produce(k, e, 1e-7, it=IT + 1)
    assert not torch.equal(ch, ch3)


@pytest.mark.parametrize("k,e", CODES + EXTRA_CODES)
def test_rate_recovery_exact(k, e):
    _, dec = _pair(k, e)
    _, _, ch, llr = _produce(k, e, _no(2.0, k, e))
    assert torch.isfinite(ch).all()
    assert torch.equal(llr, dec.rate_recover(ch))


def test_noise_distribution():
    k, e, bs = 300, 1088, 4096
    enc, _ = _pair(k, e)
    no = _no(2.0, k, e)
    u, _, ch, _ = _produce(k, e, no, bs=bs, it=0, row0=0, seed=11)
    cw = enc(u)
    z = (ch - (2.0 / no) * (2 * cw - 1)) * (no ** 0.5) / 2  # standardised noise: N(0, 1)
    stats = [float(z.mean()), float(z.var()), float((z ** 3).mean()), float((z ** 4).mean())]
    zc = z.double() - z.double().mean()
    corr = float((zc[:, :-1] * zc[:, 1:]).mean() / zc.var())
    print("mean, var, m3, m4, corr(e, e+1):", stats, corr)
    assert abs(stats[0]) < 0.005
    assert abs(stats[1] - 1.0) < 0.005
    assert abs(stats[2]) < 0.01 and abs(stats[3] - 3.0) < 0.03
    assert abs(corr) < 0.005  # a Box-Muller draw shared by neighbours would show here


@pytest.mark.parametrize("k,e", [(12, 20), (100, 180), (300, 1088)])
def test_nullable_outputs_and_batch_edges(k, e):
    enc, _ = _pair(k, e)
    no = _no(2.0, k, e)
    u, ubits, ch, llr = _produce(k, e, no)
    for wu, wb, wc in [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                       (True, True, False), (False, True, True)]:
        u2, b2, c2, llr2 = _produce(k, e, no, with_u=wu, with_ubits=wb, with_ch=wc)
        assert (u2 is None) == (not wu) and (b2 is None) == (not wb) and (c2 is None) == (not wc)
        assert torch.equal(llr2, llr)
        assert u2 is None or torch.equal(u2, u)
        assert b2 is None or torch.equal(b2, ubits)
        assert c2 is None or torch.equal(c2, ch)
    cpw = 64 // (enc.n_polar // 32)  # rows per wave
    for bs in sorted({0, 1, cpw - 1, cpw, cpw + 1} - {-1}):
        u2, b2, c2, llr2 = _produce(k, e, no, bs=bs)
        assert llr2.shape == (bs, enc.n_polar) and u2.shape == (bs, k) and c2.shape == (bs, e)
        # row r of a draw depends on (row0 + r) only: a shorter batch is a prefix of the longer one
        assert torch.equal(llr2, llr[:bs]) and torch.equal(u2, u[:bs]) and torch.equal(b2, ubits[:bs])
        assert torch.equal(c2, ch[:bs])


def test_argument_errors():
    from polar_amd import _lib, ops
    k, e = 64, 128
    enc, dec = _pair(k, e)
    dev = torch.device("cuda", torch.cuda.current_device())
    g, idx = enc.tables(dev)
    a, b, f = dec.tables(dev)
    plan = enc.plan(dev)

    def call(plan=plan, k=k, g=g, idx=idx, no=0.5, it=0):
        return ops.nr_awgn_qpsk_llr(plan, k, g, enc.crc_length, idx, a, b, f, 8, no, SEED, it)
    call()
    with pytest.raises(_lib.PolarArgumentError, match="even"):
        call(idx=idx[:127].contiguous())
    for no in (0.0, -1.0):
        with pytest.raises(_lib.PolarArgumentError):
            call(no=no)
    mask = enc._mask.copy()
    mask[np.nonzero(mask == 0)[0][0]] = 1  # the same n, one information position fewer
    with pytest.raises(_lib.PolarArgumentError, match="k_target"):
        call(plan=_lib.Plan(enc.n_polar, mask, 1, flags=_lib.PL_PLAN_GENERIC))
    with pytest.raises(_lib.PolarArgumentError, match="k_target"):
        call(k=63, g=g[:63].contiguous())
    with pytest.raises(_lib.PolarArgumentError):
        call(it=2 ** 32)
    call(it=2 ** 32 - 1)


@pytest.mark.parametrize("rows,row_len,k_cmp", [(1001, 43, 37), (64, 511, 500), (3, 1, 1), (9000, 75, 64), (17, 32, 32)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_count_errors_packed_exact(rows, row_len, k_cmp, dtype):
    from polar_amd import ops
    g = torch.Generator(device="cuda").manual_seed(rows + row_len)
    ref = torch.randint(0, 2, (rows, row_len), generator=g, device="cuda")
    packed = ops.pack_bits(ref[:, :k_cmp])
    flip = torch.rand((rows, row_len), generator=g, device="cuda") < 0.01
    got = (ref ^ flip.long()).to(dtype)
    d = flip[:, :k_cmp].cpu().numpy()
    want = [int(d.sum()), int(d.any(axis=1).sum())]
    c = ops.count_errors_packed(got, packed, k_cmp)
    assert c.tolist() == want
    ops.count_errors_packed(got, packed, k_cmp, counts=c)  # accumulates
    assert c.tolist() == [2 * want[0], 2 * want[1]]
    if k_cmp < row_len:  # flips in the columns >= k_cmp only: nothing to count
        tail = ref.clone()
        tail[:, k_cmp:] ^= 1
        assert ops.count_errors_packed(tail.to(dtype), packed, k_cmp).tolist() == [0, 0]


@pytest.mark.parametrize("k,e", [(64, 128), (100, 180)])
@pytest.mark.parametrize("kind", ["SC", "SCL", "hybrid"])
def test_model_forward_and_error_counts(k, e, kind):
    from polar_amd import channel, sim
    enc, dec = _pair(k, e, "SC" if kind == "SC" else "SCL", hybrid_sc=kind == "hybrid")
    model = channel.FusedAWGN5G(enc, dec, seed=3)
    assert model.k == k and model.keyed_streams
    b, bh = model(256, 12.0)
    assert b.shape == bh.shape == (256, k) and torch.equal(b, bh)
    # error_counts == forward() + count_errors / count_block_errors on the same keys
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    want = [0, 0]
    for key in [(0, 0), (0, 1), (2, 5)]:
        assert model.error_counts(512, 1.5, counts=counts, stream=key) is counts
        b, bh = model(512, 1.5, stream=key)
        want[0] += int(sim.count_errors(b, bh))
        want[1] += int(sim.count_block_errors(b, bh))
    assert want[1] > 0 and counts.tolist() == want
    b2, _ = model(512, 1.5, stream=(2, 5))
    model.next_epoch()
    b3, _ = model(512, 1.5, stream=(2, 5))
    assert torch.equal(b, b2) and not torch.equal(b, b3)
    with pytest.raises(ValueError):
        model(8, 1.0, stream=(0, 2 ** 32))
    with pytest.raises(ValueError):
        model(8, 1.0, stream=(2 ** 31, 0))


def test_sim_ber_with_fused_5g_model():
    from polar_amd import channel, sim
    enc, dec = _pair(64, 128)
    model = channel.FusedAWGN5G(enc, dec, seed=42)
    ber, bler, cnt = sim.sim_ber(model, [0.0, 2.0, 4.0], 4000, 5, target_block_errs=500, verbose=False,
                                 device="cuda", return_counts=True)
    assert (cnt[:, 3] % 4000 == 0).all() and cnt[0, 1] >= 500
    assert (cnt[:, 2] == cnt[:, 3] * 64).all()
    assert bler[0] > bler[1] > bler[2] > 0
    assert model.epoch == 1


def _bler_pair(dec_type, bs, ebno, seed):
    from polar_amd import channel, sim
    enc, dec = _pair(64, 128, dec_type)
    fused = channel.FusedAWGN5G(enc, dec, seed=seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    unfused = channel.System5G_AWGN_model(enc, dec, device="cuda", generator=gen)
    out = []
    for model in (fused, unfused):
        b, bh = model(bs, ebno)
        assert b.shape == bh.shape == (bs, 64)
        out.append(float(sim.count_block_errors(b, bh.to(b.device))) / bs)
    return out


def _check_parity(pf, pu, bs, what):
    p = (pf + pu) / 2  # pooled rate of two samples of bs blocks
    bound = 5 * (p * (1 - p) * 2 / bs) ** 0.5
    print(what, "bler fused", pf, "unfused", pu, "bound", bound)
    assert abs(pf - pu) < bound, (what, pf, pu, bound)


def test_bler_parity_with_unfused_chain_sc():
    """Fused link vs the op-by-op chain, (64, 128), SC, 16384 rows per path.  Points: CRC11 leaves a
    (75, 128) mother code, whose SC BLER is far above 0.05 at 1 dB and falls through it towards 3 dB."""
    bs, seen = 16384, []
    for ebno in (1.0, 2.0, 3.0):
        pf, pu = _bler_pair("SC", bs, ebno, seed=17)
        seen.append(pu)
        _check_parity(pf, pu, bs, f"SC {ebno} dB")
    assert max(seen) > 0.05, seen


def test_bler_parity_with_unfused_chain_scl():
    bs = 4096
    pf, pu = _bler_pair("SCL", bs, 2.0, seed=19)
    _check_parity(pf, pu, bs, "SCL-8 2.0 dB")


def test_cli_5g(capsys):
    from polar_amd import cli
    res = cli.main(["--code", "5g", "--k", "64", "--n", "128", "--bs", "2000", "--mc_iter", "2", "--snr_end", "1.5",
                    "--algos", "[scl]"])
    capsys.readouterr()
    assert set(res) == {"SC", "SCL-8"}
    for ber, bler in res.values():
        assert ber.shape == bler.shape == (3,) and np.isfinite(ber).all() and np.isfinite(bler).all()
    bler = res["SC"][1]
    assert bler[0] > bler[1] > bler[2] > 0
