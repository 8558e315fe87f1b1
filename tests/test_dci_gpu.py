"""The 5G downlink chain (polar_amd.dci: DCIEncoder, DCIDecoder) against the numpy restatement
tests/golden/pcl_ref.py: code bits, payload, ok and stop are np.array_equal.

The restatement restates the data path (CRC24C by long division, ones prefix, RNTI, interleaver gather, butterfly,
rate-matching gather, rate recovery, the constrained list decoder); the index tables are the package's, pinned
against the reference project by tests/test_polar5g_gpu.py and tests/test_nr_link.py.
"""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pcl_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (payload bits, code bits): puncturing, repetition and, with (100, 150), shortening
CODES = [(12, 54), (40, 216), (64, 128), (140, 576), (100, 150)]
ROWS = 33


@pytest.fixture(scope="module")
def pa():
    import polar_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return polar_amd


@functools.lru_cache(maxsize=None)
def _tables(A, E):
    from polar_amd.polar5g import _rate_match_tables
    _, n_polar, frozen, idx_rm, il = _rate_match_tables(A, E, "downlink")
    return int(n_polar), np.setdiff1d(np.arange(n_polar), frozen), np.asarray(idx_rm), np.asarray(il)


def _enc(pa, A, E, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return pa.DCIEncoder(A, E, device=DEV, **kw)


def _payload(A, seed=0):
    return np.random.default_rng(1000 * A + seed).integers(0, 2, (ROWS, A)).astype(np.uint8)


@pytest.mark.parametrize("A,E", CODES)
@pytest.mark.parametrize("rnti,prefix,inter", [(0, True, True), (0xBEEF, True, True), (0, False, True),
                                               (0xBEEF, False, True), (0xBEEF, True, False)])
def test_encoder_equals_the_restatement(pa, A, E, rnti, prefix, inter):
    n_polar, info, idx_rm, il = _tables(A, E)
    enc = _enc(pa, A, E, rnti=rnti, ones_prefix=prefix, interleave=inter)
    assert (enc.k, enc.n, enc.n_polar, enc.k_polar) == (A, E, n_polar, A + 24)
    data = _payload(A)
    want, _ = pcl_ref.dci_encode(data, info, n_polar, il if inter else None, idx_rm, rnti, prefix)
    got = enc(torch.tensor(data, dtype=torch.float32, device=DEV))
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want.astype(np.float32))
    cpu = enc(torch.tensor(data[:5].reshape(1, 5, A), dtype=torch.float32))  # CPU in, CPU out, leading dims kept
    assert cpu.device.type == "cpu" and np.array_equal(cpu[0].numpy(), want[:5])


@pytest.mark.parametrize("A,E", CODES)
@pytest.mark.parametrize("n_force", ["0", "distributed"])
def test_noiseless_round_trip(pa, A, E, n_force):
    from polar_amd import dci
    enc = _enc(pa, A, E, rnti=0xBEEF)
    nf = 0 if n_force == "0" else dci.distributed_parity_bits(enc)
    assert n_force == "0" or nf in (3, 7)
    dec = pa.DCIDecoder(enc, list_size=8, n_force=nf, return_crc_status=True)
    data = torch.tensor(_payload(A), dtype=torch.float32, device=DEV)
    a_hat, ok = dec((2.0 * enc(data) - 1.0) * 6.0)
    assert torch.equal(a_hat, data) and bool((ok == 1).all()) and bool((dec.last_stop == enc.n_polar).all())
    plain = pa.DCIDecoder(enc, list_size=2)
    assert torch.equal(plain((2.0 * enc(data) - 1.0) * 6.0), data)


@functools.lru_cache(maxsize=None)
def _noisy(A, E, rnti, L, nf):
    """(channel logits, the restatement's outputs): a third each of AWGN rows near the waterfall, of noiseless rows,
    and of pure noise."""
    n_polar, info, idx_rm, il = _tables(A, E)
    rng = np.random.default_rng(A + E)
    cw, _ = pcl_ref.dci_encode(_payload(A, 1), info, n_polar, il, idx_rm, rnti, True)
    no = 1.0 / (2.0 * ((A + 24) / E) * 10.0 ** (2.0 / 10.0))
    y = (1.0 - 2.0 * cw[:22]) + rng.standard_normal((22, E)) * np.sqrt(no)
    x = np.concatenate([(-2.0 * y / no), (2.0 * cw[22:] - 1.0) * 5.0, rng.standard_normal((ROWS, E)) * 4.0]).astype(np.float32)
    return x, pcl_ref.dci_decode(x, A, info, n_polar, il, idx_rm, L, rnti, True, nf)


@pytest.mark.parametrize("A,E", CODES)
@pytest.mark.parametrize("L,n_force", [(8, "0"), (8, "distributed"), (1, "0"), (32, "0")])
def test_awgn_and_noise_rows_equal_the_restatement(pa, A, E, L, n_force):
    from polar_amd import dci
    enc = _enc(pa, A, E, rnti=0xBEEF)
    nf = 0 if n_force == "0" else dci.distributed_parity_bits(enc)
    x, (a_hat, ok, stop, pm) = _noisy(A, E, 0xBEEF, L, nf)
    dec = pa.DCIDecoder(enc, list_size=L, n_force=nf, return_crc_status=True)
    got, gok = dec(torch.tensor(x, device=DEV))
    print((A, E, L, nf), "ok:", int(ok.sum()), "stopped early:", int((stop < enc.n_polar).sum()), "of", len(ok))
    assert np.array_equal(dec.last_stop.cpu().numpy(), stop)
    assert np.array_equal(gok.cpu().numpy(), ok.astype(np.float32))
    assert np.array_equal(got.cpu().numpy(), a_hat.astype(np.float32))
    assert np.array_equal(dec.last_pm.cpu().numpy(), pm)


@pytest.mark.parametrize("A,E", CODES)
def test_another_rnti_is_rejected_as_the_restatement_says(pa, A, E):
    """Noiseless rows of RNTI 0xBEEF decoded for RNTI 0xBEE7 (one bit apart): the restatement finds no path in any
    row -- asserted here on the CPU -- and the GPU gives its stop, zero payload and ok = 0."""
    n_polar, info, idx_rm, il = _tables(A, E)
    cw, _ = pcl_ref.dci_encode(_payload(A, 2), info, n_polar, il, idx_rm, 0xBEEF, True)
    x = ((2.0 * cw - 1.0) * 6.0).astype(np.float32)
    a_hat, ok, stop, _ = pcl_ref.dci_decode(x, A, info, n_polar, il, idx_rm, 1, 0xBEE7, True)
    assert (ok == 0).all() and (a_hat == 0).all() and (stop < n_polar).all()
    dec = pa.DCIDecoder(_enc(pa, A, E, rnti=0xBEE7), list_size=1, return_crc_status=True)
    got, gok = dec(torch.tensor(x, device=DEV))
    assert not got.any() and not gok.any() and np.array_equal(dec.last_stop.cpu().numpy(), stop)
    # with a list the wrong RNTI may survive as another word: whatever the restatement says
    a8, ok8, stop8, _ = pcl_ref.dci_decode(x, A, info, n_polar, il, idx_rm, 8, 0xBEE7, True)
    dec8 = pa.DCIDecoder(_enc(pa, A, E, rnti=0xBEE7), list_size=8, return_crc_status=True)
    got8, gok8 = dec8(torch.tensor(x, device=DEV))
    assert np.array_equal(got8.cpu().numpy(), a8) and np.array_equal(gok8.cpu().numpy(), ok8) and \
        np.array_equal(dec8.last_stop.cpu().numpy(), stop8)


def test_existing_downlink_behaviour_stays(pa):
    with contextlib.redirect_stdout(io.StringIO()):
        enc = pa.polar5g.Polar5GEncoder(40, 216, channel_type="downlink")
    with pytest.raises(Exception, match="error"):  # the refusal tests/test_polar5g_gpu.py pins
        enc(torch.zeros((2, 40)))
    for bad in (dict(k=141, n=576), dict(k=40, n=600), dict(k=40, n=50)):
        with pytest.raises((ValueError, AssertionError)):
            pa.DCIEncoder(bad["k"], bad["n"])
    with pytest.raises(ValueError):
        pa.DCIEncoder(40, 216, rnti=1 << 16)
    with pytest.raises(ValueError):
        pa.DCIDecoder(_enc(pa, 40, 216), n_force=25)


def test_cli_dci_leg():
    from polar_amd import cli
    res = cli.main(["--code", "dci", "--k", "40", "--n", "216", "--algos", "[scl]", "--bs", "200", "--mc_iter", "1",
                    "--snr_end", "1.5", "--target_block_errs", "100000", "--dci_rnti", "0xBEEF"])
    assert set(res) == {"SC", "SCL-8"}
    bler_sc, bler_l = res["SC"][1], res["SCL-8"][1]
    print("BLER SC", bler_sc, "SCL-8", bler_l)
    assert bler_sc.shape == bler_l.shape == (3,) and ((bler_l >= 0) & (bler_l <= bler_sc)).all() and (bler_sc <= 1).all()
    c = cli.parse(["--code", "dci", "--k", "64", "--n", "432", "--dci_n_force", "3", "--dci_tail_crc"])
    assert (c.dci_n_force, c.dci_tail_crc, c.dci_rnti) == (3, True, 0)
    for bad in (["--k", "141", "--n", "576"], ["--k", "40", "--n", "50"], ["--k", "40", "--n", "216", "--algos", "[pac]"],
                ["--k", "40", "--n", "216", "--dci_n_force", "25"], ["--k", "40", "--n", "216", "--dci_rnti", "65536"],
                ["--k", "40", "--n", "216", "--list_size", "3"]):
        with pytest.raises(SystemExit):
            cli.parse(["--code", "dci"] + bad)
