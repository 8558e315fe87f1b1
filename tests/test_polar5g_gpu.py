"""5G NR wrapper on the GPU against the reference's fixtures
(tests/golden/make_golden_5g.py ran my_sn/fec/polar Polar5GEncoder / Polar5GDecoder).

  * Polar5GEncoder.forward (CRC attach + polar encode + rate matching, three HIP kernels):
    codewords bit-identical to the reference's.
  * Polar5GDecoder rate recovery (pl_rate_recover): the mother-code LLRs bit-identical to the
    ones the reference hands its decoder (captured in the fixture).
  * Decoding: the mother decoders are my_sn's exact-f SC / SCL (exp/log arithmetic), gated by a
    binomial test on the row-mismatch count against the reference's decoded bits (the rates of
    tests/test_exactf_gpu.py), and exact on noiseless round trips.
"""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    assert torch.cuda.is_available()
    return np.load(os.path.join(GOLDEN, "polar5g.npz"))


def _cases(g, prefix):
    return sorted({tuple(int(v) for v in k.split("_")[1:3]) for k in g.files if k.startswith(prefix + "_")})


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def test_encoder_gpu_vs_reference(g):
    from polar_amd import polar5g
    for k, n in _cases(g, "ul"):
        tag = f"ul_{k}_{n}"
        enc = _quiet(polar5g.Polar5GEncoder, k, n)
        u = torch.from_numpy(g[tag + "_u"])
        c_gpu = enc(u.cuda())
        assert c_gpu.device.type == "cuda"
        assert np.array_equal(c_gpu.cpu().numpy(), g[tag + "_c"]), tag
        assert np.array_equal(enc(u).numpy(), g[tag + "_c"]), tag  # CPU tensors round-trip


def test_crc_attach_edge_cases():
    from polar_amd import polar5g
    enc = _quiet(polar5g.Polar5GEncoder, 64, 128)
    assert enc.crc_attach(torch.empty((0, 64), device="cuda")).shape == (0, 75)
    z = enc.crc_attach(torch.zeros((3, 64), device="cuda"))
    assert torch.all(z == 0)  # zero init register, no inversion (crc.py)
    with pytest.raises(Exception, match="error"):
        _quiet(polar5g.Polar5GEncoder, 40, 100, channel_type="downlink")(torch.zeros((2, 40)))


def test_rate_recovery_gpu_vs_reference(g):
    from polar_amd import polar5g
    for k, n in _cases(g, "ul"):
        tag = f"ul_{k}_{n}"
        enc = _quiet(polar5g.Polar5GEncoder, k, n)
        dec = _quiet(polar5g.Polar5GDecoder, enc, dec_type="SC")
        got = dec.rate_recover(torch.from_numpy(g[tag + "_llr"]).cuda())
        assert np.array_equal(got.cpu().numpy(), g[tag + "_llr_mother"]), tag


@pytest.mark.parametrize("dec_type", ["SC", "SCL"])
def test_decoder_vs_reference(g, dec_type):
    """Row mismatches against the reference's decoded bits over the uplink fixtures, within the
    one-sided binomial gate (level 1e-3) at the rates tests/test_exactf_gpu.py establishes with
    85,000 / 6,000 reference rows (SC 1e-4, SCL 5e-4).  The rate-1 mother code ((1013, 1088):
    k_polar = n_polar = 1024, no frozen bit) is gated there against the oracle's own rate (~9 % of
    its rows are decided by last-ulp rounding even between glibc and the reference), not here."""
    sys.path.insert(0, GOLDEN)
    from exactf_recipe import binom_upper_ok
    from polar_amd import polar5g
    rows = agree = 0
    for k, n in _cases(g, "ul"):
        tag = f"ul_{k}_{n}"
        key = tag + ("_sc" if dec_type == "SC" else "_scl")
        if key not in g.files or int(g[tag + "_meta"][0]) == int(g[tag + "_meta"][1]):
            continue
        enc = _quiet(polar5g.Polar5GEncoder, k, n)
        dec = _quiet(polar5g.Polar5GDecoder, enc, dec_type=dec_type, list_size=8)
        out = dec(torch.from_numpy(g[tag + "_llr"]))
        assert out.shape == (g[tag + "_llr"].shape[0], k) and out.dtype == torch.float32
        ok = (out.numpy().astype(np.uint8) == g[key]).all(1)
        rows += len(ok)
        agree += int(ok.sum())
    assert rows > 0 and binom_upper_ok(rows - agree, rows, 1e-4 if dec_type == "SC" else 5e-4), (agree, rows)


@pytest.mark.parametrize("dec_type", ["SC", "SCL"])
def test_noiseless_round_trip(g, dec_type):
    from polar_amd import polar5g
    rng = np.random.default_rng(1)
    for k, n in _cases(g, "ul"):
        if dec_type == "SCL" and n > 600:
            continue
        enc = _quiet(polar5g.Polar5GEncoder, k, n)
        dec = _quiet(polar5g.Polar5GDecoder, enc, dec_type=dec_type, return_crc_status=True)
        u = torch.from_numpy(rng.integers(0, 2, (40, k)).astype(np.float32)).cuda()
        c = enc(u)
        logits = (2.0 * c - 1.0) * 8.0  # log P(1)/P(0): positive for 1 bits
        uh, ok = dec(logits)
        assert torch.equal(uh, u), (k, n)
        assert bool(ok.all()), (k, n)
        # every row flipped at its own random half of the positions: decoding fails and the
        # CRC says so (one flip pattern shared by all rows would be a single trial, since SC
        # decoding is equivariant under codeword sign flips and the CRC is linear)
        flip = torch.from_numpy(rng.random((40, n)) < 0.5).cuda()
        _, ok2 = dec(torch.where(flip, -logits, logits))
        assert float(ok2.mean()) < 0.5, (k, n)


# ---- the op-by-op kernels past one row per block -------------------------------------------------
# pl_gather_rows and pl_rate_recover take bs // 2048 (1 ... 8) rows per block; the fixtures and the
# link tests stay below 2048 rows, where the row loop runs once and its `b >= bs` exit is never taken.

def _np_parity(u, name):
    """[information bits | parity] in numpy: parity = XOR of crc_generator_rows of the 1 bits."""
    from polar_amd import polar5g
    deg = polar5g.mysn.crc_params(name)[0]
    rows = polar5g.crc_generator_rows(name, u.shape[1])
    acc = np.bitwise_xor.reduce(np.where(u.astype(bool), rows[None, :], 0).astype(np.uint32), axis=1)
    return np.concatenate([u, ((acc[:, None] >> np.arange(deg)[None, :]) & 1).astype(np.float32)], 1)


@pytest.mark.parametrize("bs", [4099, 16389])  # 2 and 8 rows per block, the last block ragged
@pytest.mark.parametrize("k,e", [(12, 20), (64, 200), (300, 1088)])  # shortening, puncturing, repetition
def test_row_loop_of_gather_and_rate_recover(k, e, bs):
    import oracle
    from polar_amd import polar5g
    assert torch.cuda.is_available()
    enc = _quiet(polar5g.Polar5GEncoder, k, e)
    dec = _quiet(polar5g.Polar5GDecoder, enc, dec_type="SC")
    rng = np.random.default_rng([k, e, bs])
    u = rng.integers(0, 2, (bs, k)).astype(np.float32)
    want = oracle.polar_encode(_np_parity(u, enc.crc_degree), enc.frozen_pos, enc.n_polar)[:, enc._ind_rate_matching]
    assert np.array_equal(enc(torch.from_numpy(u).cuda()).cpu().numpy(), want)
    a, b, f = dec._rec
    kinds = {(12, 20): (f != 0).any(), (64, 200): ((a < 0) & (f == 0)).any(), (300, 1088): (b >= 0).any()}
    assert kinds[k, e]
    x = rng.standard_normal((bs, e)).astype(np.float32)
    rec = np.where(a[None, :] >= 0, x[:, np.maximum(a, 0)], f[None, :])
    rep = b >= 0
    rec[:, rep] = x[:, a[rep]] + x[:, b[rep]]
    assert np.array_equal(dec.rate_recover(torch.from_numpy(x).cuda()).cpu().numpy(), rec.astype(np.float32))


@pytest.mark.parametrize("bs", [1, 3, 4, 5, 4099])  # a block takes 4 rows, one per wave
@pytest.mark.parametrize("k,name", [(12, "CRC6"), (300, "CRC11")])
def test_crc_attach_and_status_at_the_block_edge(k, name, bs):
    from polar_amd import _lib, ops, polar5g
    assert torch.cuda.is_available()
    enc = _quiet(polar5g.Polar5GEncoder, k, 1088 if k == 300 else 20)
    assert enc.crc_degree == name
    deg, poly = polar5g.mysn.crc_params(name)
    rng = np.random.default_rng([k, bs])
    u = rng.integers(0, 2, (bs, k)).astype(np.float32)
    want = _np_parity(u, name)
    got = enc.crc_attach(torch.from_numpy(u).cuda())
    assert np.array_equal(got.cpu().numpy(), want)
    # pl_crc_status on a plan that carries (k + degree, CRC): the attached words pass; with one bit
    # flipped in every other row, a row passes iff its parity is still that of its information bits
    n = 1 << (k + deg - 1).bit_length()
    mask = np.zeros(n, dtype=np.uint8)
    mask[: n - (k + deg)] = 1
    plan = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
    plan.set_crc(deg, poly)
    assert bool(ops.crc_status(plan, got).all())
    bad = want.copy()
    flip = np.arange(bs) % 2 == 0
    col = rng.integers(0, k + deg, bs)
    bad[flip, col[flip]] = 1 - bad[flip, col[flip]]
    ok = (_np_parity(bad[:, :k], name) == bad).all(axis=1)
    assert np.array_equal(ok, ~flip)  # a single flip never passes
    assert np.array_equal(ops.crc_status(plan, torch.from_numpy(bad).cuda()).cpu().numpy(), ok)


def test_gather_and_rate_recover_column_limits():
    """Through the C entry points: the largest table the kernels stage in LDS is accepted and gives the
    right rows (4099 rows: two per block), one more column is PL_EINVAL."""
    import ctypes

    from polar_amd import _lib
    assert torch.cuda.is_available()
    L, st = _lib.lib(), _lib.current_stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    rng = np.random.default_rng(4096)
    bs = 4099

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    n_in = 1000
    x = rng.standard_normal((bs, n_in)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    for n_out, rc in ((4096, _lib.PL_OK), (4097, _lib.PL_EINVAL)):
        idx = rng.integers(0, n_in, n_out).astype(np.int32)
        out = torch.full((bs, n_out), float("nan"), device="cuda")
        idx_d = torch.from_numpy(idx).cuda()  # named: a table must outlive the launch that reads it
        assert L.pl_gather_rows(p(xd), bs, n_in, p(idx_d), n_out, p(out), st) == rc, n_out
        torch.cuda.synchronize()
        if rc == _lib.PL_OK:
            assert np.array_equal(out.cpu().numpy(), x[:, idx])
        else:
            assert b"pl_gather_rows" in L.pl_last_error_string() and bool(torch.isnan(out).all())
    e = 1500
    y = rng.standard_normal((bs, e)).astype(np.float32)
    yd = torch.from_numpy(y).cuda()
    for n, rc in ((2048, _lib.PL_OK), (2049, _lib.PL_EINVAL)):
        a = rng.integers(-1, e, n).astype(np.int32)
        b = np.where(rng.random(n) < 0.3, rng.integers(0, e, n), -1).astype(np.int32)
        f = rng.standard_normal(n).astype(np.float32)
        out = torch.full((bs, n), float("nan"), device="cuda")
        a_d, b_d, f_d = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(f).cuda()
        assert a_d.data_ptr() != b_d.data_ptr() != f_d.data_ptr()
        got = L.pl_rate_recover(p(yd), bs, e, p(a_d), p(b_d), p(f_d), n, p(out), st)
        assert got == rc, n
        torch.cuda.synchronize()
        if rc == _lib.PL_OK:
            want = np.where(a[None, :] >= 0, y[:, np.maximum(a, 0)], f[None, :])
            both = (a >= 0) & (b >= 0)
            want[:, both] = y[:, a[both]] + y[:, b[both]]
            assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))
        else:
            assert b"pl_rate_recover" in L.pl_last_error_string() and bool(torch.isnan(out).all())
