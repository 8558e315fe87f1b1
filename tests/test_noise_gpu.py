"""GPU tests of the noise the fused Monte-Carlo producers draw, value by value against the float64
restatement tests/golden/noise_ref.py:

  pl_awgn_qpsk_llr / pl_awgn_qpsk_llr_bits, pl_awgn_qam_llr<4|8>, pl_nr_awgn_qpsk_llr,
  pl_nr_awgn_qam_llr<4|6|8> (csrc/channel_kernel.hip) and pl_sc_sim_count (csrc/sc_static.h OUT_SIM).

Every comparison is made on the standardised noise z through noise_ref.compare, within
test_noise_ref.NOISE_BOUND_A / NOISE_BOUND_B (4x the error of the formula op by op in numpy float32,
measured there); no element is left out.  QPSK: z = (llr - a) / s with a = (2c - 1) 2 / no and
s = -2 / sqrt(no) in float64, c the code bit of the oracle's / the op-by-op encoder's code word of the
kernel's own information bits.  QAM: z = (y_out - x) / sqrt(no / 2), x the op-by-op Mapper's symbol.
no is 0.5 and 1.7: there |a| / |s| = 1 / sqrt(no) is about 1, so the float32 rounding of the logit
itself (a relative 6e-8 of a value of the size of s z) is about 1e-7 in z, far below the class A
bound; at no = 1e-7 the logit is all a and the comparison would say nothing.

Keys: (seed, iteration) = (0x123456789ABC, 7), both key words non-zero; row0 = 1000 and 2^32 - 20, so
that the batch crosses the 32-bit row boundary; batches of 301 or 37 rows (100 for the SC kernel),
no multiple of any rows-per-wave count.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import noise_ref  # noqa: E402
from test_noise_ref import (IT, NOISE_BOUND_A, NOISE_BOUND_B, NOS, NR_QAM, NR_QPSK, PLAIN_N, PLAIN_QAM, ROW0S, SEED,  # noqa: E402
                            SIM, SIM_BS, batch, rows_of)
from test_nr_link_gpu import _pair  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def _no32(no):
    """The noise variance the kernel sees (its argument is a float)."""
    return float(np.float32(no))


@functools.lru_cache(maxsize=None)
def _code(n):
    """(generic-flag plan, frozen positions) of an (n / 2, n) code: the reference's from n = 32 on, a
    random frozen set below."""
    import polar_amd
    from polar_amd import _lib
    k = n // 2
    fp = polar_amd.reference_frozen_pos(k, n).numpy() if n >= 32 else \
        np.sort(np.random.default_rng(n).permutation(n)[: n - k])
    return _lib.Plan(n, polar_amd.frozen_mask(fp, n), 1, flags=_lib.PL_PLAN_GENERIC, device=_dev()), fp


def _symbols(cw, m):
    """The op-by-op Mapper's symbols of 0/1 code rows [bs, len] -> float64 [bs, len / m, 2] (re, im)."""
    from polar_amd import channel
    x = channel.Mapper(channel.QamConstellation(m))(torch.as_tensor(cw).cpu().float()).numpy()
    return np.stack([x.real, x.imag], axis=-1).astype(np.float64)


def _z_of_symbols(y, cw, m, no):
    return (y.cpu().numpy().astype(np.float64) - _symbols(cw, m)) / np.sqrt(_no32(no) / 2)


# ---- one draw of each family: the standardised noise the kernel's outputs hold --------------------------

def _plain_qpsk(n, no, row0, bs):
    from polar_amd import ops
    from polar_amd.channel import fused_info_bits
    plan, fp = _code(n)
    u, llr = ops.awgn_qpsk_llr(plan, bs, no, SEED, IT, row0)
    ubits, llr_b = ops.awgn_qpsk_llr_bits(plan, bs, no, SEED, IT, row0)
    assert torch.equal(llr, llr_b) and torch.equal(ubits, ops.pack_bits(u))
    u = u.cpu().numpy()
    assert np.array_equal(u, fused_info_bits(SEED, IT, rows_of(row0, bs), n // 2))
    return noise_ref.noise_of_logits(llr.cpu().numpy(), oracle.polar_encode(u, fp, n), _no32(no))


def _plain_qam(n, m, no, row0, bs):
    from polar_amd import ops
    plan, fp = _code(n)
    u, _, y, _ = ops.awgn_qam_llr(plan, m, bs, no, SEED, IT, row0, with_y=True)
    return _z_of_symbols(y, oracle.polar_encode(u.cpu().numpy(), fp, n), m, no)


def _nr_tables(k, e):
    enc, dec = _pair(k, e)
    g, idx = enc.tables(_dev())
    return enc, (enc.plan(_dev()), k, g, enc.crc_length, idx, *dec.tables(_dev()))


def _nr_qpsk(k, e, no, row0, bs):
    from polar_amd import ops
    enc, tabs = _nr_tables(k, e)
    u, _, ch, _ = ops.nr_awgn_qpsk_llr(*tabs, bs, no, SEED, IT, row0, with_ubits=False, with_ch=True)
    return noise_ref.noise_of_logits(ch.cpu().numpy(), enc(u).cpu().numpy(), _no32(no))


def _nr_qam(k, e, m, no, row0, bs):
    from polar_amd import ops
    enc, tabs = _nr_tables(k, e)
    u, _, _, y, _ = ops.nr_awgn_qam_llr(tabs[0], m, *tabs[1:], bs, no, SEED, IT, row0, with_ubits=False, with_y=True)
    return _z_of_symbols(y, enc(u), m, no)


def _sim(fp, n, no, row0, bs):
    import polar_amd
    from polar_amd import _lib, channel, ops
    spec = _lib.Plan(n, polar_amd.frozen_mask(fp, n), 1, 0, flags=_lib.PL_PLAN_CACHE_ONLY)   # pre-built only
    assert spec.kernel()[0] == "specialized", spec.kernel()
    _, u, llr = ops.sc_sim_count(spec, bs, no, SEED, IT, row0, dump=True)
    cw = channel.GpuEncoder(fp, n)(u)
    return noise_ref.noise_of_logits(llr.cpu().numpy(), cw.cpu().numpy(), _no32(no))


# ---- the acceptance ------------------------------------------------------------------------------------------

def _hold(what, got, want, unit):
    a, b = noise_ref.compare(got, want, unit)
    print(f"{what}: class A {a:.3e} (bound {NOISE_BOUND_A:.2e}), class B {b:.3e} (bound {NOISE_BOUND_B:.2e})")
    assert a <= NOISE_BOUND_A and b <= NOISE_BOUND_B, (what, a, b)
    return a, b


def _hold_case(what, produce, reference, bs):
    """produce(no, row0, bs) -> z of the kernel; reference(rows) -> (z, r_unit): every row0 and no."""
    worst = (0.0, 0.0)
    for row0 in ROW0S:
        want, unit = reference(rows_of(row0, bs))
        for no in NOS:
            err = _hold(f"{what} row0={row0} no={no}", produce(no, row0, bs), want, unit)
            worst = (max(worst[0], err[0]), max(worst[1], err[1]))
    print(f"{what}: worst class A {worst[0]:.3e}, class B {worst[1]:.3e}")


def _hold_shards(what, produce, reference, bs, bs1):
    """Rows [row0, row0 + bs) drawn in two calls, (row0, bs1) and (row0 + bs1, bs - bs1): both against
    the restatement, and together the single call bit for bit."""
    row0, no = ROW0S[1], NOS[1]
    want, unit = reference(rows_of(row0, bs))
    first, second = produce(no, row0, bs1), produce(no, row0 + bs1, bs - bs1)
    _hold(f"{what} shard ({row0}, {bs1})", first, want[:bs1], unit[:bs1])
    _hold(f"{what} shard ({row0 + bs1}, {bs - bs1})", second, want[bs1:], unit[bs1:])
    assert np.array_equal(np.concatenate([first, second]), produce(no, row0, bs)), what


@pytest.mark.parametrize("n", PLAIN_N)
def test_plain_qpsk(n):
    """n = 2: CH = 2; 16: several rows per lane group; up to 128 the flat loop (fewer than 64 chunks per
    row); 256: the first rows-outer size; both entry points."""
    _hold_case(f"pl_awgn_qpsk_llr n={n}", lambda no, row0, bs: _plain_qpsk(n, no, row0, bs),
               lambda rows: noise_ref.plain_noise(SEED, IT, rows, n, with_unit=True), batch(n))


@pytest.mark.parametrize("n,m", PLAIN_QAM)
def test_plain_qam(n, m):
    """(8, 8), (4, 4): one symbol per row, the pair's second half unused."""
    _hold_case(f"pl_awgn_qam_llr n={n} m={m}", lambda no, row0, bs: _plain_qam(n, m, no, row0, bs),
               lambda rows: noise_ref.qam_noise(SEED, IT, rows, n // m, with_unit=True), batch(n))


@pytest.mark.parametrize("k,e", NR_QPSK)
def test_nr_qpsk(k, e):
    """(12, 20): n_polar = 32, 64 rows per wave; (12, 600): several passes of the LDS stage; (20, 90):
    E % 4 = 2, the last block's surplus unused.  The mother-code logits are tied to these channel
    logits by test_nr_link_gpu.test_rate_recovery_exact."""
    _hold_case(f"pl_nr_awgn_qpsk_llr ({k}, {e})", lambda no, row0, bs: _nr_qpsk(k, e, no, row0, bs),
               lambda rows: noise_ref.nr_noise(SEED, IT, rows, e, with_unit=True), batch(e))


@pytest.mark.parametrize("k,e,m", NR_QAM)
def test_nr_qam(k, e, m):
    _hold_case(f"pl_nr_awgn_qam_llr ({k}, {e}) m={m}", lambda no, row0, bs: _nr_qam(k, e, m, no, row0, bs),
               lambda rows: noise_ref.qam_noise(SEED, IT, rows, e // m, with_unit=True), batch(e))


def _sim_codes():
    import polar_amd
    from polar_amd.build import root_half_codes
    codes = [(f"({k}, {n})", polar_amd.reference_frozen_pos(k, n).numpy(), n) for k, n in SIM]
    # n = 1024: the upper channel half of a lane lives in LDS (sc_static.h Ch)
    codes.append(("root halves GEN_SPC", np.flatnonzero(dict(root_half_codes())["GEN_SPC"]), 1024))
    return codes


@pytest.mark.parametrize("which", range(len(SIM) + 1))
def test_sim_kernel(which):
    what, fp, n = _sim_codes()[which]
    _hold_case(f"pl_sc_sim_count {what}", lambda no, row0, bs: _sim(fp, n, no, row0, bs),
               lambda rows: noise_ref.sim_noise(SEED, IT, rows, n, with_unit=True), SIM_BS)


# (family, rows per wave of the case): bs1 = 13 is no multiple of any of them
@pytest.mark.parametrize("family", ["plain qpsk", "plain qam", "nr qpsk", "nr qam", "sim"])
def test_shards(family):
    bs1 = 13
    if family == "plain qpsk":      # n = 256: 8 rows per wave
        _hold_shards(family, lambda no, row0, bs: _plain_qpsk(256, no, row0, bs),
                     lambda rows: noise_ref.plain_noise(SEED, IT, rows, 256, with_unit=True), 301, bs1)
    elif family == "plain qam":     # n = 64: 32 rows per wave
        _hold_shards(family, lambda no, row0, bs: _plain_qam(64, 4, no, row0, bs),
                     lambda rows: noise_ref.qam_noise(SEED, IT, rows, 16, with_unit=True), 301, bs1)
    elif family == "nr qpsk":       # (100, 180): n_polar = 256, 8 rows per wave
        assert _pair(100, 180)[0].n_polar == 256
        _hold_shards(family, lambda no, row0, bs: _nr_qpsk(100, 180, no, row0, bs),
                     lambda rows: noise_ref.nr_noise(SEED, IT, rows, 180, with_unit=True), 301, bs1)
    elif family == "nr qam":        # (20, 90): n_polar = 128, 16 rows per wave
        assert _pair(20, 90)[0].n_polar == 128
        _hold_shards(family, lambda no, row0, bs: _nr_qam(20, 90, 6, no, row0, bs),
                     lambda rows: noise_ref.qam_noise(SEED, IT, rows, 15, with_unit=True), 301, bs1)
    else:                           # (128, 256): 16 rows per wave
        import polar_amd
        fp = polar_amd.reference_frozen_pos(128, 256).numpy()
        _hold_shards(family, lambda no, row0, bs: _sim(fp, 256, no, row0, bs),
                     lambda rows: noise_ref.sim_noise(SEED, IT, rows, 256, with_unit=True), SIM_BS, bs1)


# ---- model level ------------------------------------------------------------------------------------------------

def _keys(model, streams=((2, 5), (2, 6), (3, 5))):
    """(key, iteration, first row) of the draws of `streams` in the model's next two epochs."""
    out = []
    for _ in range(2):
        model.next_epoch()
        for s in streams:
            it, row0 = model._draw(8, s)
            out.append((model.key(), it, row0))
    return out


def test_fused_awgn_model():
    import polar_amd
    from polar_amd import channel
    k, n, bs = 128, 256, 301
    fp = polar_amd.reference_frozen_pos(k, n)
    model = channel.FusedAWGN(n, k, fp, None, device=_dev(), seed=SEED, row0=1000)
    model.next_epoch()
    u, _, llr = model.llrs(bs, 0.0, stream=(2, 5))
    no = float(channel.ebnodb2no(0.0, 2, k / n))             # 1.0
    key = model.key()
    assert model.epoch == 1 and key != SEED
    rows = rows_of((2 << 32) + 1000, bs)                      # the point is the row's high word
    assert np.array_equal(u.cpu().numpy(), channel.fused_info_bits(key, 5, rows, k))
    want, unit = noise_ref.plain_noise(key, 5, rows, n, with_unit=True)
    got = noise_ref.noise_of_logits(llr.cpu().numpy(), oracle.polar_encode(u.cpu().numpy(), fp.numpy(), n), _no32(no))
    _hold("FusedAWGN.llrs stream=(2, 5), epoch 1", got, want, unit)
    keys = _keys(model)
    assert len(set(keys)) == len(keys) == 6
    assert len({(s, it) for s, it, row in keys if row >> 32 == 2}) == 4   # two iterations x two epochs
    assert len({s for s, _, _ in keys}) == 2                              # one key per epoch


def test_fused_awgn5g_model():
    """(64, 200): puncturing, so every channel logit is one mother-code logit (no repetition sum) and
    llrs()'s mother-code rows hold the whole draw."""
    from polar_amd import channel
    k, e, bs = 64, 200, 301
    enc, dec = _pair(k, e)
    a, b, fill = dec._rec
    assert (b < 0).all() and np.array_equal(np.sort(a[a >= 0]), np.arange(e))
    model = channel.FusedAWGN5G(enc, dec, device=_dev(), seed=SEED, row0=1000)
    model.next_epoch()
    u, _, llr = model.llrs(bs, 0.0, stream=(2, 5))
    no = float(channel.ebnodb2no(0.0, 2, k / e))
    key = model.key()
    rows = rows_of((2 << 32) + 1000, bs)
    assert np.array_equal(u.cpu().numpy(), channel.fused_info_bits(key, 5, rows, k))
    llr = llr.cpu().numpy()
    assert np.array_equal(llr[:, a < 0], np.broadcast_to(fill[a < 0], (bs, int((a < 0).sum()))))
    ch = np.empty((bs, e), dtype=np.float32)
    ch[:, a[a >= 0]] = llr[:, a >= 0]                          # mother position j holds channel logit a[j]
    want, unit = noise_ref.nr_noise(key, 5, rows, e, with_unit=True)
    got = noise_ref.noise_of_logits(ch, enc(u).cpu().numpy(), _no32(no))
    _hold("FusedAWGN5G.llrs stream=(2, 5), epoch 1", got, want, unit)
    keys = _keys(model)
    assert len(set(keys)) == len(keys) == 6 and len({s for s, _, _ in keys}) == 2
