"""CPU-side checks of 16/64/256-QAM in the link producers (tests/test_qam_gpu.py runs the kernels):
the op-by-op blocks against the reference's (tests/golden/qam.npz, made by make_golden_qam.py), the
two new C-ABI symbols and their argument checks, the constructors' and the CLI's new argument.

demap_f64() is the reference's demapper formula (my_sn/trans/mapping.py:225-241, :195-205) in
float64; the GPU test measures the kernels against it within DEMAP_BOUND.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "qam.npz")
MS = (2, 4, 6, 8)

# max over the fixture's y (320 symbols, |y| up to 10, on decision boundaries, no = 0.5 and 0.002) and
# m = 2, 4, 6, 8 of |llr_fp32 - llr_f64| / max(1, |llr_f64|) for the op-by-op fp32 Demapper, measured
# on the CPU by test_demapper_fp32_error_is_the_recorded_one (2.901e-04, at m = 8, no = 0.002: |y| = 10 puts the
# exponents near 5e4, where one fp32 ulp is 4e-3, under logits of a few thousand); the fused
# kernels get 4x that (the per-axis form reorders the sums; a device exp / log is a couple of ulp).
DEMAP_ERR_FP32 = 2.91e-04
DEMAP_BOUND = 4 * DEMAP_ERR_FP32


def demap_f64(y, points, no):
    """Logits log P(b=1)/P(b=0), float64 [..., m * symbols], of complex received symbols y [..., symbols]
    for the constellation `points` (complex [2^m], label = index, first bit most significant) at noise
    variance `no`: log sum_{c: b=1} exp(-|y - c|^2 / no) - log sum_{c: b=0} exp(-|y - c|^2 / no)."""
    y = np.asarray(y, dtype=np.complex128)
    pts = np.asarray(points, dtype=np.complex128)
    m = int(np.log2(len(pts)))
    d = y[..., None] - pts
    e = -(d.real ** 2 + d.imag ** 2) / float(no)
    lab = (np.arange(len(pts))[:, None] >> np.arange(m - 1, -1, -1)[None, :]) & 1   # [2^m, m]

    def lse(mask):
        x = np.where(mask.T[(None,) * (e.ndim - 1)], e[..., None, :], -np.inf)      # [..., m, 2^m]
        mx = x.max(axis=-1, keepdims=True)
        return (mx + np.log(np.exp(x - mx).sum(axis=-1, keepdims=True)))[..., 0]
    llr = lse(lab == 1) - lse(lab == 0)                                              # [..., symbols, m]
    return llr.reshape(*y.shape[:-1], y.shape[-1] * m)


def rel_err(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))))


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("m", MS)
def test_constellation_and_mapper_match_the_reference(gold, m):
    from polar_amd import channel
    const = channel.QamConstellation(m)
    assert np.array_equal(const.points.numpy(), gold[f"points_{m}"])
    out = channel.Mapper(const)(tc.from_numpy(gold[f"map_bits_{m}"]))
    assert np.array_equal(out.numpy(), gold[f"map_out_{m}"])
    # every symbol index once, in order: the mapper's output is the constellation itself
    assert np.array_equal(out.numpy()[0, : 2 ** m], gold[f"points_{m}"])
    # the per-axis structure the kernels use: re = PAM level of b[0::2], im = that of b[1::2], the
    # levels pam / sqrt(var) computed in double and rounded once (capi.cpp qam_levels)
    h = m // 2
    var = sum(v * v for v in range(1, 2 ** h, 2)) * (2.0 if h == 1 else 1.0 / 2 ** (h - 2))

    def pam(b):
        return (1 - 2 * b[0]) * (2 ** (len(b) - 1) - pam(b[1:])) if len(b) > 1 else 1 - 2 * b[0]
    lev = np.array([pam([int(c) for c in np.binary_repr(a, h)]) / np.sqrt(var) for a in range(2 ** h)]).astype(np.float32)
    for i, p in enumerate(gold[f"points_{m}"]):
        b = np.binary_repr(i, m)
        assert p.real == lev[int(b[0::2], 2)] and p.imag == lev[int(b[1::2], 2)], (m, i)


@pytest.mark.parametrize("m", MS)
def test_demapper_matches_the_reference(gold, m):
    from polar_amd import channel
    dem = channel.Demapper(channel.QamConstellation(m))
    y = tc.from_numpy(gold[f"demap_y_{m}"])
    for i, no in enumerate(gold["demap_no"]):
        got = dem([y, tc.tensor(no, dtype=tc.float32)]).numpy()[0]
        assert np.array_equal(got, gold[f"demap_llr_{m}"][i]), (m, no)
        assert np.isfinite(got).all()


def test_demapper_fp32_error_is_the_recorded_one(gold):
    """The fp32 op-by-op Demapper against the float64 formula on the fixture's y: the measurement
    DEMAP_BOUND is 4x of.  Printed per (m, no); the recorded constant must not be below it."""
    worst = 0.0
    for m in MS:
        for i, no in enumerate(gold["demap_no"]):
            want = demap_f64(gold[f"demap_y_{m}"][0], gold[f"points_{m}"], no)
            e = rel_err(gold[f"demap_llr_{m}"][i], want)
            print(f"m={m} no={no}: fp32 demapper error {e:.3e}")
            worst = max(worst, e)
    print(f"max {worst:.3e}, recorded {DEMAP_ERR_FP32:.3e}")
    assert 0.8 * DEMAP_ERR_FP32 <= worst <= DEMAP_ERR_FP32


def test_demap_f64_is_the_per_axis_form(gold):
    """Why the kernels may work per axis: for Gray square QAM the 2-D sum factors, so the logit of a
    real-axis bit depends on Re(y) and the PAM levels only."""
    for m in (4, 6, 8):
        pts = gold[f"points_{m}"].astype(np.complex128)
        y = gold[f"demap_y_{m}"][0].astype(np.complex128)
        h = m // 2
        lev = np.array([pts[int("".join(c + "0" for c in np.binary_repr(a, h)), 2)].real for a in range(2 ** h)])
        lab = (np.arange(2 ** h)[:, None] >> np.arange(h - 1, -1, -1)[None, :]) & 1
        for no in (0.5, 0.002):
            want = demap_f64(y, pts, no).reshape(len(y), h, 2)
            for ax, comp in ((0, y.real), (1, y.imag)):
                e = -(comp[:, None] - lev[None, :]) ** 2 / no
                mx = e.max(axis=1, keepdims=True)
                w = np.exp(e - mx)
                got = np.log(w @ lab + 1e-300) - np.log(w @ (1 - lab) + 1e-300)
                ok = np.abs(want[:, :, ax]) < 600          # beyond, the shared shift underflows in float64 too
                assert np.allclose(got[ok], want[:, :, ax][ok], rtol=1e-9, atol=1e-9), (m, no, ax)


def test_system_model_16qam_reproduces_reference_llrs(gold):
    from polar_amd import channel, frozen
    k, n, m = int(gold["bler_k"]), int(gold["bler_n"]), int(gold["bler_m"])
    G, _, fp = frozen.get_Kern_frozen_bits(n, n - k, frozen.F2)
    model = channel.System_AWGN_model(n, k, channel.DenseEncoder(fp, n, G), None, num_bits_per_symbol=m)
    assert model.n_bits_per_sym == 4
    tc.manual_seed(int(gold["bler_seed"]))
    _, _, llr = model.llrs(64, tc.tensor(float(gold["bler_ebno_db"]), dtype=tc.float32))
    assert np.array_equal(llr.numpy(), gold["bler_llr64"])
    assert 0.05 <= float(gold["bler_bler"]) <= 0.5 and int(gold["bler_rows"]) == 4096


def test_new_symbols_declared_and_bound():
    from polar_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polar_mi355x.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in (("pl_awgn_qam_llr", 12), ("pl_nr_awgn_qam_llr", 21)):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(L, name).argtypes) == nargs


def test_qam_entry_points_reject_bad_arguments_without_gpu():
    """Argument validation happens before any HIP call; each message names its argument."""
    from polar_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    out = ctypes.cast(buf, ctypes.c_void_p)

    def plain(m, it=0, row0=0, bs=4, no=0.5, y=None, llr=out):
        return L.pl_awgn_qam_llr(None, m, 1, it, row0, bs, no, None, None, y, llr, None)

    def nr(m, e=96, it=0, row0=0, bs=4, no=0.5, y=None, llr=out):
        return L.pl_nr_awgn_qam_llr(None, m, 20, None, 11, None, e, None, None, None, 1, it, row0, bs, no, None, None, y,
                                    None, llr, None)
    for call, name in ((plain, b"pl_awgn_qam_llr"), (nr, b"pl_nr_awgn_qam_llr")):
        for m in (0, 1, 3, 5, 10, -4):
            assert call(m) == _lib.PL_EINVAL
            assert name in L.pl_last_error_string() and b"bits_per_symbol" in L.pl_last_error_string()
        assert call(2, y=out) == _lib.PL_EINVAL and b"y_out" in L.pl_last_error_string()
        for no in (0.0, -1.0, float("nan")):
            assert call(4, no=no) == _lib.PL_EINVAL and b"no must be" in L.pl_last_error_string()
        assert call(4, it=2 ** 32) == _lib.PL_EINVAL and b"iteration" in L.pl_last_error_string()
        assert call(4, bs=-1) == _lib.PL_EINVAL and b"bs" in L.pl_last_error_string()
        assert call(4, row0=-1) == _lib.PL_EINVAL and b"row0" in L.pl_last_error_string()
        assert call(4, llr=None) == _lib.PL_EINVAL and b"llr_out" in L.pl_last_error_string()
        assert call(4) == _lib.PL_EINVAL and b"plan" in L.pl_last_error_string()   # everything else fine
    for m, e in ((4, 98), (6, 100), (8, 100), (4, 0), (8, 2184), (6, 2178)):
        assert nr(m, e=e) == _lib.PL_EINVAL
        assert b"E must be" in L.pl_last_error_string(), (m, e, L.pl_last_error_string())
    assert nr(2, e=97) == _lib.PL_EINVAL   # m = 2: pl_nr_awgn_qpsk_llr's own checks


def test_constructors_refuse_an_m_the_length_does_not_admit():
    import contextlib
    import io
    from polar_amd import channel, frozen, ops
    from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
    fp = frozen.reference_frozen_pos(32, 64)
    for m in (6, 3, 0, 16):
        with pytest.raises(ValueError, match="num_bits_per_symbol"):
            channel.FusedAWGN(64, 32, fp, None, device="cuda:0", num_bits_per_symbol=m)
        with pytest.raises(ValueError, match="num_bits_per_symbol"):
            channel.System_AWGN_model(64, 32, None, None, num_bits_per_symbol=m)
    model = channel.FusedAWGN(64, 32, fp, None, device="cuda:0", num_bits_per_symbol=8)
    assert model.n_bits_per_sym == 8
    assert channel.FusedAWGN(64, 32, fp, None, device="cuda:0").n_bits_per_sym == 2
    with contextlib.redirect_stdout(io.StringIO()):
        enc = Polar5GEncoder(20, 100)      # E = 100: 4 divides it, 6 and 8 do not
        dec = Polar5GDecoder(enc)
    for m in (6, 8, 5):
        with pytest.raises(ValueError, match="num_bits_per_symbol"):
            channel.FusedAWGN5G(enc, dec, device="cuda:0", num_bits_per_symbol=m)
        with pytest.raises(ValueError, match="num_bits_per_symbol"):
            channel.System5G_AWGN_model(enc, dec, num_bits_per_symbol=m)
    model = channel.FusedAWGN5G(enc, dec, device="cuda:0", num_bits_per_symbol=4)
    assert model.n_bits_per_sym == 4 and model.coderate == 0.2
    assert channel.ebnodb2no(3.0, 4, 0.2) == pytest.approx(channel.ebnodb2no(3.0, 2, 0.2) / 2)
    assert ops.QAM_BITS_PER_SYMBOL == (2, 4, 6, 8)


def test_cli_flag():
    from polar_amd import cli
    assert cli.parse([]).num_bits_per_symbol == 2
    assert cli.parse(["--num_bits_per_symbol", "6", "--code", "5g"]).num_bits_per_symbol == 6
    with pytest.raises(SystemExit):
        cli.parse(["--num_bits_per_symbol", "3"])
