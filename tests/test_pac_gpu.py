"""The PAC kernels (csrc/pac_kernel.hip: pl_pac_encode, pl_pac_decode) against the numpy restatement
tests/golden/pac_ref.py, value for value: decoded bits and path metrics are np.array_equal, ties included.

Every case decodes 67 rows (9 at n = 1024) of all three input kinds of pac_ref.make_inputs: the four special
rows, AWGN rows, and integer LLRs that tie at almost every fork.  The decoder gives a row one single-wave
work-group and has no grid stride, so 67 rows are 67 work-groups: more than one, and ragged against the encoder's
codewords-per-wave share at every n.  Restatement outputs are computed once per case and shared.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pac_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C133 = pac_ref.CONV_133
CONVS = {"1": (1,), "11": (1, 1), "133": C133,
         "bit31": tuple(int(b) for b in np.r_[1, np.random.default_rng(31).integers(0, 2, 30), 1])}
LLR_MAX = 30.0


@pytest.fixture(scope="module")
def pa():
    import polar_amd
    from polar_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    assert hasattr(_lib.lib(), "pl_pac_decode") and hasattr(_lib.lib(), "pl_pac_encode")
    return polar_amd


@functools.lru_cache(maxsize=None)
def _fp(n, kind):
    if kind == "half":
        return np.sort(np.random.default_rng(n).permutation(n)[: n // 2])
    if kind == "k1":
        return np.arange(n - 1)
    if kind == "kn":
        return np.zeros(0, np.int64)
    assert kind == "rm" and n == 128
    import polar_amd
    return np.sort(polar_amd.reference_frozen_pos(64, 128).numpy().astype(np.int64))


@functools.lru_cache(maxsize=None)
def _plan(n, kind, f_mode=0, list_size=1, llr_max=LLR_MAX):
    import polar_amd
    from polar_amd import _lib
    return _lib.Plan(n, polar_amd.frozen_mask(_fp(n, kind), n), list_size, f_mode, llr_max, flags=_lib.PL_PLAN_GENERIC)


@functools.lru_cache(maxsize=None)
def _case(n, kind, L, conv):
    """(logits, restatement bits, restatement metrics), computed once."""
    fp = _fp(n, kind)
    rows = 9 if n >= 1024 else 67
    x = pac_ref.make_inputs(fp, n, CONVS[conv], LLR_MAX, rows, seed=1000 * n + L)
    bits, pm = pac_ref.pac_decode(x, fp, n, L, conv=CONVS[conv], llr_max=LLR_MAX)
    for a in (x, bits, pm):
        a.setflags(write=False)
    return x, bits, pm


def _mask(conv):
    return pac_ref.conv_mask(CONVS[conv])


CASES = [(2, "half", 4, "133"), (4, "half", 4, "133"), (8, "half", 4, "133"),
         (32, "half", 4, "133"), (128, "rm", 4, "133"), (128, "rm", 32, "133"),
         *[(64, "half", L, "133") for L in (1, 2, 8, 32)], *[(256, "half", L, "133") for L in (1, 2, 8, 32)],
         (1024, "half", 32, "133"), (512, "half", 4, "bit31"),
         *[(64, "half", 8, c) for c in ("1", "11", "bit31")], (8, "half", 4, "bit31"),
         (64, "k1", 4, "133"), (64, "kn", 4, "133"), (64, "kn", 32, "bit31"), (16, "k1", 2, "11")]


@pytest.mark.parametrize("n,kind,L,conv", CASES, ids=lambda v: str(v))
def test_decode_equals_the_restatement(pa, n, kind, L, conv):
    x, bits, pm = _case(n, kind, L, conv)
    xd = torch.tensor(x, device=DEV)
    got, gpm = pa.ops.pac_decode(_plan(n, kind), _mask(conv), L, xd, return_pm=True)
    got8 = pa.ops.pac_decode(_plan(n, kind), _mask(conv), L, xd, out_dtype=torch.uint8)  # out_pm NULL
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got8.dtype == torch.uint8 and gpm.dtype == torch.float32
    bad = np.flatnonzero((got.cpu().numpy() != bits).any(1))
    assert bad.size == 0, f"rows {bad[:8]} differ"
    assert np.array_equal(gpm.cpu().numpy(), pm)
    assert np.array_equal(got8.cpu().numpy(), bits)


def test_mask_bit31_is_set():
    assert _mask("bit31") >> 31 == 1 and _mask("bit31") & 1


@pytest.mark.parametrize("n", [64, 256])
def test_plain_l1_equals_sc_decode(pa, n):
    """conv = (1,), L = 1 is min-sum SC (the generic kernel of a PL_PLAN_GENERIC plan) wherever no leaf LLR is
    exactly zero: there SC decides 1 and the list rule, a zero penalty for both values, keeps candidate 0.  The
    inputs have no zero; inside the tree an exact zero comes from g(+-llr_max, -+llr_max) of two saturated f
    values, so the plan's llr_max is set out of the reach of these rows (both decoders clip at the plan's)."""
    fp = _fp(n, "half")
    x = pac_ref.awgn_rows(fp, n, (1,), 67, 2.0, np.random.default_rng(n))
    assert (x != 0).all() and np.abs(x).sum(1).max() < 1.0e5
    xd = torch.tensor(x, device=DEV)
    plan = _plan(n, "half", llr_max=1.0e5)
    assert plan.kernel()[0] == "generic"
    assert torch.equal(pa.ops.pac_decode(plan, 1, 1, xd), pa.ops.sc_decode(plan, xd))


@pytest.mark.parametrize("n,kind,conv", sorted({(c[0], c[1], c[3]) for c in CASES}), ids=lambda v: str(v))
def test_encode_equals_the_restatement_and_round_trips(pa, n, kind, conv):
    fp = _fp(n, kind)
    k = n - len(fp)
    rows = 9 if n >= 1024 else 67
    data = np.random.default_rng(n + k).integers(0, 2, (rows, k)).astype(np.float32)
    cw = pa.ops.pac_encode(_plan(n, kind), _mask(conv), torch.from_numpy(data).to(DEV))
    assert np.array_equal(cw.cpu().numpy(), pac_ref.pac_encode(data, fp, n, CONVS[conv]).astype(np.float32))
    back = pa.ops.pac_decode(_plan(n, kind), _mask(conv), 4, (2.0 * cw - 1.0) * 6.0)
    assert np.array_equal(back.cpu().numpy(), data)


def test_modules_and_osd_of_the_pac_code(pa):
    fp = pa.reference_frozen_pos(16, 32)
    enc = pa.PACEncoder(fp, 32)
    assert (enc.k, enc.n) == (16, 32) and pa.conv_from_octal("133") == C133 == enc.conv
    gm = enc.generator_matrix()
    assert np.array_equal(gm, pac_ref.generator_matrix(np.sort(fp.numpy()), 32, C133))
    data = torch.from_numpy(np.random.default_rng(5).integers(0, 2, (2, 5, 16)).astype(np.float32))
    cw = enc(data)  # CPU in, CPU out
    assert cw.device.type == "cpu" and cw.shape == (2, 5, 32)
    logits = (2.0 * cw - 1.0) * 7.0
    osd = pa.OSDecoder(2, enc)
    assert torch.equal(osd(logits), cw)
    dec = pa.PAC_Dec(fp, 32, list_size=8)
    assert torch.equal(dec(logits), data) and dec.last_pm.shape == (2, 5, 8) and bool((dec.last_pm[..., 0] == 0).all())
    assert torch.equal(dec(logits.to(DEV)).cpu(), data)
    from polar_amd import channel
    model = channel.System_AWGN_model(32, 16, enc, dec, device=DEV)
    b, b_hat = model(13, 30.0)
    assert torch.equal(b.cpu(), b_hat.cpu())
    for bad in (dict(list_size=3), dict(list_size=64), dict(conv=(0, 1)), dict(conv=(1,) * 33), dict(llr_max=0.0)):
        with pytest.raises(ValueError):
            pa.PAC_Dec(fp, 32, **bad)
    with pytest.raises(ValueError):
        pa.PAC_Dec(torch.arange(1024), 2048)


def test_error_codes(pa):
    from polar_amd import _lib
    L = _lib.lib()
    n, k = 64, 32
    plan = _plan(n, "half")
    x = torch.zeros((3, n), device=DEV)
    out = torch.zeros((3, k), device=DEV)
    cw = torch.zeros((3, n), device=DEV)
    P = ctypes.c_void_p

    def dec(plan_h=plan.handle, mask=1, ls=4, llr=x.data_ptr(), bs=3, o=out.data_ptr(), kind=_lib.PL_OUT_F32):
        return L.pl_pac_decode(plan_h, mask, ls, P(llr), bs, P(o), kind, P(0), P(0)), L.pl_last_error_string().decode()

    def enc(plan_h=plan.handle, mask=1, d=out.data_ptr(), bs=3, c=cw.data_ptr()):
        return L.pl_pac_encode(plan_h, mask, P(d), bs, P(c), P(0)), L.pl_last_error_string().decode()

    assert dec()[0] == _lib.PL_OK and enc()[0] == _lib.PL_OK
    assert dec(bs=0, llr=0, o=0)[0] == _lib.PL_OK and enc(bs=0, d=0, c=0)[0] == _lib.PL_OK
    for kw, word in ((dict(plan_h=None), "plan"), (dict(mask=2), "conv_mask"), (dict(mask=0), "conv_mask"),
                     (dict(ls=0), "list_size"), (dict(ls=3), "list_size"), (dict(ls=64), "list_size"),
                     (dict(ls=-8), "list_size"), (dict(bs=-1), "bs"), (dict(kind=2), "out_kind"),
                     (dict(llr=0), "llr_logits"), (dict(o=0), "out_bits")):
        rc, msg = dec(**kw)
        assert rc == _lib.PL_EINVAL and "pl_pac_decode" in msg and word in msg, (kw, rc, msg)
    for kw, word in ((dict(plan_h=None), "plan"), (dict(mask=6), "conv_mask"), (dict(bs=-1), "bs"),
                     (dict(d=0), "data_bits"), (dict(c=0), "codewords")):
        rc, msg = enc(**kw)
        assert rc == _lib.PL_EINVAL and "pl_pac_encode" in msg and word in msg, (kw, rc, msg)
    exact = _plan(n, "half", f_mode=_lib.PL_F_EXACT)
    rc, msg = dec(plan_h=exact.handle)
    assert rc == _lib.PL_ENOTSUP and "PL_F_MINSUM" in msg
    crc = _lib.Plan(n, pa.frozen_mask(_fp(n, "half"), n), 8, 0, LLR_MAX, flags=_lib.PL_PLAN_GENERIC)
    crc.set_crc(11, 0x621)
    rc, msg = dec(plan_h=crc.handle)
    assert rc == _lib.PL_ENOTSUP and "CRC" in msg
    crc.set_crc(0, 0)
    assert dec(plan_h=crc.handle)[0] == _lib.PL_OK  # the plan's own list_size is not used
    big = _lib.Plan(2048, pa.frozen_mask(np.arange(1024), 2048), 1, 0, LLR_MAX, flags=_lib.PL_PLAN_GENERIC)
    xb, ob = torch.zeros((1, 2048), device=DEV), torch.zeros((1, 2048), device=DEV)
    rc, msg = dec(plan_h=big.handle, llr=xb.data_ptr(), bs=1, o=ob.data_ptr())
    assert rc == _lib.PL_ENOTSUP and "160 KiB" in msg and "2048" in msg
    rc, msg = enc(plan_h=big.handle, d=ob.data_ptr(), bs=1, c=xb.data_ptr())
    assert rc == _lib.PL_ENOTSUP and "1024" in msg
    torch.cuda.synchronize()


def _shifted(t, off):
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size() % 16 and v.is_contiguous()
    return v


def test_shifted_strided_misshapen_and_out(pa):
    n, kind, L, conv = 64, "half", 8, "133"
    x, bits, pm = _case(n, kind, L, conv)
    plan, mask, k = _plan(n, kind), _mask(conv), n // 2
    xd = torch.tensor(x, device=DEV)
    want = torch.tensor(bits, device=DEV)
    wide = torch.zeros((x.shape[0], 2 * n), device=DEV)
    wide[:, ::2] = xd
    for what, v in (("shift 1", _shifted(xd, 1)), ("shift 3", _shifted(xd, 3)), ("column stride", wide[:, ::2]),
                    ("transposed", xd.t().contiguous().t()), ("fp64", xd.double()), ("fp16 grid", None)):
        if v is None:  # values exact in fp16: the integer rows
            v, ref = xd[-32:].half(), want[-32:]
        else:
            ref = want
        got = pa.ops.pac_decode(plan, mask, L, v, out_dtype=torch.uint8)
        assert torch.equal(got, ref), what
    for off in (1, 2, 3):  # out of both kinds past a 16-byte boundary, inside sentinels
        for dt in (torch.float32, torch.uint8):
            buf = torch.full((16 + off + want.numel() + 16,), 7, dtype=dt, device=DEV)
            out = buf[16 + off: 16 + off + want.numel()].view(want.shape)
            assert pa.ops.pac_decode(plan, mask, L, xd, out=out) is out
            assert torch.equal(out.to(torch.uint8), want) and bool((buf[:16 + off] == 7).all()) and \
                bool((buf[16 + off + want.numel():] == 7).all()), (off, dt)
    data = want.float()
    cw = pa.ops.pac_encode(plan, mask, data)
    assert torch.equal(pa.ops.pac_encode(plan, mask, _shifted(data, 1), out=_shifted(torch.zeros_like(cw), 3)), cw)
    assert torch.equal(pa.ops.pac_encode(plan, mask, want), cw)  # uint8 data bits are converted
    empty = pa.ops.pac_decode(plan, mask, L, xd[:0], return_pm=True)
    assert empty[0].shape == (0, k) and empty[1].shape == (0, L) and pa.ops.pac_encode(plan, mask, data[:0]).shape == (0, n)
    # the refusals, the exception types of the other entry points
    for bad in (xd[:, :-1], xd[0], xd[:66].reshape(-1, 2, n)):
        with pytest.raises(ValueError):
            pa.ops.pac_decode(plan, mask, L, bad)
    with pytest.raises(RuntimeError):
        pa.ops.pac_decode(plan, mask, L, xd.cpu())
    with pytest.raises(RuntimeError):
        pa.ops.pac_encode(plan, mask, data.cpu())
    for bad_out in (torch.zeros((x.shape[0], k + 1), device=DEV), torch.zeros((k, x.shape[0]), device=DEV).t(),
                    torch.zeros((x.shape[0], k)), torch.zeros((x.shape[0], k), dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError):
            pa.ops.pac_decode(plan, mask, L, xd, out=bad_out)
    with pytest.raises(ValueError):
        pa.ops.pac_encode(plan, mask, data, out=torch.zeros((x.shape[0], n), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        pa.ops.pac_encode(plan, mask, data[:, :-1])
    for bad_l in (0, 3, 64):
        with pytest.raises(ValueError):
            pa.ops.pac_decode(plan, mask, bad_l, xd)
    for bad_mask in (0, 2, 2 ** 32 + 1, 1.0, True):
        with pytest.raises(ValueError):
            pa.ops.pac_decode(plan, bad_mask, L, xd)


def test_graph_capture(pa):
    n, kind, L, conv = 64, "half", 8, "133"
    x, bits, pm = _case(n, kind, L, conv)
    plan, mask = _plan(n, kind), _mask(conv)
    xd = torch.tensor(x, device=DEV)
    static_x = torch.zeros_like(xd)
    out = torch.zeros((x.shape[0], n // 2), dtype=torch.uint8, device=DEV)
    graph = pa.ops.LaunchGraph(lambda: pa.ops.pac_decode(plan, mask, L, static_x, out=out), 1, device=DEV)
    for rows in (xd, xd.flip(0)):
        static_x.copy_(rows)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, pa.ops.pac_decode(plan, mask, L, rows, out_dtype=torch.uint8))
    assert np.array_equal(out.flip(0).cpu().numpy(), bits)
