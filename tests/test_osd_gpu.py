"""polar_amd.OSDecoder / pl_osd_decode on the GPU against the reference's recorded results
(tests/golden/osd.npz, my_sn/fec/osd/dec.py::OSDecoder) and the numpy restatement (tests/golden/osd_ref.py).

Parity with the reference is claimed on rows without equal |llr| (the fixture generator asserts there
are none, that nothing is clipped, and that the winner leads the runner-up by > 1e-9 in Delta); the tie
policy -- among equal |llr| the lower index first -- is checked against the restatement only.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import osd_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "osd.npz")
DEV = "cuda:0"


class DenseEncoder:
    """u -> u G mod 2 with .k: the reference-style dense encoder."""

    def __init__(self, g):
        self.g = torch.tensor(np.asarray(g, dtype=np.float32))
        self.k = int(self.g.shape[0])

    def __call__(self, u):
        return (u.to(self.g.device, torch.float32) @ self.g) % 2


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def _set_names():
    with np.load(GOLDEN) as d:
        return [str(s) for s in d["sets"]]


def _plan(g, t):
    from polar_amd import _lib
    return _lib.OsdPlan(np.asarray(g, dtype=np.uint8), t, device=DEV)


def _decode(plan, llr, out_dtype=torch.float32):
    from polar_amd import ops
    x = torch.as_tensor(np.asarray(llr, dtype=np.float32), device=DEV)
    cw, dist, pat = ops.osd_decode(plan, x, out_dtype=out_dtype, return_dist=True, return_pattern=True)
    return cw.cpu().numpy(), dist.cpu().numpy(), pat.cpu().numpy()


_REF = {}


def _restated(name, g, llr, t):
    """The restatement's result of a case, computed once and shared."""
    if name not in _REF:
        _REF[name] = osd_ref.osd_decode(g, llr, t)
    return _REF[name]


polar_like, awgn_logits = osd_ref.polar_like, osd_ref.awgn_logits


@pytest.mark.parametrize("name", _set_names())
def test_parity_with_the_reference_and_the_restatement(golden, name):
    g, llr, ref_cw, ref_d = (golden[f"{name}_{f}"] for f in ("G", "llr", "cw", "d"))
    t = int(name.split("t")[-1])
    cw, dist, pat = _decode(_plan(g, t), llr)
    want_cw, want_dist, want_pat, _ = _restated(name, g, llr, t)
    assert np.array_equal(cw, ref_cw.astype(np.float32)), int((cw != ref_cw).any(1).sum())
    assert np.array_equal(cw, want_cw.astype(np.float32))
    assert np.array_equal(pat, want_pat)
    # the fp64 softplus mean of the word that was returned
    l = np.clip(llr, -100, 100).astype(np.float64)
    mine = np.logaddexp(0.0, l * (1.0 - 2.0 * cw)).mean(axis=1)
    err = np.abs(dist - mine) / mine
    print(name, "max rel err of out_dist vs fp64", err.max(), "vs the reference's fp32 d",
          (np.abs(dist - ref_d) / ref_d).max())
    assert err.max() <= 1e-12
    assert np.all(np.abs(dist - ref_d) <= 256 * 2.0 ** -24 * np.abs(ref_d))
    assert np.allclose(dist, want_dist, rtol=1e-12, atol=0)


_tie_rows = osd_ref.tie_rows


@pytest.mark.parametrize("k,n,t", [(16, 32, 2), (32, 64, 2), (65, 130, 1)])
def test_tie_policy_against_the_restatement(golden, k, n, t):
    g = golden["k65n130t1_G"] if k == 65 else polar_like(k, n)
    llr = _tie_rows(n, np.random.default_rng(100 + n))
    cw, dist, pat = _decode(_plan(g, t), llr)
    want_cw, want_dist, want_pat, _ = osd_ref.osd_decode(g, llr, t)
    assert np.array_equal(pat, want_pat), np.nonzero(pat != want_pat)[0]
    assert np.array_equal(cw, want_cw.astype(np.float32))
    assert np.allclose(dist, want_dist, rtol=1e-12, atol=0)


def _solve_u(g, words):
    """The information words u with u G = words over GF(2) (G of full row rank), by elimination of
    the augmented system G^T u^T = words^T."""
    k, n = g.shape
    a = np.concatenate([g.T.astype(np.uint8), words.T.astype(np.uint8)], axis=1)  # [n, k + rows]
    r = 0
    for j in range(k):
        piv = r + int(np.nonzero(a[r:, j])[0][0])
        a[[r, piv]] = a[[piv, r]]
        others = np.nonzero(a[:, j])[0]
        others = others[others != r]
        a[others] ^= a[r]
        r += 1
    return a[:k, k:].T.copy()


def test_invariants_on_fresh_rows():
    from polar_amd import OSDecoder
    g = polar_like(32, 64)
    llr, sent = awgn_logits(g, 256, 2.0, 7)
    x = torch.as_tensor(llr, device=DEV)
    enc = DenseEncoder(g)
    prev = None
    for t in range(4):
        dec = OSDecoder(t=t, encoder=enc)
        cw = dec(x)
        d = dec.last_dist.cpu().numpy()
        if prev is not None:
            assert np.all(d <= prev), t  # the candidates of order t include those of order t - 1
        prev = d
        # a codeword: appending it to G does not raise the rank
        words = cw.cpu().numpy().astype(np.uint8)
        assert osd_ref.gf2_rank(np.concatenate([g, words], axis=0)) == 32, t
        # the same through the encoder: the information word u with u G = word re-encodes to the word
        u = _solve_u(g, words)
        assert np.array_equal((enc(torch.as_tensor(u, dtype=torch.float32)).numpy()).astype(np.uint8), words), t
        if t == 0:  # re-encoding the hard decision of the most reliable basis
            basis, idx, ls = osd_ref.most_reliable_basis(g, llr)
            u = (ls[:, :32] > 0).astype(np.uint8)
            c0 = (u[:, :, None] & basis).sum(axis=1).astype(np.uint8) & 1
            want = np.zeros_like(c0)
            np.put_along_axis(want, idx, c0, axis=1)
            assert np.array_equal(words, want)
    # a noiseless codeword comes back unchanged, at every order
    clean = (8.0 * (2.0 * sent.astype(np.float32) - 1.0))
    for t in range(4):
        back = OSDecoder(t=t, encoder=enc)(torch.as_tensor(clean, device=DEV)).cpu().numpy()
        assert np.array_equal(back, sent.astype(np.float32)), t


def test_plumbing(golden):
    from polar_amd import OSDecoder, ops
    g = polar_like(32, 64)
    llr, _ = awgn_logits(g, 67, 2.0, 11)
    want, want_dist, _, _ = osd_ref.osd_decode(g, llr, 2)
    enc = DenseEncoder(g)
    dec = OSDecoder(t=2, encoder=enc)
    x = torch.as_tensor(llr, device=DEV)
    out = dec(x)
    assert out.device.type == "cuda" and out.dtype == torch.float32 and out.shape == (67, 64)
    assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))
    assert np.allclose(dec.last_dist.cpu().numpy(), want_dist, rtol=1e-12, atol=0)
    assert np.array_equal(dec(x[:1]).cpu().numpy(), want[:1].astype(np.float32))  # bs = 1
    assert dec(x[:0]).shape == (0, 64)  # bs = 0
    # leading batch dims
    y = dec(x[:66].reshape(2, 3, 11, 64))
    assert y.shape == (2, 3, 11, 64) and dec.last_dist.shape == (2, 3, 11)
    assert np.array_equal(y.reshape(66, 64).cpu().numpy(), want[:66].astype(np.float32))
    # a CPU input round-trips
    z = dec(torch.as_tensor(llr))
    assert z.device.type == "cpu" and np.array_equal(z.numpy(), want.astype(np.float32))
    assert dec.last_dist.device.type == "cpu"
    # dtypes
    for dt in (torch.float16, torch.float64):
        o = OSDecoder(t=2, encoder=enc, dtype=dt)(x)
        assert o.dtype == dt and np.array_equal(o.cpu().numpy().astype(np.float32), want.astype(np.float32))
    # two calls identical: the word, its metric and the pattern
    plan = dec.plan(DEV)
    r1 = ops.osd_decode(plan, x, return_dist=True, return_pattern=True)
    r2 = ops.osd_decode(plan, x, return_dist=True, return_pattern=True)
    assert all(torch.equal(p, q) for p, q in zip(r1, r2))
    # u8 output equals the fp32 one
    a = ops.osd_decode(plan, x, out_dtype=torch.uint8)
    b = ops.osd_decode(plan, x, out_dtype=torch.uint8)
    assert a.dtype == torch.uint8 and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want)
    # a second stream is ordered: the decode follows the fill queued before it on that stream
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    buf = torch.zeros_like(x)
    with torch.cuda.stream(side):
        buf.copy_(x)
        c = ops.osd_decode(plan, buf)
    side.synchronize()
    assert np.array_equal(c.cpu().numpy(), want.astype(np.float32))
    # GpuEncoder builds the same G as the dense encoder of the same code
    import polar_amd
    from polar_amd.channel import GpuEncoder
    fp = polar_amd.reference_frozen_pos(32, 64)
    ge = OSDecoder(t=1, encoder=GpuEncoder(fp, 64), device=DEV)
    assert ge.k == 32 and ge.n == 64
    from polar_amd import frozen
    from polar_amd.channel import DenseEncoder as HarnessEncoder
    big_g = frozen.get_Kern_frozen_bits(64, 32, frozen.F2)[0]
    de = OSDecoder(t=1, encoder=HarnessEncoder(fp, 64, big_g))
    assert torch.equal(ge.gm, de.gm)


def test_other_devices_stream_is_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from polar_amd import _lib
    g = polar_like(16, 32)
    plan = _plan(g, 1)
    x = torch.zeros((4, 32), device="cuda:1")
    out = torch.empty((4, 32), device="cuda:1")
    with torch.cuda.device(1):
        rc = _lib.lib().pl_osd_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), 4, ctypes.c_void_p(out.data_ptr()),
                                      _lib.PL_OUT_F32, None, None, _lib.current_stream_ptr(torch.device("cuda:1")))
    assert rc == _lib.PL_EINVAL


def test_link_bler_equals_the_restatement():
    import polar_amd
    from polar_amd import OSDecoder
    from polar_amd.channel import FusedAWGN, GpuEncoder
    fp = polar_amd.reference_frozen_pos(32, 64)
    dec = OSDecoder(t=2, encoder=GpuEncoder(fp, 64), device=DEV)
    link = FusedAWGN(64, 32, fp, dec, device=DEV, seed=5, cw_estimates=True)
    cw, cw_hat = link(4096, 2.0, stream=(0, 0))
    _, _, llr = link.llrs(4096, 2.0, stream=(0, 0))
    bler = float((cw != cw_hat).any(dim=1).double().mean())
    want, _, _, gap = osd_ref.osd_decode(dec.gm.numpy(), llr.cpu().numpy(), 2)
    want_bler = float((want != cw.cpu().numpy()).any(axis=1).mean())
    print("BLER", bler, "restatement", want_bler, "min gap", gap.min())
    assert bler == want_bler
    assert 0.0 < bler < 0.2


def test_envelope_corner_128_256(golden):
    g = polar_like(128, 256)
    llr, _ = awgn_logits(g, 32, 2.0, 13)
    cw, dist, pat = _decode(_plan(g, 1), llr)
    want_cw, want_dist, want_pat, gap = osd_ref.osd_decode(g, llr, 1)
    assert gap.min() > 1e-9
    assert np.array_equal(pat, want_pat)
    assert np.array_equal(cw, want_cw.astype(np.float32))
    assert np.allclose(dist, want_dist, rtol=1e-12, atol=0)
