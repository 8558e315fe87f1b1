"""Hybrid SC / SC-list decoding (pl_hybrid_decode) and pl_crc_status on the GPU.

The definition the tests hold the decoder to:
    u_sc = SC(llr); ok_sc = crc_valid(u_sc); rows = ascending indices where ~ok_sc
    out = u_sc, out[rows] = SCL_crc(llr[rows]); crc_ok = ok_sc, crc_ok[rows] = crc_valid(out[rows])
With min-sum plans every piece is bit-exact against the CPU oracle (no transcendental slack), so
out, crc_ok, the row list and its length are compared for equality.  Inputs follow the recipe of
tests/test_mysn_gpu.py::test_mysn_scl_crc_pick_vs_oracle."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
L8 = 8


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import polar_amd
    return polar_amd


@functools.lru_cache(maxsize=None)
def _input(k, n, crc, bs, seed, amp, sig):
    """(fp, u, llr) of the recipe: CRC-carrying words, polar-encoded, BPSK amplitude amp, noise sig."""
    import polar_amd
    deg = oracle.crc_params(crc)[0]
    fp = polar_amd.reference_frozen_pos(k, n).numpy()
    rng = np.random.default_rng(seed)
    u = oracle.crc_encode(rng.integers(0, 2, (bs, k - deg)).astype(np.float32), crc)
    cw = oracle.polar_encode(u, fp, n)
    llr = ((2 * cw - 1) * amp + rng.standard_normal(cw.shape) * sig).astype(np.float32)
    return fp, u, llr


def _compose(llr, fp, crc):
    """The oracle's composition (min-sum f): out, crc_ok, rows."""
    u_sc = oracle.sc_decode(llr, fp, f_mode=0)
    ok = oracle.crc_check(u_sc, crc).astype(bool)
    rows = np.nonzero(~ok)[0]
    out, ok = u_sc.copy(), ok.copy()
    if len(rows):
        u_l, _ = oracle.scl_decode_mysn(llr[rows], fp, L8, fast_scl=True, exact_f=False, crc=crc)
        out[rows] = u_l
        ok[rows] = oracle.crc_check(u_l, crc)
    return out, ok, rows.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _expected(k, n, crc, bs, seed, amp, sig):
    fp, _, llr = _input(k, n, crc, bs, seed, amp, sig)
    return _compose(llr, fp, crc)


def _plans(pa, k, n, crc, sc_flags=0, scl_flags=0):
    from polar_amd import _lib
    from polar_amd.mysn import crc_params
    mask = pa.frozen_mask(pa.reference_frozen_pos(k, n).numpy(), n)
    sc = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, flags=sc_flags)
    scl = _lib.Plan(n, mask, L8, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_FAST_SCL | scl_flags)
    scl.set_crc(*crc_params(crc))
    return sc, scl


def _check(got, want, what):
    out, ok, rows, n_list = got
    w_out, w_ok, w_rows = want
    assert n_list == len(w_rows), (what, n_list, len(w_rows))
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), w_rows), what
    assert ok.dtype == torch.bool and np.array_equal(ok.cpu().numpy(), w_ok), what
    assert np.array_equal(out.cpu().numpy(), w_out), what


def _classes(want):
    """Rows by branch: SC passes / SC fails and the list result passes / both fail."""
    _, ok, rows = want
    listed = np.zeros(len(ok), dtype=bool)
    listed[rows] = True
    return int((~listed).sum()), int((listed & ok).sum()), int((listed & ~ok).sum())


CASES = {"k32": (32, 64, "CRC11", 256, 5, 1.6, 1.5), "k128": (128, 256, "CRC24C", 192, 9, 1.6, 1.1),
         "k512": (512, 1024, "CRC24C", 96, 3, 1.0, 0.6)}
CLASSES = {"k32": (70, 99, 87), "k128": (104, 71, 17), "k512": (46, 38, 12)}


@pytest.mark.parametrize("case,scl_kernel,sc_kernel", [
    ("k32", "scl_subtree", "default"), ("k512", "scl_subtree", "default"),
    ("k128", "scl_subtree", "default"), ("k128", "scl_subtree", "generic"),
    ("k128", "generic", "default"), ("k128", "generic", "generic")])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.uint8])
def test_hybrid_minsum_vs_oracle_composition(pa, case, scl_kernel, sc_kernel, out_dtype):
    from polar_amd import _lib, ops
    cfg = CASES[case]
    want = _expected(*cfg)
    # every branch has rows before anything is compared (counted on the oracle's result)
    assert _classes(want) == CLASSES[case] and min(_classes(want)) >= 10
    sc, scl = _plans(pa, *cfg[:3], sc_flags=_lib.PL_PLAN_GENERIC if sc_kernel == "generic" else 0,
                     scl_flags=_lib.PL_PLAN_GENERIC if scl_kernel == "generic" else 0)
    assert scl.kernel()[0] == scl_kernel
    assert sc.kernel()[0] == ("generic" if sc_kernel == "generic" else "specialized")
    llr = torch.from_numpy(_input(*cfg)[2]).cuda()
    _check(ops.hybrid_decode(sc, scl, llr, out_dtype=out_dtype, return_info=True), want, cfg)
    # without the info outputs (crc_ok, list_rows NULL): the same bits
    plain = ops.hybrid_decode(sc, scl, llr, out_dtype=out_dtype)
    assert np.array_equal(plain.cpu().numpy(), want[0])
    # pl_crc_status of the result, in the same output kind
    assert np.array_equal(ops.crc_status(scl, plain).cpu().numpy(), want[1])


def test_hybrid_is_not_pure_crc_aided_scl(pa):
    """The semantics, pinned: a row whose SC result passes the CRC keeps it even where the list
    decoder picks another CRC-valid word.  On this input that happens on at least one row."""
    from polar_amd import ops
    cfg = (128, 256, "CRC24C", 192, 9, 1.6, 1.2)
    fp, _, x = _input(*cfg)
    want = _expected(*cfg)
    pure, _ = oracle.scl_decode_mysn(x, fp, L8, fast_scl=True, exact_f=False, crc="CRC24C")
    assert (want[0] != pure).any(1).sum() >= 1
    sc, scl = _plans(pa, *cfg[:3])
    llr = torch.from_numpy(x).cuda()
    _check(ops.hybrid_decode(sc, scl, llr, return_info=True), want, cfg)
    assert np.array_equal(ops.scl_decode(scl, llr).cpu().numpy(), pure)  # the list plan alone: pure SCL


@pytest.mark.parametrize("bs", [1, 37, 193])
def test_hybrid_ragged_batch_sizes(pa, bs):
    """Sizes that are no multiple of the wave, of a block or of the codewords-per-wave count."""
    from polar_amd import ops
    cfg = CASES["k32"]
    fp, _, llr = _input(*cfg)
    llr = llr[:bs]
    want = _compose(llr, fp, cfg[2])
    if bs > 1:
        assert 0 < len(want[2]) < bs
    sc, scl = _plans(pa, *cfg[:3])
    _check(ops.hybrid_decode(sc, scl, torch.from_numpy(llr).cuda(), return_info=True), want, bs)


def test_hybrid_all_rows_pass(pa):
    from polar_amd import ops
    cfg = CASES["k32"]
    fp, u, _ = _input(*cfg)
    llr = ((2 * oracle.polar_encode(u, fp, 64) - 1) * 4).astype(np.float32)
    sc, scl = _plans(pa, *cfg[:3])
    out, ok, rows, n_list = ops.hybrid_decode(sc, scl, torch.from_numpy(llr).cuda(), return_info=True)
    assert n_list == 0 and rows.numel() == 0
    assert np.array_equal(out.cpu().numpy(), u) and bool(ok.all())
    # an empty batch is fine too
    out, ok, rows, n_list = ops.hybrid_decode(sc, scl, torch.empty((0, 64), device="cuda"), return_info=True)
    assert out.shape == (0, 32) and ok.shape == (0,) and n_list == 0


def test_hybrid_no_row_passes_and_chunk_loop(pa):
    """40000 rows of pure noise: nearly every row fails the CRC, so the list stage runs three chunks
    of at most 16384 rows.  Expected from the library's own, separately verified SC and list decodes
    of the same tensor: this tests the glue, not the decoders again."""
    from polar_amd import ops
    k, n, crc, bs = 32, 64, "CRC11", 40000
    llr = torch.from_numpy(np.random.default_rng(1).standard_normal((bs, n)).astype(np.float32)).cuda()
    sc, scl = _plans(pa, k, n, crc)
    u_sc = ops.sc_decode(sc, llr).cpu().numpy()
    u_l = ops.scl_decode(scl, llr).cpu().numpy()
    ok_sc = oracle.crc_check(u_sc, crc).astype(bool)
    w_rows = np.nonzero(~ok_sc)[0].astype(np.int32)
    w_out = np.where(ok_sc[:, None], u_sc, u_l)
    w_ok = ok_sc | oracle.crc_check(u_l, crc).astype(bool)
    got = ops.hybrid_decode(sc, scl, llr, return_info=True)
    assert got[3] > 2 * 16384
    _check(got, (w_out, w_ok, w_rows), "noise")


def test_mysn_module_hybrid_and_crc_status(pa):
    """The exact-f module path: the same kernels on the same rows as SC_Dec and SCL_Dec(crc) run one
    after the other, so the comparison is exact."""
    from polar_amd import mysn
    cfg = CASES["k32"]
    _, _, x = _input(*cfg)
    fp = pa.reference_frozen_pos(32, 64)
    llr = torch.from_numpy(x)
    hyb = mysn.SCL_Dec(fp, 64, crc_degree="CRC11", use_hybrid_sc=True, return_crc_status=True)
    u_hat, status = hyb(llr)
    u_sc = mysn.SC_Dec(fp, 64)(llr).numpy()
    ok_sc = oracle.crc_check(u_sc, "CRC11").astype(bool)
    rows = np.nonzero(~ok_sc)[0]
    assert 10 <= len(rows) <= len(x) - 10
    scl = mysn.SCL_Dec(fp, 64, crc_degree="CRC11")
    want = u_sc.copy()
    want[rows] = scl(llr[rows]).numpy()
    assert u_hat.shape == (len(x), 32) and u_hat.dtype == torch.float32
    assert np.array_equal(u_hat.numpy(), want)
    assert status.dtype == torch.bool and status.shape == (len(x),) and status.device.type == "cpu"
    assert np.array_equal(status.numpy(), oracle.crc_check(want, "CRC11").astype(bool))
    assert hyb.last_list_rows == len(rows) and isinstance(hyb.last_list_rows, int)
    assert hyb.msg_pm is None
    # leading dimensions are kept: [4, 64, n] -> bits [4, 64, k], status [4, 64]
    u3, s3 = hyb(llr.reshape(4, 64, 64))
    assert u3.shape == (4, 64, 32) and s3.shape == (4, 64)
    assert np.array_equal(u3.reshape(-1, 32).numpy(), want)
    # without hybrid, return_crc_status reports the CRC of the list decoder's output
    plain = mysn.SCL_Dec(fp, 64, crc_degree="CRC11", return_crc_status=True)
    u_p, s_p = plain(llr)
    assert np.array_equal(u_p.numpy(), scl(llr).numpy())
    assert s_p.dtype == torch.bool and np.array_equal(s_p.numpy(), oracle.crc_check(u_p.numpy(), "CRC11").astype(bool))
    assert plain.msg_pm is not None and plain.last_list_rows == len(x)


def test_polar5g_decoder_hybrid(pa):
    from polar_amd import mysn, polar5g
    with contextlib.redirect_stdout(io.StringIO()):
        enc = polar5g.Polar5GEncoder(32, 64)
        dec = polar5g.Polar5GDecoder(enc, dec_type="SCL", hybrid_sc=True)
    rng = np.random.default_rng(2)
    u = torch.from_numpy(rng.integers(0, 2, (64, 32)).astype(np.float32)).cuda()
    c = enc(u)
    assert torch.equal(dec((2.0 * c - 1.0) * 8.0), u)
    assert dec.polar_dec.last_list_rows == 0
    noisy = (2.0 * c - 1.0) * 2.0 + torch.from_numpy(rng.standard_normal(tuple(c.shape)).astype(np.float32)).cuda() * 1.5
    got = dec(noisy).cpu().numpy()
    # the same decoder's rate recovery, then the composition on the mother code
    mother = dec.rate_recover(noisy).cpu()
    fp, n, crc = enc._frozen_pos, enc.n_polar, enc.enc_crc.crc_degree
    u_sc = mysn.SC_Dec(fp, n)(mother).numpy()
    ok_sc = oracle.crc_check(u_sc, crc).astype(bool)
    rows = np.nonzero(~ok_sc)[0]
    assert 0 < len(rows) < len(u_sc)
    want = u_sc.copy()
    want[rows] = mysn.SCL_Dec(fp, n, crc_degree=crc)(mother[rows]).numpy()
    assert dec.polar_dec.last_list_rows == len(rows)
    assert np.array_equal(got, want[:, :32])


def test_hybrid_argument_errors(pa):
    """The C ABI's refusals, as PolarLibError with the stated codes; none of them launches."""
    import ctypes
    from polar_amd import _lib, ops
    sc, scl = _plans(pa, 32, 64, "CRC11")
    llr = torch.zeros((8, 64), device="cuda")

    def code(*a, **kw):
        with pytest.raises(_lib.PolarLibError) as e:
            ops.hybrid_decode(*a, **kw)
        return e.value.code

    mask64 = pa.frozen_mask(pa.reference_frozen_pos(32, 64).numpy(), 64)
    assert code(scl, scl, llr) == _lib.PL_EINVAL  # sc_plan with a list
    assert code(sc, sc, llr) == _lib.PL_EINVAL  # scl_plan without one
    nocrc = _lib.Plan(64, mask64, L8, _lib.PL_F_MINSUM)
    assert code(sc, nocrc, llr) == _lib.PL_ENOTSUP
    other_k = _lib.Plan(64, pa.frozen_mask(pa.reference_frozen_pos(48, 64).numpy(), 64), 1, _lib.PL_F_MINSUM)
    assert code(other_k, scl, llr) == _lib.PL_EINVAL
    moved = mask64.copy()  # same n and k, another frozen set
    moved[np.nonzero(mask64 == 0)[0][0]] = 1
    moved[np.nonzero(mask64 == 1)[0][-1]] = 0
    other_set = _lib.Plan(64, moved, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
    assert (other_set.n, other_set.k) == (sc.n, sc.k)
    assert code(other_set, scl, llr) == _lib.PL_EINVAL
    sc128, _ = _plans(pa, 64, 128, "CRC11")
    assert code(sc128, scl, llr) == _lib.PL_EINVAL  # another n
    # the workspace is required and must be large enough
    L = _lib.lib()
    need = int(L.pl_hybrid_workspace_size(sc.handle, scl.handle, 8))
    assert need > 0 and L.pl_hybrid_workspace_size(sc.handle, scl.handle, 0) == 0
    # bounded by one chunk of 16384 rows beyond the 5 bytes per row of the flags and the row list
    big, huge = (int(L.pl_hybrid_workspace_size(sc.handle, scl.handle, b)) for b in (16384, 10 * 16384))
    assert need < big and huge - big <= 9 * 16384 * 5 + 1024
    out = torch.empty((8, 32), device="cuda")
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    n_list = ctypes.c_int64(-1)
    st = _lib.current_stream_ptr(llr.device)

    def call(bs, ws_ptr, ws_bytes):
        return L.pl_hybrid_decode(sc.handle, scl.handle, ctypes.c_void_p(llr.data_ptr()), bs,
                                  ctypes.c_void_p(out.data_ptr()), _lib.PL_OUT_F32, None, None, ctypes.byref(n_list),
                                  ws_ptr, ws_bytes, st)
    assert call(8, None, 0) == _lib.PL_EINVAL
    assert call(8, ctypes.c_void_p(ws.data_ptr()), need - 1) == _lib.PL_EINVAL
    assert call(0, None, 0) == _lib.PL_OK and n_list.value == 0
    assert call(-1, ctypes.c_void_p(ws.data_ptr()), need) == _lib.PL_EINVAL
    with pytest.raises(_lib.PolarLibError) as e:
        ops.crc_status(nocrc, out)
    assert e.value.code == _lib.PL_ENOTSUP
