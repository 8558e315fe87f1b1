"""pl_osd_decode over its whole envelope against the numpy restatement (tests/golden/osd_ref.py): order 4,
k > 64 at t >= 2, every osd_kernel<NW, RPL> instantiation that launch_osd can select, the lane partition
of the pattern index, generator matrices with zero and repeated columns, the three corners of the
envelope and the 2^20-row chunk loop.

Which case runs which instantiation (NW = 32-bit words a row, RPL = basis rows a lane):
  <1, 1>  k10n20t2, k8n16t3, k12n24t4, the chunk loop      <1, 2>  unreachable: k > 64 forces n >= 65
  <2, 1>  k24n33t4, k16n40t2_structured*                   <2, 2>  unreachable likewise
  <4, 1>  k64n128t4                                        <4, 2>  k66n97t3, k128n128t2, k100n104t4
  <8, 1>  k40n200t3                                        <8, 2>  k70n130t2, k128n256t3

The inputs come from osd_ref.envelope_case; tests/test_osd.py asserts without a GPU that every order
1 .. t wins somewhere in each case, that every row which is not exact in fp64 leads its runner-up by more
than 1e-9 in Delta, and the lane-boundary arithmetic.  Words and pattern indices are compared exactly, the
metric to rtol 1e-12 as in tests/test_osd_gpu.py.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import osd_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8_TOO = ("k66n97t3", "k24n33t4")  # n is no multiple of 4: byte stores; and the NULL dist / pattern branches


def _plan(g, t):
    from polar_amd import _lib
    return _lib.OsdPlan(np.asarray(g, dtype=np.uint8), t, device=DEV)


def _decode(plan, llr, out_dtype=torch.float32):
    from polar_amd import ops
    x = torch.as_tensor(np.asarray(llr, dtype=np.float32), device=DEV)
    cw, dist, pat = ops.osd_decode(plan, x, out_dtype=out_dtype, return_dist=True, return_pattern=True)
    return cw.cpu().numpy(), dist.cpu().numpy(), pat.cpu().numpy()


@pytest.mark.parametrize("name", list(osd_ref.ENVELOPE_CASES))
def test_envelope_case_equals_the_restatement(name):
    from polar_amd import ops
    g, t, llr, exact = osd_ref.envelope_case(name)
    k, n = g.shape
    restate = osd_ref.osd_decode_packed if name in osd_ref.ENVELOPE_CORNERS else osd_ref.osd_decode
    want_cw, want_dist, want_pat, gap = restate(g, llr, t)
    assert gap[~exact].min() > 1e-9
    plan = _plan(g, t)
    assert plan.n_patterns == sum(math.comb(k, i) for i in range(1, t + 1))
    cw, dist, pat = _decode(plan, llr)
    print(name, "winner orders", np.bincount(osd_ref.winner_orders(want_pat, k, t), minlength=t + 1).tolist(),
          "min gap", float(gap[~exact].min()), "max rel err of dist", float((np.abs(dist - want_dist) / want_dist).max()))
    assert np.array_equal(pat, want_pat), np.nonzero(pat != want_pat)[0]
    assert np.array_equal(cw, want_cw.astype(np.float32))
    assert np.allclose(dist, want_dist, rtol=1e-12, atol=0)
    if name in U8_TOO:
        cw8, dist8, pat8 = _decode(plan, llr, out_dtype=torch.uint8)
        assert cw8.dtype == np.uint8 and np.array_equal(cw8, want_cw)
        assert np.array_equal(pat8, want_pat) and np.array_equal(dist8, dist)
        x = torch.as_tensor(llr, device=DEV)
        for dt in (torch.uint8, torch.float32):  # no metric, no pattern: the words alone
            alone = ops.osd_decode(plan, x, out_dtype=dt, return_dist=False, return_pattern=False)
            assert alone.dtype == dt and np.array_equal(alone.cpu().numpy(), want_cw)


def chunk_rows():
    """64 distinct rows of (1, 2): every pair of eight values that hold +-0, +-Inf, values beyond the
    clip and equal magnitudes (250 and -100 are equal once clipped); every Delta is exact."""
    v = np.array([0.0, -0.0, np.inf, -np.inf, 250.0, -100.0, 0.5, -3.25], dtype=np.float32)
    return np.stack([np.repeat(v, 8), np.tile(v, 8)], axis=1)


def test_chunk_loop_offsets_every_buffer():
    """bs = 2^20 + 5: the second launch of launch_osd (row0 = 2^20) must offset llr, out, dist and
    pattern alike.  The 64 rows are tiled, and the tiling is shifted by 47 past row 2^20, so that the
    five rows of the second launch differ, in their inputs, words and metrics, from rows 0 .. 4: a launch
    that ignored row0 on llr, out or dist would not pass.  At (1, 2) c0 always wins (the pivot is the more
    reliable of two equal bits), so every pattern is -1; the last call, through the C entry point, fills
    dist and pattern with a value no decode gives first, which an unwritten row would keep."""
    from polar_amd import ops
    g = np.array([[1, 1]], dtype=np.uint8)
    base = chunk_rows()
    assert len({r.tobytes() for r in base}) == 64
    want_cw, want_dist, want_pat, _ = osd_ref.osd_decode(g, base, 1)
    chunk, bs = 1 << 20, (1 << 20) + 5
    rows = np.arange(bs)
    tile = (rows + 47 * (rows >> 20)) % 64
    tail = rows[chunk:]
    assert all(want_dist[tile[r]] != want_dist[tile[r - chunk]] for r in tail)
    assert sum(want_cw[tile[r], 0] != want_cw[tile[r - chunk], 0] for r in tail) >= 3
    assert set(want_pat.tolist()) == {-1}
    x = torch.as_tensor(base, device=DEV)[torch.as_tensor(tile, device=DEV)].contiguous()
    assert x.shape == (bs, 2)
    plan = _plan(g, 1)
    kept = []  # both results stay allocated, so the second cannot inherit the first one's memory
    for dt, npdt in ((torch.uint8, np.uint8), (torch.float32, np.float32)):
        out = torch.full((bs, 2), 7, dtype=dt, device=DEV)
        res = ops.osd_decode(plan, x, out=out, return_dist=True, return_pattern=True)
        kept.append(res)
        cw, dist, pat = (r.cpu().numpy() for r in res)
        assert cw.dtype == npdt
        for r in [chunk - 1] + tail.tolist():
            assert np.array_equal(cw[r], want_cw[tile[r]].astype(npdt)), r
            assert pat[r] == want_pat[tile[r]] and dist[r] == pytest.approx(want_dist[tile[r]], rel=1e-12, abs=0), r
        assert np.array_equal(cw, want_cw[tile].astype(npdt))
        assert np.array_equal(pat, want_pat[tile])
        assert np.allclose(dist, want_dist[tile], rtol=1e-12, atol=0)
    from polar_amd import _lib
    out = torch.full((bs, 2), 7.0, dtype=torch.float32, device=DEV)
    dist = torch.full((bs,), -1.0, dtype=torch.float64, device=DEV)
    pat = torch.full((bs,), 7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        rc = _lib.lib().pl_osd_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), bs, ctypes.c_void_p(out.data_ptr()),
                                      _lib.PL_OUT_F32, ctypes.c_void_p(dist.data_ptr()), ctypes.c_void_p(pat.data_ptr()),
                                      _lib.current_stream_ptr(torch.device(DEV)))
    assert rc == _lib.PL_OK
    torch.cuda.synchronize(DEV)
    assert np.array_equal(out.cpu().numpy(), want_cw[tile].astype(np.float32))
    assert np.array_equal(pat.cpu().numpy(), want_pat[tile])
    assert np.allclose(dist.cpu().numpy(), want_dist[tile], rtol=1e-12, atol=0)
