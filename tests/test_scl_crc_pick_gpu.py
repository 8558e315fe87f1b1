"""The CRC-aided pick of both list kernels at every rank, list size and polynomial (GPU).

The pick is the last step of scl_kernel.hip (generic) and scl_tree_kernel.hip (subtree): u from the
root's partial sums, the CRC register over info_pos, the stable (metric, row) order of the 2L
logical rows, +llr_max*k on failing rows, the first argmin.  A slip in any of them still decodes
clean codewords, so the rows here (tests/golden/scl_pick_cases.py) are built to put the winner at
every rank and to make most rows fail altogether; tests/test_scl_crc_pick_ref.py asserts on the
oracle alone that they do.

  min-sum f, fast-SCL off and on: bits equal the oracle's (oracle.scl_decode_mysn), metrics within
    1e-9 absolute (the tolerance tests/test_scl_gpu.py holds these fp64 metrics to), subtree and
    generic identical in bits and metrics, the rank census of the GPU's own pm equal to the
    oracle's row by row, ops.crc_status of the decoded bits false exactly on the oracle's all-fail
    rows.  n = 2048 runs on the generic kernel alone (the subtree kernel stops at 1024);
  exact f: subtree and generic identical, and the GPU's census meets the coverage conditions (no
    oracle equality: the transcendentals differ in the last ulp);
  output forms: float32 and uint8, with and without the metrics (out_pm == nullptr), an out= tensor
    prefilled with 9, on ragged batches;
  llr_max = 7.5 at L = 32 against the oracle run with the same value;
  pl_plan_set_crc's argument contract: PL_EINVAL, nothing launched, the plan keeps
    the CRC it had.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import scl_pick_cases as C  # noqa: E402

PM_TOL = 1e-9
IDS = [c.name for c in C.CASES]


@pytest.fixture(scope="module")
def pa():
    import polar_amd
    assert torch.cuda.is_available()
    return polar_amd


def _kernels(case):
    return ("subtree", "generic") if case.n <= 1024 else ("generic",)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(frozen positions, logits on the host, logits on the device) of a case, made once."""
    case = C.BY_NAME[name]
    x = C.llr_rows(case)
    x.setflags(write=False)
    return C.frozen_pos(case), x, torch.from_numpy(x.copy()).cuda()


@functools.lru_cache(maxsize=None)
def _ref(name, fast, llr_max=C.LLR_MAX):
    """The oracle's (bits, penalised sorted metrics) of a case with the min-sum f: computed once, read-only."""
    case = C.BY_NAME[name]
    fp, x, _ = _inputs(name)
    bits, pm = oracle.scl_decode_mysn(x, fp, case.L, fast_scl=fast, exact_f=False, crc=case.crc, llr_max=llr_max)
    bits.setflags(write=False)
    pm.setflags(write=False)
    return bits, pm


def _plan(case, kernel, fast, f_mode=None, llr_max=C.LLR_MAX):
    from polar_amd import _lib
    fp, _, _ = _inputs(case.name)
    mask = np.zeros(case.n, dtype=np.uint8)
    mask[fp] = 1
    flags = (_lib.PL_PLAN_FAST_SCL if fast else 0) | (_lib.PL_PLAN_GENERIC if kernel == "generic" else 0)
    plan = _lib.Plan(case.n, mask, case.L, _lib.PL_F_MINSUM if f_mode is None else f_mode, llr_max=llr_max, flags=flags)
    assert plan.kernel()[0] == ("scl_subtree" if kernel == "subtree" else "generic")
    assert (plan.n, plan.k, plan.list_size) == (case.n, case.k, case.L)
    plan.set_crc(*C.crc_params(case.crc))
    return plan


def _check_vs_oracle(pa, case, fast, llr_max):
    _, _, xd = _inputs(case.name)
    want, wpm = _ref(case.name, fast, llr_max)
    w_rank, w_fail = C.winner_ranks(wpm, llr_max, case.k)
    got = {}
    for kernel in _kernels(case):
        plan = _plan(case, kernel, fast, llr_max=llr_max)
        bits, pm = pa.ops.scl_decode(plan, xd, return_pm=True)
        status = pa.ops.crc_status(plan, bits).cpu().numpy()
        got[kernel] = (bits, pm)
        b, m = bits.cpu().numpy(), pm.cpu().numpy()
        bad = np.nonzero((b != want).any(1))[0]
        err = np.abs(m - wpm).max()
        print(case.name, kernel, "fast" if fast else "plain", "rows", len(b), "bit-mismatch rows", bad.size,
              "max |pm - oracle|", err)
        assert bad.size == 0, (kernel, "rows", bad[:8], "oracle ranks", w_rank[bad[:8]], "all-fail", w_fail[bad[:8]])
        assert err < PM_TOL, kernel
        rank, fail = C.winner_ranks(m, llr_max, case.k)
        assert np.array_equal(rank, w_rank) and np.array_equal(fail, w_fail), kernel
        if case.kind == "tie":
            assert np.array_equal(C.tie_rows(m, llr_max, case.k), C.tie_rows(wpm, llr_max, case.k)), kernel
        assert np.array_equal(status, ~w_fail), kernel
    if len(got) == 2:
        assert torch.equal(got["subtree"][0], got["generic"][0])
        assert torch.equal(got["subtree"][1], got["generic"][1])


@pytest.mark.parametrize("fast", [False, True], ids=["plain", "fast"])
@pytest.mark.parametrize("name", IDS)
def test_crc_pick_minsum_vs_oracle(pa, name, fast):
    _check_vs_oracle(pa, C.BY_NAME[name], fast, C.LLR_MAX)


@pytest.mark.parametrize("fast", [False, True], ids=["plain", "fast"])
@pytest.mark.parametrize("name", C.LLR_MAX_OFF_CASES)
def test_crc_pick_llr_max_off_the_default(pa, name, fast):
    """llr_max = 7.5 at L = 32: the penalty is 7.5 k, and the dead paths' saturated metrics tie exactly."""
    _check_vs_oracle(pa, C.BY_NAME[name], fast, C.LLR_MAX_OFF)


@pytest.mark.parametrize("fast", [False, True], ids=["plain", "fast"])
@pytest.mark.parametrize("shape", C.EXACT_SHAPES, ids=[f"n{n}_L{L}" for n, L in C.EXACT_SHAPES])
def test_crc_pick_exact_f_subtree_equals_generic(pa, shape, fast):
    from polar_amd import _lib
    case = C.BY_NAME["rank_n%d_L%d" % shape]
    _, _, xd = _inputs(case.name)
    b1, pm1 = pa.ops.scl_decode(_plan(case, "subtree", fast, _lib.PL_F_EXACT), xd, return_pm=True)
    b2, pm2 = pa.ops.scl_decode(_plan(case, "generic", fast, _lib.PL_F_EXACT), xd, return_pm=True)
    assert torch.equal(b1, b2)
    assert torch.equal(pm1, pm2)
    hist, n_fail = C.census(pm1.cpu().numpy(), C.LLR_MAX, case.k)
    print(case.name, "exact", "fast" if fast else "plain", "hist", hist.tolist(), "all-fail", n_fail)
    assert C.coverage_gaps(case, pm1.cpu().numpy()) == []


# (case, first row, rows): one row, and counts that are no multiple of the codewords a wave of the
# subtree kernel takes (32 / L), from inside a rank case
FORMS = [("rank_n64_L2", 110, 1), ("rank_n64_L2", 93, 37), ("rank_n32_L8", 31, 1), ("rank_n64_L8", 143, 41),
         ("rank_n64_L32", 11, 1), ("rank_n128_L32", 3, 35), ("rank_n1024_L8", 39, 67), ("rank_n2048_L8", 19, 5),
         ("poly_CRC24B_37_128_L32", 4, 33), ("poly_CRC6_100_256_L8", 20, 39)]


@pytest.mark.parametrize("name,first,rows", FORMS, ids=[f"{n}_{f}_{r}" for n, f, r in FORMS])
def test_crc_pick_output_forms(pa, name, first, rows):
    case = C.BY_NAME[name]
    _, _, xd = _inputs(name)
    want, wpm = _ref(name, True)
    sl = slice(first, first + rows)
    w_rank, w_fail = C.winner_ranks(wpm[sl], C.LLR_MAX, case.k)
    assert w_rank[0] > 0 and (w_fail.any() or rows == 1)  # the slice starts at a winner below rank 0
    x = xd[sl].contiguous()
    wb = torch.from_numpy(want[sl].copy()).cuda()
    for kernel in _kernels(case):
        plan = _plan(case, kernel, True)
        f32, pm = pa.ops.scl_decode(plan, x, return_pm=True)
        assert f32.dtype == torch.float32 and torch.equal(f32, wb), kernel
        assert np.abs(pm.cpu().numpy() - wpm[sl]).max() < PM_TOL
        u8, pm8 = pa.ops.scl_decode(plan, x, out_dtype=torch.uint8, return_pm=True)
        assert u8.dtype == torch.uint8 and torch.equal(u8, wb.to(torch.uint8)), kernel
        assert torch.equal(pm8, pm)
        nopm = pa.ops.scl_decode(plan, x, return_pm=False)  # out_pm == nullptr
        assert torch.equal(nopm, wb), kernel
        assert torch.equal(pa.ops.scl_decode(plan, x, out_dtype=torch.uint8), wb.to(torch.uint8)), kernel
        for dtype in (torch.float32, torch.uint8):
            # out= is the head of a larger buffer of nines: all of it is overwritten, nothing behind it is
            buf = torch.full((rows + 3, case.k), 9, dtype=dtype, device="cuda")
            ret = pa.ops.scl_decode(plan, x, out=buf[:rows])
            assert ret.data_ptr() == buf.data_ptr()
            assert torch.equal(buf[:rows], wb.to(dtype)), (kernel, dtype)
            assert bool((buf[rows:] == 9).all()), (kernel, dtype)


def test_plan_set_crc_argument_contract(pa):
    """pl_plan_set_crc takes 0 <= degree <= min(31, k) and a mask below x^degree.  Everything else is
    PL_EINVAL with a message that names the call; nothing is launched and the plan keeps the CRC it
    had: a plan without one stays PL_ENOTSUP for pl_crc_status, a plan with CRC6 decodes as before.
    k = degree (a word of parity alone) and degree 31 are accepted."""
    from polar_amd import _lib
    L = _lib.lib()
    case = C.BY_NAME["rank_n32_L8"]  # k = 16
    _, _, xd = _inputs(case.name)
    deg6, g6 = C.crc_params("CRC6")
    assert L.pl_plan_set_crc(None, deg6, g6) == _lib.PL_EINVAL
    refused = [(-1, 0), (32, 0), (33, 1), (1 << 20, 0), (17, 1), (24, C.crc_params("CRC24C")[1]), (6, 1 << 6),
               (6, g6 | (1 << 31)), (1, 2)]
    for kernel in ("subtree", "generic"):
        plan = _plan(case, kernel, True)
        before = pa.ops.scl_decode(plan, xd, return_pm=True)
        bare = _plan(case, kernel, True)
        bare.set_crc(0, 0)  # degree 0: off
        plain = pa.ops.scl_decode(bare, xd, return_pm=True)
        assert not torch.equal(plain[0], before[0])
        for deg, g in refused:
            for p in (plan, bare):
                assert L.pl_plan_set_crc(p.handle, deg, g) == _lib.PL_EINVAL, (deg, g)
                assert b"pl_plan_set_crc" in L.pl_last_error_string()
            with pytest.raises(ValueError):
                plan.set_crc(deg, g)
        valid = torch.full((len(xd),), 9, dtype=torch.uint8, device="cuda")
        rc = L.pl_crc_status(bare.handle, ctypes.c_void_p(before[0].data_ptr()), _lib.PL_OUT_F32, len(xd),
                             ctypes.c_void_p(valid.data_ptr()), _lib.current_stream_ptr(xd.device))
        assert rc == _lib.PL_ENOTSUP
        torch.cuda.synchronize()
        assert bool((valid == 9).all())
        after = pa.ops.scl_decode(plan, xd, return_pm=True)
        assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
        again = pa.ops.scl_decode(bare, xd, return_pm=True)
        assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
        # accepted edges: k = degree = 16 (only the all-zero word passes) and degree 31 on a k = 31 code
        plan.set_crc(*C.crc_params("CRC16"))
        bits, pm = pa.ops.scl_decode(plan, xd, return_pm=True)
        fp = _inputs(case.name)[0]
        want, wpm = oracle.scl_decode_mysn(_inputs(case.name)[1], fp, case.L, fast_scl=True, exact_f=False, crc="CRC16")
        assert np.array_equal(bits.cpu().numpy(), want) and np.abs(pm.cpu().numpy() - wpm).max() < PM_TOL
        passed = pa.ops.crc_status(plan, bits).cpu().numpy()
        assert np.array_equal(passed, ~want.any(1))
    mask = np.zeros(32, dtype=np.uint8)
    mask[0] = 1
    wide = _lib.Plan(32, mask, 2, _lib.PL_F_MINSUM)
    assert wide.k == 31
    wide.set_crc(31, (1 << 30) | 0x5)
    assert L.pl_plan_set_crc(wide.handle, 32, 0) == _lib.PL_EINVAL
