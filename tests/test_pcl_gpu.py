"""The parity-constrained list decoder (csrc/pcl_kernel.hip: pl_pcl_table_create, pl_pcl_decode) against the numpy
restatement tests/golden/pcl_ref.py, value for value: decoded bits, path metrics, ok and stop are np.array_equal,
ties and +inf metrics included.

Every case decodes 67 rows (9 at n = 1024) of the four input kinds of pcl_ref.make_inputs: the four special rows,
AWGN rows of valid codewords, integer LLRs that tie at almost every fork, and pure-noise rows.  One single-wave
work-group decodes a row and there is no grid stride, so 67 rows are 67 work-groups.  The cases, their tables and
their restatement outputs are pcl_ref.GPU_CASES / gpu_case, computed once and shared; tests/test_pcl_ref.py shows
on the CPU that they hold rows that stop early and rows that run to the end.
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
import pcl_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LLR_MAX = pcl_ref.LLR_MAX
CHECK, FORCE = pcl_ref.CHECK, pcl_ref.FORCE


@pytest.fixture(scope="module")
def pa():
    import polar_amd
    from polar_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    assert hasattr(_lib.lib(), "pl_pcl_decode") and hasattr(_lib.lib(), "pl_pcl_table_create")
    return polar_amd


@functools.lru_cache(maxsize=None)
def _plan(n, kind, f_mode=0, list_size=1, llr_max=LLR_MAX):
    import polar_amd
    from polar_amd import _lib
    return _lib.Plan(n, polar_amd.frozen_mask(pcl_ref.case_frozen(n, kind), n), list_size, f_mode, llr_max,
                     flags=_lib.PL_PLAN_GENERIC)


@functools.lru_cache(maxsize=None)
def _table(n, kind, L, tkind):
    from polar_amd import _lib
    return _lib.PclTable(_plan(n, kind), *pcl_ref.case_table(n, kind, L, tkind))


@pytest.mark.parametrize("case", pcl_ref.GPU_CASES, ids=str)
def test_decode_equals_the_restatement(pa, case):
    n, kind, L, tkind = case
    fp, table, x, (bits, pm, ok, stop) = pcl_ref.gpu_case(*case)
    plan, tb = _plan(n, kind), _table(*case)
    assert (tb.n, tb.k, tb.num_constraints) == (n, n - len(fp), len(table[0]))
    xd = torch.tensor(x, device=DEV)
    got, gpm, gok, gstop = pa.ops.pcl_decode(plan, tb, L, xd, return_pm=True, return_status=True)
    got8 = pa.ops.pcl_decode(plan, tb, L, xd, out_dtype=torch.uint8)  # out_pm, out_ok, out_stop NULL
    torch.cuda.synchronize()
    assert (got.dtype, got8.dtype, gpm.dtype, gok.dtype, gstop.dtype) == \
        (torch.float32, torch.uint8, torch.float32, torch.uint8, torch.int32)
    print(case, "rows stopped early:", int((stop < n).sum()), "of", len(stop))
    assert np.array_equal(gstop.cpu().numpy(), stop)
    assert np.array_equal(gok.cpu().numpy(), ok)
    bad = np.flatnonzero((got.cpu().numpy() != bits).any(1))
    assert bad.size == 0, f"rows {bad[:8]} differ"
    assert np.array_equal(gpm.cpu().numpy(), pm)
    assert np.array_equal(got8.cpu().numpy(), bits)
    if tkind == "kill":
        assert (stop == table[0][0]).all() and not got.any() and not gok.any()


@pytest.mark.parametrize("n,L", [(64, 1), (64, 8), (256, 32), (8, 4)])
def test_no_constraints_equals_pac_decode_bit_for_bit(pa, n, L):
    fp = pcl_ref.case_frozen(n, "half")
    x = torch.tensor(pac_ref.make_inputs(fp, n, (1,), LLR_MAX, 67, seed=n + L), device=DEV)
    plan = _plan(n, "half")
    tb = _table(n, "half", 8, "none") if n == 64 else pa._lib.PclTable(plan, [], [], [], np.zeros((0, max(n // 32, 1))))
    a, apm, ok, stop = pa.ops.pcl_decode(plan, tb, L, x, return_pm=True, return_status=True)
    b, bpm = pa.ops.pac_decode(plan, 1, L, x, return_pm=True)
    assert torch.equal(a, b) and torch.equal(apm, bpm) and bool((ok == 1).all()) and bool((stop == n).all())


@pytest.mark.parametrize("n", [64, 256])
def test_l1_without_constraints_equals_sc_decode(pa, n):
    """L = 1, C = 0 is min-sum SC wherever no leaf LLR is exactly zero (there SC decides 1 and the list rule keeps
    candidate 0): the inputs have no zero and the plan's llr_max is out of their reach, as in test_pac_gpu.py."""
    fp = pcl_ref.case_frozen(n, "half")
    x = pac_ref.awgn_rows(fp, n, (1,), 67, 2.0, np.random.default_rng(n))
    assert (x != 0).all() and np.abs(x).sum(1).max() < 1.0e5
    xd = torch.tensor(x, device=DEV)
    plan = _plan(n, "half", llr_max=1.0e5)
    assert plan.kernel()[0] == "generic"
    tb = pa._lib.PclTable(plan, [], [], [], np.zeros((0, n // 32)))
    assert torch.equal(pa.ops.pcl_decode(plan, tb, 1, xd), pa.ops.sc_decode(plan, xd))


def test_module_and_helper(pa):
    n = 64
    fp = pcl_ref.case_frozen(n, "half")
    table = pcl_ref.case_table(n, "half", 8, "mixed")
    _, _, x, (bits, pm, ok, stop) = pcl_ref.gpu_case(n, "half", 8, "mixed")
    cons = [(int(p), int(kd), int(r), [int(j) for j in np.flatnonzero(m)])
            for p, kd, r, m in zip(table[0], table[1], table[2], pcl_ref.unpack_mask(table[3], n))]
    mine = pa.pack_constraints(n, cons[::-1])  # any order in, sorted out
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(mine, table))
    dec = pa.PCL_Dec(torch.tensor(fp), n, cons, list_size=8, return_status=True)
    xin = torch.tensor(x).reshape(1, 67, n)  # CPU in, CPU out
    u, gok, gstop = dec(xin)
    assert u.device.type == "cpu" and u.shape == (1, 67, 32) and dec.last_pm.shape == (1, 67, 8)
    assert np.array_equal(u[0].numpy(), bits) and np.array_equal(gok[0].numpy(), ok) and np.array_equal(gstop[0].numpy(), stop)
    assert np.array_equal(dec.last_pm[0].numpy(), pm)
    plain = pa.PCL_Dec(fp, n, table, list_size=8, device=DEV)
    assert torch.equal(plain(xin.to(DEV)).cpu(), u)
    for bad in (dict(list_size=3), dict(list_size=64), dict(llr_max=0.0)):
        with pytest.raises(ValueError):
            pa.PCL_Dec(fp, n, cons, **bad)
    with pytest.raises(ValueError):
        pa.PCL_Dec(np.arange(1024), 2048, [])
    with pytest.raises(ValueError):
        pa.pack_constraints(n, [(5, 2, 0, [])])
    with pytest.raises(ValueError):  # the library's refusal of a frozen position, as a ValueError
        pa.PCL_Dec(fp, n, [(int(fp[0]), CHECK, 0, [])], device=DEV)(xin)


def test_error_codes(pa):
    from polar_amd import _lib
    L = _lib.lib()
    n, k = 64, 32
    fp = pcl_ref.case_frozen(n, "half")
    info = pcl_ref.info_positions(fp, n)
    plan = _plan(n, "half")
    P = ctypes.c_void_p

    def create(cons, plan_h=plan.handle, raw=None):
        pos, kind, rhs, mask = raw if raw is not None else pcl_ref.pack_constraints(n, cons)
        h = P()
        rc = L.pl_pcl_table_create(ctypes.byref(h), plan_h, len(pos), pos.ctypes.data_as(P), kind.ctypes.data_as(P),
                                   rhs.ctypes.data_as(P), mask.ctypes.data_as(P))
        msg = L.pl_last_error_string().decode()
        if rc == _lib.PL_OK:
            L.pl_pcl_table_destroy(h)
        else:
            assert not h.value
        return rc, msg

    a, b, c = (int(v) for v in info[3:6])
    assert create([(b, CHECK, 1, [a])])[0] == _lib.PL_OK and create([])[0] == _lib.PL_OK
    unsorted = tuple(v[::-1].copy() for v in pcl_ref.pack_constraints(n, [(a, CHECK, 0, []), (b, FORCE, 0, [])]))
    twice = tuple(np.concatenate([v, v]) for v in pcl_ref.pack_constraints(n, [(a, CHECK, 0, [])]))
    badkind = pcl_ref.pack_constraints(n, [(a, 2, 0, [])])
    badrhs = pcl_ref.pack_constraints(n, [(a, CHECK, 2, [])])
    for kw, word in ((dict(cons=[(b, CHECK, 0, [c])]), "causal"), (dict(cons=[(b, CHECK, 0, [b])]), "causal"),
                     (dict(cons=[(int(fp[5]), CHECK, 0, [])]), "frozen"),
                     (dict(cons=[(c, FORCE, 0, [int(fp[fp < c][0])])]), "frozen"),
                     (dict(cons=None, raw=unsorted), "ascending"), (dict(cons=None, raw=twice), "ascending"),
                     (dict(cons=None, raw=badkind), "kind"), (dict(cons=None, raw=badrhs), "rhs"),
                     (dict(cons=[(n, CHECK, 0, [])]), "outside"), (dict(cons=[], plan_h=None), "plan")):
        rc, msg = create(**kw)
        assert rc == _lib.PL_EINVAL and "pl_pcl_table_create" in msg and word in msg, (kw, rc, msg)
    big = _lib.Plan(2048, pa.frozen_mask(np.arange(1024), 2048), 1, 0, LLR_MAX, flags=_lib.PL_PLAN_GENERIC)
    rc, msg = create([], plan_h=big.handle)
    assert rc == _lib.PL_ENOTSUP and "2048" in msg

    tb = _table(n, "half", 8, "mixed")
    x = torch.zeros((3, n), device=DEV)
    out = torch.zeros((3, k), device=DEV)

    def dec(plan_h=plan.handle, tb_h=tb.handle, ls=4, llr=x.data_ptr(), bs=3, o=out.data_ptr(), kind=_lib.PL_OUT_F32):
        rc = L.pl_pcl_decode(plan_h, tb_h, ls, P(llr), bs, P(o), kind, P(0), P(0), P(0), P(0))
        return rc, L.pl_last_error_string().decode()

    assert dec()[0] == _lib.PL_OK and dec(bs=0, llr=0, o=0)[0] == _lib.PL_OK
    other = _lib.Plan(n, pa.frozen_mask(np.arange(32), n), 1, 0, LLR_MAX, flags=_lib.PL_PLAN_GENERIC)  # another frozen set
    other_n = _plan(256, "half")
    for kw, word in ((dict(plan_h=None), "plan"), (dict(tb_h=None), "table"), (dict(ls=0), "list_size"),
                     (dict(ls=3), "list_size"), (dict(ls=64), "list_size"), (dict(bs=-1), "bs"),
                     (dict(kind=2), "out_kind"), (dict(llr=0), "llr_logits"), (dict(o=0), "out_bits"),
                     (dict(plan_h=other.handle), "another plan"), (dict(plan_h=other_n.handle), "another plan")):
        rc, msg = dec(**kw)
        assert rc == _lib.PL_EINVAL and "pl_pcl_decode" in msg and word in msg, (kw, rc, msg)
    same = _lib.Plan(n, pa.frozen_mask(fp, n), 8, 0, 50.0, flags=_lib.PL_PLAN_GENERIC)  # the same code: accepted
    assert dec(plan_h=same.handle)[0] == _lib.PL_OK
    same.set_crc(11, 0x621)
    rc, msg = dec(plan_h=same.handle)
    assert rc == _lib.PL_ENOTSUP and "CRC" in msg
    exact = _plan(n, "half", f_mode=_lib.PL_F_EXACT)
    rc, msg = dec(plan_h=exact.handle)
    assert rc == _lib.PL_ENOTSUP and "PL_F_MINSUM" in msg
    torch.cuda.synchronize()


def _shifted(t, off):
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size() % 16 and v.is_contiguous()
    return v


def test_shifted_strided_misshapen_and_out(pa):
    case = (64, "half", 8, "mixed")
    n, kind, L, _ = case
    _, _, x, (bits, pm, ok, stop) = pcl_ref.gpu_case(*case)
    plan, tb, k = _plan(n, kind), _table(*case), n // 2
    xd = torch.tensor(x, device=DEV)
    want = torch.tensor(bits, device=DEV)
    wide = torch.zeros((x.shape[0], 2 * n), device=DEV)
    wide[:, ::2] = xd
    ints = slice(25, 46)  # the integer rows: exact in fp16
    for what, v in (("shift 1", _shifted(xd, 1)), ("shift 3", _shifted(xd, 3)), ("column stride", wide[:, ::2]),
                    ("transposed", xd.t().contiguous().t()), ("fp64", xd.double()), ("fp16 grid", None)):
        ref = want if v is not None else want[ints]
        v = v if v is not None else xd[ints].half()
        assert torch.equal(pa.ops.pcl_decode(plan, tb, L, v, out_dtype=torch.uint8), ref), what
    for off in (1, 2, 3):  # every output past a 16-byte boundary, inside sentinels
        for dt in (torch.float32, torch.uint8):
            def guarded(numel, dtype):
                buf = torch.full((16 + off + numel + 16,), 7, dtype=dtype, device=DEV)
                return buf, buf[16 + off: 16 + off + numel]
            bo, o = guarded(want.numel(), dt)
            bp, p = guarded(x.shape[0] * L, torch.float32)
            bk, okv = guarded(x.shape[0], torch.uint8)
            bs_, sv = guarded(x.shape[0], torch.int32)
            o, p = o.view(want.shape), p.view(x.shape[0], L)
            res = pa.ops.pcl_decode(plan, tb, L, xd, out=o, return_pm=True, return_status=True, pm=p, ok=okv, stop=sv)
            assert res[0] is o and res[1] is p and res[2] is okv and res[3] is sv
            assert torch.equal(o.to(torch.uint8), want) and np.array_equal(p.cpu().numpy(), pm)
            assert np.array_equal(okv.cpu().numpy(), ok) and np.array_equal(sv.cpu().numpy(), stop)
            for buf, numel in ((bo, want.numel()), (bp, p.numel()), (bk, x.shape[0]), (bs_, x.shape[0])):
                assert bool((buf[:16 + off] == 7).all()) and bool((buf[16 + off + numel:] == 7).all()), (off, dt)
    only_stop = pa.ops.pcl_decode(plan, tb, L, xd, stop=torch.zeros(x.shape[0], dtype=torch.int32, device=DEV),
                                  return_status=True)  # ok allocated, stop given
    assert np.array_equal(only_stop[2].cpu().numpy(), stop) and np.array_equal(only_stop[1].cpu().numpy(), ok)
    empty = pa.ops.pcl_decode(plan, tb, L, xd[:0], return_pm=True, return_status=True)
    assert [tuple(e.shape) for e in empty] == [(0, k), (0, L), (0,), (0,)]
    # the refusals, the exception types of the other entry points
    for bad in (xd[:, :-1], xd[0], xd[:66].reshape(-1, 2, n)):
        with pytest.raises(ValueError):
            pa.ops.pcl_decode(plan, tb, L, bad)
    with pytest.raises(RuntimeError):
        pa.ops.pcl_decode(plan, tb, L, xd.cpu())
    rows = x.shape[0]
    for bad_out in (torch.zeros((rows, k + 1), device=DEV), torch.zeros((k, rows), device=DEV).t(),
                    torch.zeros((rows, k)), torch.zeros((rows, k), dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError):
            pa.ops.pcl_decode(plan, tb, L, xd, out=bad_out)
    for kw in (dict(pm=torch.zeros((rows, L + 1), device=DEV)), dict(pm=torch.zeros((rows, L), dtype=torch.float64, device=DEV)),
               dict(ok=torch.zeros(rows, dtype=torch.int32, device=DEV)), dict(ok=torch.zeros(rows + 1, dtype=torch.uint8, device=DEV)),
               dict(stop=torch.zeros(rows, dtype=torch.int64, device=DEV)), dict(stop=torch.zeros(rows, dtype=torch.int32)),
               dict(stop=torch.zeros(2 * rows, dtype=torch.int32, device=DEV)[::2])):
        with pytest.raises(ValueError):
            pa.ops.pcl_decode(plan, tb, L, xd, **kw)
    for bad_l in (0, 3, 64):
        with pytest.raises(ValueError):
            pa.ops.pcl_decode(plan, tb, bad_l, xd)


def test_graph_capture(pa):
    case = (64, "half", 8, "mixed")
    n, kind, L, _ = case
    _, _, x, (bits, pm, ok, stop) = pcl_ref.gpu_case(*case)
    plan, tb = _plan(n, kind), _table(*case)
    xd = torch.tensor(x, device=DEV)
    rows = x.shape[0]
    static_x = torch.zeros_like(xd)
    out = torch.zeros((rows, n // 2), dtype=torch.uint8, device=DEV)
    gpm = torch.zeros((rows, L), device=DEV)
    gok = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    gstop = torch.zeros(rows, dtype=torch.int32, device=DEV)
    graph = pa.ops.LaunchGraph(lambda: pa.ops.pcl_decode(plan, tb, L, static_x, out=out, pm=gpm, ok=gok, stop=gstop), 1,
                               device=DEV)
    for src in (xd, xd.flip(0)):
        static_x.copy_(src)
        for t in (out, gpm, gok, gstop):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = pa.ops.pcl_decode(plan, tb, L, src, out_dtype=torch.uint8, return_pm=True, return_status=True)
        assert all(torch.equal(a, b) for a, b in zip((out, gpm, gok, gstop), eager))
    assert np.array_equal(out.flip(0).cpu().numpy(), bits) and np.array_equal(gstop.flip(0).cpu().numpy(), stop)
