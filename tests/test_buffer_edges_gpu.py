"""The tensor entry points of polar_amd.ops at shifted, strided and misshapen buffers.

ops.py hands every kernel raw pointers and extents.  These tests hold it to the contract written at the top of
include/polar_mi355x.h: a float, int32 or double pointer needs only its natural alignment, a uint8 output may
start anywhere, 16-byte alignment only selects a faster path with the same values, an input of another dtype
or layout is copied (and left as it was), and an `out` or `workspace` that is not what the kernel will write
is refused with ValueError before anything is launched.

  B1  every entry that takes `out`, with `out` 1, 2 and 3 elements past a 16-byte boundary inside a buffer
      of sentinels: the aligned call's values, sentinels intact; SC and SCL also against the CPU oracle;
  B2  every entry with its float / int32 inputs one element past a 16-byte boundary;
  B3  pl_count_errors on both sides of its 16-byte / element-wise branch;
  B4  fp64, fp16, bf16, column-strided, transposed and expanded inputs, bool and int64 bit tensors;
  B5  the refusals, each on storage large enough for what a kernel would have written.

Which store branch of the specialised SC kernel (csrc/sc_static.h emit) a B1 case takes:
  K % 4 == 0 ((32,64), (128,256), (512,1024)), float32 out, offset 0      the 16-byte non-temporal stores
  K % 4 == 0, float32 out, offsets 1, 2, 3 floats                          element by element
  K % 4 == 0, uint8 out, any offset                                        element by element (OUT != F32)
  K % 4 != 0 ((63,64), (1023,1024): the pinned reference sets k63_n64 and
  k1023_n1024, pre-built like every pinned set), any out, any offset       element by element
(512,1024) and (1023,1024) read their right channel half by LDS-DMA (sc_static.h load_channel).  hybrid_decode
and scf_decode run the same kernel first; hybrid_decode's row copies (hybrid_kernel.hip unit_bytes) move 16
bytes where `out` (or the logits) and the row size allow it, 4 bytes for a float32 buffer off by whole
floats, and single bytes for a uint8 `out` at offsets 1, 2, 3.
pl_count_errors (channel_kernel.hip count_errors_kernel), B3: k = 4, 64, 260 are all k % 4 == 0, so the aligned
call reads 16 bytes at a time and a shifted `a`, a shifted `b` or both read element by element (k % 4 != 0 on
aligned rows is tests/test_channel_gpu.py::test_count_errors_exact).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import osd_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 67, 131)  # ragged against every codewords-per-wave count
ROWS = max(BATCHES)
SPEC_CODES = ((32, 64), (128, 256), (512, 1024))  # K % 4 == 0; pinned and pre-built
ODD_CODES = ((63, 64), (1023, 1024))  # K % 4 != 0; pinned and pre-built
NOISE = {64: (1.6, 1.5), 256: (1.6, 1.1), 1024: (1.0, 0.6)}  # (amplitude, sigma): SC results on both sides of the CRC
OSD_CODES = ((32, 64), (24, 33))  # (k, n) of the OSD generator matrices; n = 33: rows never 16-byte aligned
GUARD = 16  # sentinel elements on each side of a guarded out
F32, U8 = torch.float32, torch.uint8


# ---- helpers ------------------------------------------------------------------------------------
def _shifted(t, off):
    """A contiguous view with t's shape and values that starts `off` elements past a 16-byte aligned address."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == off * t.element_size() % 16 and v.is_contiguous()
    return v


class _Guarded:
    """.out: a contiguous view of `shape`, `off` elements past a 16-byte aligned address, inside .buf, which
    is filled with the sentinel 7 and has at least GUARD elements on each side of the view."""

    def __init__(self, shape, dtype, off):
        numel = int(np.prod(shape))
        self.lo, self.hi = GUARD + off, GUARD + off + numel
        self.buf = torch.full((self.hi + GUARD,), 7, dtype=dtype, device=DEV)
        self.out = self.buf[self.lo:self.hi].view(shape)
        size = self.buf.element_size()
        assert self.buf.data_ptr() % 16 == 0 and GUARD * size % 16 == 0
        assert self.out.data_ptr() % 16 == off * size % 16 and self.out.is_contiguous()

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:self.lo] == 7).all()), ("written in front of out", what)
        assert bool((self.buf[self.hi:] == 7).all()), ("written past the end of out", what)
        assert bool((self.out != 7).all()), ("out not written everywhere", what)  # results are 0 / 1

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == 7).all())


def _guarded_out(shape, dtype, off):
    return _Guarded(shape, dtype, off)


def _dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    assert t.numel() == 0 or t.data_ptr() % 16 == 0
    return t


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (what, "output", i)


# ---- inputs and plans, made once ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(k, n):
    """(frozen positions, CRC name, u [ROWS, k] with the CRC in its last bits, logits [ROWS, n] fp32: the
    encoded rows over BPSK and Gaussian noise -- continuous values, no ties)."""
    import polar_amd
    crc = "CRC11" if k < 100 else "CRC24C"
    fp = polar_amd.reference_frozen_pos(k, n).numpy()
    rng = np.random.default_rng(1000 * n + k)
    u = oracle.crc_encode(rng.integers(0, 2, (ROWS, k - oracle.crc_params(crc)[0])).astype(np.float32), crc)
    amp, sig = NOISE[n]
    llr = ((2 * oracle.polar_encode(u, fp, n) - 1) * amp + rng.standard_normal((ROWS, n)) * sig).astype(np.float32)
    return fp, crc, u, llr


@functools.lru_cache(maxsize=None)
def _oracle_sc(k, n):
    fp, _, _, llr = _case(k, n)
    return oracle.sc_decode(llr, fp)


@functools.lru_cache(maxsize=None)
def _oracle_scl(k, n):
    """(bits, sorted path metrics) of the first 67 rows at n = 1024 (the oracle's time grows with n L), else all."""
    fp, _, _, llr = _case(k, n)
    return oracle.scl_decode(llr[:67 if n >= 1024 else ROWS], fp, 8, lazy=True)


@functools.lru_cache(maxsize=None)
def _grid(rows, n):
    """Multiples of 0.25 in [-8, 8]: exact in fp16 and bf16."""
    return (np.random.default_rng(n).integers(-32, 33, (rows, n)) * 0.25).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _plan(kind, k, n):
    """sc_spec: the specialised SC kernel from the pre-built cache only (nothing compiles on the GPU machine);
    sc_gen: the generic one; sc_crc: sc_spec with the case's CRC (SC-Flip, crc_status); scl_tree / scl_gen:
    L = 8 on the subtree / generic list kernel; scl_crc: L = 8 with fast-SCL and the CRC (hybrid_decode);
    scl_exact: L = 8 with the exact f, the one list plan that has a workspace."""
    import polar_amd
    from polar_amd import _lib
    fp, crc = _case(k, n)[:2]
    mask = polar_amd.frozen_mask(fp, n)
    args, want = {"sc_spec": ((1, 0, 30.0, _lib.PL_PLAN_CACHE_ONLY), "specialized"),
                  "sc_crc": ((1, 0, 30.0, _lib.PL_PLAN_CACHE_ONLY), "specialized"),
                  "sc_gen": ((1, 0, 30.0, _lib.PL_PLAN_GENERIC), "generic"),
                  "scl_tree": ((8, 0, 30.0, 0), "scl_subtree"),
                  "scl_gen": ((8, 0, 30.0, _lib.PL_PLAN_GENERIC), "generic"),
                  "scl_crc": ((8, 0, 30.0, _lib.PL_PLAN_FAST_SCL), "scl_subtree"),
                  "scl_exact": ((8, 1, 30.0, 0), "scl_subtree")}[kind]
    p = _lib.Plan(n, mask, args[0], args[1], args[2], flags=args[3], device=DEV)
    assert p.kernel()[0] == want, (kind, k, n, p.kernel())
    if kind in ("sc_crc", "scl_crc"):
        p.set_crc(*oracle.crc_params(crc))
    return p


@functools.lru_cache(maxsize=None)
def _perm_table(n):
    """Identity, bit reversal and a random permutation: pl_ae_decode takes any table."""
    from polar_amd import ops
    bits = n.bit_length() - 1
    rev = [int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)]
    return ops.ae_perm_table(np.stack([np.arange(n), np.array(rev), np.random.default_rng(n).permutation(n)]), DEV)


@functools.lru_cache(maxsize=None)
def _osd(k, n):
    """(OSD plan of order 2 of a random rank-k generator matrix, logits [ROWS, n])."""
    from polar_amd import _lib
    rng = np.random.default_rng(100 * n + k)
    plan = _lib.OsdPlan(osd_ref.random_full_rank(k, n, rng), 2, device=DEV)
    return plan, (rng.standard_normal((ROWS, n)) * 2.0).astype(np.float32)


class _Entry:
    """One entry point: run(*inputs, out=, out_dtype=) -> tuple of tensors (the first is what `out` receives),
    its inputs for a batch, the columns of `out` (None: the entry takes no `out`) and its out dtypes.
    bits: the first input is a 0/1 bit tensor (B4 also passes bool and int64)."""

    def __init__(self, run, ins, cols=None, dtypes=(F32, U8), bits=False):
        self.run, self.ins, self.cols, self.dtypes, self.bits = run, ins, cols, dtypes, bits


def _entry(name, k, n):
    from polar_amd import ops
    if name == "osd":
        plan, llr = _osd(k, n)
        return _Entry(lambda x, **kw: ops.osd_decode(plan, x, return_dist=True, return_pattern=True, **kw),
                      lambda bs: [_dev(llr[:bs])], cols=n)
    fp, crc, u, llr = _case(k, n)

    def logits(bs):
        return [_dev(llr[:bs])]

    def tup(f):
        return lambda *a, **kw: (f(*a, **kw),)
    if name in ("sc_spec", "sc_gen"):
        p = _plan(name, k, n)
        return _Entry(tup(lambda x, **kw: ops.sc_decode(p, x, **kw)), logits, cols=k)
    if name in ("scl_tree", "scl_gen"):
        p = _plan(name, k, n)
        return _Entry(lambda x, **kw: ops.scl_decode(p, x, return_pm=True, **kw), logits, cols=k)
    if name == "hybrid":
        sc, scl = _plan("sc_spec", k, n), _plan("scl_crc", k, n)

        def hybrid(x, **kw):
            out, ok, rows, n_list = ops.hybrid_decode(sc, scl, x, return_info=True, **kw)
            return out, ok, rows, torch.tensor(n_list)
        return _Entry(hybrid, logits, cols=k)
    if name == "scf":
        p = _plan("sc_crc", k, n)
        return _Entry(lambda x, **kw: ops.scf_decode(p, x, 4, return_info=True, **kw), logits, cols=k)
    if name == "ae":
        p, table = _plan("sc_gen", k, n), _perm_table(n)
        return _Entry(lambda x, **kw: ops.ae_decode(p, x, table, return_info=True, **kw), logits, cols=k)
    if name == "scq":  # logits -> llr_quantize -> scq_decode: the int8 rows are a fresh, aligned tensor
        p = _plan("sc_gen", k, n)
        return _Entry(tup(lambda x, **kw: ops.scq_decode(p, ops.llr_quantize(x, 2.0, 5), 6, **kw)), logits, cols=k)
    if name == "bp":
        p = _plan("sc_gen", k, n)

        def bp(x, out_dtype=F32):
            r = ops.bp_decode(p, x, 3, out_dtype=out_dtype, soft=True, ext=True, iters=True)
            return r["bits"], r["soft_u"], r["ext_x"], r["iters"]
        return _Entry(bp, logits)
    if name == "polar_encode":
        p = _plan("sc_gen", k, n)
        return _Entry(tup(lambda x, out=None, out_dtype=F32: ops.polar_encode(p, x, out=out)),
                      lambda bs: [_dev(u[:bs])], cols=n, dtypes=(F32,), bits=True)
    if name == "genie":
        words = ops.pack_bits(torch.as_tensor(np.random.default_rng(n).integers(0, 2, (ROWS, n)))).numpy()
        return _Entry(lambda x, w: ops.genie_count(n, x, w, return_leaf=True),
                      lambda bs: [_dev(llr[:bs]), _dev(words[:bs])])
    sent = ops.pack_bits(torch.as_tensor(u)).numpy()  # the information bits that were sent, packed
    if name == "sc_decode_count":
        p = _plan("sc_spec", k, n)
        return _Entry(tup(lambda x, w: ops.sc_decode_count(p, x, w)), lambda bs: [_dev(llr[:bs]), _dev(sent[:bs])])
    decoded = _oracle_sc(k, n)
    if name in ("count_errors_packed", "count_errors_packed_u8"):
        cast = np.float32 if name == "count_errors_packed" else np.uint8
        return _Entry(tup(lambda b, w: ops.count_errors_packed(b, w)),
                      lambda bs: [_dev(decoded[:bs].astype(cast)), _dev(sent[:bs])], bits=True)
    assert name in ("crc_status", "crc_status_u8"), name
    p = _plan("sc_crc", k, n)
    cast = np.float32 if name == "crc_status" else np.uint8
    return _Entry(tup(lambda b: ops.crc_status(p, b)), lambda bs: [_dev(decoded[:bs].astype(cast))], bits=True)


def _sent_errors(k, n, bs):
    """[bit errors, block errors] of the oracle's SC result of the first bs rows against the bits sent."""
    diff = _oracle_sc(k, n)[:bs] != _case(k, n)[2][:bs]
    return [int(diff.sum()), int(diff.any(axis=1).sum())]


def _ids(cases):
    return [f"{e}-{c[0]}_{c[1]}" for e, c in cases]


OUT_ENTRIES = ("sc_spec", "sc_gen", "scl_tree", "scl_gen", "hybrid", "scf", "ae", "scq", "polar_encode")
B1_CASES = [(e, c) for e in OUT_ENTRIES for c in SPEC_CODES] + [("sc_spec", c) for c in ODD_CODES] + \
    [("sc_gen", ODD_CODES[0])] + [("osd", c) for c in OSD_CODES]


# ---- B1: shifted out ----------------------------------------------------------------------------
@pytest.mark.parametrize("entry,code", B1_CASES, ids=_ids(B1_CASES))
def test_shifted_out_equals_the_aligned_call(entry, code):
    """float32 out 1, 2 and 3 floats, uint8 out 1, 2 and 3 bytes past a 16-byte boundary (and at it), in
    sentinels: bit for bit the call that allocates its own (aligned) out, every other output too, nothing
    written outside out.  sc_decode and scl_decode also equal the CPU oracle on the same rows, so the pair
    cannot be wrong together.  The branch of the specialised kernel each case takes: the module docstring."""
    k, n = code
    e = _entry(entry, k, n)
    for bs in BATCHES:
        ins = e.ins(bs)
        for dtype in e.dtypes:
            want = e.run(*ins, out_dtype=dtype)
            assert want[0].dtype == dtype and want[0].shape == (bs, e.cols) and want[0].data_ptr() % 16 == 0
            first = want[0].cpu().numpy()
            if entry in ("sc_spec", "sc_gen"):
                assert np.array_equal(first, _oracle_sc(k, n)[:bs].astype(first.dtype)), (entry, code, bs)
            if entry in ("scl_tree", "scl_gen") and bs <= len(_oracle_scl(k, n)[0]):
                bits, pm = _oracle_scl(k, n)
                assert np.array_equal(first, bits[:bs].astype(first.dtype)), (entry, code, bs)
                assert np.abs(want[1].cpu().numpy() - pm[:bs]).max() <= 1e-9  # tests/test_scl_gpu.py PM_TOL
            for off in (0, 1, 2, 3):
                g = _guarded_out((bs, e.cols), dtype, off)
                got = e.run(*ins, out=g.out)
                assert got[0] is g.out
                g.check((entry, code, bs, dtype, off))
                _same(got, want, (entry, code, bs, dtype, off))


def test_hybrid_and_scf_cases_reach_both_stages():
    """The shared inputs leave SC results on both sides of the CRC at bs = 67 and 131, so hybrid_decode
    gathers, list-decodes and scatters some rows and keeps the others, and SC-Flip has rows to flip."""
    from polar_amd import ops
    for k, n in SPEC_CODES:
        failing = ~oracle.crc_check(_oracle_sc(k, n), _case(k, n)[1]).astype(bool)
        for bs in BATCHES[1:]:
            x = _dev(_case(k, n)[3][:bs])
            n_list = ops.hybrid_decode(_plan("sc_spec", k, n), _plan("scl_crc", k, n), x, return_info=True)[3]
            assert 0 < n_list < bs and n_list == int(failing[:bs].sum()), (k, n, bs, n_list)
            att = ops.scf_decode(_plan("sc_crc", k, n), x, 4, return_info=True)[3]
            assert np.array_equal((att > 1).cpu().numpy(), failing[:bs]), (k, n, bs)


# ---- B2: shifted inputs -------------------------------------------------------------------------
IN_ENTRIES = ("sc_spec", "sc_gen", "scl_tree", "scl_gen", "hybrid", "scf", "ae", "bp", "polar_encode", "genie",
              "crc_status", "crc_status_u8", "sc_decode_count", "count_errors_packed", "count_errors_packed_u8")
B2_CASES = [(e, c) for e in IN_ENTRIES for c in SPEC_CODES] + [("sc_spec", c) for c in ODD_CODES] + \
    [("osd", c) for c in OSD_CODES]


@pytest.mark.parametrize("entry,code", B2_CASES, ids=_ids(B2_CASES))
def test_shifted_inputs_equal_the_aligned_call(entry, code):
    """Logits one float, packed words one int32 word, uint8 bits one byte past a 16-byte boundary -- each input
    alone, then all of them: every output equals the aligned call's.  (scq_decode's int8 rows are copied when
    misaligned: tests/test_scq_gpu.py.)  The counters also equal the errors counted in numpy."""
    k, n = code
    e = _entry(entry, k, n)
    for bs in BATCHES:
        ins = e.ins(bs)
        want = e.run(*ins)
        if entry in ("sc_decode_count", "count_errors_packed", "count_errors_packed_u8"):
            assert want[0].tolist() == _sent_errors(k, n, bs), (entry, code, bs)
        if entry.startswith("crc_status"):
            ok = oracle.crc_check(_oracle_sc(k, n)[:bs], _case(k, n)[1]).astype(bool)
            assert np.array_equal(want[0].cpu().numpy(), ok), (entry, code, bs)
        moved = [[i] for i in range(len(ins))] + ([list(range(len(ins)))] if len(ins) > 1 else [])
        for which in moved:
            shifted = [_shifted(t, 1) if i in which else t for i, t in enumerate(ins)]
            _same(e.run(*shifted), want, (entry, code, bs, which))


# ---- B3: pl_count_errors on both sides of its branch ----------------------------------------------
@pytest.mark.parametrize("k", [4, 64, 260])
@pytest.mark.parametrize("rows", [1, 3, 1001])
def test_count_errors_aligned_and_shifted(rows, k):
    """k % 4 == 0 throughout: the aligned call takes the 16-byte loads, a shifted `a`, a shifted `b` and both
    take the element-wise loop.  All four equal the bit and block errors counted in numpy."""
    from polar_amd import ops
    rng = np.random.default_rng(rows * 1000 + k)
    a = rng.integers(0, 2, (rows, k)).astype(np.float32)
    b = np.where(rng.random((rows, k)) < 0.02, 1 - a, a).astype(np.float32)
    b[rows // 2] = a[rows // 2]  # at least one clean row ...
    b[0, k - 1] = 1 - a[0, k - 1]  # ... and one error, in the last column
    want = [int((a != b).sum()), int((a != b).any(axis=1).sum())]
    at, bt = _dev(a), _dev(b)
    aligned = ops.count_errors(at, bt)
    assert aligned.tolist() == want
    for sa, sb in ((1, 0), (0, 1), (1, 1)):
        got = ops.count_errors(_shifted(at, sa), _shifted(bt, sb))
        assert got.tolist() == want and torch.equal(got, aligned), (rows, k, sa, sb)


# ---- B4: coerced inputs ---------------------------------------------------------------------------
B4_CODE = (128, 256)
B4_BS = 67
B4_ENTRIES = ("sc_spec", "sc_gen", "scl_tree", "scl_gen", "hybrid", "scf", "ae", "scq", "bp", "genie",
              "sc_decode_count", "polar_encode", "crc_status", "count_errors_packed")
B4_CASES = [(e, B4_CODE) for e in B4_ENTRIES] + [("sc_spec", SPEC_CODES[2]), ("osd", OSD_CODES[0])]


def _views(x):
    """(name, tensor with x's values in another dtype or layout); the last has the values of x's first row."""
    bs, n = x.shape
    x2 = torch.full((bs, 2 * n), 5.0, device=DEV)
    x2[:, ::2] = x
    xt = x.t().contiguous()
    out = [("fp64", x.double()), ("fp16", x.half()), ("bf16", x.bfloat16()), ("cols", x2[:, ::2]), ("t", xt.t()),
           ("expand", x[:1].expand(bs, n))]
    for name, v in out[:5]:
        assert torch.equal(v.float(), x), name  # the grid is exact in every format
    assert not out[3][1].is_contiguous() and not out[4][1].is_contiguous() and out[5][1].stride(0) == 0
    return out


@pytest.mark.parametrize("entry,code", B4_CASES, ids=_ids(B4_CASES))
def test_coerced_inputs_equal_their_float32_copy(entry, code):
    """fp64, fp16, bf16 (values on a grid all three hold exactly), every second column of a [bs, 2n] tensor,
    the transpose of an [n, bs] tensor and a row expanded with stride 0 (bit inputs: also bool and int64):
    each result equals the call on x.to(float32).contiguous(), and the caller's tensor is as it was -- the
    same object, dtype, strides and values.  Packed int32 words pass as every second column too."""
    k, n = code
    e = _entry(entry, k, n)
    ins = e.ins(B4_BS)
    x = ins[0].float() if e.bits else _dev(_grid(B4_BS, ins[0].shape[1]))
    views = _views(x)
    if e.bits:
        views += [("bool", x != 0), ("int64", x.long())]
    for name, v in views:
        want = e.run(v.to(F32).contiguous(), *ins[1:])
        keep, meta = v.clone(), (v.dtype, v.shape, v.stride(), v.data_ptr())
        _same(e.run(v, *ins[1:]), want, (entry, name))
        assert (v.dtype, v.shape, v.stride(), v.data_ptr()) == meta and torch.equal(v, keep), (entry, name)
    if len(ins) > 1:  # the packed words: int32 only, any layout
        w2 = torch.full((B4_BS, 2 * ins[1].shape[1]), 5, dtype=torch.int32, device=DEV)
        w2[:, ::2] = ins[1]
        keep = w2.clone()
        _same(e.run(ins[0], w2[:, ::2]), e.run(*ins), (entry, "words"))
        assert torch.equal(w2, keep)


# ---- B5: refusals ---------------------------------------------------------------------------------
R_K, R_N, R_BS = 32, 64, 5


def _refused_outs(rows, cols, dtype=F32):
    """[bs, cols]-like tensors that are not a contiguous [bs, cols] tensor, each a view of at least rows * cols
    elements of storage."""
    return {"transposed": torch.full((cols, rows), 7, dtype=dtype, device=DEV).t(),
            "flat": torch.full((rows * cols,), 7, dtype=dtype, device=DEV),
            "one_row_more": torch.full((rows + 1, cols), 7, dtype=dtype, device=DEV),
            "one_column_more": torch.full((rows, cols + 1), 7, dtype=dtype, device=DEV),
            "row_stride": torch.full((rows, cols + 1), 7, dtype=dtype, device=DEV)[:, :cols]}


def _raises_and_leaves(call, t, what):
    with pytest.raises(ValueError):
        call()
    torch.cuda.synchronize()
    assert bool((t == 7).all()), ("written before the refusal", what)  # refused before any launch


@pytest.mark.parametrize("kind", ["scl_tree", "scl_gen"])
@pytest.mark.parametrize("bad", ["transposed", "flat", "one_row_more", "one_column_more", "row_stride"])
def test_scl_decode_refuses_a_misshapen_out(kind, bad):
    from polar_amd import ops
    plan, x = _plan(kind, R_K, R_N), _dev(_case(R_K, R_N)[3][:R_BS])
    for dtype in (F32, U8):
        out = _refused_outs(R_BS, R_K, dtype)[bad]
        _raises_and_leaves(lambda: ops.scl_decode(plan, x, out=out), out, (kind, bad, dtype))


@pytest.mark.parametrize("bad", ["float32", "every_second_byte", "off_by_one_byte"])
def test_scl_decode_refuses_a_workspace_that_is_not_plain_bytes(bad):
    """The exact-f subtree plan: the one list plan whose workspace the kernel uses (fp64 tables).  Every refused
    workspace has at least ws_bytes bytes of storage behind its pointer."""
    from polar_amd import _lib, ops
    plan, x = _plan("scl_exact", R_K, R_N), _dev(_case(R_K, R_N)[3][:R_BS])
    ws_bytes = int(_lib.lib().pl_scl_workspace_size(plan.handle, R_BS))
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    ws = {"float32": lambda: torch.zeros(ws_bytes, dtype=F32, device=DEV),
          "every_second_byte": lambda: torch.zeros(2 * ws_bytes, dtype=U8, device=DEV)[::2],
          "off_by_one_byte": lambda: torch.zeros(ws_bytes + 8, dtype=U8, device=DEV)[1:1 + ws_bytes]}[bad]()
    assert ws.numel() == ws_bytes
    g = _guarded_out((R_BS, R_K), F32, 0)
    with pytest.raises(ValueError, match="workspace"):
        ops.scl_decode(plan, x, out=g.out, workspace=ws)
    assert g.untouched()


@pytest.mark.parametrize("bad", ["float64", "uint8", "transposed", "flat", "one_row_more", "one_column_more",
                                 "row_stride"])
def test_polar_encode_refuses_an_out_that_is_not_float32_bs_n(bad):
    from polar_amd import ops
    plan, u = _plan("sc_gen", R_K, R_N), _dev(_case(R_K, R_N)[2][:R_BS])
    if bad == "float64":
        out = torch.full((R_BS, R_N), 7, dtype=torch.float64, device=DEV)
    elif bad == "uint8":  # [bs, n] bytes at the head of the 4 bs n bytes the kernel would have written
        out = torch.full((4 * R_BS * R_N,), 7, dtype=U8, device=DEV)[:R_BS * R_N].view(R_BS, R_N)
    else:
        out = _refused_outs(R_BS, R_N)[bad]
    _raises_and_leaves(lambda: ops.polar_encode(plan, u, out=out), out, bad)


def test_sc_decode_count_refuses_ref_bits_that_are_no_tensor():
    """The ValueError of count_errors_packed, for a numpy array and for a nested list, and counts untouched."""
    from polar_amd import ops
    e = _entry("sc_decode_count", R_K, R_N)
    x, words = e.ins(R_BS)
    plan = _plan("sc_spec", R_K, R_N)
    for bad in (words.cpu().numpy(), words.cpu().tolist(), None):
        counts = torch.full((2,), 7, dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError, match="ref_bits must be int32"):
            ops.sc_decode_count(plan, x, bad, counts=counts)
        with pytest.raises(ValueError, match="ref_bits must be int32"):
            ops.count_errors_packed(_dev(_oracle_sc(R_K, R_N)[:R_BS]), bad, counts=counts)
        torch.cuda.synchronize()
        assert counts.tolist() == [7, 7]


def test_out_on_another_device_is_refused():
    from polar_amd import ops
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: an out on another device needs two")
    x, u = _dev(_case(R_K, R_N)[3][:R_BS]), _dev(_case(R_K, R_N)[2][:R_BS])
    far = torch.full((R_BS, R_K), 7.0, device="cuda:1")
    _raises_and_leaves(lambda: ops.scl_decode(_plan("scl_tree", R_K, R_N), x, out=far), far, "scl_decode")
    far_n = torch.full((R_BS, R_N), 7.0, device="cuda:1")
    _raises_and_leaves(lambda: ops.polar_encode(_plan("sc_gen", R_K, R_N), u, out=far_n), far_n, "polar_encode")
    plan = _plan("scl_exact", R_K, R_N)
    with pytest.raises(ValueError, match="workspace"):
        ops.scl_decode(plan, x, workspace=ops.scl_workspace(plan, R_BS, "cuda:1"))


def test_a_valid_out_and_workspace_are_used_and_returned():
    from polar_amd import ops
    fp, _, u, llr = _case(R_K, R_N)
    x = _dev(llr[:R_BS])
    for kind in ("scl_tree", "scl_gen", "scl_exact"):
        plan = _plan(kind, R_K, R_N)
        want, want_pm = ops.scl_decode(plan, x, return_pm=True)
        ws = ops.scl_workspace(plan, R_BS, x.device)
        larger = torch.zeros(ws.numel() + 64, dtype=U8, device=DEV)
        for w in (ws, larger):
            out = torch.full((R_BS, R_K), 7.0, device=DEV)
            back, pm = ops.scl_decode(plan, x, out=out, return_pm=True, workspace=w)
            assert back is out and torch.equal(out, want) and torch.equal(pm, want_pm), kind
    enc = _plan("sc_gen", R_K, R_N)
    cw = torch.full((R_BS, R_N), 7.0, device=DEV)
    assert ops.polar_encode(enc, _dev(u[:R_BS]), out=cw) is cw
    assert np.array_equal(cw.cpu().numpy(), oracle.polar_encode(u[:R_BS], fp, R_N))
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    e = _entry("sc_decode_count", R_K, R_N)
    assert ops.sc_decode_count(_plan("sc_spec", R_K, R_N), *e.ins(R_BS), counts=counts) is counts
    assert counts.tolist() == _sent_errors(R_K, R_N, R_BS)
