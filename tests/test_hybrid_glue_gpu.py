"""The device-side glue of pl_hybrid_decode and pl_crc_status (csrc/hybrid_kernel.hip) at its edges.

tests/test_hybrid_gpu.py holds the hybrid decoder to its definition at three codes whose k is a
power of two and whose rows are multiples of 16 bytes, with random failure patterns in batches of
at most 40000 rows.  This file runs the branches those shapes leave out:
  1. crc_flag: the table x^(deg+j) mod G built by doubling, for ten generators (degrees 1 ... 31,
     g = 0 among them) and k from deg to 2048, against a plain shift register;
  2. gather_rows_idx / scatter_bits_idx with 16-, 4- and 1-byte units, one unit per row and unit
     counts that are no power of two, against the oracle's composition;
  3. compact_failed with failures placed exactly on the 64- and 256-row boundaries, and batches
     past 262144 rows, where a block makes more than one trip over its span;
  4. the cached workspace, reused by a smaller and then the larger batch again.
All of it is integer work: every comparison is for equality."""
import functools

import numpy as np
import pytest
import torch

import oracle
from test_hybrid_gpu import CASES, L8, _check, _classes, _compose, _expected, _input, _plans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import polar_amd
    return polar_amd


# ---- the reference: an MSB-first shift register over any (deg, g) -------------------------------

def _register(bits, deg, g):
    """The register of x^deg + g after the bits of every row ([rows, k] 0/1), MSB first."""
    bits = np.asarray(bits)
    reg = np.zeros(bits.shape[0], dtype=np.uint64)
    mask, top, gen = np.uint64((1 << deg) - 1), np.uint64(deg - 1), np.uint64(g)
    one = np.uint64(1)
    for m in range(bits.shape[1]):
        fb = ((reg >> top) & one) ^ bits[:, m].astype(np.uint64)
        reg = ((reg << one) & mask) ^ (fb * gen)
    return reg


def _crc_valid(bits, deg, g):
    return _register(bits, deg, g) == 0


def _with_parity(info, deg, g):
    """[rows, k - deg] information bits -> [rows, k] words that leave the register at zero."""
    rem = _register(info, deg, g)
    par = (rem[:, None] >> np.arange(deg - 1, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)
    return np.concatenate([np.asarray(info, dtype=np.uint8), par.astype(np.uint8)], axis=1)


@pytest.mark.parametrize("name", sorted(oracle.CRC_POLYS))
def test_register_is_the_oracles_crc(name):
    """Ties the register of this file to the project's oracle: same validity, same parity bits."""
    deg, g = oracle.crc_params(name)
    rng = np.random.default_rng(deg)
    info = rng.integers(0, 2, (300, 53), dtype=np.uint8)
    words = oracle.crc_encode(info.astype(np.float32), name).astype(np.uint8)
    assert np.array_equal(_with_parity(info, deg, g), words)
    words[100:200] ^= (rng.random((100, words.shape[1])) < 0.03).astype(np.uint8)
    words[200:] = rng.integers(0, 2, (100, words.shape[1]), dtype=np.uint8)
    want = oracle.crc_check(words.astype(np.float32), name)
    assert want[:100].all() and not want[200:].all()
    assert np.array_equal(_crc_valid(words, deg, g), want)


# ---- 1. pl_crc_status against the register ------------------------------------------------------

GENERATORS = {name: oracle.crc_params(name) for name in sorted(oracle.CRC_POLYS)}
GENERATORS.update({"deg1": (1, 1), "deg7": (7, 0x09), "deg31": (31, (1 << 30) | 0x5), "deg16_g0": (16, 0)})
CRC_KS = (63, 64, 65, 100, 127, 128, 129, 191, 257, 1000, 2047, 2048)
CRC_CASES = [(name, k) for name, (deg, _) in GENERATORS.items()
             for k in sorted({deg, deg + 1, *CRC_KS}) if k >= deg and k >= 2]


def test_crc_case_list_covers_what_it_must():
    for name in GENERATORS:
        assert {65, 100, 129, 1000} <= {k for n_, k in CRC_CASES if n_ == name}
    for k in (2047, 2048):
        assert sum(1 for _, kk in CRC_CASES if kk == k) >= 2


def _crc_plan(k, deg, g):
    """A generic L = 1 plan that carries (k, CRC): n the smallest power of two >= max(k, 2), the
    first n - k positions frozen."""
    from polar_amd import _lib
    n = 1 << (max(k, 2) - 1).bit_length()
    mask = np.zeros(n, dtype=np.uint8)
    mask[: n - k] = 1
    plan = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
    plan.set_crc(deg, g)
    assert (plan.n, plan.k) == (n, k)
    return plan


def _crc_rows(k, deg, g, rng):
    """64 valid words, the zero word, every single flip of one valid word, 64 double flips, 32
    random words; one more random word if that is a multiple of the 8 rows a block takes a pass."""
    valid = _with_parity(rng.integers(0, 2, (64, k - deg), dtype=np.uint8), deg, g)
    single = valid[:1] ^ np.eye(k, dtype=np.uint8)
    double = valid.copy()
    for i in range(64):
        double[i, rng.choice(k, 2, replace=False)] ^= 1
    rows = np.concatenate([valid, np.zeros((1, k), dtype=np.uint8), single, double,
                           rng.integers(0, 2, (32, k), dtype=np.uint8)])
    if len(rows) % 8 == 0:
        rows = np.concatenate([rows, rng.integers(0, 2, (1, k), dtype=np.uint8)])
    return rows


def _as_float(bits, rng):
    """0/1 -> fp32 with some ones written as 2.0 and some zeros as -0.0 (the kernel's rule: != 0)."""
    x = bits.astype(np.float32)
    pick = rng.random(bits.shape) < 0.25
    x[pick & (bits == 1)] = 2.0
    x[pick & (bits == 0)] = -0.0
    return x


def _check_crc_status(plan, bits, want, rng, what):
    from polar_amd import ops
    x = _as_float(bits, rng)
    assert (x == 2.0).any() and (np.signbit(x) & (x == 0)).any()
    for host in (x, bits):
        got = ops.crc_status(plan, torch.from_numpy(host).cuda())
        assert got.dtype == torch.bool and got.shape == (len(bits),)
        got = got.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, host.dtype, "rows", bad[:8], "kernel", got[bad[:8]], "register", want[bad[:8]])


@pytest.mark.parametrize("name,k", CRC_CASES)
def test_crc_status_vs_register(pa, name, k):
    deg, g = GENERATORS[name]
    rng = np.random.default_rng([deg, g, k])
    bits = _crc_rows(k, deg, g, rng)
    assert len(bits) % 8 != 0
    want = _crc_valid(bits, deg, g)
    assert want[:65].all()  # the words built as valid, and the zero word
    _check_crc_status(_crc_plan(k, deg, g), bits, want, rng, (name, k))


def test_crc_status_grid_stride(pa):
    """16384 + 9 rows: more than the 2048 blocks of 8 rows the launch is capped at."""
    k, bs = 65, 16384 + 9
    deg, g = GENERATORS["CRC11"]
    rng = np.random.default_rng(65)
    bits = _with_parity(rng.integers(0, 2, (bs, k - deg), dtype=np.uint8), deg, g)
    flip = rng.random(bs) < 0.5
    bits[flip, rng.integers(0, k, bs)[flip]] ^= 1
    want = _crc_valid(bits, deg, g)
    assert np.array_equal(want, ~flip)  # a single flip is always detected
    _check_crc_status(_crc_plan(k, deg, g), bits, want, rng, "grid stride")


# ---- codes of any k: the 5G frozen set ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frozen_5g(k, n):
    from polar_amd import polar5g
    return polar5g.generate_5g_ranking(k, n)[0]


def _plans_5g(pa, k, n, crc):
    """The SC plan (generic: nothing is compiled) and the L = 8 min-sum fast-SCL plan with the CRC."""
    from polar_amd import _lib
    mask = pa.frozen_mask(_frozen_5g(k, n), n)
    sc = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
    scl = _lib.Plan(n, mask, L8, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_FAST_SCL)
    scl.set_crc(*oracle.crc_params(crc))
    assert sc.kernel()[0] == "generic" and scl.kernel()[0] == "scl_subtree"
    assert (sc.k, scl.k) == (k, k)
    return sc, scl


# ---- 2. row copies at every unit width ----------------------------------------------------------

COPY_BS = 151
# (k, n, CRC) -> (seed, amp, sig), chosen on the CPU with the oracle alone so that every branch has
# rows, and the rows by branch (SC passes, list passes, both fail) that choice gives
COPY_SHAPES = {(16, 32, "CRC6"): (1, 1.3, 1.5), (24, 32, "CRC6"): (1, 1.0, 0.8), (36, 64, "CRC11"): (1, 1.6, 1.5),
               (37, 64, "CRC11"): (1, 1.3, 1.2), (40, 64, "CRC11"): (1, 2.0, 1.8)}
COPY_CLASSES = {(16, 32, "CRC6"): (46, 61, 44), (24, 32, "CRC6"): (59, 52, 40), (36, 64, "CRC11"): (58, 49, 44),
                (37, 64, "CRC11"): (52, 49, 50), (40, 64, "CRC11"): (41, 52, 58)}
# (unit bytes, units per row) of the scatter launch_copy_rows makes, by (k, element size)
COPY_UNITS = {(16, 4): (16, 4), (16, 1): (16, 1), (24, 4): (16, 6), (24, 1): (4, 6), (36, 4): (16, 9),
              (36, 1): (4, 9), (37, 4): (4, 37), (37, 1): (1, 37), (40, 4): (16, 10), (40, 1): (4, 10)}


def _unit(row_bytes):
    """unit_bytes of hybrid_kernel.hip for 16-byte aligned bases (the caching allocator's and the
    workspace's are): the widest of 16, 4, 1 bytes that divides the row."""
    ub = 16 if row_bytes % 16 == 0 else 4 if row_bytes % 4 == 0 else 1
    return ub, row_bytes // ub


def test_copy_shapes_cover_every_unit_width():
    got = {(k, size): _unit(k * size) for k, _, _ in COPY_SHAPES for size in (4, 1)}
    assert got == COPY_UNITS
    assert {ub for ub, _ in got.values()} == {16, 4, 1}
    assert {4, 6, 9, 10, 37} <= {units for _, units in got.values()}
    assert (16, 1) in got.values()  # one unit per row: log_lpr = 0, 64 rows per wave
    assert all(_unit(n * 4)[0] == 16 for _, n, _ in COPY_SHAPES)  # the gather of LLR rows


@functools.lru_cache(maxsize=None)
def _copy_case(k, n, crc):
    """(llr, the oracle's composition) of a shape: the recipe of test_hybrid_gpu._input on the 5G set."""
    seed, amp, sig = COPY_SHAPES[(k, n, crc)]
    deg = oracle.crc_params(crc)[0]
    fp = _frozen_5g(k, n)
    rng = np.random.default_rng(seed)
    u = oracle.crc_encode(rng.integers(0, 2, (COPY_BS, k - deg)).astype(np.float32), crc)
    cw = oracle.polar_encode(u, fp, n)
    llr = ((2 * cw - 1) * amp + rng.standard_normal(cw.shape) * sig).astype(np.float32)
    return llr, _compose(llr, fp, crc)


@pytest.mark.parametrize("shape", list(COPY_SHAPES), ids=lambda s: f"k{s[0]}n{s[1]}")
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.uint8])
def test_hybrid_row_copies_vs_oracle_composition(pa, shape, out_dtype):
    from polar_amd import ops
    k, n, crc = shape
    itemsize = torch.empty((), dtype=out_dtype).element_size()
    assert _unit(k * itemsize) == COPY_UNITS[(k, itemsize)]
    llr, want = _copy_case(*shape)
    assert _classes(want) == COPY_CLASSES[shape] and min(_classes(want)) >= 10
    sc, scl = _plans_5g(pa, k, n, crc)
    got = ops.hybrid_decode(sc, scl, torch.from_numpy(llr).cuda(), out_dtype=out_dtype, return_info=True)
    assert got[0].dtype == out_dtype
    _check(got, want, (shape, out_dtype))
    assert np.array_equal(ops.crc_status(scl, got[0]).cpu().numpy(), want[1])


# ---- 3. compaction with chosen failure patterns -------------------------------------------------

CK, CN, CCRC = 16, 32, "CRC6"
BS_SMALL, BS_SPAN256, BS_SPAN512 = 1025, 262144, 262144 + 257


def _small_patterns(bs):
    r = np.arange(bs)
    inside = (r >= 256) & (r < 512)
    return {"row0": [0], "last_row": [bs - 1], "block_edge": [255, 256],
            "wave_edges": [63, 64, 127, 128, 191, 192], "block1_only": r[inside], "all_but_block1": r[~inside],
            "even_rows": r[::2], "wave1_of_every_block": r[(r % 256) // 64 == 1]}


def _large_patterns(bs):
    # every3rd: failures in both trips of every block of the 512-row span (the carry between the
    # trips), and more than five chunks of 16384 rows for the list stage
    return {"edges": [0, 255, 256, 511, 512, 513, bs - 257, bs - 1], "run300": np.arange(70037, 70037 + 300),
            "every4099th": np.arange(0, bs, 4099), "every3rd": np.arange(1, bs, 3)}


@pytest.fixture(scope="module")
def batch(pa):
    """bs -> (plans, u, clean LLRs) of bs CRC-carrying words of the (16, 32, CRC6) code, on the
    device.  One batch at a time is kept, and none after the module."""
    from polar_amd import ops
    state = {}

    def get(bs):
        if state.get("bs") != bs:
            state.clear()
            sc, scl = _plans_5g(pa, CK, CN, CCRC)
            deg = oracle.crc_params(CCRC)[0]
            info = np.random.default_rng(bs).integers(0, 2, (bs, CK - deg)).astype(np.float32)
            u = torch.from_numpy(oracle.crc_encode(info, CCRC)).cuda()
            llr = (2.0 * ops.polar_encode(sc, u) - 1.0) * 4.0
            state.update(bs=bs, got=((sc, scl), u, llr))
        return state["got"]

    yield get
    state.clear()


def _check_compaction(batch, bs, P, out_dtype, what):
    """Rows P carry a word whose last parity bit is flipped, without noise: SC returns every row's
    word exactly, so exactly the rows of P fail the CRC (a single flip is always detected)."""
    from polar_amd import ops
    (sc, scl), u, clean = batch(bs)
    P = np.asarray(P, dtype=np.int64)
    assert np.all(np.diff(P) > 0) and 0 <= P[0] and P[-1] < bs
    idx = torch.from_numpy(P).cuda()
    sent = u[idx].clone()
    sent[:, -1] = 1.0 - sent[:, -1]
    llr = clean.clone()
    llr[idx] = (2.0 * ops.polar_encode(sc, sent) - 1.0) * 4.0
    out, ok, rows, n_list = ops.hybrid_decode(sc, scl, llr, out_dtype=out_dtype, return_info=True)
    assert n_list == len(P), (what, n_list, len(P))
    assert rows.dtype == torch.int32 and torch.equal(rows, idx.to(torch.int32)), what
    want = u.clone()
    want[idx] = ops.scl_decode(scl, llr[idx])  # the list decoder alone, verified in test_scl_gpu.py
    assert out.dtype == out_dtype and torch.equal(out, want.to(out_dtype)), what
    deg, g = oracle.crc_params(CCRC)
    out_h = out.cpu().numpy()
    assert ok.dtype == torch.bool and np.array_equal(ok.cpu().numpy(), _crc_valid(out_h, deg, g)), what
    assert bool(ok[torch.from_numpy(np.setdiff1d(np.arange(bs), P)).cuda()].all()), what
    return llr, (out_h, ok.cpu().numpy(), rows.cpu().numpy())


@pytest.mark.parametrize("pattern", list(_small_patterns(BS_SMALL)))
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.uint8])
def test_compaction_small_batch_patterns(batch, pattern, out_dtype):
    """1025 rows: four full blocks of 256 and a block of one row."""
    P = _small_patterns(BS_SMALL)[pattern]
    llr, got = _check_compaction(batch, BS_SMALL, P, out_dtype, pattern)
    w_out, w_ok, w_rows = _compose(llr.cpu().numpy(), _frozen_5g(CK, CN), CCRC)
    assert np.array_equal(got[2], w_rows) and np.array_equal(got[1], w_ok) and np.array_equal(got[0], w_out)


@pytest.mark.parametrize("pattern", list(_large_patterns(BS_SPAN256)))
@pytest.mark.parametrize("bs", [BS_SPAN256, BS_SPAN512])
def test_compaction_large_batch_patterns(batch, bs, pattern):
    """262144 rows: 1024 blocks with a span of 256.  262144 + 257 rows: the span is 512, so every
    one of the 513 blocks carries its offset into a second trip; the last block's holds one row."""
    _check_compaction(batch, bs, _large_patterns(bs)[pattern], torch.float32, (bs, pattern))


# ---- 4. workspace reuse -------------------------------------------------------------------------

def test_hybrid_workspace_reuse_on_one_stream(pa):
    """4096 rows, then 37, then the 4096 again through the cached workspace (grown, never shrunk):
    the same results as calls that each start without one."""
    from polar_amd import _lib, ops
    cfg = CASES["k32"]
    fp, _, x = _input(*cfg)
    sc, scl = _plans(pa, *cfg[:3], sc_flags=_lib.PL_PLAN_GENERIC)
    big = torch.from_numpy(np.tile(x, (16, 1))).cuda()
    small = big[:37].contiguous()
    assert big.shape == (4096, 64)

    def run(llr):
        out, ok, rows, n_list = ops.hybrid_decode(sc, scl, llr, return_info=True)
        return out.clone(), ok.clone(), rows.clone(), n_list

    def same(a, b):
        return a[3] == b[3] and all(torch.equal(p, q) for p, q in zip(a[:3], b[:3]))

    fresh = []
    for llr in (big, small):
        ops._hybrid_ws.clear()
        fresh.append(run(llr))
    ops._hybrid_ws.clear()
    first = run(big)
    ws = ops.hybrid_workspace(sc, scl, 4096, big.device)
    second = run(small)
    assert ops.hybrid_workspace(sc, scl, 37, big.device) is ws  # kept, not replaced by a smaller one
    third = run(big)
    assert ops.hybrid_workspace(sc, scl, 4096, big.device) is ws
    assert same(first, fresh[0]) and same(second, fresh[1]) and same(third, fresh[0])
    # and they are the right results: the oracle's composition of the 256 rows, tiled
    w_out, w_ok, w_rows = _expected(*cfg)
    w_rows = np.concatenate([w_rows + 256 * t for t in range(16)]).astype(np.int32)
    _check(third, (np.tile(w_out, (16, 1)), np.tile(w_ok, 16), w_rows), "tiled")
    _check(second, _compose(x[:37], fp, cfg[2]), "37 rows")
