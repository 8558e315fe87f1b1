"""CPU checks of tests/golden/noise_ref.py, the float64 restatement of the fused producers' noise
draws, and the measurement of the bounds tests/test_noise_gpu.py holds the kernels to.

  * gauss4 is a standard-normal sampler (moments and I/Q correlation on 2^22 Philox blocks), and its
    edge words are finite and as computed by hand;
  * the counter words of the four streams (information bits and noise of the plain / QAM / NR
    producers, information bits and noise of the producer inside the SC kernel) never meet;
  * the bounds: the same formula evaluated op by op in numpy float32 against gauss4, on the 2^22
    blocks plus the edge words, in two classes of the radius term u = 32 - log2 v':
        class A, u >= 1/16   measured 2.25e-06   kernel bound 4x = 9.00e-06
        class B, u <  1/16   measured 1.14e-03   kernel bound 4x = 4.56e-03
    (absolute errors of the standardised noise z; in class B the float32 difference 32 - log2 v'
    cancels, down to exactly 0 against a true radius of up to 1e-3).  The factor 4 is
    test_qam.DEMAP_BOUND's: room for hardware log2 / sqrt / sin / cos a few ulp worse than libm's;
  * the mutation table: compare() reports a violation of these bounds for every fault of the list
    in MUTATIONS applied to the restatement itself, on the shapes the GPU tests use, and none for
    the float32 evaluation of the unmutated draw.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import noise_ref  # noqa: E402

# worst |z_fp32 - z_f64| per class, measured by test_fp32_error_is_the_recorded_one
NOISE_ERR_A_FP32 = 2.25e-06
NOISE_ERR_B_FP32 = 1.14e-03
NOISE_BOUND_A = 4 * NOISE_ERR_A_FP32
NOISE_BOUND_B = 4 * NOISE_ERR_B_FP32

# ---- the cases of tests/test_noise_gpu.py (the mutation table runs on the same shapes) -------------
SEED, IT = 0x1234_5678_9ABC, 7                 # both key words non-zero
ROW0S = (1000, 2 ** 32 - 20)                   # the second: the batch crosses the 32-bit row boundary
NOS = (0.5, 1.7)
PLAIN_N = (2, 4, 16, 32, 64, 128, 256, 1024, 2048)
PLAIN_QAM = ((8, 8), (4, 4), (32, 8), (64, 4), (1024, 4), (1024, 8))                   # (n, m)
NR_QPSK = ((12, 20), (19, 100), (100, 180), (300, 1088), (12, 600), (20, 90))          # (k, E); 90 % 4 = 2
NR_QAM = ((12, 20, 4), (20, 90, 6), (100, 184, 8), (30, 1088, 4), (12, 600, 6))        # (k, E, m)
SIM = ((32, 64), (128, 256), (512, 1024))                                              # (k, n)
SIM_BS = 100


def batch(size):
    """Rows of a case whose rows hold `size` positions: 301 or 37, no multiple of any rows-per-wave count."""
    return 301 if size < 1024 else 37


def rows_of(row0, bs):
    return row0 + np.arange(bs, dtype=np.int64)


def violates(err):
    return err[0] > NOISE_BOUND_A or err[1] > NOISE_BOUND_B


# ---- the sampler ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample():
    """2^22 Philox blocks of a fixed key."""
    return noise_ref.stream_blocks(0x0BAD_5EED_0000_0001, 3, np.arange(2 ** 11), np.arange(2 ** 11)).reshape(-1, 4)


def test_gauss4_is_a_standard_normal(sample):
    z = noise_ref.gauss4(sample)
    cnt = z.size
    assert z.shape == (2 ** 22, 4) and np.isfinite(z).all()
    mean, var, m4 = z.mean(), (z ** 2).mean(), (z ** 4).mean()
    iq = (z[:, 0::2] * z[:, 1::2]).mean()
    print(f"values {cnt}: mean {mean:.3e} var-1 {var - 1:.3e} m4-3 {m4 - 3:.3e} I/Q {iq:.3e}")
    assert abs(mean) < 5 / math.sqrt(cnt)
    assert abs(var - 1) < 5 * math.sqrt(2 / cnt)               # Var z^2 = 2
    assert abs(m4 - 3) < 5 * math.sqrt(96 / cnt)               # Var z^4 = 105 - 9
    assert abs(iq) < 5 / math.sqrt(cnt / 2)                    # Var (z_I z_Q) = 1, cnt / 2 pairs
    for c in range(4):                                         # each component on its own
        assert abs(z[:, c].mean()) < 5 / math.sqrt(cnt / 4)
        assert abs((z[:, c] ** 2).mean() - 1) < 5 * math.sqrt(2 / (cnt / 4))


EDGE_V = (0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1)
EDGE_W = (0, 511, 512, 2 ** 31, 2 ** 32 - 1)


def edge_blocks():
    """Every (v, w) of EDGE_V x EDGE_W as pair 0, with the pairs of the list in reverse as pair 1."""
    vw = [(v, w) for v in EDGE_V for w in EDGE_W]
    return np.array([[a[0], a[1], b[0], b[1]] for a, b in zip(vw, vw[::-1])], dtype=np.uint32)


def test_edge_words_by_hand():
    blk = edge_blocks()
    z, unit = noise_ref.gauss4(blk, with_unit=True)
    assert np.isfinite(z).all() and (unit >= 0).all()
    # v' = float32(v | 1): 2^24 + 1 rounds to 2^24 (a tie, to the even mantissa); 2^32 - 129 to 2^32 - 256,
    # the largest float32 below 2^32; from 2^32 - 128 on (| 1: 2^32 - 127, above the midpoint) to 2^32
    hand_unit = {0: 32.0, 1: 32.0, 2 ** 24: 8.0, 2 ** 24 + 1: 8.0, 2 ** 32 - 129: -math.log2(1 - 2.0 ** -24),
                 2 ** 32 - 128: 0.0, 2 ** 32 - 1: 0.0}
    hand_t = {0: 0.0, 511: 0.0, 512: 2.0 ** -23, 2 ** 31: 0.5, 2 ** 32 - 1: 1 - 2.0 ** -23}
    for row, zz, uu in zip(blk.tolist(), z, unit):
        for p in range(2):
            v, w = row[2 * p], row[2 * p + 1]
            r = math.sqrt(2 * math.log(2) * hand_unit[v])
            want = (r * math.cos(2 * math.pi * hand_t[w]), r * math.sin(2 * math.pi * hand_t[w]))
            assert uu[2 * p] == uu[2 * p + 1] == pytest.approx(hand_unit[v], rel=1e-12, abs=0), (v, w)
            assert zz[2 * p] == pytest.approx(want[0], rel=1e-12, abs=1e-15), (v, w)
            assert zz[2 * p + 1] == pytest.approx(want[1], rel=1e-12, abs=1e-15), (v, w)
    r0 = noise_ref.gauss4(np.array([0, 0, 2 ** 32 - 128, 12345], dtype=np.uint32))
    assert r0[0] == pytest.approx(math.sqrt(2 * math.log(2) * 32), rel=1e-14) and 6.66 < r0[0] < 6.67   # the tail's end
    assert r0[1] == 0.0 and r0[2] == 0.0 and r0[3] == 0.0                                               # R = 0


# ---- the streams never meet ------------------------------------------------------------------------------

def info_word3(k):
    """Information bits of the plain / QAM / NR producers (channel_kernel.hip's head comment): bit r of
    a row is bit r % 32 of stream word r // 32 = component (r // 32) % 4 of block r // 128, domain 0."""
    return np.arange((k + 127) // 128, dtype=np.int64)


def sim_info_word3(n):
    """Information bits of the producer inside the SC kernel (sc_static.h OUT_SIM): residue r < G = n / 64
    reads the block with word 3 = 0x40000000 | r >> 1."""
    return noise_ref.SIM_INFO | (np.arange(n // 64, dtype=np.int64) >> 1)


def _injective(layout, blocks, size):
    """The layout sends the positions of a row to distinct (block, component) pairs."""
    ids = np.arange(blocks * 4, dtype=np.int64).reshape(1, blocks, 4)
    got = layout(ids, size).reshape(-1)
    return len(np.unique(got)) == got.size


def test_streams_never_meet():
    info, noise, sim_info, sim_nz = set(), set(), set(), set()

    def add(into, w3, what):
        assert len(np.unique(w3)) == len(w3), what       # within a stream no (row, word 3) repeats
        into.update(int(v) for v in w3)

    for n in range(2, 2049):
        add(info, info_word3(n), ("info", n))            # k <= n
        w3 = noise_ref.plain_word3(n)
        add(noise, w3, ("plain", n))
        assert _injective(noise_ref.plain_layout, len(w3), n), n
        for m in (4, 8):
            if n % m == 0:
                w3 = noise_ref.qam_word3(n // m)
                add(noise, w3, ("qam", n, m))
                assert _injective(noise_ref.qam_layout, len(w3), n // m), (n, m)
    for e in range(2, 1089):
        w3 = noise_ref.plain_word3(e)                    # nr_noise
        add(noise, w3, ("nr", e))
        assert len(w3) * 4 >= e
        for m in (4, 6, 8):
            if e % m == 0:
                add(noise, noise_ref.qam_word3(e // m), ("nr qam", e, m))
                assert _injective(noise_ref.qam_layout, (e // m + 1) // 2, e // m), (e, m)
    for n in (64, 128, 256, 512, 1024):
        add(sim_info, np.unique(sim_info_word3(n)), ("sim info", n))   # two residues share a block's halves
        w3 = noise_ref.sim_word3(n)
        add(sim_nz, w3, ("sim noise", n))
        assert _injective(noise_ref.sim_layout, len(w3), n), n
    streams = {"info": info, "noise": noise, "sim info": sim_info, "sim noise": sim_nz}
    names = sorted(streams)
    for i, a in enumerate(names):
        assert streams[a] and all(0 <= v < 2 ** 32 for v in streams[a]), a
        for b in names[i + 1:]:
            assert not (streams[a] & streams[b]), (a, b)
    # the two bits that tell them apart
    assert {v >> 30 for v in info} == {0} and {v >> 30 for v in sim_info} == {1}
    assert {v >> 30 for v in noise} == {2} and {v >> 30 for v in sim_nz} == {3}


def test_noise_shapes_and_rows_past_2_32():
    rows = rows_of(ROW0S[1], 37)
    assert rows[-1] >= 2 ** 32
    z = noise_ref.plain_noise(SEED, IT, rows, 16)
    assert z.shape == (37, 16)
    # a row's draw depends on the row alone, and on all 64 bits of it
    assert np.array_equal(z[25:], noise_ref.plain_noise(SEED, IT, rows[25:], 16))
    assert not np.array_equal(z[25], noise_ref.plain_noise(SEED, IT, rows[25:26] - 2 ** 32, 16)[0])
    q = noise_ref.qam_noise(SEED, IT, rows, 5)
    assert q.shape == (37, 5, 2)
    # QAM with two bits per symbol is the plain layout: symbol s = positions 2s (re), 2s + 1 (im)
    assert np.array_equal(noise_ref.qam_noise(SEED, IT, rows, 8).reshape(37, 16), z)
    assert np.array_equal(noise_ref.nr_noise(SEED, IT, rows, 18), noise_ref.plain_noise(SEED, IT, rows, 20)[:, :18])
    s = noise_ref.sim_noise(SEED, IT, rows, 128)
    assert s.shape == (37, 128) and len(np.unique(s)) == s.size
    z2, unit = noise_ref.plain_noise(SEED, IT, rows, 2, with_unit=True)
    assert z2.shape == unit.shape == (37, 2) and np.array_equal(unit[:, 0], unit[:, 1])   # CH = 2: one pair
    # logits_from and its inverse; the sign: positive noise on a component lowers the logit
    cw = (np.arange(37 * 16).reshape(37, 16) % 3 == 0).astype(np.float64)
    llr = noise_ref.logits_from(z, cw.astype(np.float32), 1.7)
    assert np.allclose(noise_ref.noise_of_logits(llr, cw, 1.7), z, rtol=0, atol=1e-12)
    assert np.allclose(llr, (2 * cw - 1) * 2 / 1.7 - 2 / math.sqrt(1.7) * z, rtol=0, atol=1e-12)
    y = (1 - 2 * cw) / math.sqrt(2) + math.sqrt(1.7 / 2) * z          # the received component
    assert np.allclose(llr, -2 * math.sqrt(2) * y / 1.7, rtol=0, atol=1e-12)


# ---- the bounds: the formula op by op in float32 -----------------------------------------------------------

def gauss4_variant(blk, dtype=np.float64, or1=True, shift=9, c=noise_ref.SQRT_2LN2):
    """gauss4's formula evaluated op by op in `dtype`, with the faults of the mutation table as options:
    or1=False drops the | 1, shift=8 takes w >> 8, c replaces sqrt(2 ln 2)."""
    f = dtype
    blk = np.asarray(blk, dtype=np.uint32)
    v = blk[..., 0::2] | np.uint32(1) if or1 else blk[..., 0::2]
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = f(32) - np.log2(v.astype(np.float32).astype(f))
        r = f(c) * np.sqrt(unit)
        t = ((blk[..., 1::2] >> np.uint32(shift)).astype(f) / f(2 ** 23))
        ang = f(2 * np.pi) * t
        cs, sn = np.cos(ang), np.sin(ang)
        z = np.stack([r[..., 0] * cs[..., 0], r[..., 0] * sn[..., 0], r[..., 1] * cs[..., 1], r[..., 1] * sn[..., 1]],
                     axis=-1)
    assert z.dtype == f
    return z


def test_fp32_error_is_the_recorded_one(sample):
    """The measurement the kernel bounds are 4x of; the recorded constants must not be below it."""
    blk = np.concatenate([sample, edge_blocks()])
    want, unit = noise_ref.gauss4(blk, with_unit=True)
    assert np.allclose(gauss4_variant(blk), want, rtol=0, atol=1e-10)   # the variant at float64 is gauss4
    got = gauss4_variant(blk, np.float32)
    a, b = noise_ref.compare(got, want, unit)
    share_b = float((unit < noise_ref.CLASS_SPLIT).mean())
    print(f"fp32 op by op: class A {a:.3e} (recorded {NOISE_ERR_A_FP32:.3e}), class B {b:.3e} "
          f"(recorded {NOISE_ERR_B_FP32:.3e}), class B share {share_b:.4f}")
    assert 0.04 < share_b < 0.045                                # 1 - 2^(-1/16) = 0.0424
    assert 0.5 * NOISE_ERR_A_FP32 <= a <= NOISE_ERR_A_FP32
    assert 0.5 * NOISE_ERR_B_FP32 <= b <= NOISE_ERR_B_FP32
    assert NOISE_BOUND_A == 4 * NOISE_ERR_A_FP32 and NOISE_BOUND_B == 4 * NOISE_ERR_B_FP32


def test_compare_classes():
    want = np.array([1.0, 2.0, 3.0, 4.0])
    unit = np.array([1.0, 1 / 16, 1 / 32, 0.0])
    assert noise_ref.compare(want, want, unit) == (0.0, 0.0)
    assert noise_ref.compare(want + np.array([0.25, -0.5, 0.0, 0.0]), want, unit) == (0.5, 0.0)
    assert noise_ref.compare(want + np.array([0.0, 0.0, 0.125, -2.0]), want, unit) == (0.0, 2.0)
    assert noise_ref.compare(np.array([np.nan, 2.0, 3.0, 4.0]), want, unit) == (np.inf, 0.0)
    assert noise_ref.compare(np.array([1.0, 2.0, 3.0, np.inf]), want, unit) == (0.0, np.inf)
    assert noise_ref.compare(want[:2], want[:2], unit[:2]) == (0.0, 0.0)      # an empty class


# ---- the mutation table ---------------------------------------------------------------------------------------

FAMILIES = {   # word 3 of a row's blocks, the gather
    "plain": (noise_ref.plain_word3, noise_ref.plain_layout),
    "qam": (noise_ref.qam_word3, noise_ref.qam_layout),
    "sim": (noise_ref.sim_word3, noise_ref.sim_layout),
}
# (family, size, rows) of every GPU case: plain n, QAM symbols, NR E (the plain layout), NR QAM symbols, sim n
SHAPES = sorted({("plain", n, batch(n)) for n in PLAIN_N} | {("qam", n // m, batch(n)) for n, m in PLAIN_QAM} |
                {("plain", e, batch(e)) for _, e in NR_QPSK} | {("qam", e // m, batch(e)) for _, e, m in NR_QAM} |
                {("sim", n, SIM_BS) for _, n in SIM})


def draw(family, size, row0, bs, rows_fn=None, word3_fn=None, blk_fn=None, gauss=None, z_fn=None, poke_zero=False):
    """The restatement's draw of a case with faults put in: rows_fn(rows, row0), word3_fn(word3),
    blk_fn(blocks [rows, blocks, 4]), gauss(blocks) -> z in place of gauss4, z_fn(z [rows, ...]).
    poke_zero: v = 0 in the first pair of row 3's first block (an input on which | 1 matters).
    Returns (z, r_unit of the unmutated draw)."""
    word3_of, layout = FAMILIES[family]
    rows = rows_of(row0, bs)
    blk = noise_ref.stream_blocks(SEED, IT, rows_fn(rows, row0) if rows_fn else rows,
                                  word3_fn(word3_of(size)) if word3_fn else word3_of(size))
    if poke_zero:
        blk[3, 0, 0] = 0
    if blk_fn:
        blk = blk_fn(blk)
    z = layout(gauss(blk) if gauss else noise_ref.gauss4(blk), size)
    return z_fn(z) if z_fn else z


def _ragged(z):
    z = z.copy()
    z[-1] = z[-2]
    return z


# name -> (draw()'s arguments, the row0s at which the fault must show)
MUTATIONS = {
    "block index + 1": (dict(word3_fn=lambda w: w + 1), ROW0S),
    "row + 1 for odd rows": (dict(rows_fn=lambda r, r0: r + (r & 1)), ROW0S),
    "row >> 32 forced to 0": (dict(rows_fn=lambda r, r0: r & 0xFFFFFFFF), ROW0S[1:]),   # rows >= 2^32 only
    "row0 ignored": (dict(rows_fn=lambda r, r0: r - r0), ROW0S),
    "cos <-> sin": (dict(gauss=lambda b: noise_ref.gauss4(b)[..., [1, 0, 3, 2]]), ROW0S),
    "pair 0 <-> pair 1": (dict(blk_fn=lambda b: b[..., [2, 3, 0, 1]]), ROW0S),
    "| 1 dropped": (dict(gauss=lambda b: gauss4_variant(b, or1=False), poke_zero=True), ROW0S),
    ">> 8 in place of >> 9": (dict(gauss=lambda b: gauss4_variant(b, shift=8)), ROW0S),
    "domain bit cleared": (dict(word3_fn=lambda w: w & 0x7FFFFFFF), ROW0S),
    "sqrt(2 ln 2) replaced by 1.1773": (dict(gauss=lambda b: gauss4_variant(b, c=1.1773)), ROW0S),
    "last ragged row given its neighbour's block": (dict(z_fn=_ragged), ROW0S),
}


@pytest.fixture(scope="module")
def references():
    """(z, r_unit) of every (shape, row0), and of the draws with v = 0 poked in, computed once."""
    out = {}
    for family, size, bs in SHAPES:
        word3_of, layout = FAMILIES[family]
        for row0 in ROW0S:
            for poke in (False, True):
                blk = noise_ref.stream_blocks(SEED, IT, rows_of(row0, bs), word3_of(size))
                if poke:
                    blk[3, 0, 0] = 0
                z, unit = noise_ref.gauss4(blk, with_unit=True)
                out[family, size, bs, row0, poke] = (layout(z, size), layout(unit, size), blk)
    return out


def test_unmutated_pairs_are_clean(references):
    worst = [0.0, 0.0]
    for (family, size, bs, row0, poke), (z, unit, blk) in references.items():
        assert np.array_equal(draw(family, size, row0, bs, poke_zero=poke), z)
        assert noise_ref.compare(z, z, unit) == (0.0, 0.0)
        # the float32 evaluation of the same draw: what a correct kernel looks like
        got = FAMILIES[family][1](gauss4_variant(blk, np.float32), size)
        err = noise_ref.compare(got, z, unit)
        assert not violates(err), (family, size, row0, err)
        worst = [max(worst[0], err[0]), max(worst[1], err[1])]
    print(f"fp32 evaluation of the GPU cases' draws: class A {worst[0]:.3e}, class B {worst[1]:.3e}")
    # the restatement's named entry points are these draws
    z = references["plain", 16, 301, ROW0S[1], False][0]
    assert np.array_equal(noise_ref.plain_noise(SEED, IT, rows_of(ROW0S[1], 301), 16), z)
    z = references["qam", 5, 301, ROW0S[0], False][0]
    assert np.array_equal(noise_ref.qam_noise(SEED, IT, rows_of(ROW0S[0], 301), 5), z)
    z = references["sim", 256, SIM_BS, ROW0S[1], False][0]
    assert np.array_equal(noise_ref.sim_noise(SEED, IT, rows_of(ROW0S[1], SIM_BS), 256), z)


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_caught(references, name):
    kw, row0s = MUTATIONS[name]
    poke = bool(kw.get("poke_zero"))
    least = None
    for family, size, bs in SHAPES:
        for row0 in row0s:
            want, unit, _ = references[family, size, bs, row0, poke]
            err = noise_ref.compare(draw(family, size, row0, bs, **kw), want, unit)
            assert violates(err), (name, family, size, row0, err)
            least = err if least is None else (min(least[0], err[0]), min(least[1], err[1]))
    print(f"{name}: smallest worst error over the cases, class A {least[0]:.3e}, class B {least[1]:.3e}")
