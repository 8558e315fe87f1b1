"""The noise draws of the fused Monte-Carlo producers, restated in numpy float64 (test
infrastructure, like osd_ref.py).

Written from the stream conventions the kernel sources state in their comments, not from the
kernels' code:

  csrc/channel_kernel.hip  Philox4x32-10, key = seed, counter (row, row >> 32, iteration,
                           domain << 31 | block).  Domain 1 is the noise; block c of a row serves
                           positions 4c .. 4c+3 (QPSK), or the symbol pair (2c, 2c+1) (QAM: x, y =
                           re, im of symbol 2c; z, w = re, im of symbol 2c+1).
                           Box-Muller: radius sqrt(2 ln 2) sqrt(32 - log2 v'), v' = float(v | 1);
                           angle (w >> 9) / 2^23 revolutions; components (x, y) make pair 0
                           (cos, sin), (z, w) pair 1.
  csrc/sc_static.h OUT_SIM the same generator and Box-Muller; G = n / 64; the block with counter word
                           3 = 0xC0000000 | (16 r + t) serves slots 4t .. 4t+3 of residue r,
                           slot j of residue r being position r + G j.

polar_amd.channel.philox4x32_10 is the generator (tests/test_channel.py pins it to the Random123
known answers).  tests/test_noise_ref.py checks this file on the CPU and measures the bounds;
tests/test_noise_gpu.py holds the kernels to it.
"""
import numpy as np

from polar_amd.channel import philox4x32_10

NOISE_DOMAIN = 0x80000000     # bit 31 of counter word 3: the noise of the plain, QAM and NR producers
SIM_NOISE = 0xC0000000        # the noise of the producer inside the SC kernel (OUT_SIM)
SIM_INFO = 0x40000000         # its information bits
CLASS_SPLIT = 1.0 / 16        # compare(): class A where 32 - log2 v' >= CLASS_SPLIT, class B below
SQRT_2LN2 = float(np.sqrt(2.0 * np.log(2.0)))


def stream_blocks(seed, it, rows, word3):
    """Philox blocks uint32 [len(rows), len(word3), 4]: key = the 64-bit seed (low word, high word),
    counter (row low word, row high word, it, word3).  rows: int64, may exceed 2^32."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    word3 = np.asarray(word3, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((len(rows), len(word3), 4), dtype=np.uint64)
    ctr[..., 0] = (rows & 0xFFFFFFFF).astype(np.uint64)[:, None]
    ctr[..., 1] = ((rows >> 32) & 0xFFFFFFFF).astype(np.uint64)[:, None]
    ctr[..., 2] = np.uint64(int(it) & 0xFFFFFFFF)
    ctr[..., 3] = word3[None, :]
    key = np.zeros((len(rows), len(word3), 2), dtype=np.uint64)
    key[..., 0] = np.uint64(int(seed) & 0xFFFFFFFF)
    key[..., 1] = np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    return philox4x32_10(ctr, key)


def radius_unit(blk):
    """32 - log2 v' of the two pairs, float64 [..., 2]: v' = float64(float32(v | 1)), v = components
    x and z.  The float32 conversion of the integer is part of the definition of the uniform.
    Evaluated as -log2(1 + (v' - 2^32) / 2^32) through log1p: the same number, without the float64
    cancellation of 32 - log2 v' next to v' = 2^32 (v' - 2^32 is exact)."""
    v = np.asarray(blk, dtype=np.uint32)[..., 0::2] | np.uint32(1)
    vp = v.astype(np.float32).astype(np.float64)
    return np.log1p((vp - 2.0 ** 32) / 2.0 ** 32) / -np.log(2.0) + 0.0


def gauss4(blk, with_unit=False):
    """A Philox block uint32 [..., 4] -> four standard-normal values float64 [..., 4]:
    (R0 cos 2 pi t0, R0 sin 2 pi t0, R1 cos 2 pi t1, R1 sin 2 pi t1), R = sqrt(2 ln 2 (32 - log2 v')),
    t = (w >> 9) / 2^23, (v, w) = (x, y) for pair 0 and (z, w) for pair 1.
    with_unit: also 32 - log2 v' of each value's pair, [..., 4] (compare()'s r_unit)."""
    blk = np.asarray(blk, dtype=np.uint32)
    unit = radius_unit(blk)
    r = SQRT_2LN2 * np.sqrt(unit)
    ang = 2.0 * np.pi * ((blk[..., 1::2] >> np.uint32(9)).astype(np.float64) / 2.0 ** 23)
    z = np.stack([r[..., 0] * np.cos(ang[..., 0]), r[..., 0] * np.sin(ang[..., 0]),
                  r[..., 1] * np.cos(ang[..., 1]), r[..., 1] * np.sin(ang[..., 1])], axis=-1)
    if with_unit:
        return z, np.repeat(unit, 2, axis=-1)
    return z


# ---- which block and component serve a position: word 3 of the blocks, and the gather -------------

def plain_word3(n):
    """Counter word 3 of the blocks of a row of n positions: one block per CH = min(4, n)."""
    return NOISE_DOMAIN | np.arange((n + min(4, n) - 1) // min(4, n), dtype=np.int64)


def plain_layout(g, n):
    """[rows, blocks, 4] -> [rows, n]: position p = component p % CH of block p // CH."""
    ch = min(4, n)
    p = np.arange(n)
    return g[:, p // ch, p % ch]


def qam_word3(n_sym):
    return NOISE_DOMAIN | np.arange((n_sym + 1) // 2, dtype=np.int64)


def qam_layout(g, n_sym):
    """[rows, blocks, 4] -> [rows, n_sym, 2]: symbol s = block s // 2, components 2 (s % 2) (re), + 1 (im)."""
    s = np.arange(n_sym)
    return np.stack([g[:, s // 2, 2 * (s % 2)], g[:, s // 2, 2 * (s % 2) + 1]], axis=-1)


def sim_word3(n):
    return SIM_NOISE | np.arange((n // 64) * 16, dtype=np.int64)


def sim_layout(g, n):
    """[rows, 16 G, 4] -> [rows, n]: position r + G j = component j % 4 of block 16 r + j // 4."""
    G = n // 64
    p = np.arange(n)
    r, j = p % G, p // G
    return g[:, 16 * r + j // 4, j % 4]


def _noise(seed, it, rows, word3, layout, size, with_unit):
    z, unit = gauss4(stream_blocks(seed, it, rows, word3), with_unit=True)
    return (layout(z, size), layout(unit, size)) if with_unit else layout(z, size)


def plain_noise(seed, it, rows, n, with_unit=False):
    """z [rows, n] of pl_awgn_qpsk_llr / _bits (and, with_unit, 32 - log2 v' of each element)."""
    return _noise(seed, it, rows, plain_word3(n), plain_layout, n, with_unit)


def nr_noise(seed, it, rows, e, with_unit=False):
    """z [rows, E] of pl_nr_awgn_qpsk_llr: plain_noise over the E transmitted positions (the surplus
    components of the last block are unused where E is no multiple of 4)."""
    return plain_noise(seed, it, rows, e, with_unit)


def qam_noise(seed, it, rows, n_sym, with_unit=False):
    """z [rows, n_sym, 2] (re, im) of pl_awgn_qam_llr (n_sym = n / m) and pl_nr_awgn_qam_llr (E / m)."""
    return _noise(seed, it, rows, qam_word3(n_sym), qam_layout, n_sym, with_unit)


def sim_noise(seed, it, rows, n, with_unit=False):
    """z [rows, n] of pl_sc_sim_count (n a multiple of 64)."""
    assert n % 64 == 0
    return _noise(seed, it, rows, sim_word3(n), sim_layout, n, with_unit)


def logits_from(z, cw, no):
    """The QPSK logits in float64: the component carrying code bit c is y = (1 - 2c) / sqrt(2) +
    sqrt(no / 2) z, and the logit is -2 sqrt(2) y / no = (2c - 1)(2 / no) - (2 / sqrt(no)) z."""
    no = float(no)
    return (2.0 * np.asarray(cw, dtype=np.float64) - 1.0) * (2.0 / no) - (2.0 / np.sqrt(no)) * np.asarray(z)


def noise_of_logits(llr, cw, no):
    """logits_from solved for z (float64): the standardised noise a kernel's logits hold."""
    no = float(no)
    a = (2.0 * np.asarray(cw, dtype=np.float64) - 1.0) * (2.0 / no)
    return (np.asarray(llr, dtype=np.float64) - a) / (-2.0 / np.sqrt(no))


def compare(z_got, z_want, r_unit):
    """The acceptance measure of every noise comparison: (worst class A error, worst class B error),
    each max |z_got - z_want| over the elements of its class -- A where r_unit = 32 - log2 v' >=
    CLASS_SPLIT, B below (the float32 difference cancels there).  No element is left out; a value that
    is not finite counts as an infinite error; an empty class gives 0."""
    got, want = np.asarray(z_got, dtype=np.float64), np.asarray(z_want, dtype=np.float64)
    unit = np.broadcast_to(np.asarray(r_unit, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    err = np.where(np.isfinite(err), err, np.inf)
    a = unit >= CLASS_SPLIT
    return (float(err[a].max()) if a.any() else 0.0, float(err[~a].max()) if (~a).any() else 0.0)
