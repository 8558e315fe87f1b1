"""CRC-aided SC-Flip decoding in plain numpy: the rule pl_scf_decode is pinned to.

TEST INFRASTRUCTURE ONLY.  The contract is that of include/polar_mi355x.h (pl_scf_decode):

    attempt 0   u^0 = leaf-by-leaf SC of a = -logits (f min-sum or exact, g = (1 - 2 u) x + y, HD(x) = !(x > 0),
                frozen leaves 0).  alpha_i = the leaf LLR position i was decided on.
    candidates  the information positions in ascending (|alpha_i|, i) order (fp32 magnitudes, +0 == -0),
                the first T' = min(max_flips, k) of them.
    attempt t   the same SC with the decision at c_t inverted; the first t whose k bits pass the CRC wins.

sc_flip() is the SC decoder, vectorised over rows, each row with its own flip position (-1: none).  A
node of nothing but frozen leaves decides 0 and its LLRs are not looked at; every other LLR is computed
leaf by leaf, with no repetition or parity-check shortcut.  Min-sum f and g are genie_ref's, the exact f
is exactf_cr.f_cr, whose fragile flag (an f so near a rounding midpoint that a correct device form may
round the other way) is kept per row: a fragile row may differ on the device.  The CRC is the MSB-first
shift register of the list decoders (fb = msb ^ bit; reg <<= 1; if fb: reg ^= g).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genie_ref  # noqa: E402

F32 = np.float32

# 5G CRC polynomials (3GPP TS 38.212 5.1), exponents: the names polar_amd.mysn.crc_params takes
CRC_POLYS = {"CRC24C": [24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0], "CRC16": [16, 12, 5, 0],
             "CRC11": [11, 10, 9, 5, 0], "CRC6": [6, 5, 0],
             # no 5G polynomials: x^3 + x + 1, x^2 + x + 1 and the parity check x + 1, for codes of fewer than 6
             # information bits
             "CRC3": [3, 1, 0], "CRC2": [2, 1, 0], "CRC1": [1, 0]}


def crc_params(name):
    """(degree, generator mask without x^degree)."""
    ex = CRC_POLYS[name]
    return ex[0], sum(1 << e for e in ex if e < ex[0])


def crc_register(bits, deg, g):
    """The register [rows] (Python ints in a uint64 array) after shifting in bits [rows, m], MSB first."""
    bits = (np.asarray(bits) != 0).astype(np.uint64)
    reg = np.zeros(bits.shape[0], dtype=np.uint64)
    mask = np.uint64((1 << deg) - 1)
    for m in range(bits.shape[1]):
        fb = ((reg >> np.uint64(deg - 1)) & np.uint64(1)) ^ bits[:, m]
        reg = ((reg << np.uint64(1)) & mask) ^ (fb * np.uint64(g))
    return reg


def crc_attach(msg, deg, g):
    """[rows, m] 0/1 -> [rows, m + deg]: the message and its parity (the register, MSB first)."""
    msg = (np.asarray(msg) != 0).astype(np.uint8)
    reg = crc_register(msg, deg, g)
    par = np.stack([((reg >> np.uint64(deg - 1 - j)) & np.uint64(1)).astype(np.uint8) for j in range(deg)], axis=1)
    return np.concatenate([msg, par], axis=1)


def crc_ok(bits, deg, g):
    """bool [rows]: the k bits leave the register at zero (pl_crc_status)."""
    return crc_register(bits, deg, g) == 0


def sc_flip(llr_logits, frozen_pos, n, flip, llr_max=30.0, exact=False, false_r0=None, bl0=None):
    """Leaf-by-leaf SC of logits [rows, n] with the decision at flip[row] (-1: none) inverted.
    Returns (u [rows, n] uint8, alpha [rows, n] fp32 -- NaN at leaves of all-frozen nodes, which SC never
    computes --, fragile [rows] bool).
    false_r0 / bl0 name one node (s, q), the stage-s node at position q << s, at which a deliberately WRONG
    decoder is modelled (tests/test_tree_zoo_ref.py only): false_r0 treats the node as all frozen although it
    is not; bl0 computes the node's g with the left child's partial sums taken as 0 although the left child was
    decoded."""
    x = np.ascontiguousarray(llr_logits, dtype=F32)
    rows = x.shape[0]
    assert x.shape[1] == n and n >= 2 and n & (n - 1) == 0
    frozen = np.zeros(n, dtype=bool)
    frozen[np.asarray(frozen_pos, dtype=np.int64)] = True
    flip = np.asarray(flip, dtype=np.int64).reshape(rows)
    u = np.zeros((rows, n), dtype=np.uint8)
    alpha = np.full((rows, n), np.nan, dtype=F32)
    fragile = np.zeros(rows, dtype=bool)
    if exact:
        from exactf_cr import f_cr

    def node(a, llr):
        m = llr.shape[1]
        here = (m.bit_length() - 1, a // m)
        if frozen[a:a + m].all() or here == false_r0:
            return np.zeros((rows, m), dtype=np.uint8)
        if m == 1:
            alpha[:, a] = llr[:, 0]
            d = genie_ref.hard(llr[:, 0]) ^ (flip == a).astype(np.uint8)
            u[:, a] = d
            return d[:, None]
        h = m // 2
        lo, hi = np.ascontiguousarray(llr[:, :h]), np.ascontiguousarray(llr[:, h:])
        if frozen[a:a + h].all():
            bl = np.zeros((rows, h), dtype=np.uint8)
        else:
            if exact:
                f, fr = f_cr(lo, hi, llr_max)
                fragile[:] |= fr.any(axis=1)
            else:
                f = genie_ref.f_minsum(lo, hi, llr_max)
            bl = node(a, f)
        br = node(a + h, genie_ref.g_op(lo, hi, np.zeros_like(bl) if here == bl0 else bl))
        return np.concatenate([bl ^ br, br], axis=1)

    with np.errstate(over="ignore", invalid="ignore"):
        node(0, F32(-1.0) * x)
    return u, alpha, fragile


def candidates(alpha, frozen_pos, n, t):
    """[rows, t] int64: the information positions in ascending (|alpha|, i) order, the first t."""
    info = np.setdiff1d(np.arange(n), np.asarray(frozen_pos, dtype=np.int64))
    mag = np.abs(alpha[:, info]).astype(F32)  # +0 and -0 both 0.0
    order = np.argsort(mag, axis=1, kind="stable")  # info ascending: stable = the lower index first
    return info[order[:, :t]]


def scf_decode(llr_logits, frozen_pos, n, crc, max_flips, llr_max=30.0, exact=False, flip_tree=None):
    """crc: (degree, mask).  Returns a dict: bits [rows, k] uint8, crc_ok [rows] bool, flip_pos and attempts
    [rows] int32, fragile [rows] bool, alpha [rows, n] fp32 (attempt 0), cand [rows, T'] (-1 rows that pass).
    flip_tree: sc_flip's false_r0 / bl0 switches, applied to the flip attempts alone (on the device attempt 0
    and the candidates come from other kernels than the flip decodes)."""
    x = np.ascontiguousarray(llr_logits, dtype=F32)
    rows = x.shape[0]
    deg, g = crc
    info = np.setdiff1d(np.arange(n), np.asarray(frozen_pos, dtype=np.int64))
    k = len(info)
    tp = min(int(max_flips), k)
    u0, alpha, fragile = sc_flip(x, frozen_pos, n, np.full(rows, -1), llr_max, exact)
    bits = u0[:, info].copy()
    ok = crc_ok(bits, deg, g)
    flip_pos = np.full(rows, -1, dtype=np.int32)
    attempts = np.where(ok, 1, 1 + tp).astype(np.int32)
    cand = np.full((rows, tp), -1, dtype=np.int64)
    fail = np.flatnonzero(~ok)
    if tp > 0 and len(fail):
        cand[fail] = c = candidates(alpha[fail], frozen_pos, n, tp)
        # every (failing row, attempt) pair as one batch
        ut, _, fr = sc_flip(np.repeat(x[fail], tp, axis=0), frozen_pos, n, c.reshape(-1), llr_max, exact,
                            **(flip_tree or {}))
        okt = crc_ok(ut[:, info], deg, g).reshape(len(fail), tp)
        fragile[fail] |= fr.reshape(len(fail), tp).any(axis=1)
        ut = ut[:, info].reshape(len(fail), tp, k)
        for j, row in enumerate(fail):
            hit = np.flatnonzero(okt[j])
            if len(hit):
                t = int(hit[0])
                bits[row] = ut[j, t]
                ok[row] = True
                flip_pos[row] = c[j, t]
                attempts[row] = 2 + t
    return {"bits": bits, "crc_ok": ok, "flip_pos": flip_pos, "attempts": attempts, "fragile": fragile,
            "alpha": alpha, "cand": cand}


# ---- the inputs tests/test_scf_gpu.py compares on (tests/test_scf_ref.py asserts they are valid) ----
def encode(u):
    """x = u G_n over GF(2), the butterfly of genie_ref.beta_states carried through all stages."""
    b = (np.asarray(u) != 0).astype(np.uint8).copy()
    n = b.shape[1]
    p = np.arange(n)
    h = 1
    while h < n:
        lo = p[(p & h) == 0]
        b[:, lo] ^= b[:, lo + h]
        h <<= 1
    return b


def rate_half_frozen(n, seed, k=None):
    """A seeded frozen set of n - k positions (k = n / 2 by default), ascending (bp_ref's)."""
    k = n // 2 if k is None else k
    rng = np.random.default_rng(seed)
    return np.sort(rng.permutation(n)[: n - k]).astype(np.int64)


def awgn_rows(seed, frozen_pos, n, crc, rows, ebno_db):
    """(info bits [rows, k] with a valid CRC, logits [rows, n] fp32) of seeded codewords over BPSK / AWGN."""
    deg, g = crc
    rng = np.random.default_rng(seed)
    info = np.setdiff1d(np.arange(n), np.asarray(frozen_pos, dtype=np.int64))
    k = len(info)
    msg = (rng.random((rows, k - deg)) < 0.5).astype(np.uint8)
    bits = crc_attach(msg, deg, g)
    u = np.zeros((rows, n), dtype=np.uint8)
    u[:, info] = bits
    xs = 1.0 - 2.0 * encode(u).astype(np.float64)
    sigma = np.sqrt(1.0 / (2.0 * k / n * 10.0 ** (ebno_db / 10.0)))
    y = xs + sigma * rng.standard_normal((rows, n))
    return bits, (-2.0 * y / sigma ** 2).astype(F32)


ROWS = 67  # a wave of the SC kernels ends in a partial set

# min-sum cases: (name, n, frozen set, CRC, max_flips, Eb/N0 dB).  Frozen sets: "half:<seed>" is
# rate_half_frozen(n, seed), "ref" the pinned reference set (k = n / 2; polar_amd.reference_frozen_pos),
# "none" k = n.  The Eb/N0 were chosen on the CPU (tests/test_scf_ref.py) so that every outcome class occurs.
MINSUM_CASES = [
    ("n8", 8, "none", "CRC6", 1, 4.0),
    ("n16", 16, "half:16", "CRC6", 5, 3.0),
    ("n32", 32, "ref", "CRC6", 16, 3.0),
    ("n64_full", 64, "none", "CRC11", 64, 6.0),
    ("n64", 64, "ref", "CRC11", 16, 3.0),
    ("n128", 128, "half:128", "CRC24C", 5, 6.0),
    ("n256", 256, "ref", "CRC24C", 16, 2.5),
    ("n512", 512, "ref", "CRC11", 1, 3.0),
    ("n1024", 1024, "ref", "CRC24C", 64, 3.5),
    ("n16_T_above_k", 16, "half:17", "CRC6", 40, 3.0),
]

# exact-f cases: (name, n, frozen, CRC, max_flips, Eb/N0, llr_max); llr_max 60 takes the full-range forms
EXACT_CASES = [
    ("x16_wide", 16, "half:16", "CRC6", 5, 3.0, 60.0),
    ("x64", 64, "ref", "CRC11", 16, 3.0, 30.0),
    ("x256", 256, "ref", "CRC24C", 16, 2.5, 30.0),
]
FRAGILE_CAP = 4  # fragile rows (left out of the device comparison) of an exact-f case, of ROWS


def frozen_of(spec, n):
    if spec == "none":
        return np.zeros(0, dtype=np.int64)
    if spec.startswith("half:"):
        return rate_half_frozen(n, int(spec[5:]))
    import polar_amd
    return np.sort(np.asarray(polar_amd.reference_frozen_pos(n // 2, n), dtype=np.int64))


def case_inputs(case):
    """(frozen_pos, (degree, mask), logits [ROWS, n]) of a MINSUM_CASES / EXACT_CASES entry: seeded AWGN rows,
    the last four replaced by genie_ref.special_llrs rows (zeros, -0, integer ties, a saturated row)."""
    name, n, spec, crc_name, _, ebno = case[:6]
    fp = frozen_of(spec, n)
    crc = crc_params(crc_name)
    seed = 4000 + 7 * n + len(name)
    _, x = awgn_rows(seed, fp, n, crc, ROWS, ebno)
    x[-4:] = genie_ref.special_llrs(np.random.default_rng(seed + 1), 4, n)
    return fp, crc, x


# ---- n = 2 and n = 4: every frozen pattern, every row of a small integer grid --------------------------
# pl_plan_set_crc takes no CRC of a degree above k, so none of the pinned ones (CRC6 is the smallest) at
# n <= 4: tests/test_scf_gpu.py checks that refusal and runs these lengths on the two small polynomials.
TINY_GRID = {2: (-3, -2, -1, 0, 1, 2, 3), 4: (-2, -1, 0, 1, 2)}


def tiny_cases(n):
    """[(name, frozen_pos, CRC name, max_flips = k)]: every frozen pattern of n = 2 / 4 with k >= 1, on CRC1,
    and on CRC3 as well where k >= 3."""
    out = []
    for pattern in range((1 << n) - 1):
        fp = np.array([i for i in range(n) if (pattern >> i) & 1], dtype=np.int64)
        k = n - len(fp)
        for crc_name in ("CRC1", "CRC3"):
            if k >= crc_params(crc_name)[0]:
                out.append((f"n{n}_frozen{pattern:0{n}b}_{crc_name}", fp, crc_name, k))
    return out


def tiny_rows(n):
    """Every row of TINY_GRID[n]^n, in lexicographic order: zeros and ties in (|alpha|, i) in most of them."""
    import itertools
    return np.array(list(itertools.product(TINY_GRID[n], repeat=n)), dtype=F32)


# ---- the in-kernel CRC remainder table: k up to kScfMaxK = 1024, k just above a power of two -----------
# (name, n, k, CRC, seed).  min-sum, max_flips = 4.  Position 0 is an information position (rank 0).
CRC_TABLE_CASES = [
    ("k1024_all_information", 1024, 1024, "CRC24C", 0),
    ("k1000", 1024, 1000, "CRC16", 1),
    ("k129", 1024, 129, "CRC11", 2),
    ("k65", 1024, 65, "CRC6", 3),
    ("k63_n64_no_doubling", 64, 63, "CRC11", 4),
]
CRC_TABLE_FLIPS = 4
CRC_TABLE_ROWS = 16


def crc_table_inputs(case):
    """(frozen_pos, (degree, mask), logits [16, n], sent bits [8, k]).  The frozen set is seeded and leaves
    position 0 free.  Rows 0 ... 7: a codeword with a valid CRC at +-8 whose channel position 0 is weakly wrong
    (-1/16 of its value): every f that sees it passes its sign and magnitude 1/2 on and every g outweighs it, so
    attempt 0 gets u_0 alone wrong, with the smallest |alpha|, and attempt 1 (a flip at position 0) must pass
    the CRC over all k bits -- about half of them 1, u_0 = 1 in rows 0 ... 3.  Rows 8 ... 15: noise alone."""
    name, n, k, crc_name, seed = case
    rng = np.random.default_rng([77, seed])
    fp = np.sort(1 + rng.permutation(n - 1)[: n - k]).astype(np.int64)
    deg, g = crc_params(crc_name)
    info = np.setdiff1d(np.arange(n), fp)
    half = CRC_TABLE_ROWS // 2
    msg = (rng.random((half, k - deg)) < 0.5).astype(np.uint8)
    msg[:, 0] = np.arange(half) < half // 2
    bits = crc_attach(msg, deg, g)
    u = np.zeros((half, n), dtype=np.uint8)
    u[:, info] = bits
    x = ((2.0 * encode(u) - 1.0) * 8.0).astype(F32)
    x[:, 0] = -x[:, 0] / F32(16.0)
    noise = (rng.standard_normal((CRC_TABLE_ROWS - half, n)) * 4).astype(F32)
    return fp, (deg, g), np.concatenate([x, noise]), bits
