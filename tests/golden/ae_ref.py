"""Automorphism-ensemble SC decoding in plain numpy: the rule pl_ae_decode is pinned to.

TEST INFRASTRUCTURE ONLY.  The contract is that of include/polar_mi355x.h (pl_ae_decode), a = -logits:

    candidate t   a'[i] = a[pi_t(i)]; x' = the codeword leaf-by-leaf SC decides on for a' (scf_ref.sc_flip with
                  no flip, re-encoded); the candidate codeword is x_t[pi_t(i)] = x'[i].
    metric        m_t = sum_i |a_i| [x_t[i] != HD(a_i)], here in fp64 over the natural positions, so equal
                  codewords get equal metrics.
    winner        the smallest metric, the lowest t among equal ones; bits = (x_t G_n) at the information positions.

On exact_grid_llrs every f (min-sum, llr_max 30), every g and every metric sum is exact in fp32 in any order
(magnitudes below 2^15 at a 2^-3 step), so the device must match this file exactly there: bits, best_idx with
the lowest-index tie rule, and best_metric bit for bit.  On other inputs the device's fp32 metric sum may order
near-equal candidates differently; tests/test_ae_gpu.py states the bound.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genie_ref  # noqa: E402
import scf_ref  # noqa: E402

F32 = np.float32
ROWS = 37
FRAGILE_CAP = 4  # fragile rows (left out of the device comparison) of an exact-f case, of ROWS


def ae_decode(logits, frozen_pos, n, perms, llr_max=30.0, exact=False, tree=None):
    """perms [M, n]; tree: scf_ref.sc_flip's false_r0 / bl0 switches (a deliberately wrong SC, for
    tests/test_tree_zoo_ref.py).  Returns a dict: bits [M, rows, k] uint8 (every candidate's information bits), metric
    [M, rows] fp64, best_idx [rows] int32 (the first minimum of the fp64 metrics), fragile [rows] bool (exact f:
    some candidate's decode had an f too near a rounding midpoint to pin)."""
    x = np.ascontiguousarray(logits, dtype=F32)
    rows = x.shape[0]
    perms = np.asarray(perms, dtype=np.int64)
    m_tot = perms.shape[0]
    fp = np.asarray(frozen_pos, dtype=np.int64)
    info = np.setdiff1d(np.arange(n), fp)
    # all candidates as one batch of M * rows rows
    stacked = np.concatenate([x[:, pi] for pi in perms], axis=0)
    u, _, fr = scf_ref.sc_flip(stacked, fp, n, np.full(m_tot * rows, -1), llr_max, exact, **(tree or {}))
    xp = scf_ref.encode(u).reshape(m_tot, rows, n)
    a = (F32(-1.0) * x).astype(np.float64)
    hd = genie_ref.hard(a)
    bits = np.zeros((m_tot, rows, len(info)), dtype=np.uint8)
    metric = np.zeros((m_tot, rows), dtype=np.float64)
    for t, pi in enumerate(perms):
        xt = np.zeros((rows, n), dtype=np.uint8)
        xt[:, pi] = xp[t]
        metric[t] = (np.abs(a) * (xt != hd)).sum(axis=1)
        bits[t] = scf_ref.encode(xt)[:, info]
    return {"bits": bits, "metric": metric, "best_idx": np.argmin(metric, axis=0).astype(np.int32),
            "fragile": fr.reshape(m_tot, rows).any(axis=0)}


def winner(ref):
    """(bits [rows, k], metric fp64 [rows]) of the reference's own winner."""
    r = np.arange(ref["best_idx"].shape[0])
    return ref["bits"][ref["best_idx"], r], ref["metric"][ref["best_idx"], r]


# ---- codes and permutation tables ------------------------------------------------------------------
def frozen_of(spec, n):
    """'rm:r' RM(r, log2 n); 'pin:k' the pinned reference set (k, n); 'low:f' positions 0 ... f-1 frozen;
    'rand:seed' a seeded rate-1/2 set."""
    kind, arg = spec.split(":")
    if kind == "low":
        return np.arange(int(arg), dtype=np.int64)
    if kind == "rand":
        return scf_ref.rate_half_frozen(n, int(arg))
    import polar_amd
    if kind == "rm":
        return polar_amd.automorphism.rm_code(int(arg), n.bit_length() - 1)[1]
    assert kind == "pin"
    return np.sort(np.asarray(polar_amd.reference_frozen_pos(int(arg), n), dtype=np.int64))


@functools.lru_cache(maxsize=None)
def _table(spec, n, m_tot, kind):
    from polar_amd import automorphism
    fp = frozen_of(spec, n)
    if kind == "stage":
        return automorphism.stage_permutations(fp, n, m_tot, seed=n + m_tot)
    if kind == "linear":
        return automorphism.linear_permutations(fp, n, m_tot, seed=n + m_tot)
    if kind == "mixed":  # the identity, one bit-index permutation, one seeded random permutation (no automorphism)
        m = n.bit_length() - 1
        return np.stack([np.arange(n), automorphism.perm_table([1 << (m - 1 - b) for b in range(m)], n),
                         np.random.default_rng(n + 1).permutation(n)])[:m_tot]
    assert kind == "random_first"  # the deliberate non-automorphism: a seeded random permutation, then the identity
    return np.stack([np.random.default_rng(n).permutation(n), np.arange(n)])


def table_of(case):
    return _table(case[2], case[1], case[3], case[4]).copy()


# (name, n, frozen set, M, table kind[, Eb/N0 dB[, llr_max]])
# G = 1, 2, 4, 8 lanes per decode (n <= 128, 256, 512, 1024), C = 64 / G candidates a pass: M < C, M = C,
# M = C + 1 (n = 256: 33; n = 512: 17; n = 1024: 9) and eight full passes (n = 1024: 64)
GRID_CASES = [
    ("g2", 2, "low:1", 1, "stage"),
    ("g4", 4, "low:1", 2, "stage"),
    ("g8_all6", 8, "rm:1", 6, "stage"),
    ("g16_rm1_m8", 16, "rm:1", 8, "stage"),
    ("g32", 32, "rm:2", 8, "stage"),
    ("g64_rm2_m64", 64, "rm:2", 64, "stage"),
    ("g128_m3", 128, "rm:3", 3, "stage"),
    ("g128_m64", 128, "rm:3", 64, "stage"),
    ("g256_m33", 256, "rm:3", 33, "stage"),
    ("g256_pinned_m4", 256, "pin:64", 4, "stage"),
    ("g512_m17_linear", 512, "rm:4", 17, "linear"),
    ("g1024_m9", 1024, "rm:4", 9, "stage"),
    ("g1024_m64", 1024, "rm:4", 64, "stage"),
]
# more rows than the kernel's 4096-block grid: rows 4096 and up are the second stride of a work-group that has
# already used its LDS row and codeword buffers.  (case, rows)
PAST_GRID_CASE = (("g8_past_grid", 8, "low:3", 3, "mixed"), 4099 + 37)
NON_AUTOMORPHISM_CASE = ("g64_random", 64, "pin:32", 2, "random_first")
AWGN_CASES = [
    ("a32", 32, "rm:2", 8, "stage", 4.0),
    ("a128", 128, "rm:3", 64, "stage", 3.0),
    ("a256", 256, "rm:3", 33, "stage", 3.0),
    ("a1024", 1024, "rm:4", 9, "stage", 3.0),
]
EXACT_CASES = [
    ("x32", 32, "rm:2", 8, "stage", 4.0, 30.0),
    ("x128", 128, "rm:3", 8, "stage", 3.0, 30.0),
    ("x256", 256, "rm:3", 8, "stage", 3.0, 30.0),
    ("x32_wide", 32, "rm:2", 8, "stage", 4.0, 60.0),
]


def _seed(case):
    return 9000 + 13 * case[1] + 7 * case[3] + len(case[0])


def awgn_rows(seed, frozen_pos, n, rows, ebno_db):
    """(info bits [rows, k], logits [rows, n] fp32) of seeded codewords over BPSK / AWGN."""
    rng = np.random.default_rng(seed)
    info = np.setdiff1d(np.arange(n), np.asarray(frozen_pos, dtype=np.int64))
    k = len(info)
    bits = (rng.random((rows, k)) < 0.5).astype(np.uint8)
    u = np.zeros((rows, n), dtype=np.uint8)
    u[:, info] = bits
    xs = 1.0 - 2.0 * scf_ref.encode(u).astype(np.float64)
    sigma = np.sqrt(1.0 / (2.0 * k / n * 10.0 ** (ebno_db / 10.0)))
    y = xs + sigma * rng.standard_normal((rows, n))
    return bits, (-2.0 * y / sigma ** 2).astype(F32)


def exact_grid_llrs(seed, rows, n, frozen_pos=None):
    """Logits that are integers in [-128, 128] divided by 8: seeded codewords (of frozen_pos; none: k = n) at
    +-4 plus noise of deviation 3, rounded to the grid, so candidates often agree and tie; about 6 % of
    the entries are exact zeros and the last row is all zero (every candidate ties at metric 0)."""
    rng = np.random.default_rng(seed)
    fp = np.zeros(0, dtype=np.int64) if frozen_pos is None else np.asarray(frozen_pos, dtype=np.int64)
    info = np.setdiff1d(np.arange(n), fp)
    u = np.zeros((rows, n), dtype=np.uint8)
    u[:, info] = rng.random((rows, len(info))) < 0.5
    y = (2.0 * scf_ref.encode(u) - 1.0) * 4.0 + 3.0 * rng.standard_normal((rows, n))
    q = np.clip(np.rint(y * 8.0), -128, 128)
    q[rng.random((rows, n)) < 0.06] = 0.0
    q[-1] = 0.0
    return (q / 8.0).astype(F32)


def case_inputs(case, rows=ROWS):
    """(frozen_pos, perms [M, n], logits [rows, n]) of a case: grid logits for the cases without an Eb/N0,
    seeded AWGN rows for those with one."""
    fp = frozen_of(case[2], case[1])
    if len(case) > 5:
        _, x = awgn_rows(_seed(case), fp, case[1], rows, case[5])
    else:
        x = exact_grid_llrs(_seed(case), rows, case[1], fp)
    return fp, table_of(case), x
