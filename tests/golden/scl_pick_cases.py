"""Cases, input recipes and the rank census for the CRC-aided list pick (plain data and numpy).

The pick is the last step of both list kernels: u from the root's partial sums, the CRC register
over info_pos, the stable (metric, row) order of the 2L logical rows, +llr_max*k on failing rows,
the first argmin.  On AWGN rows around CRC-carrying codewords the winner is almost always the
best-metric path or no path, so these recipes spread it over the whole list instead:

  rank cases   pure-noise rows (standard_normal, no codeword) under CRC6: every list entry passes
               with probability near 1/64, about independently, so the first passing rank is
               spread over the list and most rows are all-fail;
  poly cases   every polynomial at one short and one long code: AWGN rows (sd 1) around
               CRC-carrying codewords on an amplitude ramp, so that rows won at rank 0 and all-fail
               rows both occur;
  tie cases    LLRs drawn from {-2 .. 2}, every second one zeroed, under CRC6: paths with exactly
               equal metrics that differ in CRC outcome or tie with the winner.

tests/test_scl_crc_pick_ref.py asserts on the CPU oracle alone that every case reaches what it is
for (the coverage conditions); tests/test_scl_crc_pick_gpu.py runs the same rows on both kernels.
The row counts and seeds below were chosen with the oracle alone, as the fewest rows (in steps of
100) at which the conditions hold.
"""
import os
from collections import namedtuple

import numpy as np

_FROZEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "polar-code-pytorch-sionna_amd",
                       "polar_amd", "data", "frozen_sets.npz")

# 5G polynomials (3GPP TS 38.212 5.1), exponents; the same table as oracle.CRC_POLYS (the CPU test
# compares the two)
CRC_POLYS = {"CRC24A": [24, 23, 18, 17, 14, 11, 10, 7, 6, 5, 4, 3, 1, 0], "CRC24B": [24, 23, 6, 5, 1, 0],
             "CRC24C": [24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0], "CRC16": [16, 12, 5, 0],
             "CRC11": [11, 10, 9, 5, 0], "CRC6": [6, 5, 0]}

LLR_MAX = 30.0  # the decoders' default clipping bound; the penalty is LLR_MAX * k

# kind: "rank" | "poly" | "tie".  frozen: "ref" (the pinned reference set for (k, n)), "bec" (the
# n - k largest Bhattacharyya parameters of the erasure channel at 0.5: any k) or an int seed (a
# random set of n - k positions).  rows: the batch.  amp: (lo, hi) amplitude ramp (poly cases).
Case = namedtuple("Case", "name kind n k L crc rows seed frozen amp")


def crc_params(name):
    """(degree, generator mask without the leading term)."""
    ex = CRC_POLYS[name]
    return ex[0], sum(1 << e for e in ex if e < ex[0])


def crc_parity(info, name):
    """[bs, m] 0/1 -> [bs, m + degree] uint8: the MSB-first shift register, parity appended."""
    deg, g = crc_params(name)
    info = np.asarray(info, dtype=np.uint8)
    reg = np.zeros(len(info), dtype=np.uint32)
    mask = np.uint32((1 << deg) - 1)
    for i in range(info.shape[1]):
        fb = ((reg >> np.uint32(deg - 1)) & np.uint32(1)) ^ info[:, i]
        reg = (reg << np.uint32(1)) & mask
        reg ^= np.where(fb != 0, np.uint32(g), np.uint32(0)).astype(np.uint32)
    par = ((reg[:, None] >> np.arange(deg - 1, -1, -1, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.uint8)
    return np.concatenate([info, par], axis=1)


def polar_encode(u, frozen_pos, n):
    """[bs, k] 0/1 at the information positions -> [bs, n] codeword bits (x = u F2^(x)m)."""
    info = np.setdiff1d(np.arange(n), frozen_pos)
    x = np.zeros((len(u), n), dtype=np.uint8)
    x[:, info] = u
    h = 1
    while h < n:
        v = x.reshape(len(u), n // (2 * h), 2, h)
        v[:, :, 0, :] ^= v[:, :, 1, :]
        h *= 2
    return x


def frozen_pos(case):
    """Sorted int64 frozen positions of a case."""
    if case.frozen == "ref":
        with np.load(_FROZEN) as d:
            return np.sort(d[f"k{case.k}_n{case.n}"].astype(np.int64))
    if case.frozen == "bec":
        z = np.array([0.5])
        while len(z) < case.n:
            z = np.stack([2 * z - z * z, z * z], axis=1).reshape(-1)
        return np.sort(np.argsort(-z, kind="stable")[: case.n - case.k]).astype(np.int64)
    rng = np.random.default_rng([case.frozen, case.n, case.k])
    return np.sort(rng.permutation(case.n)[: case.n - case.k]).astype(np.int64)


def llr_rows(case):
    """[rows, n] float32 logits of a case (seeded; the same array on every call)."""
    rng = np.random.default_rng([case.seed, case.n, case.k, case.L])
    if case.kind == "rank":
        return rng.standard_normal((case.rows, case.n)).astype(np.float32)
    if case.kind == "tie":
        x = rng.integers(-2, 3, size=(case.rows, case.n))
        return np.where(rng.random(x.shape) < 0.5, 0, x).astype(np.float32)
    deg = CRC_POLYS[case.crc][0]
    u = crc_parity(rng.integers(0, 2, (case.rows, case.k - deg)), case.crc)
    cw = polar_encode(u, frozen_pos(case), case.n).astype(np.float64)
    amp = np.linspace(case.amp[0], case.amp[1], case.rows)[:, None]
    return ((2.0 * cw - 1.0) * amp + rng.standard_normal(cw.shape)).astype(np.float32)


def winner_ranks(pm, llr_max, k):
    """The rank census of penalised sorted metrics pm [bs, 2L] (scl_decode_mysn's second output,
    the kernels' out_pm): (rank int64 [bs], all_fail bool [bs]).

    Row r passed its CRC iff pm[r] < llr_max * k.  Rows 2j and 2j+1 are state j (in metric order)
    and its copy, with equal metrics, so the winner's rank among the L paths is
    first_passing_row // 2.  (Where m paths tie exactly their 2m rows are the m states, then the m
    copies; the census keeps the same formula there, it is compared between decoders, not read as
    a path index.)  Where nothing passes the row is all-fail and rank 0 wins."""
    passed = np.asarray(pm) < float(llr_max) * k
    all_fail = ~passed.any(axis=1)
    rank = np.where(all_fail, 0, passed.argmax(axis=1) // 2).astype(np.int64)
    return rank, all_fail


def census(pm, llr_max, k):
    """(histogram of winning ranks over the rows with a passing path [L], number of all-fail rows)."""
    rank, all_fail = winner_ranks(pm, llr_max, k)
    return np.bincount(rank[~all_fail], minlength=np.shape(pm)[1] // 2), int(all_fail.sum())


def tie_rows(pm, llr_max, k):
    """bool [bs]: rows in which paths with exactly equal metrics differ in CRC outcome, or tie with
    the winner.  From pm alone.  The 2L logical rows are in stable (metric, row) order, so m paths
    with one metric fill 2m neighbouring rows: the m states in index order, then their copies in
    the same order.  Rows are compared after the penalty: key = pm where the row failed, else
    fl(pm + llr_max*k), the addition the decoder itself makes.  Equal metrics give equal keys; the
    converse can fail only for metrics closer than an ulp of the penalty (the CPU test checks
    against the oracle's metrics without a CRC that it does not on these rows).  A row counts if
    some run of more than two equal keys has both outcomes in it, or holds the winner's row (the
    first passing row; row 0 where nothing passes)."""
    pm = np.asarray(pm, dtype=np.float64)
    pen = float(llr_max) * k
    failed = pm >= pen
    key = np.where(failed, pm, pm + pen)
    win = np.where(failed.all(axis=1), 0, (~failed).argmax(axis=1))
    hit = np.zeros(len(pm), dtype=bool)
    for b in range(len(pm)):
        start = 0
        for r in range(1, pm.shape[1] + 1):
            if r == pm.shape[1] or key[b, r] != key[b, start]:
                if r - start > 2 and (failed[b, start:r].any() != failed[b, start:r].all() or start <= win[b] < r):
                    hit[b] = True
                start = r
    return hit


# (n, L) -> rows of a rank case: the fewest, in steps of 100, at which the oracle meets the coverage
# conditions of tests/test_scl_crc_pick_ref.py with fast-SCL off and on (and with the exact f at
# the shapes in EXACT_SHAPES).  n <= 64: every rank wins at least 3 times; above: a winner in
# every quarter of the list.
RANK_ROWS = {(32, 2): 300, (32, 4): 500, (32, 8): 300, (32, 16): 600, (32, 32): 700,
             (64, 2): 300, (64, 4): 400, (64, 8): 500, (64, 16): 600, (64, 32): 1000,
             (128, 2): 100, (128, 8): 200, (128, 32): 100, (256, 2): 100, (256, 8): 200, (256, 32): 100,
             (512, 2): 300, (512, 8): 100, (512, 32): 100, (1024, 2): 100, (1024, 8): 200, (1024, 32): 200,
             (2048, 2): 100, (2048, 8): 100, (2048, 16): 200}
RANK_CASES = [Case(f"rank_n{n}_L{L}", "rank", n, n // 2, L, "CRC6", rows, 1, "ref", None)
              for (n, L), rows in RANK_ROWS.items()]
# the rank cases that also run with the exact f (subtree against generic, census conditions)
EXACT_SHAPES = [(n, L) for n in (64, 1024) for L in (2, 8, 32)]

# Every polynomial at a short and a long code, list sizes spread over 2 .. 32.  CRC6 at (7, 32)
# and CRC24C at (25, 32) have k = degree + 1 (one payload bit); k = 100, 30, 37, 500 and 300 are
# no multiples of 32 at n >= 64.  The ramps: the lowest of (0.5, 1.3), (0.6, 1.6), ... at which the
# oracle has at least 5 rows won at rank 0 and at least 5 all-fail rows among 120.
POLY_ROWS = 120
POLY_CASES = [Case(f"poly_{crc}_{k}_{n}_L{L}", "poly", n, k, L, crc, POLY_ROWS, 2, fz, amp)
              for crc, n, k, L, fz, amp in [
                  ("CRC6", 32, 7, 2, "bec", (0.5, 1.3)), ("CRC6", 256, 100, 8, "bec", (0.5, 1.3)),
                  ("CRC11", 64, 24, 2, "bec", (0.5, 1.3)), ("CRC11", 1024, 512, 8, "ref", (0.6, 1.6)),
                  ("CRC16", 64, 30, 16, "bec", (0.5, 1.3)), ("CRC16", 512, 256, 4, "ref", (0.6, 1.6)),
                  ("CRC24A", 64, 40, 8, 5, (0.6, 1.6)), ("CRC24A", 1024, 500, 2, "bec", (0.5, 1.3)),
                  ("CRC24B", 128, 37, 32, "bec", (0.5, 1.3)), ("CRC24B", 512, 300, 16, "bec", (0.5, 1.3)),
                  ("CRC24C", 32, 25, 8, "bec", (0.5, 1.3)), ("CRC24C", 1024, 512, 32, "ref", (0.6, 1.6))]]

# Uniform draws from {-2 .. 2} gave 2 to 5 tie rows in 2000 at (128, 256); with every second entry
# zeroed (a zero leaf LLR ties the two children exactly) 3 % of the rows there are tie rows.
# (128, 256): the fewest rows, in steps of 100, with at least 20 tie rows; (32, 64) has them in
# most rows and takes 300 so that some are rows with a passing winner.
TIE_ROWS = {(64, 4): 300, (64, 8): 300, (64, 16): 300, (256, 4): 700, (256, 8): 700, (256, 16): 500}
TIE_CASES = [Case(f"tie_n{n}_L{L}", "tie", n, n // 2, L, "CRC6", rows, 3, "ref", None)
             for (n, L), rows in TIE_ROWS.items()]

CASES = RANK_CASES + POLY_CASES + TIE_CASES
BY_NAME = {c.name: c for c in CASES}

# llr_max off the default: the penalty is llr_max * k, dead paths start at llr_max
LLR_MAX_OFF = 7.5
LLR_MAX_OFF_CASES = ["rank_n64_L32", "rank_n512_L32"]


def coverage_gaps(case, pm, llr_max=LLR_MAX):
    """What the penalised metrics pm [rows, 2L] of a case fail to reach: a list of strings, empty
    when the coverage conditions hold.

      rank, n <= 64   every rank 0 .. L-1 wins at least 3 times;
      rank, n >= 128  a winner in every quarter of the list (every rank at L = 2);
      rank, both      all-fail rows, and rows won at rank 0;
      poly            at least 5 rows won at rank 0 and at least 5 all-fail rows;
      tie             at least 20 tie rows (tie_rows)."""
    hist, n_fail = census(pm, llr_max, case.k)
    gaps = []
    if case.kind == "rank":
        if n_fail == 0:
            gaps.append("no all-fail row")
        if hist[0] == 0:
            gaps.append("no row won at rank 0")
        if case.n <= 64:
            gaps += [f"rank {r} wins {hist[r]} times" for r in range(case.L) if hist[r] < 3]
        else:
            q = max(case.L // 4, 1)
            gaps += [f"no winner in ranks {a} .. {a + q - 1}" for a in range(0, case.L, q) if hist[a:a + q].sum() == 0]
    elif case.kind == "poly":
        if hist[0] < 5:
            gaps.append(f"{hist[0]} rows won at rank 0")
        if n_fail < 5:
            gaps.append(f"{n_fail} all-fail rows")
    else:
        t = int(tie_rows(pm, llr_max, case.k).sum())
        if t < 20:
            gaps.append(f"{t} tie rows")
    return gaps
