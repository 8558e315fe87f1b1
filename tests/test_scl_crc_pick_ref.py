"""The CRC-aided pick cases (tests/golden/scl_pick_cases.py) reach what they are for: CPU oracle alone.

tests/test_scl_crc_pick_gpu.py holds both list kernels to the oracle on these rows; it could pass
on rows that never reach the code (a winner deep in the list, an all-fail row, an exact tie), so
the coverage conditions are asserted here, on the oracle's own output, where there is no GPU:

  rank cases   CRC6 on pure-noise rows, n = 32 and 64 at every L in {2, 4, 8, 16, 32}: every rank
               wins at least 3 times; n = 128 .. 1024 at L in {2, 8, 32} and n = 2048 at L in
               {2, 8, 16}: a winner in every quarter of the list (every rank at L = 2); all of them:
               all-fail rows and rows won at rank 0.  With fast-SCL off and on, and with the exact
               f at the shapes the GPU test runs with it;
  poly cases   every polynomial of oracle.CRC_POLYS at a short and a long code, AWGN rows around
               CRC-carrying codewords: at least 5 rows won at rank 0 and at least 5 all-fail rows;
               one case with a single payload bit (k = degree + 1), one with k no multiple of 32 at
               n >= 64;
  tie cases    LLRs from {-2 .. 2} at (32, 64) and (128, 256), CRC6, L in {4, 8, 16}: at least 20
               rows in which paths with exactly equal metrics differ in CRC outcome or tie with
               the winner, read from pm alone.

The tie order.  oracle/polar_oracle.c (orc_scl_decode_mysn) sorts the 2L logical rows (row r < L =
state r, row r >= L its copy) by insertion with a strict `>` on the metric, so equal metrics keep
their row order: the stable (metric, row) order.  scl_kernel.hip runs the same insertion sort;
scl_tree_kernel.hip ranks row gl by counting the rows c with v < mv or (v == mv and c < gl), which
is that order again.  Both then take the first argmin (strict `<`) of the penalised values.  So
the tie cases hold for both kernels.
"""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import scl_pick_cases as C  # noqa: E402


def _modes(case):
    """(fast_scl, exact_f) the oracle runs a case with."""
    modes = [(False, False), (True, False)]
    if case.kind == "rank" and (case.n, case.L) in C.EXACT_SHAPES:
        modes += [(False, True), (True, True)]
    return modes


def test_recipes_agree_with_the_oracle():
    """The numpy CRC register and encoder of the case file are the oracle's."""
    assert C.CRC_POLYS == oracle.CRC_POLYS
    rng = np.random.default_rng(0)
    info = rng.integers(0, 2, (50, 41))
    for name in C.CRC_POLYS:
        assert C.crc_params(name) == oracle.crc_params(name)
        assert np.array_equal(C.crc_parity(info, name), oracle.crc_encode(info.astype(np.float32), name))
    for case in (C.BY_NAME["poly_CRC24B_37_128_L32"], C.BY_NAME["poly_CRC24A_40_64_L8"]):
        fp = C.frozen_pos(case)
        assert len(fp) == case.n - case.k and len(np.unique(fp)) == len(fp)
        u = rng.integers(0, 2, (20, case.k))
        assert np.array_equal(C.polar_encode(u, fp, case.n), oracle.polar_encode(u.astype(np.float32), fp, case.n))


def test_case_list_covers_what_it_must():
    rank = {(c.n, c.L) for c in C.RANK_CASES}
    assert rank == {(n, L) for n in (32, 64) for L in (2, 4, 8, 16, 32)} | \
        {(n, L) for n in (128, 256, 512, 1024) for L in (2, 8, 32)} | {(2048, L) for L in (2, 8, 16)}
    assert all(c.crc == "CRC6" and c.frozen == "ref" and 2 * c.k == c.n for c in C.RANK_CASES)
    for name in oracle.CRC_POLYS:
        ns = sorted(c.n for c in C.POLY_CASES if c.crc == name)
        assert len(ns) == 2 and ns[0] <= 128 and ns[1] >= 256, (name, ns)
    assert any(c.k == C.CRC_POLYS[c.crc][0] + 1 for c in C.POLY_CASES)
    assert any(c.k % 32 != 0 and c.n >= 64 for c in C.POLY_CASES)
    assert {(c.n, c.k, c.L) for c in C.TIE_CASES} == {(n, n // 2, L) for n in (64, 256) for L in (4, 8, 16)}
    assert set(C.EXACT_SHAPES) <= rank and all(C.BY_NAME[c].L == 32 for c in C.LLR_MAX_OFF_CASES)
    assert len(C.BY_NAME) == len(C.CASES)
    for c in C.CASES:
        x = C.llr_rows(c)
        assert x.shape == (c.rows, c.n) and x.dtype == np.float32


def test_recorded_census_lists_every_case():
    """tests/golden/scl_pick_census.txt (the oracle's census per case, recorded when the rows were chosen)
    names every case with its row count, and each recorded line is a whole census: L ranks that, with the
    all-fail rows, add up to the rows.  The figures themselves are printed by the test below, not compared."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scl_pick_census.txt")
    lines = [ln.split() for ln in open(path) if ln.strip() and not ln.startswith("#")]
    assert [ln[0] for ln in lines] == [c.name for c in C.CASES]
    for ln, c in zip(lines, C.CASES):
        rows, n_fail, hist = int(ln[1]), int(ln[2]), [int(v) for v in ln[4:]]
        assert rows == c.rows and len(hist) == c.L and sum(hist) + n_fail == rows, c.name


def test_winner_ranks_on_a_hand_made_row():
    pen = 30.0 * 4
    pm = np.array([[1.0, 1.0, 2.0, 2.0, 3.0, 3.0],                    # rank 0 passes
                   [1.0 + pen, 1.0 + pen, 2.0 + pen, 2.0 + pen, 3.0, 3.0],  # only the last path passes
                   [1.0 + pen, 1.0 + pen, 2.0 + pen, 2.0 + pen, 3.0 + pen, 3.0 + pen],  # nothing passes
                   [1.0 + pen, 1.0, 1.0 + pen, 1.0, 3.0, 3.0]])        # states 0 and 1 tie, state 1 passes
    rank, all_fail = C.winner_ranks(pm, 30.0, 4)
    assert rank.tolist() == [0, 2, 0, 0] and all_fail.tolist() == [False, False, True, False]
    hist, n_fail = C.census(pm, 30.0, 4)
    assert hist.tolist() == [2, 0, 1] and n_fail == 1
    assert C.tie_rows(pm, 30.0, 4).tolist() == [False, False, False, True]
    tied_winner = np.array([[1.0 + pen, 1.0 + pen, 2.0, 2.0, 2.0, 2.0], [1.0 + pen] * 4 + [2.0 + pen] * 2])
    assert C.tie_rows(tied_winner, 30.0, 4).tolist() == [True, True]


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_oracle_reaches_the_coverage_conditions(case):
    fp = C.frozen_pos(case)
    x = C.llr_rows(case)
    pen = C.LLR_MAX * case.k
    for fast, exact in _modes(case):
        bits, pm = oracle.scl_decode_mysn(x, fp, case.L, fast_scl=fast, exact_f=exact, crc=case.crc)
        hist, n_fail = C.census(pm, C.LLR_MAX, case.k)
        print(case.name, "fast" if fast else "plain", "exact" if exact else "minsum", "rows", case.rows, "hist",
              hist.tolist(), "all-fail", n_fail, "tie rows", int(C.tie_rows(pm, C.LLR_MAX, case.k).sum()))
        assert C.coverage_gaps(case, pm) == [], (fast, exact)
        # the census reads pass/fail off the penalty: the decoded word passes its CRC exactly where a
        # row is below it, and without a CRC the same rows carry the same metrics, all below it
        _, all_fail = C.winner_ranks(pm, C.LLR_MAX, case.k)
        assert np.array_equal(oracle.crc_check(bits, case.crc), ~all_fail)
        _, base = oracle.scl_decode_mysn(x, fp, case.L, fast_scl=fast, exact_f=exact)
        assert base.max() < pen
        failed = pm >= pen
        assert np.array_equal(pm, np.where(failed, base + pen, base))
        if case.kind == "tie":
            # equal keys of tie_rows are equal metrics on these rows, not two metrics within an ulp of the penalty
            key = np.where(failed, pm, pm + pen)
            assert np.array_equal(key[:, 1:] == key[:, :-1], base[:, 1:] == base[:, :-1])


@pytest.mark.parametrize("name", C.LLR_MAX_OFF_CASES)
def test_oracle_llr_max_off_the_default(name):
    """llr_max = 7.5: the penalty is 7.5 k, dead paths start at 7.5.  All-fail rows, winners below
    rank 0, and the same pass/fail reading of pm."""
    case = C.BY_NAME[name]
    fp, x = C.frozen_pos(case), C.llr_rows(case)
    for fast in (False, True):
        bits, pm = oracle.scl_decode_mysn(x, fp, case.L, fast_scl=fast, exact_f=False, crc=case.crc,
                                          llr_max=C.LLR_MAX_OFF)
        hist, n_fail = C.census(pm, C.LLR_MAX_OFF, case.k)
        print(name, "fast" if fast else "plain", "hist", hist.tolist(), "all-fail", n_fail, "tie rows",
              int(C.tie_rows(pm, C.LLR_MAX_OFF, case.k).sum()))
        assert C.coverage_gaps(case, pm, C.LLR_MAX_OFF) == []
        _, all_fail = C.winner_ranks(pm, C.LLR_MAX_OFF, case.k)
        assert np.array_equal(oracle.crc_check(bits, case.crc), ~all_fail)
        _, base = oracle.scl_decode_mysn(x, fp, case.L, fast_scl=fast, exact_f=False, llr_max=C.LLR_MAX_OFF)
        assert base.max() < C.LLR_MAX_OFF * case.k
