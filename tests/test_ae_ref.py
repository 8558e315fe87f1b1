"""The numpy restatement of automorphism-ensemble decoding (tests/golden/ae_ref.py), its case tables and
polar_amd.automorphism, on the CPU: the tables are permutations and automorphisms, the grid cases exercise the
lowest-index tie rule, the grid's fp32 sums are exact, rm_code is the reference recipe, and the permutation
search counts what a frozen set admits.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import ae_ref  # noqa: E402
import scf_ref  # noqa: E402

import polar_amd  # noqa: E402
from polar_amd import automorphism  # noqa: E402

ALL_CASES = ae_ref.GRID_CASES + ae_ref.AWGN_CASES + ae_ref.EXACT_CASES


@pytest.mark.parametrize("case", ALL_CASES + [ae_ref.NON_AUTOMORPHISM_CASE], ids=lambda c: c[0])
def test_case_tables_are_permutations_and_automorphisms(case):
    n, m_tot = case[1], case[3]
    fp = ae_ref.frozen_of(case[2], n)
    table = ae_ref.table_of(case)
    assert table.shape == (m_tot, n) and 1 <= m_tot <= 64
    assert len({bytes(row.tobytes()) for row in table}) == m_tot  # distinct
    for t, pi in enumerate(table):
        assert automorphism.is_permutation(pi, n), (case[0], t)
        want = not (case is ae_ref.NON_AUTOMORPHISM_CASE and t == 0)
        assert automorphism.is_automorphism(pi, fp, n) == want, (case[0], t)
    if case[4] != "random_first":
        assert np.array_equal(table[0], np.arange(n))  # identity first


def test_all_stage_permutations_of_the_small_cases():
    by_name = {c[0]: c for c in ae_ref.GRID_CASES}
    assert by_name["g8_all6"][3] == 6  # 3! bit-index permutations, all of them
    fp = ae_ref.frozen_of("pin:64", 256)
    assert len(automorphism.stage_permutations(fp, 256, 4)) == 4
    with pytest.raises(ValueError, match="only 4"):
        automorphism.stage_permutations(fp, 256, 5)


@pytest.mark.parametrize("case", [c for c in ae_ref.GRID_CASES if c[1] <= 256], ids=lambda c: c[0])
def test_grid_cases_tie_and_are_exact_in_fp32(case):
    """At least one row has its minimum attained by two or more candidates (M >= 2); the inputs are on the grid;
    and the fp32 metric sum of every candidate is the fp64 one whatever the order (forwards, backwards, permuted)."""
    fp, table, x = ae_ref.case_inputs(case)
    n = case[1]
    assert np.array_equal(x * 8, np.rint(x * 8)) and np.abs(x).max() <= 16 and not x[-1].any() and (x == 0).sum() > n
    ref = ae_ref.ae_decode(x, fp, n, table)
    best = ref["metric"].min(axis=0)
    ties = (ref["metric"] == best).sum(axis=0)
    print(case[0], "rows with a tied minimum:", int((ties >= 2).sum()), "winners:", np.bincount(ref["best_idx"]))
    if case[3] >= 2:
        assert (ties >= 2).any()
        assert (ties[:-1] >= 2).any() or n <= 4  # not only the all-zero row
    assert np.array_equal(ref["best_idx"], np.argmax(ref["metric"] == best, axis=0))  # the lowest index
    # exactness: fp32 partial sums in three orders
    a = np.abs(x).astype(np.float32)
    info = np.setdiff1d(np.arange(n), fp)
    hd = (~(-x > 0)).astype(np.uint8)
    rng = np.random.default_rng(1)
    for t in range(case[3]):
        u = np.zeros((len(x), n), dtype=np.uint8)
        u[:, info] = ref["bits"][t]
        terms = np.where(scf_ref.encode(u) != hd, a, np.float32(0))
        for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
            acc = np.zeros(len(x), dtype=np.float32)
            for i in order:
                acc = (acc + terms[:, i]).astype(np.float32)
            assert np.array_equal(acc.astype(np.float64), ref["metric"][t]), (case[0], t)


def test_past_grid_case_winners_spread_over_both_strides():
    """The 4136-row case: its table is valid, and rows past the grid's 4096 work-groups are won by every
    candidate, with ties among them."""
    case, rows = ae_ref.PAST_GRID_CASE
    fp, table, x = ae_ref.case_inputs(case, rows)
    n = case[1]
    assert rows == 4099 + 37 and table.shape == (3, n)
    assert all(automorphism.is_permutation(pi, n) for pi in table) and np.array_equal(table[0], np.arange(n))
    ref = ae_ref.ae_decode(x, fp, n, table)
    late = ref["best_idx"][4096:]
    ties = (ref["metric"] == ref["metric"].min(axis=0)).sum(axis=0)
    print("winners past the grid:", np.bincount(late, minlength=3), "tied rows there:", int((ties[4096:] >= 2).sum()))
    assert set(late) == {0, 1, 2} and (ties[4096:-1] >= 2).any()


def test_large_grid_cases_tie():
    for case in [c for c in ae_ref.GRID_CASES if c[1] > 256]:
        fp, table, x = ae_ref.case_inputs(case)
        ref = ae_ref.ae_decode(x, fp, case[1], table)
        ties = (ref["metric"] == ref["metric"].min(axis=0)).sum(axis=0)
        print(case[0], "rows with a tied minimum:", int((ties >= 2).sum()), "winners:", np.bincount(ref["best_idx"]))
        assert (ties[:-1] >= 2).any()
        assert ref["metric"].max() < 2 ** 15


def test_candidates_are_codewords_and_identity_is_sc():
    """Every candidate of an automorphism table is a codeword (its frozen positions re-encode to 0), candidate 0
    (the identity) is plain SC, and the winner's metric is the distance of the re-encoded winner."""
    case = next(c for c in ae_ref.AWGN_CASES if c[0] == "a128")
    fp, table, x = ae_ref.case_inputs(case)
    n = case[1]
    ref = ae_ref.ae_decode(x, fp, n, table)
    info = np.setdiff1d(np.arange(n), fp)
    u0, _, _ = scf_ref.sc_flip(x, fp, n, np.full(len(x), -1))
    assert np.array_equal(ref["bits"][0], u0[:, info])
    a = -x.astype(np.float64)
    for t in (0, 1, len(table) - 1):
        xt = np.zeros((len(x), n), dtype=np.uint8)
        xp = scf_ref.encode(scf_ref.sc_flip(x[:, table[t]], fp, n, np.full(len(x), -1))[0])
        xt[:, table[t]] = xp
        assert not scf_ref.encode(xt)[:, fp].any()
        assert np.array_equal(scf_ref.encode(xt)[:, info], ref["bits"][t])
        assert np.allclose(ref["metric"][t], (np.abs(a) * (xt != (~(a > 0)))).sum(axis=1), rtol=1e-12)
    sent, _ = ae_ref.awgn_rows(ae_ref._seed(case), fp, n, ae_ref.ROWS, case[5])
    bits, _ = ae_ref.winner(ref)
    err_sc = int((ref["bits"][0] != sent).any(axis=1).sum())
    err_ae = int((bits != sent).any(axis=1).sum())
    print("block errors of", ae_ref.ROWS, "rows: SC", err_sc, "AE-64", err_ae)
    assert err_ae <= err_sc


@pytest.mark.parametrize("rm", [(2, 5), (3, 7), (3, 8), (4, 9), (4, 10), (1, 3), (0, 4), (4, 4)])
def test_rm_code_is_the_reference_recipe(rm):
    r, m = rm
    n = 1 << m
    k, fp = automorphism.rm_code(r, m)
    _, _, want = polar_amd.get_Kern_frozen_bits(n, n - k, polar_amd.F2)
    assert k == sum(__import__("math").comb(m, j) for j in range(r + 1))
    assert np.array_equal(fp, np.sort(want.numpy()))
    if (k, n) in ((16, 32), (64, 128), (256, 512)):
        assert np.array_equal(fp, polar_amd.reference_frozen_pos(k, n).numpy())


@pytest.mark.parametrize("case", ae_ref.EXACT_CASES, ids=lambda c: c[0])
def test_exact_cases_keep_fragile_rows_within_the_cap(case):
    fp, table, x = ae_ref.case_inputs(case)
    ref = ae_ref.ae_decode(x, fp, case[1], table, llr_max=case[6], exact=True)
    print(case[0], "fragile rows:", int(ref["fragile"].sum()), "of", ae_ref.ROWS)
    assert ref["fragile"].sum() <= ae_ref.FRAGILE_CAP


def test_stage_permutations_of_the_pinned_32_64_set():
    fp = polar_amd.reference_frozen_pos(32, 64).numpy()
    two = automorphism.stage_permutations(fp, 64, 2)
    assert two.shape == (2, 64) and np.array_equal(two[0], np.arange(64)) and not np.array_equal(two[1], two[0])
    assert automorphism.is_automorphism(two[1], fp, 64)
    with pytest.raises(ValueError, match="only 2"):
        automorphism.stage_permutations(fp, 64, 3)


def test_perm_table_and_linear_permutations():
    assert np.array_equal(automorphism.perm_table([1, 2, 4], 8), np.arange(8))
    assert np.array_equal(automorphism.perm_table([2, 1, 4], 8), [0, 2, 1, 3, 4, 6, 5, 7])  # bits 0 and 1 swapped
    assert np.array_equal(automorphism.perm_table([1, 3, 4], 8), [0, 1, 3, 2, 4, 5, 7, 6])  # x1 -> x1 + x0
    with pytest.raises(ValueError):
        automorphism.perm_table([1, 2], 8)
    k, fp = automorphism.rm_code(2, 5)
    lin = automorphism.linear_permutations(fp, 32, 12, seed=3)
    assert lin.shape == (12, 32) and len({row.tobytes() for row in lin}) == 12
    assert all(automorphism.is_permutation(pi, 32) and automorphism.is_automorphism(pi, fp, 32) for pi in lin)
    assert np.array_equal(lin, automorphism.linear_permutations(fp, 32, 12, seed=3))  # seeded
    # a GL map that is no bit-index permutation is in general no automorphism of a non-RM set
    pinned = polar_amd.reference_frozen_pos(32, 64).numpy()
    with pytest.raises(ValueError, match="only"):
        automorphism.linear_permutations(pinned, 64, 64)
    assert not automorphism.is_automorphism(np.random.default_rng(0).permutation(64), pinned, 64)


def test_ae_dec_constructor_checks():
    """The module's argument checks need no GPU: plans and tables are made on first use."""
    k, fp = automorphism.rm_code(2, 5)
    dec = polar_amd.AE_Dec(fp, 32, num_perms=8)
    assert dec.k == 16 and dec.perms.shape == (8, 32) and dec.num_perms == 8
    with pytest.raises(ValueError, match="only 2"):
        polar_amd.AE_Dec(polar_amd.reference_frozen_pos(32, 64), 64, num_perms=3)
    for kw in (dict(num_perms=0), dict(num_perms=65), dict(kind="affine"), dict(f="maxlog"), dict(llr_max=0.0)):
        with pytest.raises(ValueError):
            polar_amd.AE_Dec(fp, 32, **kw)
    with pytest.raises(ValueError, match="n = 2048"):
        polar_amd.AE_Dec(np.arange(1024), 2048)
    with pytest.raises(ValueError, match="not a permutation"):
        polar_amd.AE_Dec(fp, 32, perms=np.zeros((2, 32), dtype=np.int64))
    with pytest.warns(UserWarning, match="not an automorphism"):
        rnd = np.stack([np.arange(64), np.random.default_rng(0).permutation(64)])
        polar_amd.AE_Dec(polar_amd.reference_frozen_pos(32, 64), 64, perms=rnd)
