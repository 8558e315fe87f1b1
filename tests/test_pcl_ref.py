"""The numpy restatement of parity-constrained list decoding and of the DCI chain (tests/golden/pcl_ref.py) pinned
on the CPU.

The GPU tests hold the kernel and polar_amd.dci to pcl_ref value for value; these tests hold pcl_ref to things
written independently of it: pac_ref (no constraints is the PAC decoder with conv = (1,)), an exhaustive search
over all words that satisfy the constraints with the metric of a scalar forced-decision SC recursion, the package's
own derivation of the DCI table from its generator-row CRC, and the figures the distributed CRC is known by.
"""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import pac_ref  # noqa: E402
import pcl_ref  # noqa: E402

CHECK, FORCE = pcl_ref.CHECK, pcl_ref.FORCE


def _half(n, k, seed):
    return np.sort(np.random.default_rng(seed).permutation(n)[: n - k])


@pytest.mark.parametrize("n", [8, 64, 256])
@pytest.mark.parametrize("L", [1, 4, 32])
def test_no_constraints_is_the_pac_decoder_with_conv_1(n, L):
    fp = _half(n, n // 2, n)
    x = pac_ref.make_inputs(fp, n, (1,), 30.0, 40 if n < 256 else 16, seed=n + L)
    bits, pm, ok, stop = pcl_ref.pcl_decode(x, fp, n, L, pcl_ref.pack_constraints(n, []), 30.0)
    wb, wpm = pac_ref.pac_decode(x, fp, n, L, conv=(1,), llr_max=30.0)
    assert np.array_equal(bits, wb) and np.array_equal(pm, wpm)
    assert (ok == 1).all() and (stop == n).all()


def _forced_metric(a, u, lmax):
    """The path metric of the decisions u (length n) over the LLRs a (positive favours 0), by plain recursion:
    returns (metric summed in leaf order in fp32, codeword bits of the node)."""
    def walk(a, u):
        if len(a) == 1:
            return [a[0]], u.copy()
        h = len(a) // 2
        x, y = a[:h], a[h:]
        fl = (np.sign(x) * np.sign(y) * np.minimum(np.minimum(np.abs(x), np.abs(y)), np.float32(lmax))).astype(np.float32)
        ll, bl = walk(fl, u[:h])
        lr, br = walk((np.where(bl != 0, -x, x) + y).astype(np.float32), u[h:])
        return ll + lr, np.concatenate([bl ^ br, br])
    leaf, _ = walk(a, u)
    pm = np.float32(0.0)
    for l, b in zip(leaf, u):
        if bool(b) != bool(l < 0):
            pm = np.float32(pm + np.abs(l))
    return pm


TIE_SHARE = {}


@pytest.mark.parametrize("n,k,num,kinds,seed", [(8, 4, 2, (CHECK,), 1), (8, 5, 3, (FORCE,), 2), (16, 5, 2, (CHECK, FORCE), 3),
                                                (16, 5, 4, (CHECK,), 4), (16, 4, 4, (CHECK, FORCE), 5), (8, 3, 0, (CHECK,), 6)])
def test_full_list_is_the_exhaustive_search(n, k, num, kinds, seed):
    """L = 32 >= 2^k: no valid word is ever ranked out (a CHECK leaf has at most 2^(k-1) <= 16 live parents, so all
    of their children are kept), hence the output is the valid word of smallest metric and the metrics are those of
    all valid words, for CHECK and FORCE alike.  Rows in which two valid words tie are left out (the order among
    equal metrics is the list's, not the search's): their share is printed and capped at 5 %."""
    L = 32
    fp = _half(n, k, 11 * n + seed)
    info = pcl_ref.info_positions(fp, n)
    table = pcl_ref.random_table(fp, n, num, seed, kinds=kinds)
    assert pcl_ref.check_table(fp, n, table) is None
    rng = np.random.default_rng(100 + seed)
    x = np.concatenate([pcl_ref.awgn_rows(fp, n, table, 20, 1.0, rng), pcl_ref.noise_rows(n, 20, rng)])
    words = ((np.arange(2 ** k)[:, None] >> np.arange(k)) & 1).astype(np.uint8)
    u = np.zeros((2 ** k, n), np.uint8)
    u[:, info] = words
    valid = pcl_ref.satisfies(u, table)
    assert valid.sum() == 2 ** (k - num)
    bits, pm, ok, stop = pcl_ref.pcl_decode(x, fp, n, L, table, 30.0)
    ties = 0
    for r in range(x.shape[0]):
        a = (-x[r]).astype(np.float32)
        metrics = np.array([_forced_metric(a, u[w], 30.0) for w in np.flatnonzero(valid)], np.float32)
        if len(np.unique(metrics)) != len(metrics):
            ties += 1
            continue
        best = np.flatnonzero(valid)[int(np.argmin(metrics))]
        assert np.array_equal(bits[r], words[best]), r
        want = np.full(L, np.inf, np.float32)
        want[: len(metrics)] = np.sort(metrics)
        assert np.array_equal(pm[r], want), r
        assert ok[r] == 1 and stop[r] == n
    TIE_SHARE[(n, k, num, seed)] = ties / x.shape[0]
    print(f"rows left out for ties: {ties} of {x.shape[0]}")
    assert ties / x.shape[0] <= 0.05


def _downlink(A, E):
    from polar_amd.polar5g import _rate_match_tables
    _, n_polar, frozen, idx_rm, il = _rate_match_tables(A, E, "downlink")
    info = np.setdiff1d(np.arange(n_polar), frozen)
    return int(n_polar), info, np.asarray(idx_rm), np.asarray(il)


def _e_for(A):
    return int(min(576, max(25, 3 * (A + 24))))


def test_dci_table_is_causal_for_every_payload_length():
    for A in range(1, 141):
        n_polar, info, _, il = _downlink(A, _e_for(A))
        frozen = np.setdiff1d(np.arange(n_polar), info)
        for rnti, prefix in ((0, True), (0xBEEF, False)):
            table = pcl_ref.dci_table(A, info, n_polar, il, rnti, prefix)
            assert len(table[0]) == 24 and pcl_ref.check_table(frozen, n_polar, table) is None, A
        assert pcl_ref.check_table(frozen, n_polar, pcl_ref.dci_table(A, info, n_polar, None)) is None, A


def test_distributed_parity_bit_counts():
    got = []
    for A in (12, 16, 32, 40, 64, 100, 140):
        n_polar, info, _, il = _downlink(A, _e_for(A))
        got.append(pcl_ref.dci_distributed(A, info, il))
        assert pcl_ref.dci_distributed(A, info, None) == 0
    assert got == [3, 3, 3, 3, 3, 7, 7]


def test_crc24c_long_division_equals_the_generator_rows():
    """Two derivations of one code: the polynomial divided out bit by bit, and the package's generator rows."""
    from polar_amd.polar5g import crc_generator_rows
    rows = crc_generator_rows("CRC24C", 37)
    want = ((rows[:, None] >> np.arange(24, dtype=np.uint32)) & np.uint32(1)).astype(np.uint8)
    assert np.array_equal(pcl_ref.crc24c(np.eye(37, dtype=np.uint8)), want)


@pytest.mark.parametrize("A,E", [(12, 54), (40, 216), (64, 128), (140, 576), (100, 150)])
def test_encoded_words_satisfy_the_table_and_the_package_derives_the_same(A, E):
    import contextlib
    import io

    from polar_amd import dci, pcl
    n_polar, info, idx_rm, il = _downlink(A, E)
    rng = np.random.default_rng(A)
    data = rng.integers(0, 2, (33, A)).astype(np.uint8)
    for rnti, prefix, inter in ((0, True, True), (0xBEEF, True, True), (0xBEEF, False, True), (0x1234, True, False),
                                (0, False, False)):
        ilx = il if inter else None
        cw, u = pcl_ref.dci_encode(data, info, n_polar, ilx, idx_rm, rnti, prefix)
        assert cw.shape == (33, E)
        for n_force in (0, pcl_ref.dci_distributed(A, info, ilx), 24):
            table = pcl_ref.dci_table(A, info, n_polar, ilx, rnti, prefix, n_force)
            assert pcl_ref.satisfies(u, table).all()
            assert (table[1] == FORCE).sum() == n_force
            with contextlib.redirect_stdout(io.StringIO()):
                enc = dci.DCIEncoder(A, E, rnti=rnti, ones_prefix=prefix, interleave=inter)
            mine = pcl.pack_constraints(n_polar, dci.dci_constraints(enc, n_force))
            assert all(np.array_equal(a, b) for a, b in zip(mine, table))
            assert dci.distributed_parity_bits(enc) == pcl_ref.dci_distributed(A, info, ilx)
        wrong = pcl_ref.dci_table(A, info, n_polar, ilx, rnti ^ 0x0100, prefix)
        assert not pcl_ref.satisfies(u, wrong).any()  # another RNTI: every word fails the same parity bit
    # a noiseless round trip through the restatement
    cw, _ = pcl_ref.dci_encode(data[:5], info, n_polar, il, idx_rm, 0xBEEF, True)
    a_hat, ok, stop, _ = pcl_ref.dci_decode((2.0 * cw - 1.0) * 6.0, A, info, n_polar, il, idx_rm, 4, 0xBEEF, True)
    assert np.array_equal(a_hat, data[:5]) and (ok == 1).all() and (stop == n_polar).all()


@pytest.mark.parametrize("case", pcl_ref.GPU_CASES, ids=str)
def test_gpu_cases_hold_rows_that_stop_and_rows_that_run_to_the_end(case):
    """What tests/test_pcl_gpu.py decodes: every case whose table can stop a row (pcl_ref.NEVER_STOPS lists the
    others and why) holds at least one row that stops early and, but for the "kill" cases, one that runs to n;
    a "kill" case stops every row at its single CHECK with zero bits and ok = 0."""
    n, kind, L, tkind = case
    fp, table, x, (bits, pm, ok, stop) = pcl_ref.gpu_case(*case)
    assert x.shape == (9 if n >= 1024 else 67, n) and pcl_ref.check_table(fp, n, table) is None
    early = stop < n
    assert ((ok == 0) == early).all() and (bits[early] == 0).all() and np.isinf(pm[early]).all()
    assert (table[1][np.searchsorted(table[0], stop[early])] == CHECK).all()  # a row stops at a CHECK leaf only
    if tkind == "kill":
        assert (stop == table[0][0]).all() and (ok == 0).all() and (bits == 0).all()
    elif case in pcl_ref.NEVER_STOPS:
        assert not early.any()
    else:
        assert early.any() and (~early).any(), (int(early.sum()), case)


def test_inputs_have_the_four_kinds():
    fp = _half(64, 32, 1)
    table = pcl_ref.random_table(fp, 64, 8, 3)
    x = pcl_ref.make_inputs(fp, 64, table, 30.0, 67, 3)
    assert x.shape == (67, 64) and x.dtype == np.float32
    assert (x[0] == 0).all() and (np.abs(x[1]) == 30).all() and (np.abs(x[2]) == 75).all() and (np.abs(x[3]) == 8).all()
    assert (x[25:46] == np.round(x[25:46])).all() and np.abs(x[25:46]).max() == 3
    assert np.array_equal(x, pcl_ref.make_inputs(fp, 64, table, 30.0, 67, 3))
    u = pcl_ref.constrained_words(np.random.default_rng(0).integers(0, 2, (9, 24)), fp, 64, table)
    assert pcl_ref.satisfies(u, table).all() and not pcl_ref.satisfies(u ^ np.eye(64, dtype=np.uint8)[table[0][0]], table).any()


def test_shortening_case_of_the_dci_tests_is_one():
    n_polar, _, _, _ = _downlink(100, 150)
    assert n_polar == 256 and 124 / 150 > 7 / 16  # E < n_polar and a rate above 7/16: shortening


@pytest.mark.parametrize("A,E", [(40, 216), (64, 128)])
def test_a_list_accepts_another_rnti_and_a_single_path_does_not(A, E):
    """What DESIGN section 20 says of CHECK after the ranking, on noiseless rows of RNTI 0xBEEF decoded for 0xBEE7:
    L = 1 rejects every row at the parity bit that carries the differing RNTI bit; L = 8 keeps both children of the
    few live parents there, so every row ends with ok = 1 -- with the transmitted payload: only the parity bit differs."""
    n_polar, info, idx_rm, il = _downlink(A, E)
    data = np.random.default_rng(A).integers(0, 2, (33, A)).astype(np.uint8)
    cw, _ = pcl_ref.dci_encode(data, info, n_polar, il, idx_rm, 0xBEEF, True)
    x = ((2.0 * cw - 1.0) * 6.0).astype(np.float32)
    a1, ok1, stop1, _ = pcl_ref.dci_decode(x, A, info, n_polar, il, idx_rm, 1, 0xBEE7, True)
    assert (ok1 == 0).all() and (a1 == 0).all() and len(set(stop1.tolist())) == 1 and stop1[0] < n_polar
    a8, ok8, stop8, _ = pcl_ref.dci_decode(x, A, info, n_polar, il, idx_rm, 8, 0xBEE7, True)
    assert (ok8 == 1).all() and (stop8 == n_polar).all() and np.array_equal(a8, data)
