"""The numpy restatement of PAC coding (tests/golden/pac_ref.py) pinned on the CPU.

The GPU tests hold the kernels to pac_ref value for value; these tests hold pac_ref to things written
independently of it: the reference's SC fixtures (conv = (1,), L = 1 is plain min-sum SC), a Toeplitz-matrix
encoder, a brute-force minimum over all data words through a forced-decision SC walk without list bookkeeping,
noiseless round trips, and the row-order independence of the tie rule.
"""
import glob
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import pac_ref  # noqa: E402

C133 = pac_ref.CONV_133
FIXTURE_LLR_MAX = 30.0  # tests/golden/make_golden.py: the reference's SC_Dec clips at 30


def _forced_walk(a, u, lmax):
    """SC over one row's LLRs a (positive favours 0) with every decision forced to u (length n, the
    polar-domain bits): returns (leaf LLRs [n], the codeword bits of the node).  Plain recursion."""
    n = len(a)
    if n == 1:
        return a.copy(), u.copy()
    h = n // 2
    x, y = a[:h], a[h:]
    fl = (np.sign(x) * np.sign(y) * np.minimum(np.minimum(np.abs(x), np.abs(y)), np.float32(lmax))).astype(np.float32)
    leaf_l, bl = _forced_walk(fl, u[:h], lmax)
    gr = (np.where(bl != 0, -x, x) + y).astype(np.float32)
    leaf_r, br = _forced_walk(gr, u[h:], lmax)
    return np.concatenate([leaf_l, leaf_r]), np.concatenate([bl ^ br, br])


def _forced_metric(a, u, lmax):
    """Path metric of the forced path: |l_i| summed, in leaf order and in fp32, over the leaves with u_i != (l_i < 0)."""
    leaf, _ = _forced_walk(a, u, lmax)
    pm = np.float32(0.0)
    for l, b in zip(leaf, u):
        if bool(b) != bool(l < 0):
            pm = np.float32(pm + np.abs(l))
    return pm, leaf


def _half_rate_set(n, k, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.permutation(n)[: n - k])


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "sc_*.npz"))), ids=os.path.basename)
def test_plain_sc_fixtures(path):
    """conv = (1,), L = 1 is min-sum SC: the decoded bits of the reference's fixtures.  One rule differs by
    design: at a leaf LLR of exactly zero the reference decides 1 (u = 1 iff not l > 0), a list decoder's zero
    penalty for both values keeps candidate 0.  A row in which the fixture's own walk meets an exactly zero LLR at
    an information leaf is therefore compared up to that leaf's column, where it must show exactly this difference;
    every other row must agree in every bit, and the rand and AWGN sets hold only such rows."""
    d = np.load(path)
    n, fp = int(d["n"]), d["frozen_pos"].astype(np.int64)
    info = pac_ref.info_positions(fp, n)
    rows = 6 if n >= 1024 else 16
    strict = 0
    for name in [k[4:] for k in d.files if k.startswith("llr_")]:
        x, want = d["llr_" + name][:rows], d["bits_" + name][:rows]
        got, _ = pac_ref.pac_decode(x, fp, n, 1, conv=(1,), llr_max=FIXTURE_LLR_MAX)
        for r in range(x.shape[0]):
            u = np.zeros(n, np.uint8)
            u[info] = want[r]
            leaf, _ = _forced_walk((-x[r]).astype(np.float32), u, FIXTURE_LLR_MAX)
            zero = np.flatnonzero(leaf[info] == 0)
            upto = len(info) if zero.size == 0 else int(zero[0])
            strict += zero.size == 0
            assert np.array_equal(got[r, :upto], want[r, :upto]), (name, r, upto)
            if zero.size:  # the documented difference, and nothing else, at the first zero leaf
                assert want[r, upto] == 1 and got[r, upto] == 0, (name, r, upto)
    assert strict >= 3 * rows, strict  # the rand and AWGN sets have no zero leaves


@pytest.mark.parametrize("n,k,conv", [(8, 4, C133), (16, 5, (1, 1)), (64, 32, C133), (128, 64, C133), (32, 32, C133),
                                      (64, 1, (1,) + (0,) * 30 + (1,))])
def test_encode_is_toeplitz_times_transform(n, k, conv):
    fp = _half_rate_set(n, k, n + k)
    info = pac_ref.info_positions(fp, n)
    rng = np.random.default_rng(7)
    data = rng.integers(0, 2, (21, k)).astype(np.uint8)
    v = np.zeros((21, n), np.int64)
    v[:, info] = data
    T = np.zeros((n, n), np.int64)  # u = v T: T[i, i + j] = c_j
    for j, c in enumerate(conv):
        if c:
            T += np.eye(n, k=j, dtype=np.int64)
    G = np.array([[1]], np.int64)
    for _ in range(n.bit_length() - 1):
        G = np.kron(np.array([[1, 0], [1, 1]], np.int64), G)
    want = (v @ T % 2) @ G % 2
    assert np.array_equal(pac_ref.pac_encode(data, fp, n, conv), want)
    gm = pac_ref.generator_matrix(fp, n, conv)
    assert gm.shape == (k, n)
    m, rank = gm.copy(), 0  # GF(2) rank by elimination
    for j in range(n):
        rows = np.flatnonzero(m[rank:, j])
        if rows.size == 0:
            continue
        p = rank + rows[0]
        m[[rank, p]] = m[[p, rank]]
        others = np.flatnonzero(m[:, j])
        others = others[others != rank]
        m[others] ^= m[rank]
        rank += 1
        if rank == k:
            break
    assert rank == k


@pytest.mark.parametrize("n,k,L", [(8, 4, 16), (16, 5, 32)])
def test_unpruned_list_is_the_brute_force_minimum(n, k, L):
    """L = 2^k: nothing is pruned, so the output is the data word whose forced path has the smallest metric."""
    fp = _half_rate_set(n, k, 3 * n)
    info = pac_ref.info_positions(fp, n)
    rng = np.random.default_rng(n)
    x = pac_ref.awgn_rows(fp, n, C133, 12, 1.0, rng)
    words = ((np.arange(2 ** k)[:, None] >> np.arange(k)) & 1).astype(np.uint8)
    v = np.zeros((2 ** k, n), np.uint8)
    v[:, info] = words
    u = pac_ref.precode(v, C133)
    bits, pm = pac_ref.pac_decode(x, fp, n, L, conv=C133, llr_max=30.0)
    for r in range(x.shape[0]):
        a = (-x[r]).astype(np.float32)
        metrics = np.array([_forced_metric(a, u[w], 30.0)[0] for w in range(2 ** k)], np.float32)
        assert len(np.unique(metrics)) == len(metrics), "two data words tie: pick other rows"
        best = int(np.argmin(metrics))
        assert np.array_equal(bits[r], words[best]), r
        assert np.array_equal(pm[r], np.sort(metrics)[:L]), r


@pytest.mark.parametrize("L", [1, 2, 4, 8, 16, 32])
def test_noiseless_rows_decode_to_the_data(L):
    for n, k, conv in ((2, 1, C133), (8, 8, C133), (64, 32, C133), (128, 64, (1, 1, 1)), (32, 7, (1,))):
        fp = _half_rate_set(n, k, n)
        rng = np.random.default_rng(L)
        data = rng.integers(0, 2, (9, k)).astype(np.uint8)
        x = ((2.0 * pac_ref.pac_encode(data, fp, n, conv) - 1.0) * 5.0).astype(np.float32)
        bits, pm = pac_ref.pac_decode(x, fp, n, L, conv=conv)
        assert np.array_equal(bits, data), (n, k, L)
        assert (pm[:, 0] == 0).all()


def test_integer_rows_do_not_depend_on_row_order():
    n, k = 64, 32
    fp = _half_rate_set(n, k, 5)
    rng = np.random.default_rng(11)
    x = pac_ref.integer_rows(n, 40, rng)
    perm = rng.permutation(40)
    for L in (2, 8):
        b0, p0 = pac_ref.pac_decode(x, fp, n, L, conv=C133)
        b1, p1 = pac_ref.pac_decode(x[perm], fp, n, L, conv=C133)
        assert np.array_equal(b0[perm], b1) and np.array_equal(p0[perm], p1)
        assert np.isfinite(p0).all()  # k >= log2 L information leaves: every path came alive


def test_inputs_have_the_three_kinds():
    fp = _half_rate_set(64, 32, 1)
    x = pac_ref.make_inputs(fp, 64, C133, 30.0, 67, 3)
    assert x.shape == (67, 64) and x.dtype == np.float32
    assert (x[0] == 0).all() and (np.abs(x[1]) == 30).all() and (np.abs(x[2]) == 75).all() and (np.abs(x[3]) == 8).all()
    assert (x[-32:] == np.round(x[-32:])).all() and np.abs(x[-32:]).max() == 3
    assert np.array_equal(x, pac_ref.make_inputs(fp, 64, C133, 30.0, 67, 3))
