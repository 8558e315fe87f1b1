"""Frozen-set design without a GPU: the numpy genie-aided SC transform (tests/golden/genie_ref.py)
against the reference decoder's own leaf LLRs (tests/golden/genie.npz), select_frozen's ordering,
a designed code against the RM-weight one under the C oracle's SC, the argument checks of
pl_genie_count (they run before any HIP call) and the command-line options."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import genie_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "genie.npz")
CASES = [f"{fam}_n{n}" for n in (8, 64, 256) for fam in ("ok", "last")]


def test_fixture_cases():
    with np.load(GOLDEN) as d:
        for name in CASES:
            n = int(name.split("_n")[1])
            assert d[name + "_logits"].shape == (64, n) and d[name + "_logits"].dtype == np.float32
            assert d[name + "_u"].shape == (64, n) and d[name + "_leaf"].shape == (64, n)
        for n in (8, 64, 256):  # the rows that pin the awkward inputs do hold them
            x = d[f"last_n{n}_logits"]
            assert (x == 0).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
            assert np.abs(x[-1]).max() > 30 and not d[f"last_n{n}_u"][:, : n - 1].any()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    """genie_ref's min-sum transform reproduces msg_llr[:, 0, :] of the reference's SC_Dec: every
    value equal, every nonzero value bit for bit.  The sign of a zero is the one difference there can
    be: the reference multiplies by torch.sign, which is 0 for -0 and +0 alike and so forgets the
    sign, where the kernels (sc_kernel.hip fop) and genie_ref carry the xor of the sign bits; no later
    value or decision depends on it (-0 + y = y, min(|0|, .) = 0, HD(+-0) = 1)."""
    with np.load(GOLDEN) as d:
        logits, u, leaf = d[name + "_logits"], d[name + "_u"], d[name + "_leaf"]
    mine = genie_ref.leaf_llrs(logits, u)
    assert mine.dtype == np.float32 and np.array_equal(mine, leaf)
    diff = mine.view(np.uint32) != leaf.view(np.uint32)
    assert not diff[leaf != 0].any() and np.all(mine[diff] == 0)
    if name.startswith("ok"):
        assert not diff.any()
        assert np.array_equal(genie_ref.hard(mine)[:, u.any(axis=0)], u[:, u.any(axis=0)])  # decoded correctly


def test_beta_states_are_the_encoder_butterfly():
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2, (5, 32)).astype(np.uint8)
    beta = genie_ref.beta_states(u)
    assert np.array_equal(beta[0], u)
    full = beta[-1].copy()
    full[:, :16] ^= full[:, 16:]
    assert np.array_equal(full, oracle.polar_encode(u, np.zeros(0, np.int64), 32).astype(np.uint8))


def test_exact_variant_agrees_with_the_oracle_sc():
    """The f_cr variant decides like the oracle's exact-f SC wherever SC decodes correctly (then SC's
    own feedback is the genie's) and no f was fragile."""
    rng = np.random.default_rng(11)
    n, k = 64, 32
    from polar_amd.frozen import reference_frozen_pos
    fp = reference_frozen_pos(k, n).numpy()
    info = np.setdiff1d(np.arange(n), fp)
    u = np.zeros((64, n), dtype=np.uint8)
    u[:, info] = rng.integers(0, 2, (64, k))
    x = oracle.polar_encode(u[:, info], fp, n)
    logits = ((2 * x - 1) * 3 + rng.standard_normal(x.shape)).astype(np.float32)
    dec = oracle.sc_decode(logits, fp, f_mode=1)
    leaf, fragile = genie_ref.leaf_llrs(logits, u, exact=True)
    ok = (dec == u[:, info]).all(axis=1) & ~fragile
    assert ok.sum() >= 32
    assert np.array_equal(genie_ref.hard(leaf)[ok][:, info], u[ok][:, info])


def test_select_frozen_ordering_and_ties():
    from polar_amd.design import select_frozen
    counts = np.array([9, 5, 5, 0, 7, 0, 0, 0])
    # key (count, -popcount, -i): 7 (0, pc 3), 6 (0, pc 2), 5 (0, pc 2), 3 (0, pc 2) ... 6 > 5 > 3 by position
    order = [7, 6, 5, 3, 2, 1, 4, 0]  # 2 and 1: count 5, popcount 1, the later first; then 4 (7), 0 (9)
    for k in range(9):
        fp = select_frozen(counts, k)
        assert fp.dtype == torch.int64 and fp.tolist() == sorted(order[k:])
    assert select_frozen(torch.tensor(counts), 3).tolist() == sorted(order[3:])
    with pytest.raises(ValueError):
        select_frozen(counts, 9)
    with pytest.raises(ValueError):
        select_frozen(counts, -1)


@pytest.mark.parametrize("n", [2, 8, 64, 1024])
def test_select_frozen_edges_and_rm_weight_order(n):
    from polar_amd.design import select_frozen
    zero = np.zeros(n, dtype=np.int64)
    assert select_frozen(zero, n).numel() == 0
    assert select_frozen(zero, 0).tolist() == list(range(n))
    pop = np.array([bin(i).count("1") for i in range(n)])
    for k in sorted({1, n // 2, n - 1}):
        fp = select_frozen(zero, k).numpy()
        assert len(fp) == n - k and np.all(np.diff(fp) > 0)  # sorted, unique
        info = np.setdiff1d(np.arange(n), fp)
        # all-zero counts: the RM-weight order, the later position first among equal weights
        assert pop[info].min() >= pop[fp].max()
        edge = pop[info].min()
        at_edge_info, at_edge_frozen = info[pop[info] == edge], fp[pop[fp] == edge]
        assert at_edge_frozen.size == 0 or at_edge_info.min() > at_edge_frozen.max()


def _qpsk_logits(rng, x, ebno_db, rate):
    from polar_amd.channel import ebnodb2no
    no = ebnodb2no(ebno_db, 2, rate)
    y = (1.0 - 2.0 * x) / np.sqrt(2.0) + rng.standard_normal(x.shape) * np.sqrt(no / 2.0)
    return (-2.0 * np.sqrt(2.0) * y / no).astype(np.float32)


def test_designed_code_beats_rm_weight_under_the_oracle_sc():
    """(32,64) designed at 3 dB from genie_ref counts over 40000 numpy rows (random bits on all 64
    positions, the noise of rate 1/2) has fewer SC block errors than the pinned RM-weight (32,64) set
    on the same 20000 noisy rows, decoded by the C oracle.  Seeded: deterministic.  Counts: DESIGN.md
    section 13."""
    from polar_amd.design import select_frozen
    from polar_amd.frozen import reference_frozen_pos
    n, k, ebno = 64, 32, 3.0
    rng = np.random.default_rng(2024)
    u = rng.integers(0, 2, (40000, n)).astype(np.uint8)
    x = oracle.polar_encode(u, np.zeros(0, np.int64), n)
    leaf = genie_ref.leaf_llrs(_qpsk_logits(rng, x, ebno, k / n), u)
    designed = select_frozen(genie_ref.error_counts(leaf, u), k).numpy()
    rm = reference_frozen_pos(k, n).numpy()
    assert len(designed) == n - k and not np.array_equal(designed, rm)

    rows = 20000
    noise = np.random.default_rng(7).standard_normal((rows, n))
    bits = np.random.default_rng(8).integers(0, 2, (rows, k)).astype(np.float32)
    from polar_amd.channel import ebnodb2no
    no = ebnodb2no(ebno, 2, k / n)
    errs = {}
    for name, fp in (("designed", designed), ("rm", rm)):
        cw = oracle.polar_encode(bits, fp, n)
        y = (1.0 - 2.0 * cw) / np.sqrt(2.0) + noise * np.sqrt(no / 2.0)
        logits = (-2.0 * np.sqrt(2.0) * y / no).astype(np.float32)
        errs[name] = int((oracle.sc_decode(logits, fp) != bits).any(axis=1).sum())
    print("block errors of", rows, errs)
    assert errs["designed"] < errs["rm"], errs


def test_genie_count_argument_checks_without_gpu():
    from polar_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(64)  # never dereferenced: every check below fails, or returns, before a HIP call
    call = L.pl_genie_count

    def err():
        return L.pl_last_error_string().decode()
    for n in (0, 1, 3, 48, 4096, -8):
        assert call(n, 0, 30.0, one, one, 4, one, None, None) == _lib.PL_EINVAL and "n must" in err()
    assert call(64, 2, 30.0, one, one, 4, one, None, None) == _lib.PL_EINVAL and "f_mode" in err()
    assert call(64, 0, 30.0, one, one, -1, one, None, None) == _lib.PL_EINVAL and "bs" in err()
    assert call(64, 0, 30.0, one, one, 4, None, None, None) == _lib.PL_EINVAL and "both NULL" in err()
    assert call(64, 0, 30.0, None, one, 4, one, None, None) == _lib.PL_EINVAL and "llr_logits" in err()
    assert call(64, 0, 30.0, one, None, 4, one, None, None) == _lib.PL_EINVAL and "u_bits" in err()
    assert call(64, 0, 30.0, None, None, 0, one, None, None) == _lib.PL_OK  # no rows
    assert call(64, 1, 60.0, None, None, 0, None, one, None) == _lib.PL_OK


def test_ops_genie_count_checks_without_gpu():
    from polar_amd import ops
    with pytest.raises(RuntimeError):
        ops.genie_count(64, torch.zeros(2, 64), torch.zeros(2, 2, dtype=torch.int32))


def test_cli_design_options():
    from polar_amd import cli
    c = cli.parse(["--frozen", "design", "--design_ebno", "2.5"])
    assert c.frozen == "design" and c.design_ebno == 2.5 and c.design_rows == 2 ** 20
    assert cli.parse(["--frozen", "design", "--design_ebno", "3", "--design_rows", "65536",
                      "--num_bits_per_symbol", "4"]).design_rows == 65536
    assert cli.parse([]).frozen == "reference"
    for bad in (["--frozen", "design"],  # no --design_ebno
                ["--frozen", "design", "--design_ebno", "3", "--code", "5g"],
                ["--frozen", "design", "--design_ebno", "3", "--llr_device", "cpu"],
                ["--frozen", "design", "--design_ebno", "3", "--design_rows", "0"]):
        with pytest.raises(SystemExit):
            cli.parse(bad)


def test_public_names():
    import polar_amd
    for name in ("bit_channel_errors", "select_frozen", "design_frozen_pos"):
        assert name in polar_amd.__all__ and callable(getattr(polar_amd, name))
    assert "pl_genie_count" in polar_amd._lib.EXPORTED_SYMBOLS
