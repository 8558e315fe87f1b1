"""pl_genie_count / polar_amd.design on the GPU: the kernel's leaf LLRs against the numpy restatement
(tests/golden/genie_ref.py, itself pinned to the reference's SC_Dec by tests/golden/genie.npz) bit for
bit, the counters, the fused producer over a plan without frozen positions, designed codes against
the RM-weight ones, and the CLI's --frozen design."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import genie_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "genie.npz")
DEV = "cuda:0"


def _run(n, logits, u, **kw):
    from polar_amd import ops
    x = torch.as_tensor(np.ascontiguousarray(logits, dtype=np.float32), device=DEV)
    w = torch.as_tensor(genie_ref.pack_u(u), device=DEV)
    return ops.genie_count(n, x, w, **kw)


def _inputs(n, rows, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (rows, n)).astype(np.uint8)
    return genie_ref.special_llrs(rng, rows, n), u


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [2, 4, 8, 32, 64, 128, 256, 1024, 2048])
def test_leaf_equals_restatement_minsum(n):
    """130 rows: no multiple of any codewords-per-wave count, several blocks at small n; random u on all
    positions; zeros of both signs, integer ties and a x40 saturated row."""
    logits, u = _inputs(n, 130, 100 + n)
    counts, leaf = _run(n, logits, u, return_leaf=True)
    ref = genie_ref.leaf_llrs(logits, u)
    assert np.array_equal(_bits(leaf.cpu().numpy()), _bits(ref))
    assert np.array_equal(counts.cpu().numpy(), genie_ref.error_counts(ref, u))


@pytest.mark.parametrize("name", [f"{fam}_n{n}" for n in (8, 64, 256) for fam in ("ok", "last")])
def test_leaf_equals_the_reference_rows(name):
    with np.load(GOLDEN) as d:
        logits, u, ref_leaf = d[name + "_logits"], d[name + "_u"], d[name + "_leaf"]
    n = logits.shape[1]
    _, leaf = _run(n, logits, u, return_leaf=True)
    leaf = leaf.cpu().numpy()
    assert np.array_equal(_bits(leaf), _bits(genie_ref.leaf_llrs(logits, u)))
    assert np.array_equal(leaf, ref_leaf)  # the reference: equal values (it drops the sign of a zero)
    assert np.array_equal(_bits(leaf)[ref_leaf != 0], _bits(ref_leaf)[ref_leaf != 0])


@pytest.mark.parametrize("llr_max", [30.0, 60.0])
@pytest.mark.parametrize("n", [8, 64, 256])
def test_leaf_equals_restatement_exact(n, llr_max):
    """Exact f (fast forms at llr_max 30, full-range forms at 60) against the correctly rounded f_cr
    variant; rows where some f lay within the fragile band of a rounding midpoint are left out (there a
    correct device form may round the other way, tests/golden/exactf_cr.py)."""
    rng = np.random.default_rng(500 + n)
    u = rng.integers(0, 2, (64, n)).astype(np.uint8)
    logits = (rng.standard_normal((64, n)) * 3).astype(np.float32)
    logits[-1] *= 12  # beyond llr_max = 30
    logits[0, ::3] = 0.0
    _, leaf = _run(n, logits, u, f_mode=1, llr_max=llr_max, return_leaf=True)
    ref, fragile = genie_ref.leaf_llrs(logits, u, llr_max=llr_max, exact=True)
    # At llr_max = 60 the saturated row overflows (e^120 = inf in fp32, then inf - inf = NaN in a g, as in the
    # reference); NaN LLRs are outside the library's contract (include/polar_mi355x.h), and clip(NaN) is
    # NaN in numpy and the bound on the device, so a row is left out from its first NaN on -- only that row.
    nan_row = np.isnan(ref).any(axis=1)
    assert fragile.sum() <= 8 and not nan_row[:-1].any() and (llr_max > 43 or not nan_row.any())
    keep = ~fragile & ~nan_row
    leaf = leaf.cpu().numpy()
    diff = _bits(leaf)[keep] != _bits(ref)[keep]
    print(f"n={n} llr_max={llr_max}: rows kept {int(keep.sum())} of 64, differing leaves {int(diff.sum())}")
    assert not diff.any()


def test_counts_accumulate_and_outputs_are_optional():
    from polar_amd import ops
    n = 256
    logits, u = _inputs(n, 130, 9)
    x = torch.as_tensor(logits, device=DEV)
    w = torch.as_tensor(genie_ref.pack_u(u), device=DEV)
    ref = genie_ref.error_counts(genie_ref.leaf_llrs(logits, u), u)
    assert ref.sum() > 0
    counts = ops.genie_count(n, x, w)  # counts only
    assert counts.dtype == torch.int64 and counts.shape == (n,)
    assert np.array_equal(counts.cpu().numpy(), ref)
    again = ops.genie_count(n, x, w, counts=counts)  # accumulates
    assert again is counts and np.array_equal(counts.cpu().numpy(), 2 * ref)
    none, leaf = ops.genie_count(n, x, w, counts=False, return_leaf=True)  # leaf only
    assert none is None and np.array_equal(_bits(leaf.cpu().numpy()), _bits(genie_ref.leaf_llrs(logits, u)))
    ops.genie_count(n, x[:0], w[:0], counts=counts)  # bs = 0: untouched
    assert np.array_equal(counts.cpu().numpy(), 2 * ref)
    one = ops.genie_count(n, x[5:6].contiguous(), w[5:6].contiguous())  # rows = 1
    assert np.array_equal(one.cpu().numpy(), genie_ref.error_counts(genie_ref.leaf_llrs(logits[5:6], u[5:6]), u[5:6]))


def test_counts_are_reproducible_over_many_blocks():
    """140000 rows of n = 64 (the 1024-block cap covers 131072: some waves take a second grid stride): two
    runs agree, and both equal the host's column sums."""
    n, rows = 64, 140000
    rng = np.random.default_rng(77)
    u = rng.integers(0, 2, (rows, n)).astype(np.uint8)
    logits = (rng.standard_normal((rows, n)) * 2).astype(np.float32)
    a = _run(n, logits, u).cpu().numpy()
    b = _run(n, logits, u).cpu().numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(a, genie_ref.error_counts(genie_ref.leaf_llrs(logits, u), u))


def test_argument_errors():
    from polar_amd import _lib, ops
    x = torch.zeros(4, 64, device=DEV)
    w = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.genie_count(48, x, w)
    with pytest.raises(ValueError):
        ops.genie_count(64, x[:, :32], w)
    with pytest.raises(ValueError):
        ops.genie_count(64, x, w[:, :1])
    with pytest.raises(ValueError):
        ops.genie_count(64, x, w.to(torch.int64))
    with pytest.raises(ValueError):
        ops.genie_count(64, x, w, counts=torch.zeros(64, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.genie_count(64, x, w, counts=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.genie_count(64, x, w, counts=False)
    with pytest.raises(_lib.PolarLibError) as e:
        ops.genie_count(64, x, w, f_mode=3)
    assert isinstance(e.value, ValueError) and e.value.code == _lib.PL_EINVAL and "f_mode" in str(e.value)


@pytest.mark.parametrize("n,m", [(64, 2), (2048, 2), (64, 4), (2048, 8)])
def test_producer_without_frozen_positions(n, m):
    """A plan with k = n: the packed u of the producer is channel.fused_info_bits on all n positions, and
    at very low noise the signs of the logits are the encoder output of that u."""
    from polar_amd import _lib, channel, ops
    plan = _lib.Plan(n, np.zeros(n, dtype=np.uint8), 1, flags=_lib.PL_PLAN_GENERIC, device=DEV)
    assert plan.k == n
    rows, seed, it = 70, 1234, 3
    _, ubits, _, llr = ops.awgn_qam_llr(plan, m, rows, 1e-4, seed, it, with_u=False, with_ubits=True)
    u = channel.fused_info_bits(seed, it, np.arange(rows), n)
    assert np.array_equal(ubits.cpu().numpy(), genie_ref.pack_u(u))
    cw = oracle.polar_encode(u, np.zeros(0, np.int64), n)
    assert np.array_equal((llr.cpu().numpy() > 0).astype(np.float32), cw)


def _block_errors(fp, n, k, ebno, rows, m):
    from polar_amd import SC_Dec, _lib, channel

    class GenericSC(SC_Dec):  # SC_Dec on the generic kernel: a designed set has no pre-built specialised one
        def _make_plan(self, dev):
            return _lib.Plan(self.n, self._mask, 1, _lib.PL_F_MINSUM, self.llr_max, flags=_lib.PL_PLAN_GENERIC,
                             device=dev)
    model = channel.FusedAWGN(n, k, fp, GenericSC(fp, n, device=DEV), device=DEV, seed=5, num_bits_per_symbol=m)
    bits, hat = model(rows, ebno)
    return int((bits != hat).any(dim=1).sum())


@pytest.mark.parametrize("m", [2, 4])
def test_designed_code_beats_rm_weight(m):
    """(128,256) designed at 3 dB over 2^17 rows against the pinned RM-weight set, FusedAWGN + SC_Dec over
    2^14 rows at 3 dB; QPSK and 16-QAM (designed with num_bits_per_symbol = 4).  Philox is keyed: the
    counts are the same every run (DESIGN.md section 13 records them)."""
    from polar_amd import design_frozen_pos, reference_frozen_pos
    n, k, ebno = 256, 128, 3.0
    fp = design_frozen_pos(k, n, ebno, rows=2 ** 17, num_bits_per_symbol=m, device=DEV)
    assert fp.dtype == torch.int64 and fp.numel() == n - k and bool((fp[1:] > fp[:-1]).all())
    again = design_frozen_pos(k, n, ebno, rows=2 ** 17, num_bits_per_symbol=m, device=DEV)
    assert torch.equal(fp, again)
    designed = _block_errors(fp, n, k, ebno, 2 ** 14, m)
    rm = _block_errors(reference_frozen_pos(k, n), n, k, ebno, 2 ** 14, m)
    print(f"m={m}: block errors of 16384 at 3 dB: designed {designed}, RM-weight {rm}")
    assert designed < rm


def test_bit_channel_errors_batches():
    """Batches are Philox iterations 0, 1, ...: the total is the sum of the per-batch counts, the last
    batch shorter; rows_done is what was asked for."""
    from polar_amd import _lib, bit_channel_errors, channel, ops
    n, k = 64, 32
    counts, done = bit_channel_errors(n, k, 2.0, 1000, batch=384, seed=9, device=DEV)
    assert done == 1000 and counts.dtype == np.int64 and counts.shape == (n,)
    plan = _lib.Plan(n, np.zeros(n, dtype=np.uint8), 1, flags=_lib.PL_PLAN_GENERIC, device=DEV)
    no = float(channel.ebnodb2no(2.0, 2, k / n))
    tot = torch.zeros(n, dtype=torch.int64, device=DEV)
    for it, bs in enumerate((384, 384, 232)):
        _, ub, _, llr = ops.awgn_qam_llr(plan, 2, bs, no, 9, it, with_u=False, with_ubits=True)
        ops.genie_count(n, llr, ub, counts=tot)
    assert np.array_equal(counts, tot.cpu().numpy()) and counts.sum() > 0


def test_cli_design(capsys):
    from polar_amd import cli
    res = cli.main(["--frozen", "design", "--k", "32", "--n", "64", "--bs", "4096", "--mc_iter", "1", "--design_ebno", "3",
                    "--design_rows", "65536", "--snr_end", "1"])
    out = capsys.readouterr().out
    hashes = re.findall(r"^(\S+): frozen set designed at 3.0 dB over 65536 rows, hash ([0-9a-f]{16}), union bound (\S+)$",
                        out, flags=re.M)
    assert [h[0] for h in hashes] == ["SC", "SCL-8"] and hashes[0][1] == hashes[1][1], out
    assert float(hashes[0][2]) > 0
    assert set(res) == {"SC", "SCL-8"}
