"""Ordered-statistics decoding without a GPU: the numpy restatement against the reference's recorded
results, OSDecoder's constructor checks, the argument checks of pl_osd_plan_create (they run before
any HIP call) and the command-line options."""
import ctypes
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import osd_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "osd.npz")


class DenseEncoder:
    def __init__(self, g, k="shape"):
        self.g = torch.tensor(np.asarray(g, dtype=np.float32))
        self.k = int(self.g.shape[0]) if k == "shape" else k

    def __call__(self, u):
        return (u @ self.g) % 2


def _names():
    with np.load(GOLDEN) as d:
        return [str(s) for s in d["sets"]]


def test_fixture_sets_are_the_ones_the_decoder_is_specified_on():
    assert _names() == ["k16n32t0", "k16n32t1", "k16n32t2", "k16n32t3", "k32n64t2", "k64n128t1", "k64n128t2",
                        "k65n130t1", "k3n7t3", "k1n2t1", "k8n8t1"]
    rows = {"k16n32": 256, "k32n64": 256, "k64n128": 128, "k65n130": 64, "k3n7": 64, "k1n2": 32, "k8n8": 32}
    with np.load(GOLDEN) as d:
        for name in _names():
            llr = d[name + "_llr"]
            assert llr.shape[0] == rows[name.split("t")[0]], name
            mag = np.abs(llr)
            assert mag.max() < 100 and all(len(np.unique(r)) == llr.shape[1] for r in mag), name


@pytest.mark.parametrize("name", _names())
def test_restatement_equals_the_reference(name):
    with np.load(GOLDEN) as d:
        g, llr, ref_cw, ref_d = (d[f"{name}_{f}"] for f in ("G", "llr", "cw", "d"))
    t = int(name.split("t")[-1])
    cw, dist, pattern, gap = osd_ref.osd_decode(g, llr, t)
    assert np.array_equal(cw, ref_cw)
    assert gap.min() > 1e-9
    assert np.all(np.abs(dist - ref_d) <= 256 * 2.0 ** -24 * np.abs(ref_d))
    assert pattern.min() >= -1 and pattern.max() < max(1, sum(math.comb(g.shape[0], i) for i in range(1, t + 1)))
    # chunking the batch does not change a row
    cw2, dist2, pattern2, _ = osd_ref.osd_decode(g, llr[:40], t, chunk_elems=1)
    assert np.array_equal(cw2, cw[:40]) and np.array_equal(pattern2, pattern[:40])


def test_restatement_tie_order_is_lower_index_first():
    # two equally reliable positions, one information bit: the pivot is the lower index
    g = np.array([[1, 1, 1]], dtype=np.uint8)
    basis, idx, ls = osd_ref.most_reliable_basis(g, np.array([[2.0, -2.0, 1.0]], dtype=np.float32))
    assert idx[0].tolist() == [0, 1, 2] and ls[0, 0] == 2.0
    cw, _, pattern, _ = osd_ref.osd_decode(g, np.array([[-0.0, 0.0, 0.0]], dtype=np.float32), 1)
    assert cw.tolist() == [[0, 0, 0]] and pattern.tolist() == [-1]  # zero decides 0; a tie in Delta keeps c0


def test_constructor_checks():
    from polar_amd import OSDecoder
    g = np.eye(4, 8, dtype=np.uint8)
    g[:, 4:] = 1
    enc = DenseEncoder(g)
    dec = OSDecoder(t=2, encoder=enc)
    assert (dec.k, dec.n, dec.t, dec.n_patterns) == (4, 8, 2, 10)
    assert dec.gm.dtype == torch.float32 and np.array_equal(dec.gm.numpy(), g)
    assert OSDecoder(t=1, encoder=enc, dtype=torch.float64).gm.dtype == torch.float64
    assert OSDecoder(t=2.0, encoder=enc).t == 2
    with pytest.raises(ValueError):
        OSDecoder(t=1, encoder=enc, dtype=torch.int32)
    with pytest.raises(AssertionError):
        OSDecoder(t=1.5, encoder=enc)
    with pytest.raises(AttributeError):
        OSDecoder(t=1, encoder=DenseEncoder(g, k=None))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):  # no CPU decoder behind it
            dec(torch.zeros(2, 8))


def test_envelope_errors_at_construction():
    from polar_amd import OSDecoder
    from polar_amd.osd import check_supported
    rng = np.random.default_rng(0)

    def systematic(k, n):
        return np.concatenate([np.eye(k, dtype=np.uint8), rng.integers(0, 2, (k, n - k)).astype(np.uint8)], axis=1)
    for k, n, t in ((129, 256, 1), (64, 257, 1), (64, 128, 5), (3, 7, 4), (128, 256, 4), (16, 32, -1)):
        with pytest.raises(ValueError, match="128"):
            OSDecoder(t=t, encoder=DenseEncoder(systematic(k, n)))
    check_supported(128, 256, 3)
    check_supported(64, 128, 4)
    check_supported(1, 1, 1)
    deficient = systematic(8, 16)
    deficient[5] = deficient[2] ^ deficient[3]
    with pytest.raises(ValueError, match="rank"):
        OSDecoder(t=1, encoder=DenseEncoder(deficient))


def _create(k, n, gm, t, out=True):
    from polar_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    ptr = gm.ctypes.data_as(ctypes.c_void_p) if gm is not None else None
    rc = L.pl_osd_plan_create(ctypes.byref(h) if out else None, k, n, ptr, t)
    return rc, L.pl_last_error_string().decode(), h


def test_plan_create_argument_checks_without_gpu():
    from polar_amd import _lib
    g = np.concatenate([np.eye(16, dtype=np.uint8), np.ones((16, 16), dtype=np.uint8)], axis=1)
    rc, msg, _ = _create(16, 32, None, 1)
    assert rc == _lib.PL_EINVAL and "gm" in msg
    rc, msg, _ = _create(16, 32, g, 1, out=False)
    assert rc == _lib.PL_EINVAL and "out" in msg
    for args, name in (((-1, 32, g, 1), "k"), ((16, -2, g, 1), "n"), ((16, 32, g, -1), "t")):
        rc, msg, _ = _create(*args)
        assert rc == _lib.PL_EINVAL and f" {name} is negative" in msg, (args[:2], msg)
    big = np.concatenate([np.eye(129, dtype=np.uint8), np.zeros((129, 200), dtype=np.uint8)], axis=1)
    for args in ((129, 256, big, 1), (0, 32, g, 0), (16, 257, g, 1), (16, 15, g, 1), (16, 32, g, 5),
                 (2, 32, g, 3)):
        rc, msg, _ = _create(*args)
        assert rc == _lib.PL_ENOTSUP and "envelope" in msg, (args[0], args[1], args[3], rc, msg)
    # the 2^22 cap: sum C(128, i), i <= 4 = 11017632 patterns
    g128 = np.concatenate([np.eye(128, dtype=np.uint8), np.ones((128, 128), dtype=np.uint8)], axis=1)
    rc, msg, _ = _create(128, 256, g128, 4)
    assert rc == _lib.PL_ENOTSUP and "2^22" in msg
    # a generator matrix whose rows are dependent
    bad = g.copy()
    bad[7] = bad[1] ^ bad[2]
    rc, msg, _ = _create(16, 32, bad, 1)
    assert rc == _lib.PL_EINVAL and "rank" in msg
    rc, msg, _ = _create(16, 32, np.zeros((16, 32), dtype=np.uint8), 0)
    assert rc == _lib.PL_EINVAL and "rank" in msg
    L = _lib.lib()
    assert L.pl_osd_plan_info(None, None, None, None, None) == _lib.PL_EINVAL
    assert L.pl_osd_decode(None, None, 0, None, 0, None, None, None) == _lib.PL_EINVAL
    assert L.pl_osd_plan_destroy(None) == _lib.PL_OK


@pytest.mark.parametrize("k,n,t", [(1, 2, 1), (3, 7, 3), (16, 32, 0), (32, 64, 3), (64, 128, 4), (128, 256, 3),
                                   (65, 130, 1)])
def test_plan_info_pattern_counts(k, n, t):
    """The plan's pattern count is sum C(k, i), i = 1 .. t (a plan made where there is no GPU answers
    pl_osd_plan_info and nothing else)."""
    from polar_amd import _lib
    g = np.concatenate([np.eye(k, dtype=np.uint8), np.ones((k, n - k), dtype=np.uint8)], axis=1)
    plan = _lib.OsdPlan(g, t)
    assert (plan.k, plan.n, plan.t) == (k, n, t)
    assert plan.n_patterns == sum(math.comb(k, i) for i in range(1, t + 1))
    if not torch.cuda.is_available():
        L = _lib.lib()
        x = np.zeros((1, n), dtype=np.float32)
        rc = L.pl_osd_decode(plan.handle, x.ctypes.data_as(ctypes.c_void_p), 1, x.ctypes.data_as(ctypes.c_void_p), 0,
                             None, None, None)
        assert rc == _lib.PL_EHIP and b"without a GPU" in L.pl_last_error_string()
        assert L.pl_osd_decode(plan.handle, None, 0, None, 0, None, None, None) == _lib.PL_OK  # bs == 0


def test_cli_parses_osd_options(capsys):
    from polar_amd import cli
    c = cli.parse(["--algos", "[osd]", "--osd_t", "3"])
    assert c.algos == ["osd"] and c.osd_t == 3
    assert cli.parse(["--algos", "[scl,osd]"]).osd_t == 2
    assert cli.parse([]).osd_t == 2 and "osd" not in cli.parse([]).algos
    cli.parse(["--k", "512", "--n", "1024"])  # no OSD leg: nothing to check
    for bad in (["--k", "512", "--n", "1024"], ["--osd_t", "5"], ["--k", "128", "--n", "256", "--osd_t", "4"],
                ["--code", "5g"]):
        with pytest.raises(SystemExit):  # an argparse error that names the limits
            cli.parse(["--algos", "[osd]"] + bad)
        if bad[0] != "--code":
            assert "k <= 128" in capsys.readouterr().err


def test_harness_dense_encoder_builds_the_code():
    """channel.DenseEncoder (the reference harness encoder) carries .k, and the G OSDecoder builds from it
    is the information rows of the polar transform."""
    import polar_amd
    from polar_amd import OSDecoder, channel, frozen
    fp = polar_amd.reference_frozen_pos(32, 64)
    big_g = frozen.get_Kern_frozen_bits(64, 32, frozen.F2)[0]
    enc = channel.DenseEncoder(fp, 64, big_g)
    assert enc.k == 32
    dec = OSDecoder(t=2, encoder=enc)
    info = np.setdiff1d(np.arange(64), fp.numpy())
    assert (dec.k, dec.n) == (32, 64)
    assert np.array_equal(dec.gm.numpy(), (big_g.numpy()[info] % 2).astype(np.float32))


def test_cli_builds_the_osd_leg_on_the_cpu_llr_path():
    """gen_code with --llr_device cpu: the op-by-op model around an OSDecoder built from the dense
    encoder, comparing codewords (no GPU needed to construct it)."""
    from polar_amd import OSDecoder, channel, cli
    c = cli.parse(["--algos", "[osd]", "--llr_device", "cpu", "--osd_t", "1"])
    model, name = cli.gen_code(c, "OSD-1 (codeword BER)", "osd", torch.device("cpu"))
    assert isinstance(model, channel.System_AWGN_model) and model.cw_estimates
    assert isinstance(model.decoder, OSDecoder) and (model.decoder.k, model.decoder.n, model.decoder.t) == (32, 64, 1)
    assert "codeword BER" in name
    bits, codewords, llr = model.llrs(5, 2.0)
    assert codewords.shape == (5, 64) and llr.shape == (5, 64)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):  # decoding itself needs the GPU
            model(5, 2.0)


def _assert_packed_equals_dense(g, llr, t, exact):
    cw, dist, pattern, gap = osd_ref.osd_decode(g, llr, t)
    cw2, dist2, pattern2, gap2 = osd_ref.osd_decode_packed(g, llr, t)
    assert np.array_equal(cw2, cw) and np.array_equal(pattern2, pattern)
    assert cw2.dtype == cw.dtype and pattern2.dtype == pattern.dtype and dist2.dtype == np.float64
    assert np.allclose(dist2, dist, rtol=1e-12, atol=0)
    assert np.array_equal(gap2[exact], gap[exact])  # every Delta of these rows is exact: the same gap
    both = np.isfinite(gap)
    assert np.array_equal(both, np.isfinite(gap2))
    assert np.all(np.abs(gap2[both] - gap[both]) <= 1e-12)


@pytest.mark.parametrize("name", _names())
def test_packed_search_equals_the_dense_one_on_the_fixtures(name):
    with np.load(GOLDEN) as d:
        g, llr = d[name + "_G"], d[name + "_llr"]
    _assert_packed_equals_dense(g, llr, int(name.split("t")[-1]), np.zeros(len(llr), dtype=bool))


@pytest.mark.parametrize("k,n,t", [(10, 20, 2), (8, 16, 3), (12, 24, 4), (24, 33, 4), (16, 40, 2), (70, 130, 2)])
def test_packed_search_equals_the_dense_one_on_tie_rows(k, n, t):
    rng = np.random.default_rng(200 + n)
    g = osd_ref.random_full_rank(k, n, rng)
    llr = osd_ref.tie_rows(n, rng)
    _assert_packed_equals_dense(g, llr, t, np.ones(len(llr), dtype=bool))
    # a block boundary inside an order changes nothing
    a, b = osd_ref.osd_decode_packed(g, llr[:9], t), osd_ref.osd_decode_packed(g, llr[:9], t, block=7)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_packed_patterns_are_the_combinations():
    for k, i in ((5, 1), (6, 3), (9, 4), (4, 4)):
        p = osd_ref.packed_patterns(k, i)
        assert p.tolist() == [list(c) for c in itertools.combinations(range(k), i)]
    assert len(osd_ref.packed_patterns(3, 4)) == 0


def test_the_2_22_cap_is_at_k_100_for_order_4():
    """(100, 104, 4) with 4 087 975 patterns is the largest order-4 search; k = 101 (4 254 726) is refused."""
    from polar_amd.osd import check_supported
    assert sum(math.comb(100, i) for i in range(1, 5)) == 4087975 <= 1 << 22 < sum(math.comb(101, i) for i in range(1, 5))
    check_supported(100, 104, 4)
    with pytest.raises(ValueError):
        check_supported(101, 104, 4)


def _lane_starts(k, t):
    """(per, the lane whose first pattern is the first of order i, for i = 2 .. t; None where no lane's is):
    the kernel gives lane l the patterns l * per .. (l + 1) * per - 1, per = ceil(n_patterns / 64)."""
    counts = [math.comb(k, i) for i in range(1, t + 1)]
    per = -(-sum(counts) // 64)
    starts = np.cumsum(counts)[:-1]
    return per, [int(s // per) if s % per == 0 else None for s in starts]


# What the seeds of osd_ref.ENVELOPE_CASES give: the number of rows won by c0 and by each order 1 .. t.
# Two cases cannot meet "every order wins somewhere", whatever the input:
#   * k128n128t2 has no redundant position.  c0 is the hard decision of every position, every a_j is
#     <= 0 and every Delta >= 0, so c0 wins every row: the case checks the elimination at rate 1, the
#     search only in that no pattern may win.
#   * k100n104t4 has four redundant positions.  A pattern J wins only if, for every non-empty R within J,
#     the redundant positions of the sum of the rows R outweigh the pivots of R (else J without R is at
#     least as good and comes first).  A redundant position is less reliable than every pivot whose row
#     reaches it.  Four rows restricted to four positions are dependent, and some R gains nothing, or
#     a basis, and some R sums to a single position, which does not outweigh R.  So no pattern of order
#     4 can win at n - k = 4; order 2 is the highest found in a search over seeds, and the order-4
#     patterns are checked in that 3 921 225 of them must lose.
ENVELOPE_WINNERS = {
    "k10n20t2": [80, 34, 10],
    "k8n16t3": [92, 27, 6, 2],
    "k12n24t4": [66, 45, 14, 1, 3],
    "k24n33t4": [66, 46, 15, 1, 1],
    "k40n200t3": [5, 16, 35, 70],
    "k66n97t3": [28, 39, 36, 23],
    "k70n130t2": [12, 46, 66],
    "k128n128t2": [124, 0, 0],
    "k16n40t2_structured": [90, 27, 7],
    "k16n40t2_structured_permuted": [85, 31, 8],
    "k64n128t4": [0, 1, 0, 2, 1],
    "k128n256t3": [1, 1, 1, 1],
    "k100n104t4": [2, 1, 1, 0, 0],
}


@pytest.mark.parametrize("name", list(osd_ref.ENVELOPE_CASES))
def test_envelope_inputs_meet_their_conditions(name):
    """The inputs of tests/test_osd_envelope_gpu.py, judged by the restatement alone: which orders win,
    the margin of every row that is not exact in fp64, the shapes' lane-boundary facts."""
    g, t, llr, exact = osd_ref.envelope_case(name)
    k, n = g.shape
    corner = name in osd_ref.ENVELOPE_CORNERS
    assert osd_ref.gf2_rank(g) == k
    assert (len(llr), exact.sum()) == (4, 0) if corner else ((~exact).sum() >= 48 and exact.sum() == 73)
    cw, dist, pattern, gap = (osd_ref.osd_decode_packed if corner else osd_ref.osd_decode)(g, llr, t)
    hist = np.bincount(osd_ref.winner_orders(pattern, k, t), minlength=t + 1).tolist()
    print(name, "rows", len(llr), "winner orders", hist, "min gap", float(gap[~exact].min()))
    assert hist == ENVELOPE_WINNERS[name]
    assert gap[~exact].min() > 1e-9
    if name == "k128n128t2":
        assert hist[0] == len(llr)
    elif name == "k100n104t4":
        assert hist[0] > 0 and hist[1] > 0 and hist[2] > 0
    elif corner:
        assert hist[t] > 0
    else:
        assert all(h > 0 for h in hist)
    if name == "k10n20t2":  # per == 1, lanes 55 .. 63 idle, lane 10 starts order 2 and its pattern wins a row
        assert _lane_starts(k, t) == (1, [10]) and math.comb(10, 1) + math.comb(10, 2) == 55 < 64
        assert 10 in pattern
    if name == "k8n16t3":  # per == 2, lane 4 starts order 2 (its pattern wins a row), lane 18 order 3
        assert _lane_starts(k, t) == (2, [4, 18]) and 8 in pattern
    if name.startswith("k16n40t2_structured"):
        cols = {c.tobytes() for c in g.T}
        assert (g.sum(0) == 0).sum() == 8 and len(cols) == 17  # 8 zero columns, 16 columns repeated
        dependent = [osd_ref.gf2_rank(g[:, np.argsort(-np.abs(np.clip(r, -100, 100)), kind="stable")[:k]]) < k for r in llr]
        assert sum(dependent) > len(llr) // 2  # the first k sorted columns do not span: the pivots skip
    if name in ("k66n97t3", "k70n130t2", "k128n256t3", "k100n104t4"):  # rows past lane 63's first slot take part
        members = [osd_ref.packed_patterns(k, o)[p - sum(math.comb(k, i) for i in range(1, o))]
                   for o, p in zip(osd_ref.winner_orders(pattern, k, t), pattern) if o > 0]
        assert max(int(m.max()) for m in members) > 63
