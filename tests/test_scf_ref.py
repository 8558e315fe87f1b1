"""The numpy restatement of CRC-aided SC-Flip decoding (tests/golden/scf_ref.py) against independent forms:
the committed reference SC rows, the genie butterfly's leaf LLRs, a naive per-row recursive SC that tries
the candidates in turn, and a hand case; the validity of the inputs tests/test_scf_gpu.py compares on; and
the parts of the feature that need no GPU (bindings, argument checks, the Python surface).  CPU only.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import genie_ref  # noqa: E402
import scf_ref  # noqa: E402

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "polar_mi355x.h")


@pytest.mark.parametrize("name", ["sc_16_64", "sc_32_64", "sc_48_64", "sc_128_256", "sc_512_1024"])
def test_max_flips_0_reproduces_the_reference_sc_rows(name):
    """The goldens hold the reference SC decoders' own outputs (bits_*: min-sum, exact_*: the exact f): with
    max_flips = 0 the restatement is SC, whatever the CRC."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as d:
        n, fp = int(d["n"]), d["frozen_pos"].astype(np.int64)
        sets = [(d["llr_" + t][:16], d["bits_" + t][:16], d["exact_" + t][:16])
                for t in ("rand", "zeros", "ties", "sat", "awgn2")]
    for llr, want, want_exact in sets:
        r = scf_ref.scf_decode(llr, fp, n, scf_ref.crc_params("CRC6"), 0)
        assert np.array_equal(r["bits"], want)
        assert (r["flip_pos"] == -1).all() and (r["attempts"] == 1).all()
        if n <= 256:
            rx = scf_ref.scf_decode(llr, fp, n, scf_ref.crc_params("CRC6"), 0, exact=True)
            keep = ~rx["fragile"]
            assert keep.sum() >= 12 and np.array_equal(rx["bits"][keep], want_exact[keep])


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n", [8, 64, 1024])
def test_attempt_0_leaf_llrs_are_the_genie_butterfly(n, exact):
    """alpha_i of attempt 0 == genie_ref.leaf_llrs(x, u^0): the identity the kernel's candidate selection uses."""
    fp = scf_ref.rate_half_frozen(n, 90 + n)
    rows = 6 if exact else 24
    _, x = scf_ref.awgn_rows(n, fp, n, (3, 0b011) if n == 8 else scf_ref.crc_params("CRC11"), rows, 1.0)
    x[-2:] = genie_ref.special_llrs(np.random.default_rng(n), 2, n)
    u0, alpha, _ = scf_ref.sc_flip(x, fp, n, np.full(rows, -1), 30.0, exact)
    leaf = genie_ref.leaf_llrs(x, u0, 30.0, exact)
    leaf = leaf[0] if exact else leaf
    seen = ~np.isnan(alpha)  # leaves of all-frozen nodes are never computed by SC
    info = np.setdiff1d(np.arange(n), fp)
    assert seen[:, info].all()
    assert np.array_equal(alpha[seen].view(np.uint32), leaf[seen].view(np.uint32))


def _naive_sc(a, frozen, flip, llr_max):
    """One row, plain recursion on Python lists of fp32: returns (u, alpha) over all n positions."""
    n = len(a)
    u, alpha = [0] * n, [None] * n

    def f(x, y):
        m = min(abs(x), abs(y), F32(llr_max))
        neg = bool(np.signbit(x)) != bool(np.signbit(y))
        return F32(-m) if neg else F32(m)

    def rec(pos, v):
        if len(v) == 1:
            alpha[pos] = v[0]
            d = 0 if frozen[pos] else (0 if v[0] > 0 else 1)
            if pos == flip:
                d ^= 1
            u[pos] = d
            return [d]
        h = len(v) // 2
        bl = rec(pos, [f(v[j], v[j + h]) for j in range(h)])
        br = rec(pos + h, [F32((-v[j] if bl[j] else v[j]) + v[j + h]) for j in range(h)])
        return [bl[j] ^ br[j] for j in range(h)] + br

    rec(0, [F32(-t) for t in a])
    return u, alpha


def _naive_scf(x, fp, n, crc, T, llr_max=30.0):
    frozen = np.zeros(n, dtype=bool)
    frozen[fp] = True
    info = [i for i in range(n) if not frozen[i]]
    deg, g = crc
    out = []
    for row in x:
        u0, alpha = _naive_sc(list(row), frozen, -1, llr_max)
        bits0 = [u0[i] for i in info]
        tp = min(T, len(info))
        if scf_ref.crc_ok(np.array([bits0]), deg, g)[0]:
            out.append((bits0, True, -1, 1))
            continue
        cands = sorted(info, key=lambda i: (abs(float(alpha[i])), i))[:tp]
        res = (bits0, False, -1, 1 + tp)
        for t, c in enumerate(cands, start=1):
            ut, _ = _naive_sc(list(row), frozen, c, llr_max)
            bits = [ut[i] for i in info]
            if scf_ref.crc_ok(np.array([bits]), deg, g)[0]:
                res = (bits, True, c, 1 + t)
                break
        out.append(res)
    return out


@pytest.mark.parametrize("n,seed,T", [(8, 1, 1), (8, 2, 3), (16, 3, 5), (16, 4, 40)])
def test_brute_force_on_small_codes(n, seed, T):
    fp = scf_ref.rate_half_frozen(n, seed, k=n - 2 if n == 8 else 12)
    crc = (3, 0b011) if n == 8 else scf_ref.crc_params("CRC6")  # x^3 + x + 1 at n = 8 (k = 6)
    _, x = scf_ref.awgn_rows(50 + seed, fp, n, crc, 40, 2.0)
    x[-4:] = genie_ref.special_llrs(np.random.default_rng(seed), 4, n)
    r = scf_ref.scf_decode(x, fp, n, crc, T)
    want = _naive_scf(x, fp, n, crc, T)
    assert np.array_equal(r["bits"], np.array([w[0] for w in want], dtype=np.uint8))
    assert np.array_equal(r["crc_ok"], np.array([w[1] for w in want]))
    assert np.array_equal(r["flip_pos"], np.array([w[2] for w in want]))
    assert np.array_equal(r["attempts"], np.array([w[3] for w in want]))
    assert (r["attempts"] > 1).any() and (r["flip_pos"] >= 0).any()


def test_hand_case_n4():
    """n = 4, position 0 frozen, CRC x + 1 (degree 1, mask 1: the k = 3 bits must have even parity), min-sum.
    a = -logits = (1, 4, 3, -6).  Stage 2: f(1, 3) = 1, f(4, -6) = -4.  Leaf 0 = f(1, -4) = -1: frozen, 0.
    Leaf 1 = g(1, -4, 0) = -3: u1 = 1.  The left half's partial sums are (1, 1): g(1, 3, 1) = 2, g(4, -6, 1) = -10.
    Leaf 2 = f(2, -10) = -2: u2 = 1.  Leaf 3 = g(2, -10, 1) = -12: u3 = 1.  u^0 = (1, 1, 1): odd, the row fails.
    |alpha| = (3, 2, 12) at positions (1, 2, 3): the candidates are 2, 1, 3.  Attempt 1 inverts position 2:
    u2 = 0, leaf 3 = g(2, -10, 0) = -8: u3 = 1, so (1, 0, 1), even: it passes, flip_pos = 2, attempts = 2."""
    n, fp, crc = 4, np.array([0]), (1, 1)
    x = -np.array([[1, 4, 3, -6]], dtype=F32)
    r = scf_ref.scf_decode(x, fp, n, crc, 2)
    assert np.array_equal(r["alpha"][0, 1:], np.array([-3, -2, -12], dtype=F32))
    assert r["cand"][0].tolist() == [2, 1]
    assert r["bits"][0].tolist() == [1, 0, 1] and r["crc_ok"][0]
    assert r["flip_pos"][0] == 2 and r["attempts"][0] == 2
    r0 = scf_ref.scf_decode(x, fp, n, crc, 0)
    assert r0["bits"][0].tolist() == [1, 1, 1] and not r0["crc_ok"][0] and r0["attempts"][0] == 1


def test_crc_register_against_polynomial_division():
    rng = np.random.default_rng(5)
    for name in ("CRC6", "CRC11", "CRC24C"):
        deg, g = scf_ref.crc_params(name)
        msg = (rng.random((5, 40)) < 0.5).astype(np.uint8)
        cw = scf_ref.crc_attach(msg, deg, g)
        assert scf_ref.crc_ok(cw, deg, g).all()
        poly = (1 << deg) | g
        for row in cw:  # the codeword as an integer is a multiple of the generator
            v = int("".join(map(str, row)), 2)
            while v.bit_length() > deg:
                v ^= poly << (v.bit_length() - deg - 1)
            assert v == 0
        cw[:, 3] ^= 1
        assert not scf_ref.crc_ok(cw, deg, g).any()


@pytest.mark.parametrize("n", [2, 4])
def test_tiny_cases_against_the_naive_decoder(n):
    """Every frozen pattern of n = 2 and n = 4 with k >= 1 is there; on every grid row the restatement equals the
    naive per-row decoder; rows fail, rows are rescued, candidates tie, and CRC3 leaves rows no flip rescues."""
    x = scf_ref.tiny_rows(n)
    cases = scf_ref.tiny_cases(n)
    assert {tuple(c[1]) for c in cases} == {tuple(i for i in range(n) if (p >> i) & 1) for p in range((1 << n) - 1)}
    tied = never = 0
    for name, fp, crc_name, T in cases:
        crc = scf_ref.crc_params(crc_name)
        assert T == n - len(fp) >= crc[0]
        r = scf_ref.scf_decode(x, fp, n, crc, T)
        want = _naive_scf(x, fp, n, crc, T)
        assert np.array_equal(r["bits"], np.array([w[0] for w in want], dtype=np.uint8)), name
        assert np.array_equal(r["flip_pos"], np.array([w[2] for w in want])), name
        assert np.array_equal(r["attempts"], np.array([w[3] for w in want])), name
        assert (r["attempts"] > 1).any() and (r["flip_pos"] >= 0).any(), name
        tied += T > 1 and _has_tie(r)
        never += int((~r["crc_ok"]).sum())
    print(f"n={n}: {len(cases)} cases, {tied} with tied candidates, {never} rows never rescued")
    assert (tied > 0 and never > 0) or n == 2  # n = 2: CRC1 alone, and no failing row of the k = 2 code ties


@pytest.mark.parametrize("case", scf_ref.CRC_TABLE_CASES, ids=[c[0] for c in scf_ref.CRC_TABLE_CASES])
def test_crc_table_inputs(case):
    """Every row fails attempt 0; rows 0 ... 7 are rescued by the flip at position 0 (information rank 0) and
    decode to the sent bits, u_0 = 1 in some; the noise rows are never rescued."""
    fp, crc, x, sent = scf_ref.crc_table_inputs(case)
    name, n, k = case[:3]
    assert n - len(fp) == k <= 1024 and 0 not in fp and len(x) <= 16
    r = scf_ref.scf_decode(x, fp, n, crc, scf_ref.CRC_TABLE_FLIPS)
    assert (r["attempts"] > 1).all()
    assert (r["flip_pos"][:8] == 0).all() and (r["attempts"][:8] == 2).all() and np.array_equal(r["bits"][:8], sent)
    assert (sent[:4, 0] == 1).all() and (sent[4:, 0] == 0).all()
    assert not r["crc_ok"][8:].any() and not r["fragile"].any()


def _classes(r):
    first = int(r["crc_ok"].sum() - (r["flip_pos"] >= 0).sum())
    return first, int((r["flip_pos"] >= 0).sum()), int((~r["crc_ok"]).sum())


def _has_tie(r):
    """Some failing row has equal |alpha| at two of its candidates."""
    for row in np.flatnonzero(r["cand"][:, :1].ravel() >= 0) if r["cand"].shape[1] else []:
        mag = np.abs(r["alpha"][row, r["cand"][row]])
        if len(np.unique(mag)) < len(mag):
            return True
    return False


@pytest.mark.parametrize("case", scf_ref.MINSUM_CASES, ids=[c[0] for c in scf_ref.MINSUM_CASES])
def test_minsum_gpu_inputs_are_valid(case):
    fp, crc, x = scf_ref.case_inputs(case)
    n, T = case[1], case[4]
    r = scf_ref.scf_decode(x, fp, n, crc, T)
    cls = _classes(r)
    print(case[0], "passes at 0 / rescued / never:", cls, "ties:", _has_tie(r))
    assert min(cls) > 0, cls
    assert not r["fragile"].any()


def test_minsum_gpu_inputs_have_exact_ties():
    tied = [c[0] for c in scf_ref.MINSUM_CASES if c[4] > 1 and _has_tie(scf_ref.scf_decode(*_args(c)))]
    print("cases with exact |alpha| ties among the candidates:", tied)
    assert len(tied) >= 3


def _args(case):
    fp, crc, x = scf_ref.case_inputs(case)
    return x, fp, case[1], crc, case[4]


@pytest.mark.parametrize("case", scf_ref.EXACT_CASES, ids=[c[0] for c in scf_ref.EXACT_CASES])
def test_exact_gpu_inputs_are_valid_and_fragile_rows_few(case):
    """A row at n = 256 with 16 attempts evaluates about 17 x 1024 f, each with five roundings and a 2^-27-ulp
    window: far fewer than one fragile row in 67 is expected; the GPU test leaves fragile rows out, so their
    number is capped here (another seed, never a higher cap)."""
    fp, crc, x = scf_ref.case_inputs(case)
    r = scf_ref.scf_decode(x, fp, case[1], crc, case[4], llr_max=case[6], exact=True)
    cls = _classes(r)
    print(case[0], "classes:", cls, "fragile rows:", int(r["fragile"].sum()), "of", scf_ref.ROWS)
    assert r["fragile"].sum() <= scf_ref.FRAGILE_CAP
    assert min(cls) > 0, cls


def test_bindings_and_argument_checks_without_a_gpu():
    from polar_amd import _lib
    assert "pl_scf_decode" in _lib.EXPORTED_SYMBOLS and "pl_scf_workspace_size" in _lib.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert "int pl_scf_decode(const pl_plan* plan" in text and "size_t pl_scf_workspace_size(const pl_plan* plan" in text
    L = _lib.lib()
    assert L.pl_scf_workspace_size(None, 16, 4) == 0
    buf = (ctypes.c_uint8 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = L.pl_scf_decode(None, p, 1, 4, p, _lib.PL_OUT_U8, None, None, None, p, 16, None)
    assert rc == _lib.PL_EINVAL and b"plan" in L.pl_last_error_string()
    with pytest.raises(_lib.PolarArgumentError, match="plan"):
        _lib.check(rc, "pl_scf_decode")


def test_python_surface_argument_errors():
    import polar_amd
    from polar_amd import cli
    from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
    assert "SCF_Dec" in polar_amd.__all__ and callable(polar_amd.ops.scf_decode)
    fp = np.arange(32)
    with pytest.raises(ValueError, match="CRC"):
        polar_amd.SCF_Dec(fp, 64, None)
    with pytest.raises(ValueError):
        polar_amd.SCF_Dec(fp, 64, "CRC7")
    with pytest.raises(ValueError, match="f must be"):
        polar_amd.SCF_Dec(fp, 64, "CRC6", f="maxlog")
    for bad in (-1, 65, 2.5):
        with pytest.raises(ValueError, match="max_flips"):
            polar_amd.SCF_Dec(fp, 64, "CRC6", max_flips=bad)
    with pytest.raises(ValueError, match="not supported"):
        polar_amd.SCF_Dec(np.arange(1024), 2048, "CRC11")
    with pytest.raises(ValueError, match="too small"):
        polar_amd.SCF_Dec(np.arange(60), 64, "CRC6")
    d = polar_amd.SCF_Dec(fp, 64, "CRC6", max_flips=0)
    assert (d.n, d.k, d.k_crc, d.max_flips) == (64, 32, 6, 0) and d.last_attempts is None
    enc = Polar5GEncoder(40, 128)
    dec = Polar5GDecoder(enc, dec_type="SCF", list_size=8, return_crc_status=True)
    assert isinstance(dec.polar_dec, polar_amd.SCF_Dec) and dec.polar_dec.max_flips == 8
    assert dec.polar_dec.k == enc.k_polar and dec.polar_dec.f == "exact"
    with pytest.raises(ValueError, match="max_flips"):
        Polar5GDecoder(enc, dec_type="SCF", list_size=128)
    with pytest.raises(ValueError, match="hybrid_sc"):
        Polar5GDecoder(enc, dec_type="SCF", hybrid_sc=True)
    c = cli.parse(["--code", "5g", "--k", "40", "--n", "128", "--algos", "[scf]", "--scf_flips", "4", "--scf_f", "minsum"])
    assert c.scf_flips == 4 and c.scf_f == "minsum"
    assert cli.parse(["--code", "5g", "--algos", "[scf]"]).scf_flips == 16
    for argv in (["--algos", "[scf]"], ["--code", "5g", "--algos", "[scf]", "--scf_flips", "65"],
                 ["--code", "5g", "--algos", "[scf]", "--scf_flips", "-1"]):
        with pytest.raises(SystemExit):
            cli.parse(argv)
