"""Genie-aided SC in plain numpy: the transform pl_genie_count is pinned to.

TEST INFRASTRUCTURE ONLY.  With the true u fed back, the partial sums SC uses at stage s are the
encoder butterfly of u stopped after s - 1 stages, so the n leaf LLRs are a log2 n-stage butterfly
of (f, g) pairs over a = -logits (include/polar_mi355x.h, pl_genie_count):

    beta_0 = u;  beta_s = beta_{s-1} with b[p] ^= b[p + 2^(s-1)] for every p whose index bit s-1 is 0
    for s = S .. 1, h = 2^(s-1), p with bit s-1 clear:
        x, y = a[p], a[p+h];  a[p] = f(x, y);  a[p+h] = g(x, y, beta_{s-1}[p])

f is the reference's min-sum (x_run_sn_polar/polar/polar_sc.py:46: sign(x) sign(y) min(|x|, |y|) on
inputs clipped to +-llr_max, the sign taken from the sign bits so that +-0 behave as the kernels'),
or the exact boxplus restated with correctly rounded exp / log (exactf_cr.f_cr); g is
(1 - 2 beta) x + y in fp32, one rounding (polar_sc.py:49-53).  tests/golden/genie.npz holds the
reference's own msg_llr[:, 0, :] for the min-sum form.
"""
import numpy as np

F32 = np.float32


def f_minsum(x, y, llr_max):
    m = np.minimum(np.minimum(np.abs(x), np.abs(y)), F32(llr_max)).astype(F32)
    sg = (x.view(np.uint32) ^ y.view(np.uint32)) & np.uint32(0x80000000)
    return (m.view(np.uint32) | sg).view(F32)


def g_op(x, y, bit):
    xs = (x.view(np.uint32) ^ (bit.astype(np.uint32) << np.uint32(31))).view(F32)
    with np.errstate(invalid="ignore"):  # inf - inf = NaN (exact f, llr_max > 43, saturated rows), as the reference
        return (xs + y).astype(F32)


def beta_states(u):
    """[S, rows, n] uint8: beta_0 .. beta_{S-1} of u [rows, n] (0/1)."""
    u = (np.asarray(u) != 0).astype(np.uint8)
    n = u.shape[1]
    s_tot = n.bit_length() - 1
    p = np.arange(n)
    out, b = [], u.copy()
    for s in range(1, s_tot + 1):
        out.append(b.copy())
        h = 1 << (s - 1)
        lo = p[(p & h) == 0]
        b[:, lo] ^= b[:, lo + h]
    return np.stack(out) if out else np.zeros((0,) + u.shape, np.uint8)


def leaf_llrs(llr_logits, u, llr_max=30.0, exact=False):
    """Leaf LLRs [rows, n] fp32 (positive favours 0) of genie-aided SC.  With exact=True returns
    (leaf, fragile [rows] bool): f is exactf_cr.f_cr and a row is fragile when any of its f lay so
    near a rounding midpoint that a correct device form may round the other way."""
    a = np.ascontiguousarray(-np.asarray(llr_logits, dtype=F32))
    rows, n = a.shape
    assert n >= 2 and n & (n - 1) == 0
    beta = beta_states(u)
    s_tot = n.bit_length() - 1
    p = np.arange(n)
    fragile = np.zeros(rows, dtype=bool)
    if exact:
        from exactf_cr import f_cr
    for s in range(s_tot, 0, -1):
        h = 1 << (s - 1)
        lo = p[(p & h) == 0]
        x, y = np.ascontiguousarray(a[:, lo]), np.ascontiguousarray(a[:, lo + h])
        if exact:
            f, fr = f_cr(x, y, llr_max)
            fragile |= fr.any(axis=1)
        else:
            f = f_minsum(x, y, llr_max)
        a[:, lo + h] = g_op(x, y, beta[s - 1][:, lo])
        a[:, lo] = f
    return (a, fragile) if exact else a


def hard(leaf):
    """HD(x) = !(x > 0) (polar_sc.py:94-97)."""
    return (~(np.asarray(leaf) > 0)).astype(np.uint8)


def error_counts(leaf, u):
    """int64 [n]: rows whose leaf decision misses u."""
    return (hard(leaf) != (np.asarray(u) != 0)).sum(axis=0).astype(np.int64)


def pack_u(u):
    """[rows, n] 0/1 -> int32 [rows, ceil(n/32)]: bit m % 32 of word m // 32 = position m."""
    u = (np.asarray(u) != 0).astype(np.uint64)
    rows, n = u.shape
    nq = (n + 31) // 32
    pad = np.zeros((rows, nq * 32), dtype=np.uint64)
    pad[:, :n] = u
    w = (pad.reshape(rows, nq, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return w.astype(np.uint32).view(np.int32)


def special_llrs(rng, rows, n):
    """Logit rows with the awkward values: exact zeros, -0, pairwise integer ties, and a x40
    saturated last row (beyond llr_max = 30)."""
    x = (rng.standard_normal((rows, n)) * 2).astype(F32)
    x[rng.random((rows, n)) < 0.15] = F32(0.0)
    x[rng.random((rows, n)) < 0.10] = F32(-0.0)
    t = rows // 3
    x[:t] = np.round(x[:t])  # integer ties (and more zeros of both signs)
    x[-1] = (rng.standard_normal(n) * 40).astype(F32)
    return x
