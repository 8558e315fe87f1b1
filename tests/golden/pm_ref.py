"""Plain restatement of the generic list decoder's path metrics, with the error budget of every
operation propagated next to its value (tests/test_pm_ref.py, tests/test_pm_ulp_gpu.py).

One decoder skeleton (decode) runs over three arithmetics:
  MpArith   mpmath at 80 digits, the reference: softplus = log1p(exp z), the boxplus in the
            reference's own form log(1 + e^(x+y)) - log(e^x + e^y) on the clipped inputs;
  LdArith   numpy.longdouble, the stable forms (sign (m + log1p(-t)), z + log1p(exp -z)): an
            independent evaluation that guards the generator against a slip;
  DevArith  an fp64 transcription of csrc/softplus.h (Cody-Waite, the economised polynomials, the
            2^(j/64) table, the atanh series) with knobs that damage it: the power check.
A value travels as (v, d): v in the arithmetic's own number type, d the bound (a float) on
|device - v| that the budgets below allow.  No pruning of the tree unless fast=True (fast-SCL:
rate-0 and repetition nodes summed in numpy's pairwise order).

Budgets (absolute; d inherited from the inputs):
  min-sum f, clip, sign   exact; f inherits max(dx, dy) (the d of the smaller magnitude alone where
                          the other cannot be the smaller one; a value beyond the clip by more
                          than its d clips exactly, d = 0)
  g = y +- x              dx + dy + ulp(g)/2 (the device rounds once; the reference rounds too
                          when both inputs are fp64 numbers, and then equals the device)
  exact f                 dx + dy + 2 ulp(max(|f|, 1))
  softplus(z)             dz + 2^-51 + 2 ulp(result)
  every metric addition   ulp(sum)/2
  the stored metric       ulp/2, the fixture's own rounding of the mpmath value to fp64
"""
import ctypes
import ctypes.util
import math

import mpmath as mp
import numpy as np

DPS = 80
BIG = 1.0e6  # "far beyond the clip" for every llr_max <= 700


def ulp(x):
    return math.ulp(abs(float(x)))


# ------------------------------------------------------------------ arithmetics ----
class MpArith:
    name = "mp"

    def num(self, x):
        return mp.mpf(float(x))

    def is64(self, v):
        return mp.mpf(float(v)) == v

    def round64(self, v):
        return mp.mpf(float(v))

    def softplus(self, z):
        return mp.log1p(mp.exp(z))

    def f_exact(self, x, y, lmax):
        xc, yc = min(max(x, -lmax), lmax), min(max(y, -lmax), lmax)
        return mp.log(1 + mp.exp(xc + yc)) - mp.log(mp.exp(xc) + mp.exp(yc))


class LdArith:
    name = "ld"
    T = np.longdouble

    def num(self, x):
        return self.T(float(x))

    def is64(self, v):
        return self.T(np.float64(v)) == v

    def round64(self, v):
        return self.T(np.float64(v))

    def softplus(self, z):
        return z + np.log1p(np.exp(-z)) if z > 0 else np.log1p(np.exp(z))

    def f_exact(self, x, y, lmax):
        a, b = min(abs(x), lmax), min(abs(y), lmax)
        m, M = min(a, b), max(a, b)
        E = np.exp(-(M - m))
        G = -np.expm1(-2 * m)
        v = m + np.log1p(-(E * G / (1 + E)))
        return -v if (x < 0) != (y < 0) else v


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = _libm.fma

# csrc/softplus.h: kSpP, kSpRL, kS and the constants of the two reductions
_SPP = [0.5000000000000001, 0.1666666666666667, 0.04166666666662413, 0.008333333333326136, 0.001388888891721154,
        0.00019841269874817515, 2.4801521299750923e-05, 2.75572554044176e-06, 2.7620086491464514e-07,
        2.5105215165649368e-08]
_SPRL = [0.666666666666667, 0.39999999999898955, 0.2857142862619623, 0.22222211102348335, 0.18182891280109284,
         0.15331655663402047, 0.14617206088074544]
_KS = [0.6666666666666666, 0.39999999999999514, 0.28571428571603413, 0.22222222197853667, 0.18181819920440906,
       0.15384543207664578, 0.133351941539121, 0.11734082174871642, 0.10846687166200544, 0.07485743922141379,
       0.1564211337480669]
_LOG2E = 1.4426950408889634
_LN2HI, _LN2LO = float.fromhex("0x1.62e42fefa39efp-1"), float.fromhex("0x1.abc9e3b39803fp-56")
_KINV = float.fromhex("0x1.71547652b82fep+6")
_CHI, _CLO = float.fromhex("0x1.62e42fefa39efp-7"), float.fromhex("0x1.abc9e3b39803fp-62")


def _tab64():
    with mp.workdps(40):
        return [float(mp.power(2, mp.mpf(j) / 64)) for j in range(64)]


class DevArith:
    """softplus_pm (PL_SP_FORM 2) and f_exact_pm_n of csrc/softplus.h in host fp64 with a true
    fma; the reciprocal is the host's division (the device's Newton-corrected quotient is the
    correctly rounded one on all but a 2^-97 fraction of inputs).  tab_mut = (j, rel), ks_mut =
    (i, delta), exp_ulps damage one table entry, one series coefficient, the penalty's exp."""
    name = "dev"

    def __init__(self, tab_mut=None, ks_mut=None, exp_ulps=0):
        self.tab = _tab64()
        self.ks = list(_KS)
        if tab_mut:
            self.tab[tab_mut[0]] *= 1.0 + tab_mut[1]
        if ks_mut:
            self.ks[ks_mut[0]] += ks_mut[1]
        self.exp_ulps = exp_ulps

    def num(self, x):
        return float(x)

    def is64(self, v):
        return True

    def round64(self, v):
        return v

    def _exp(self, z):
        k = float(round(z * _LOG2E))
        r = _fma(-k, _LN2HI, z)
        r = _fma(-k, _LN2LO, r)
        r2 = r * r
        P = _SPP
        a, b, c = _fma(P[9], r, P[8]), _fma(P[7], r, P[6]), _fma(P[5], r, P[4])
        d, e = _fma(P[3], r, P[2]), _fma(P[1], r, P[0])
        r4 = r2 * r2
        ab, cd = _fma(a, r2, b), _fma(c, r2, d)
        p = _fma(_fma(ab, r4, cd), r2, e)
        v = math.ldexp(_fma(r2, p, r) + 1.0, int(k))
        return v + self.exp_ulps * math.ulp(v)

    def _log(self, y):
        m, e = math.frexp(y)
        if m < 0.70710678118654752:
            m, e = m + m, e - 1
        f = m - 1.0
        den = 2.0 + f
        s = f / den
        z = s * s
        R = _SPRL
        p01, p23, p45 = _fma(R[1], z, R[0]), _fma(R[3], z, R[2]), _fma(R[5], z, R[4])
        z2 = z * z
        z4 = z2 * z2
        r = _fma(_fma(R[6], z2, p45), z4, _fma(p23, z2, p01))
        lm = _fma(s * z, r, s + s)
        de = float(e)
        return _fma(de, _LN2HI, _fma(de, _LN2LO, lm))

    def softplus(self, z):
        return self._log(1.0 + self._exp(z))

    def _fex(self, z):
        t = _fma(z, _KINV, 6755399441055744.0)
        nd = t - 6755399441055744.0
        n = int(nd)
        r = _fma(-nd, _CHI, z)
        r = _fma(-nd, _CLO, r)
        h = _fma(1.0 / 120.0, r, 1.0 / 24.0)
        h = _fma(h, r, 1.0 / 6.0)
        h = _fma(h, r, 0.5)
        return math.ldexp(self.tab[n & 63], n >> 6), _fma(r * r, h, r)

    def f_exact(self, x, y, lmax):
        a, b = min(abs(x), lmax), min(abs(y), lmax)
        m, M = min(a, b), max(a, b)
        Ae, qe = self._fex(max(m - M, -2000.0))
        Am, qm = self._fex(max(-2.0 * m, -2000.0))
        E = _fma(Ae, qe, Ae)
        G = _fma(-Am, qm, 1.0 - Am)
        eg = E * G
        den = _fma(2.0, E, 2.0) - eg
        s = -(eg / den)
        w = s * s
        R = self.ks[10]
        for c in range(9, -1, -1):
            R = _fma(R, w, self.ks[c])
        v = m + _fma(s * w, R, s + s)
        return -v if (math.copysign(1.0, x) < 0) != (math.copysign(1.0, y) < 0) else v


# --------------------------------------------------------------------- decoder ----
def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + 0.5 * ulp(v)


def pairwise_sum(t):
    """numpy's pairwise order (np.sum over a contiguous last axis; oracle.np_pairwise_sum)."""
    n = len(t)
    if n < 8:
        r = t[0]
        for x in t[1:]:
            r = _add(r, x)
        return r
    if n <= 128:
        r = list(t[:8])
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = _add(r[j], t[i + j])
            i += 8
        res = _add(_add(_add(r[0], r[1]), _add(r[2], r[3])), _add(_add(r[4], r[5]), _add(r[6], r[7])))
        for x in t[i:]:
            res = _add(res, x)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _add(pairwise_sum(t[:n2]), pairwise_sum(t[n2:]))


class _Ctx:
    def __init__(self, ar, n, f_mode, lmax):
        self.ar, self.n, self.S, self.f_mode = ar, n, n.bit_length() - 1, f_mode
        self.lmax_f, self.lmax = float(lmax), ar.num(lmax)

    def clipd(self, v, d):  # the budget after the clip: a value beyond it by more than d clips exactly
        return 0.0 if float(abs(v)) - d > self.lmax_f else d

    def f(self, a, b):
        (x, dx), (y, dy) = a, b
        dx, dy = self.clipd(x, dx), self.clipd(y, dy)
        if self.f_mode == 0:
            ax, ay = min(abs(x), self.lmax), min(abs(y), self.lmax)
            m = min(ax, ay)
            # the larger magnitude matters only where it may be the smaller one on the device
            d = dx if ax < ay else dy
            if float(abs(ax - ay)) <= dx + dy:
                d = max(dx, dy)
            return (-m if (x < 0) != (y < 0) else m), d
        v = self.ar.f_exact(x, y, self.lmax)
        return v, dx + dy + 2.0 * ulp(max(abs(float(v)), 1.0))

    def g(self, a, b, bit):
        (x, dx), (y, dy) = a, b
        v = (-x if bit else x) + y
        if self.ar.is64(x) and self.ar.is64(y):
            v = self.ar.round64(v)
        return v, dx + dy + 0.5 * ulp(v)

    def sp(self, z, dz):
        v = self.ar.softplus(z)
        return v, dz + 2.0 ** -51 + 2.0 * ulp(v)


class _State:
    """The SC state after one history of decided bits, shared by every path that has it."""

    def __init__(self, ctx, alpha, beta, i):
        self.ctx, self.alpha, self.beta, self.i = ctx, alpha, beta, i
        self.kids, self.pen = {}, {}

    def a(self, s):  # LLRs of the stage-s node that holds leaf i (f from above, on demand)
        if self.alpha[s] is None:
            up, h = self.a(s + 1), 1 << s
            self.alpha[s] = [self.ctx.f(up[j], up[j + h]) for j in range(h)]
        return self.alpha[s]

    def pens(self, s):  # node sums of softplus(-l) (bits 0) and softplus(+l) (bits 1), l clipped
        if s not in self.pen:
            c, t0, t1 = self.ctx, [], []
            for v, d in self.a(s):
                l = min(max(v, -c.lmax), c.lmax)
                t0.append(c.sp(-l, c.clipd(v, d)))
                t1.append(c.sp(l, c.clipd(v, d)))
            self.pen[s] = (t0[0], t1[0]) if s == 0 else (pairwise_sum(t0), pairwise_sum(t1))
        return self.pen[s]

    def child(self, s, bit):  # the stage-s node at i decided as all-`bit` partial sums
        if (s, bit) not in self.kids:
            c, i2 = self.ctx, self.i + (1 << s)
            beta = list(self.beta)
            for j in range(self.i, i2):
                beta[j] = bit
            st = None
            if i2 < c.n:
                tz = (i2 & -i2).bit_length() - 1
                for ss in range(s + 1, tz + 1):
                    pos, h = (i2 - 1) & ~((1 << ss) - 1), 1 << (ss - 1)
                    for j in range(h):
                        beta[pos + j] ^= beta[pos + h + j]
                pos, h = i2 & ~((1 << (tz + 1)) - 1), 1 << tz
                up = self.a(tz + 1)
                alpha = list(self.alpha)
                for ss in range(tz):
                    alpha[ss] = None
                alpha[tz] = [c.g(up[j], up[j + h], beta[pos + j]) for j in range(h)]
                st = _State(c, alpha, beta, i2)
            self.kids[(s, bit)] = st
        return self.kids[(s, bit)]


def make_root(ar, logits, f_mode, lmax):
    """The state before the first leaf: the channel is a = -logit (fp32 values, exact)."""
    n = len(logits)
    ctx = _Ctx(ar, n, f_mode, lmax)
    alpha = [None] * ctx.S + [[(ar.num(-float(x)), 0.0) for x in logits]]
    return _State(ctx, alpha, [0] * n, 0)


def decode(root, mask, L, fast=False, margin=4.0):
    """The L survivors' metrics in the device's final order (each appears twice among the 2L
    returned rows): (values [L], tolerances [L], fragile).  fragile: a selection that later
    leaves depend on had a survivor and a loser of different histories closer than `margin`
    times their summed budgets, so the device may legitimately keep the other one."""
    c = root.ctx
    n, ar = c.n, c.ar
    paths = [(root, ar.num(0.0 if p == 0 else c.lmax_f), 0.0) for p in range(L)]
    i, fragile = 0, False
    while i < n:
        s, fork = 0, not mask[i]
        if fast:
            for ss in range(c.S if i == 0 else (i & -i).bit_length() - 1, 0, -1):
                nfz = int(sum(1 for j in range(i, i + (1 << ss)) if mask[j]))
                if nfz == 1 << ss or (nfz == (1 << ss) - 1 and not mask[i + (1 << ss) - 1]):
                    s, fork = ss, nfz != 1 << ss
                    break
        if not fork:
            paths = [(st.child(s, 0),) + _add((v, d), st.pens(s)[0]) for st, v, d in paths]
        else:
            cand = [(st, 0) + _add((v, d), st.pens(s)[0]) for st, v, d in paths]
            cand += [(st, 1) + _add((v, d), st.pens(s)[1]) for st, v, d in paths]
            order = sorted(range(2 * L), key=lambda q: (cand[q][2], q))
            if i + (1 << s) < n:
                for q in order[:L]:
                    for r in order[L:]:
                        a, b = cand[q], cand[r]
                        same = a[0] is b[0] and a[1] == b[1] and a[2] == b[2]
                        if not same and abs(float(a[2] - b[2])) <= margin * (a[3] + b[3]):
                            fragile = True
            paths = [(cand[q][0].child(s, cand[q][1]), cand[q][2], cand[q][3]) for q in order[:L]]
        i += 1 << s
    order = sorted(range(L), key=lambda q: (paths[q][1], q))
    vals = [paths[q][1] for q in order]
    ds = [paths[q][2] for q in order]
    # sorting is 1-Lipschitz in the sup norm: entries closer than their budgets may swap places
    tol = [max(ds[j] for j in range(L) if abs(float(vals[j] - vals[r])) <= ds[j] + ds[r]) for r in range(L)]
    return vals, tol, fragile


def reference(logits, mask, L, f_mode, lmax, fast=False, ar=None):
    """(metrics float64 [L], tolerances float64 [L], fragile) of one row in mpmath."""
    with mp.workdps(DPS):
        return stored(*decode(make_root(ar or MpArith(), logits, f_mode, lmax), mask, L, fast))


def stored(vals, tol, fragile):
    """What the fixture keeps: the values rounded to fp64, that rounding (ulp/2) added to the budget."""
    v = np.array([float(x) for x in vals])
    return v, np.array(tol) + 0.5 * np.spacing(v), fragile


# ------------------------------------------------------- cases of the fixture ----
TINY_LMAX = (7.5, 30.0, 300.0, 700.0)
DEEP_N = (8, 32, 64, 256, 1024, 2048)
DEEP_L = (2, 8)
DEEP_LMAX = (30.0, 700.0)


def tiny_mask(n, code):
    """Frozen mask of information pattern `code` (bit i set: position i carries information)."""
    return np.array([0 if (code >> i) & 1 else 1 for i in range(n)], dtype=np.uint8)


def tiny_L(n, code):
    """The list size at which no real path is pruned: 2 at n = 2, max(4, 2^k) at n = 4."""
    return 2 if n == 2 else max(4, 1 << bin(code).count("1"))


def deep_mask(n, fset):
    """fset 0: every position frozen; 1: position 1 the only information bit."""
    m = np.ones(n, dtype=np.uint8)
    if fset == 1:
        m[1] = 0
    return m


def deep_rows(n):
    return 8 if n >= 1024 else 16


def deep_logits(n):
    """AWGN-like fp32 logits (all-zero codeword, LLR mean 2 sigma 2) from a 64-bit LCG in integer
    arithmetic, so the rows need no storage; the last two rows scaled by 40."""
    rows = deep_rows(n)
    state = np.arange(1, rows * n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(n)
    acc = np.zeros(rows * n, dtype=np.float64)
    with np.errstate(over="ignore"):
        for _ in range(4):
            state = state * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
            acc += (state >> np.uint64(40)).astype(np.float64) / 2.0 ** 24 - 0.5
    x = (-(2.0 + 2.0 * acc * math.sqrt(3.0))).astype(np.float32).reshape(rows, n)
    x[-2:] *= np.float32(40.0)
    return x


def deep_cases():
    return [(L, fm, lmax, fset, fast) for L in DEEP_L for fm in (0, 1) for lmax in DEEP_LMAX for fset in (0, 1)
            for fast in (0, 1)]


def deep_key(n, L, fm, lmax, fset, fast):
    return f"d{n}_L{L}_f{fm}_l{int(lmax)}_s{fset}_p{fast}"
