"""A correctly rounded restatement of the exact-boxplus SC decoder, in plain numpy.

TEST INFRASTRUCTURE ONLY (imported the way exactf_recipe.py is).  csrc/exactf.h promises fp32
exp and log that are CORRECTLY ROUNDED, inside the reference's five fp32 roundings of
    f(x, y) = log(1 + exp(xc + yc)) - log(exp(xc) + exp(yc)),   xc, yc = clip(x, y, +-llr_max).
This module is what that promise is held to on the device (tests/test_exactf_ulp*.py):

  exp_cr, log_cr   fp32 in, (fp32 correctly rounded, fragile mask) out.  The value is taken in
                   float64 first; wherever that lies within 2^-20 fp32-ulp of a rounding midpoint
                   (numpy's float64 exp/log are good to ~2^-29 fp32-ulp) it is taken again in
                   np.longdouble (64-bit significand, error ~2^-35 fp32-ulp) and rounded once.
                   FRAGILE marks the arguments whose extended value lies within 2^-27 fp32-ulp
                   of a midpoint: there the device (fp64 error ~3 2^-29 fp32-ulp) may
                   legitimately round the other way, and a comparison must leave the row out.
                   IEEE at the ends: overflow to +inf, underflow through subnormals to 0,
                   log(+inf) = +inf, log(0) = -inf.
  f_cr             the clip and the five roundings of oracle/polar_oracle.c:f_exact.
  sc_decode_cr     orc_sc_decode_lmax vectorised over rows: bits and a per-row fragile mask (the
                   OR over every f the row's decisions depend on).

Hooks for the CPU test's own conditions: `Trace` collects the table cells the device forms would
index, `Mutate` moves every 8th exp / log result up one ulp (the sensitivity check).
"""
import numpy as np

F32 = np.float32
_LD = np.longdouble
_FLT_MAX = np.finfo(np.float32).max
_FRAGILE = 2.0 ** -27  # of an fp32 ulp
_RECHECK = 2.0 ** -44  # relative (>= 2^-20 fp32-ulp): float64 values this near a midpoint are taken again in longdouble
_OVER_MID = float(_FLT_MAX) + 2.0 ** 103  # midpoint between FLT_MAX and 2^128: above rounds to +inf


def _near_midpoint(v, r, tol):
    """v: float64 / longdouble values, r = v rounded to fp32.  True where v lies within tol (in
    units of the fp32 gap on that side of r) of a midpoint between neighbouring fp32 values."""
    t = v.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        lo = np.nextafter(r, F32(-np.inf)).astype(t)
        hi = np.nextafter(r, F32(np.inf)).astype(t)
        rr = r.astype(t)
        near = np.abs(v - (rr + lo) / 2) < tol * (rr - lo)
        near |= np.abs(v - (rr + hi) / 2) < tol * (hi - rr)
        near |= np.abs(v - t(_OVER_MID)) < tol * 2.0 ** 104  # inf has no finite gap
    return near


def _round_once(fn, x):
    x = np.asarray(x, dtype=F32)
    shape = x.shape
    x = x.ravel()
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        v = fn(x.astype(np.float64))
        r = v.astype(F32)
        # an fp32 ulp is at least 2^-24 of the value: v (1 +- 2^-44) rounding alike means that no
        # midpoint lies within 2^-20 ulp of v (the overflow threshold and subnormal results included)
        idx = np.flatnonzero((v * (1.0 - _RECHECK)).astype(F32) != (v * (1.0 + _RECHECK)).astype(F32))
        fragile = np.zeros(x.shape, dtype=bool)
        if idx.size:
            vl = fn(x[idx].astype(_LD))
            rl = vl.astype(F32)
            r[idx] = rl
            fragile[idx] = _near_midpoint(vl, rl, _FRAGILE)
    return r.reshape(shape), fragile.reshape(shape)


def exp_cr(x):
    """(correctly rounded fp32 exp(x), fragile mask) for an fp32 array x."""
    return _round_once(np.exp, x)


def log_cr(x):
    """(correctly rounded fp32 log(x), fragile mask) for an fp32 array x >= 0 (or +inf)."""
    return _round_once(np.log, x)


class Trace:
    """Collects, over every f evaluated, the table cells the device's lean forms index
    (csrc/exactf.h exp_d: rint(x 256/ln2) & 255; log_d: bits 15..22 of bits(v) - 0x3F3504F3)."""

    def __init__(self):
        self.exp_cells = np.zeros(256, dtype=np.int64)
        self.log_cells = np.zeros(256, dtype=np.int64)

    def exp_args(self, x):
        n = np.rint(x.astype(np.float64).ravel() * (256.0 / np.log(2.0))).astype(np.int64)
        self.exp_cells += np.bincount(n & 255, minlength=256)

    def log_args(self, v):
        v = v.ravel()
        v = v[np.isfinite(v) & (v > 0)]
        d = v.view(np.uint32).astype(np.int64) - 0x3F3504F3
        self.log_cells += np.bincount((d >> 15) & 255, minlength=256)


class Mutate:
    """A deliberately wrong libm: every 8th exp result and every 8th log result one ulp up (the
    phase moves from call to call, so no row is spared or hit throughout)."""

    def __init__(self):
        self.calls = 0

    def __call__(self, r):
        out = r.copy().ravel()
        s = self.calls % 8
        self.calls += 3
        out[s::8] = np.nextafter(out[s::8], F32(np.inf))
        return out.reshape(r.shape)


def f_cr(x, y, llr_max, trace=None, mutate=None):
    """(f, fragile) of fp32 arrays x, y: oracle/polar_oracle.c:f_exact with correctly rounded
    exp / log -- clip, then fp32 roundings of the sum, each exp, each add, each log, the difference."""
    lm = F32(llr_max)
    xc = np.minimum(np.maximum(np.asarray(x, dtype=F32), -lm), lm)
    yc = np.minimum(np.maximum(np.asarray(y, dtype=F32), -lm), lm)
    s = xc + yc
    with np.errstate(over="ignore", invalid="ignore"):
        es, g0 = exp_cr(s)
        ex, g1 = exp_cr(xc)
        ey, g2 = exp_cr(yc)
        if mutate:
            es, ex, ey = mutate(es), mutate(ex), mutate(ey)
        a = F32(1.0) + es
        b = ex + ey
        la, g3 = log_cr(a)
        lb, g4 = log_cr(b)
        if mutate:
            la, lb = mutate(la), mutate(lb)
        o = la - lb
    if trace is not None:
        trace.exp_args(xc)
        trace.exp_args(yc)
        trace.log_args(a)
        trace.log_args(b)
    return o, g0 | g1 | g2 | g3 | g4


def sc_decode_cr(llr_logits, frozen_pos, n, llr_max=30.0, trace=None, mutate=None, root_llr=None):
    """(bits float32 [rows, k], fragile bool [rows]) -- orc_sc_decode_lmax (f_mode 1) over all rows
    at once: the logits are negated; a node [a, a + 2^s) takes f of its halves, decodes the left
    child, takes g = (1 - 2u) x + y on the unclipped fp32 values, decodes the right child and
    combines the partial sums; a leaf is 1 iff !(llr > 0), a frozen one 0.  A node with nothing but
    frozen leaves decides nothing: its partial sums are 0 and its f are not evaluated (nor counted
    as fragile).  root_llr: a dict that receives {leaf position: the LLR it was decided from}."""
    x = np.ascontiguousarray(llr_logits, dtype=F32)
    rows = x.shape[0]
    assert x.shape[1] == n and n & (n - 1) == 0
    frozen = np.zeros(n, dtype=bool)
    frozen[np.asarray(frozen_pos, dtype=np.int64)] = True
    fragile = np.zeros(rows, dtype=bool)
    uhat = np.zeros((rows, n), dtype=F32)

    def node(a, llr):
        """llr [rows, len] of positions [a, a + len): returns the node's partial sums."""
        m = llr.shape[1]
        if frozen[a:a + m].all():
            return np.zeros((rows, m), dtype=F32)
        if m == 1:
            if root_llr is not None:
                root_llr[a] = llr[:, 0].copy()
            u = np.where(llr > 0, F32(0), F32(1))
            uhat[:, a] = u[:, 0]
            return u
        h = m // 2
        lo, hi = llr[:, :h], llr[:, h:]
        if frozen[a:a + h].all():
            ul = np.zeros((rows, h), dtype=F32)
        else:
            fl, fr = f_cr(lo, hi, llr_max, trace, mutate)
            fragile[:] |= fr.any(axis=1)
            ul = node(a, fl)
        with np.errstate(over="ignore", invalid="ignore"):
            ur = node(a + h, (F32(1) - F32(2) * ul) * lo + hi)
        return np.concatenate([(ul != ur).astype(F32), ur], axis=1)

    with np.errstate(over="ignore"):
        node(0, F32(-1.0) * x)
    return uhat[:, ~frozen], fragile
