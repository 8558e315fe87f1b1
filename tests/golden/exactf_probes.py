"""Inputs that turn pl_sc_decode into a probe of the last ulp of the exact-boxplus f, and their
correctly rounded references (exactf_cr.py).  TEST INFRASTRUCTURE ONLY, shared by
tests/test_exactf_ulp.py (which checks on the CPU that the inputs probe what they claim) and
tests/test_exactf_ulp_gpu.py (which decodes them on the device).

Everything here is in the decoder's LLR domain and handed over as logits = -LLR (SC_Dec negates).

  tiny codes   n = 2, position 0 information: the bit is !(f(l0, l1) > 0).
               n = 4, position 0 frozen, position 1 information: !(f(l0, l2) + f(l1, l3) > 0).
               With l1 = -l0 nudged by -3..+3 ulps and l3 = l2 the two f cancel to within a few
               ulps at every magnitude, so the bit follows the last ulp of both.
  long codes   n = 8 ... 1024, only position 1 information: !(P + Q > 0), P the f tree over the
               even-indexed inputs, Q over the odd-indexed ones, Q's inputs P's with one negated.
  whole codes  (128, 256) and (512, 1024) on AWGN logits (exactf_recipe.awgn_logits).
"""
import functools
import os

import numpy as np

import exactf_cr as C
import exactf_recipe as R

F32 = np.float32
GOLDEN = os.path.dirname(os.path.abspath(__file__))
FLT_MAX = np.finfo(np.float32).max

TINY_LMAX = (7.5, 30.0, 43.0, 60.0, 80.0)  # 43: the last on the fast forms; 60, 80: full range
TINY_ROWS = 65000  # random rows per case; the edge rows come on top (the total is ragged)
LONG_CASES = [(n, lmax) for n in (8, 64, 256, 1024) for lmax in (30.0, 60.0)]
LONG_ROWS = 16411
WHOLE_CASES = [(k, n, rows, ebno) for k, n, rows in ((128, 256, 1024), (512, 1024, 256)) for ebno in (1.0, 2.0, 3.0)]
WHOLE_LMAX = 30.0


def nudge(x, ulps):
    """fp32 x moved by `ulps` (int array) steps along the ordered fp32 values (x != 0, finite)."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.int32)
    return (b + np.where(b < 0, -1, 1).astype(np.int32) * ulps.astype(np.int32)).view(F32)


def _mixed(rng, shape, lmax):
    """N(0, 1) times a scale drawn per element from 0.01 / 0.3 / 3 / 12 / 0.95 llr_max."""
    scales = np.array([0.01, 0.3, 3.0, 12.0, 0.95 * lmax])
    return (rng.standard_normal(shape) * scales[rng.integers(0, len(scales), shape)]).astype(F32)


def edge_values(lmax):
    """+-0, subnormals, +-llr_max and its fp32 neighbours, values far beyond the clip."""
    lm = F32(lmax)
    pos = [F32(0.0), F32(1e-45), F32(1e-40), np.nextafter(np.finfo(F32).tiny, F32(0)), np.finfo(F32).tiny,
           np.nextafter(lm, F32(0)), lm, np.nextafter(lm, F32(np.inf)), F32(100.0), F32(1e4), F32(1e30)]
    v = np.array(pos, dtype=F32)
    return np.concatenate([v, -v])


def _edge_rows(rng, n, lmax):
    v = edge_values(lmax)
    a, b = (g.ravel() for g in np.meshgrid(v, v, indexing="ij"))
    if n == 2:
        rows = [np.stack([a, b], axis=1)]
    else:
        # the mirrored probe on edge values, the same value everywhere, and random 4-tuples
        rows = [np.stack([a, -a, b, b], axis=1), np.stack([a, a, b, b], axis=1), np.stack([a, b, a, b], axis=1),
                v[rng.integers(0, len(v), (1024, 4))]]
    # +-FLT_MAX: one element of a row (so that no g adds two of them into an infinity)
    big = v[rng.integers(0, len(v), (8 * n, n))]
    for i in range(8 * n):
        big[i, i % n] = FLT_MAX if (i // n) % 2 else -FLT_MAX
    return np.concatenate(rows + [big], axis=0).astype(F32)


def tiny_mask(n, code):
    """Frozen mask of the n-bit pattern `code` (bit i set: position i information), as
    polar_amd.build.reference_codes() pre-builds them."""
    return np.array([((code >> i) & 1) ^ 1 for i in range(n)], dtype=np.uint8)


TINY_PROBE = {2: 0b01, 4: 0b0010}  # the codes whose one decided bit is the probe above


@functools.lru_cache(maxsize=None)
def tiny_llr(n, lmax):
    """LLRs [rows, n] of one (n, llr_max) group, shared by every frozen pattern."""
    rng = np.random.default_rng([n, int(lmax * 2)])
    rows = TINY_ROWS
    if n == 2:
        x = _mixed(rng, (rows, 2), lmax)
        # second half: one input within a few fp32 steps of where the sign of f is decided --
        # f(x, y) ~ x tanh(y / 2), while the two logs are rounded at the scale of log(1 + e^|y|)
        h = rows // 2
        y = x[h:, 1]
        step = np.spacing(np.maximum(np.abs(y), F32(0.7)).astype(F32))
        x[h:, 0] = (rng.uniform(-4.0, 4.0, rows - h) * step).astype(F32)
        swap = rng.random(rows) < 0.5
        x[swap] = x[swap][:, ::-1]
    else:
        a = _mixed(rng, rows, lmax)
        c = _mixed(rng, rows, lmax)
        a[a == 0] = F32(1.0)
        b = nudge(-a, rng.integers(-3, 4, rows))
        x = np.stack([a, b, c, c], axis=1)
    out = np.concatenate([x, _edge_rows(rng, n, lmax)], axis=0).astype(F32)
    assert out.shape[0] % 64 != 0 and np.isfinite(out).all()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tiny_reference(n, lmax, code):
    """(bits, fragile) of frozen pattern `code` on tiny_llr(n, lmax)."""
    fp = np.flatnonzero(tiny_mask(n, code))
    return C.sc_decode_cr(-tiny_llr(n, lmax), fp, n, lmax)


def long_frozen(n):
    return np.array([0] + list(range(2, n)), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def long_llr(n, lmax):
    """LLRs [rows, n]: even positions of magnitude 15-30 (a share beyond the clip, and at llr_max
    60 up to 0.95 llr_max) with one to three "carriers" per row at the scales 0.01 ... 12, which
    set the magnitude of P; odd positions the same with one element negated and, when it is a
    carrier, nudged by -3..+3 ulps."""
    rng = np.random.default_rng([n, int(lmax), 7])
    rows, h = LONG_ROWS, n // 2
    e = (rng.uniform(15.0, 30.0, (rows, h)) * rng.choice([-1.0, 1.0], (rows, h))).astype(F32)
    wide = rng.random(rows) < 0.125
    top = max(30.0, 0.95 * lmax)
    e[wide] = (rng.uniform(15.0, top, (int(wide.sum()), h)) * rng.choice([-1.0, 1.0], (int(wide.sum()), h))).astype(F32)
    over = rng.random((rows, h)) < 0.03
    e[over] *= F32(1.5)
    scales = np.array([0.01, 0.3, 3.0, 12.0])
    r = np.arange(rows)
    first = rng.integers(0, h, rows)
    for c in range(3):
        pos = first if c == 0 else rng.integers(0, h, rows)
        use = np.ones(rows, dtype=bool) if c == 0 else rng.random(rows) < 0.4
        val = (rng.standard_normal(rows) * scales[rng.integers(0, 4, rows)]).astype(F32)
        val[val == 0] = F32(0.5)
        e[r[use], pos[use]] = val[use]
    o = e.copy()
    on_carrier = rng.random(rows) < 0.5
    j = np.where(on_carrier, first, rng.integers(0, h, rows))
    ulps = np.where(on_carrier, rng.integers(-3, 4, rows), 0)
    o[r, j] = nudge(-e[r, j], ulps)
    out = np.empty((rows, n), dtype=F32)
    out[:, 0::2] = e
    out[:, 1::2] = o
    assert rows % 64 != 0 and np.isfinite(out).all()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def long_reference(n, lmax):
    return C.sc_decode_cr(-long_llr(n, lmax), long_frozen(n), n, lmax)


def whole_frozen(k, n):
    with np.load(os.path.join(GOLDEN, "frozen_sets.npz")) as fs:
        return fs[f"k{k}_n{n}"].astype(np.int64)


@functools.lru_cache(maxsize=None)
def whole_logits(k, n, rows, ebno):
    out = R.awgn_logits(whole_frozen(k, n), n, rows, ebno, seed=[k, n, int(ebno * 10)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def whole_reference(k, n, rows, ebno):
    return C.sc_decode_cr(whole_logits(k, n, rows, ebno), whole_frozen(k, n), n, WHOLE_LMAX)
