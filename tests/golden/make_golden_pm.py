"""Writes tests/golden/pm_probes.npz: probe rows for the list decoders' fp64 softplus and exact f
(csrc/softplus.h) with their mpmath path metrics and tolerances (tests/golden/pm_ref.py).

    python tests/golden/make_golden_pm.py            (CPU only, a few minutes on 16 cores)

Tiny codes (n = 2, 4): per llr_max about 4k decoded rows -- R2 rows at n = 2 and R4 at n = 4, each
decoded with min-sum and with the exact f under one information pattern (drawn per row, so every
family of rows meets every pattern).  Rows are stored sorted by pattern:
    t{n}_{i}_logits [R, n] f32, t{n}_{i}_code [R] u8, t{n}_{i}_f{fm}_pm / _tol: the L survivors'
    metrics (f64) and tolerances (f32, rounded up) of every row, concatenated (L = tiny_L(n, code)).
A row is left out here, at generation, when a selection that later leaves depend on is closer
than four times the budgets (pm_ref.decode: fragile): a dead path at llr_max + p0 ties, up to
rounding, with a real path at p1 whenever a leaf LLR sits on the clip.
Deep trees: d{n}_L.._pm / _tol [rows, L] per case of pm_ref.deep_cases(), _rows the rows of
pm_ref.deep_logits(n) that the case keeps (fragile ones left out in the same way: with the exact
f at n >= 256 the position-1 LLR is ~1e-20, so at L = 8 the dead paths' u = 0 and u = 1 copies tie).
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pm_ref as R  # noqa: E402

R2, R4 = 1400, 600
LN2 = math.log(2.0)
FLT_MAX = float(np.finfo(np.float32).max)
f32 = lambda v: float(np.float32(v))  # noqa: E731


def _spread(xs, k):
    xs = list(xs)
    return xs if len(xs) <= k else [xs[int(round(j * (len(xs) - 1) / (k - 1)))] for j in range(k)]


def z_targets(lmax):
    """Penalty arguments: exp reduction boundaries (k + 1/2) ln 2 for k in [-1010, 1010], the log's
    mantissa branch (1 + e^z beside sqrt(2) 2^j), z <= -37, log-spaced magnitudes, the clip."""
    top = min(lmax, 700.0)
    z = []
    for k in _spread([k for k in range(-1010, 1011) if abs((k + 0.5) * LN2) <= top], 150):
        b = (k + 0.5) * LN2
        z += [b, b * (1 - 2.0 ** -45), b * (1 + 2.0 ** -45)]
    for j in _spread(range(0, int(top / LN2)), 70):
        b = math.log(2.0 ** (j + 0.5) - 1.0)
        z += [b, b - abs(b) * 2.0 ** -44, b + abs(b) * 2.0 ** -44]
    z += [-v for v in (36.0, 36.7, 37.0, 37.5, 38.0, 40.0, 50.0, 100.0, 300.0, 690.0, 699.5) if v <= top]
    for v in np.geomspace(1.5e-45, 4.0 * lmax, 60):
        z += [float(v), -float(v)]
    for v in (lmax, float(np.nextafter(np.float32(lmax), np.float32(0))),
              float(np.nextafter(np.float32(lmax), np.float32(1e9)))):
        z += [v, -v]
    return z


def f_targets(lmax):
    """Exact-f argument pairs (x, y): E = 1, |x| >> |y|, |y| -> 0, M - m and 2m beside the table's
    cell edges (multiples of ln2/64 and ln2/128), 2m and M - m up to the table exponent's
    underflow, every sign combination."""
    p = []
    mags = [float(v) for v in np.geomspace(1.5e-45, 4.0 * lmax, 48)]
    p += [(v, v) for v in mags]
    p += [(lmax, v) for v in mags] + [(mags[-3 - j % 20], v) for j, v in enumerate(mags[:30])]
    tiny = (0.0, 1.4e-45, 1e-40, 1e-30, 1e-20, 1e-10)
    p += [(v, t) for j, v in enumerate(mags[::3]) for t in (tiny[j % 6], tiny[(j + 3) % 6])]
    for i in range(1, 200):
        for eps in (-2.0 ** -21, 0.0, 2.0 ** -21):
            m = 0.5 * i * (LN2 / 128) * (1 + eps)
            p.append((m, m + ((i * 7) % 150 + 1) * (LN2 / 128) * (1 - eps)))
    for v in np.linspace(350.0, 700.0, 24):
        if v <= lmax:
            p += [(float(v), lmax), (float(v), float(v)), (lmax - float(v), lmax)]
    for d in np.linspace(0.0, 8.0, 17):
        p.append((max(lmax - 745.0 - d, 0.0) + d * 1e-3, lmax))
    sg = ((1, 1), (1, -1), (-1, 1), (-1, -1))
    return [(sx * x, sy * y) for j, (x, y) in enumerate(p) for sx, sy in (sg[j % 4], sg[(j + 1 + j // 4) % 4])]


def _split(v):  # v = hi + lo with both fp32: a g leaf then carries a genuine fp64 argument
    hi = f32(v)
    return hi, (f32(v - hi) if math.isfinite(hi) else 0.0)


def tiny_llr(n, lmax):
    """The LLR rows (fp32 values) of one (n, llr_max): the pools above laid on the tree."""
    Z, F = z_targets(lmax), f_targets(lmax)
    edge = [0.0, -0.0, FLT_MAX, -FLT_MAX, lmax, -lmax, 1.4e-45, -1.4e-45]
    rows = []
    if n == 2:  # leaf 0 = f(a0, a1), leaf 1 = a1 +- a0
        for j, z in enumerate(Z):
            far = R.BIG if j % 2 else -R.BIG
            rows += [(f32(z), far), (far, f32(z))]       # the other leaf pinned on the clip
            hi, lo = _split(z)
            rows.append((lo, hi))                        # leaf 1 = sp(-+z), z a sum of two fp32
        rows += [(f32(x), f32(y)) for x, y in F]
        rows += [(a, b) for a in edge for b in edge]
        want = R2
    else:  # g0 = a2 +- a0, g1 = a3 +- a1; leaf 2 = f(g0, g1), leaf 3 = g1 +- g0
        def lay(x, y):
            (xh, xl), (yh, yl) = _split(x), _split(y)
            return (xl, yl, xh, yh)
        for j, z in enumerate(Z):
            far = R.BIG if j % 2 else -R.BIG
            rows += [lay(z, far), lay(far, z), lay(z, Z[(7 * j + 3) % len(Z)])]
        rows += [lay(x, y) for x, y in F]
        rows += [(f32(x), f32(y), f32(F[(5 * j + 1) % len(F)][0]), f32(F[(5 * j + 1) % len(F)][1]))
                 for j, (x, y) in enumerate(F)]
        rows += [(a, b, edge[(3 * j + i) % 8], edge[(5 * i + j) % 8]) for i, a in enumerate(edge)
                 for j, b in enumerate(edge)]
        want = R4
    return np.array(rows, dtype=np.float32), want


def _tiny_job(args):
    n, lmax, code, llr = args
    mask, L = R.tiny_mask(n, code), R.tiny_L(n, code)
    out = []
    for fm in (0, 1):
        v, t, fragile = R.reference(-llr, mask, L, fm, lmax)
        out.append(None if fragile else (v, t))
    return out


def _deep_job(args):
    n, row, x = args
    out = {}
    with R.mp.workdps(R.DPS):
        for fm in (0, 1):
            for lmax in R.DEEP_LMAX:
                root = R.make_root(R.MpArith(), x, fm, lmax)  # shared by L, frozen set and fast
                for L in R.DEEP_L:
                    for fset in (0, 1):
                        for fast in (0, 1):
                            out[R.deep_key(n, L, fm, lmax, fset, fast)] = R.stored(
                                *R.decode(root, R.deep_mask(n, fset), L, bool(fast)))
    return row, out


def _tol32(t):  # float32, rounded up
    t = np.asarray(t, dtype=np.float64)
    u = t.astype(np.float32)
    return np.where(u.astype(np.float64) < t, np.nextafter(u, np.float32(np.inf)), u).astype(np.float32)


def main():
    out = {"tiny_lmax": np.array(R.TINY_LMAX)}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for n in (2, 4):
            for li, lmax in enumerate(R.TINY_LMAX):
                llr, want = tiny_llr(n, lmax)
                codes = np.random.default_rng(1000 * n + li).permutation(len(llr)) % (1 << n)
                res = pool.map(_tiny_job, [(n, lmax, int(c), r) for c, r in zip(codes, llr)], chunksize=8)
                keep = np.array([r[0] is not None and r[1] is not None for r in res])
                idx = []
                for c in range(1 << n):  # the robust rows of each pattern, thinned evenly to its share
                    ok = np.flatnonzero(keep & (codes == c))
                    share = want >> n
                    idx += ok[np.round(np.linspace(0, len(ok) - 1, share)).astype(int)].tolist() if len(ok) > share \
                        else ok.tolist()
                idx = np.array(idx)
                print(f"n={n} llr_max={lmax}: {len(llr)} candidate rows, {int((~keep).sum())} fragile, kept per pattern "
                      f"{np.bincount(codes[idx], minlength=1 << n).tolist()}", flush=True)
                out[f"t{n}_{li}_logits"] = (-llr[idx]).astype(np.float32)
                out[f"t{n}_{li}_code"] = codes[idx].astype(np.uint8)
                for fm in (0, 1):
                    out[f"t{n}_{li}_f{fm}_pm"] = np.concatenate([res[i][fm][0] for i in idx])
                    out[f"t{n}_{li}_f{fm}_tol"] = _tol32(np.concatenate([res[i][fm][1] for i in idx]))
        for n in R.DEEP_N:
            x = R.deep_logits(n)
            res = dict(pool.map(_deep_job, [(n, r, x[r]) for r in range(len(x))], chunksize=1))
            for key in res[0]:
                rows = [r for r in range(len(x)) if not res[r][key][2]]
                if len(rows) < len(x):
                    print(f"{key}: fragile rows left out, {len(rows)} of {len(x)} kept", flush=True)
                out[key + "_rows"] = np.array(rows, dtype=np.uint8)
                out[key + "_pm"] = np.stack([res[r][key][0] for r in rows]) if rows else np.zeros((0, len(res[0][key][0])))
                out[key + "_tol"] = _tol32(out[key + "_pm"] * 0 + (np.stack([res[r][key][1] for r in rows]) if rows else 0))
            print(f"deep n={n} done", flush=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pm_probes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
