"""Belief-propagation polar decoding in plain numpy: the contract pl_bp_decode is pinned to.

TEST INFRASTRUCTURE ONLY.  A restatement of include/polar_mi355x.h (pl_bp_decode), every operation fp32
in the stated order.  Internally an LLR is a = -logit (positive favours 0); lmax is llr_max; S = log2 n.

    L[S][i] = clip(-logit[i]);  R[0][i] = +lmax (frozen) or 0 (information);  every other message 0
    one iteration, h = 2^(s-1), p over the positions whose index bit s-1 is 0:
      R pass, s = 1 .. S:  R[s][p]   = clip(f(R[s-1][p], L[s][p+h] + R[s-1][p+h]))
                           R[s][p+h] = clip(f(R[s-1][p], L[s][p]) + R[s-1][p+h])
      L pass, s = S .. 1:  L[s-1][p]   = clip(f(L[s][p], L[s][p+h] + R[s-1][p+h]))
                           L[s-1][p+h] = clip(f(L[s][p], R[s-1][p]) + L[s][p+h])
    bits = !(L[0] > 0) at the information positions, soft_u = -L[0] there, ext_x = -R[S]
    early stop: u^ = the hard decisions (frozen positions 0), x^ = !(L[S] + R[S] > 0); a row whose u^
    encodes to x^ stops and keeps its messages.

f is the min-sum of csrc/genie_kernel.hip fop<0> (magnitude min(|x|, |y|, lmax), times scale with one
rounding when scale != 1, sign = xor of the sign bits) or the exact boxplus with correctly rounded exp /
log (exactf_cr.f_cr).  With the exact f a row is FRAGILE when any f it evaluated lay so near a rounding
midpoint that a correct device form may round the other way; a comparison leaves such rows out.
"""
import numpy as np

F32 = np.float32


def f_minsum(x, y, llr_max, scale=1.0):
    m = np.minimum(np.minimum(np.abs(x), np.abs(y)), F32(llr_max)).astype(F32)
    if float(scale) != 1.0:
        m = (m * F32(scale)).astype(F32)
    sg = (x.view(np.uint32) ^ y.view(np.uint32)) & np.uint32(0x80000000)
    return (m.view(np.uint32) | sg).view(F32)


def clip(v, llr_max):
    lm = F32(llr_max)
    return np.minimum(np.maximum(v, -lm), lm).astype(F32)


def encode(u):
    """x = u G_n on [rows, n] 0/1 arrays: for s = 1 .. S, v[p] ^= v[p + 2^(s-1)] where bit s-1 of p is 0."""
    v = (np.asarray(u) != 0).astype(np.uint8).copy()
    n = v.shape[1]
    p = np.arange(n)
    h = 1
    while h < n:
        lo = p[(p & h) == 0]
        v[:, lo] ^= v[:, lo + h]
        h *= 2
    return v


def bp_decode(llr_logits, frozen_pos, n, num_iter, llr_max=19.3, exact=False, scale=1.0, early_stop=False):
    """dict(bits uint8 [rows, k], soft_u fp32 [rows, k], ext_x fp32 [rows, n], iters int32 [rows],
    fragile bool [rows]) of [rows, n] fp32 logits."""
    x = np.ascontiguousarray(llr_logits, dtype=F32)
    rows = x.shape[0]
    assert x.shape[1] == n and n >= 2 and n & (n - 1) == 0 and num_iter >= 1
    s_tot = n.bit_length() - 1
    frozen = np.zeros(n, dtype=bool)
    frozen[np.asarray(frozen_pos, dtype=np.int64)] = True
    if exact:
        assert float(scale) == 1.0
        from exactf_cr import f_cr

    L = np.zeros((s_tot + 1, rows, n), dtype=F32)
    R = np.zeros((s_tot + 1, rows, n), dtype=F32)
    L[s_tot] = clip(-x, llr_max)
    R[0][:, frozen] = F32(llr_max)
    fragile = np.zeros(rows, dtype=bool)
    iters = np.full(rows, num_iter, dtype=np.int32)
    act = np.arange(rows)  # the rows still iterating
    pos = np.arange(n)

    def f(a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if exact:
            o, fr = f_cr(a, b, llr_max)
            fragile[act] |= fr.any(axis=1)
            return o
        return f_minsum(a, b, llr_max, scale)

    with np.errstate(over="ignore", invalid="ignore"):
        for it in range(num_iter):
            if act.size == 0:
                break
            for s in range(1, s_tot + 1):
                h = 1 << (s - 1)
                lo = pos[(pos & h) == 0]
                ra, rb = R[s - 1][np.ix_(act, lo)], R[s - 1][np.ix_(act, lo + h)]
                la, lb = L[s][np.ix_(act, lo)], L[s][np.ix_(act, lo + h)]
                R[s][np.ix_(act, lo)] = clip(f(ra, (lb + rb).astype(F32)), llr_max)
                R[s][np.ix_(act, lo + h)] = clip((f(ra, la) + rb).astype(F32), llr_max)
            for s in range(s_tot, 0, -1):
                h = 1 << (s - 1)
                lo = pos[(pos & h) == 0]
                ra, rb = R[s - 1][np.ix_(act, lo)], R[s - 1][np.ix_(act, lo + h)]
                la, lb = L[s][np.ix_(act, lo)], L[s][np.ix_(act, lo + h)]
                L[s - 1][np.ix_(act, lo)] = clip(f(la, (lb + rb).astype(F32)), llr_max)
                L[s - 1][np.ix_(act, lo + h)] = clip((f(la, ra) + lb).astype(F32), llr_max)
            if early_stop:
                uh = (~(L[0][act] > 0)) & ~frozen[None, :]
                xh = ~((L[s_tot][act] + R[s_tot][act]).astype(F32) > 0)
                stop = (encode(uh) == xh.astype(np.uint8)).all(axis=1)
                iters[act[stop]] = it + 1
                act = act[~stop]

    info = ~frozen
    return {"bits": (~(L[0][:, info] > 0)).astype(np.uint8), "soft_u": (-L[0][:, info]).astype(F32),
            "ext_x": (-R[s_tot]).astype(F32), "iters": iters, "fragile": fragile}


def rate_half_frozen(n, seed, k=None):
    """A seeded frozen set of n - k positions (k = n / 2 by default), ascending."""
    k = n // 2 if k is None else k
    rng = np.random.default_rng(seed)
    return np.sort(rng.permutation(n)[: n - k]).astype(np.int64)


def awgn_logits(rng, frozen_pos, n, rows, ebno_db=2.0, sigma=None):
    """(u [rows, n] uint8 with the frozen positions 0, logits [rows, n] fp32 log P(1)/P(0)) of random
    codewords over BPSK (0 -> +1) and AWGN at ebno_db (rate k / n), or of noise deviation sigma."""
    frozen = np.zeros(n, dtype=bool)
    frozen[np.asarray(frozen_pos, dtype=np.int64)] = True
    k = int((~frozen).sum())
    u = (rng.random((rows, n)) < 0.5).astype(np.uint8)
    u[:, frozen] = 0
    xs = 1.0 - 2.0 * encode(u).astype(np.float64)
    if sigma is None:
        sigma = np.sqrt(1.0 / (2.0 * max(k, 1) / n * 10.0 ** (ebno_db / 10.0)))
    y = xs + sigma * rng.standard_normal((rows, n))
    return u, (-2.0 * y / sigma ** 2).astype(F32)


def noiseless_logits(u, mag=8.0):
    """Logits -mag (bit 0) / +mag (bit 1) of the codewords of u [rows, n]."""
    return ((2.0 * encode(u).astype(np.float64) - 1.0) * mag).astype(F32)


N_SPECIAL = 4


def make_inputs(seed, n, frozen_pos, rows, llr_max=19.3, ebno_db=2.0):
    """(u, logits) of `rows` >= 5 seeded rows: BPSK-AWGN logits of random codewords around ebno_db, the
    first N_SPECIAL rows replaced by the special ones -- all zeros, entries exactly +-lmax, entries
    beyond lmax, and the noiseless +-8 of the row's own codeword."""
    assert rows > N_SPECIAL
    rng = np.random.default_rng(seed)
    u, x = awgn_logits(rng, frozen_pos, n, rows, ebno_db)
    sg = np.where(rng.random((2, n)) < 0.5, -1.0, 1.0)
    x[0] = F32(0.0)
    x[1] = (sg[0] * float(F32(llr_max))).astype(F32)
    x[2] = (sg[1] * float(F32(llr_max)) * (1.5 + 2.0 * rng.random(n))).astype(F32)
    x[3] = noiseless_logits(u[3:4])[0]
    return u, x


# The exact-f cases tests/test_bp_gpu.py compares on and tests/test_bp_ref.py counts the fragile rows of:
# (n, num_iter, llr_max); llr_max 60 takes the full-range forms of the exact f.
EXACT_CASES = [(n, it, 19.3) for n in (2, 4, 64, 256, 1024) for it in (1, 3)] + [(4, 1, 60.0), (4, 3, 60.0)]
EXACT_ROWS, FRAGILE_CAP = 128, 4


def exact_case_inputs(n, num_iter, llr_max):
    """(frozen_pos, logits [EXACT_ROWS, n]) of one exact-f case."""
    fp = rate_half_frozen(n, 7000 + n)
    _, x = make_inputs(7100 + n + num_iter + int(llr_max), n, fp, EXACT_ROWS, llr_max)
    return fp, x


def early_stop_inputs(n, frozen_pos):
    """44 seeded rows for the early-stop comparison: 6 noiseless ones (they stop after one iteration), 8 each
    at 1, 2, 3 and 4 dB (some stop after a few iterations, some never) and 6 of pure noise (they never stop)."""
    rng = np.random.default_rng(900 + n)
    u, _ = awgn_logits(rng, frozen_pos, n, 6)
    parts = [noiseless_logits(u)]
    for ebno_db in (1.0, 2.0, 3.0, 4.0):
        parts.append(awgn_logits(rng, frozen_pos, n, 8, ebno_db)[1])
    parts.append((rng.standard_normal((6, n)) * 4).astype(F32))
    return np.concatenate(parts)


# Early stop at every size of the two stop paths (n <= 64: several codewords a wave; n >= 128: the butterfly over
# n / 32 words): the frozen set is rate_half_frozen(n, EARLY_STOP_FROZEN_SEED), chosen on the CPU
# (tests/test_bp_ref.py) so that early_stop_inputs shows rows that stop after 1 iteration, after 2 ... 9 and never.
# At n = 2 no message depends on an earlier iteration and every row of early_stop_inputs stops after the first.
EARLY_STOP_SIZES = (2, 4, 8, 16, 32, 128, 256, 512)
EARLY_STOP_FROZEN_SEED = 0
EARLY_STOP_ITERS = 10
PAST_GRID_ROWS = 64 * 1024 * 2 + 5  # n = 8: 64 codewords a work-group, 1024 work-groups at most


def past_grid_early_stop_inputs():
    """(frozen_pos, logits [PAST_GRID_ROWS, 8]): early_stop_inputs' 44 rows (noiseless, noisy, noise) tiled over
    the batch with seeded row order, so every work-group of both strides holds rows of every class."""
    fp = rate_half_frozen(8, EARLY_STOP_FROZEN_SEED)
    base = early_stop_inputs(8, fp)
    idx = np.random.default_rng(8).integers(0, len(base), PAST_GRID_ROWS)
    return fp, base[idx]
