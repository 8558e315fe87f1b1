"""Plain-numpy restatement of ordered-statistics decoding, the CPU checker of polar_amd.OSDecoder.

TEST INFRASTRUCTURE ONLY.  The contract (OSDecoder.forward of the reference, my_sn/fec/osd/dec.py:148-192),
for logits log P(1)/P(0):
  1. clip to +-100;
  2. order the positions by |llr| descending, stably: among equal |llr| the lower index first;
  3. permute the columns of G [k, n] into that order;
  4. for row c = 0 .. k-1 in turn: the pivot is the first 1 of row c, and row c is XORed into every
     other row with a 1 there; the final order is the k pivots in row order, then the other positions
     ascending;
  5. hard-decide the k pivot LLRs (llr > 0 is 1) and re-encode them to c0;
  6. for order i = 1 .. t, every i-subset of the k basis rows in itertools.combinations order is the
     candidate c0 ^ (sum of the rows); the metric is mean_j log(1 + exp(llr_j (1 - 2 c_j))); within an
     order the first minimum wins, and an order replaces the incumbent only on strict <;
  7. undo the permutations.
Since softplus(x) - softplus(-x) = x, the metric of c0 ^ e minus that of c0 is Delta(e) / n with
Delta(e) = -sum_{j in supp e} llr_j (1 - 2 c0_j): the search below compares Delta in fp64 (the lexicographic
minimum of (Delta, pattern index) with Delta < 0 required) and evaluates the softplus form once, for the
returned word.  A pattern's index counts the orders in turn, each in combinations order; -1 means c0.
"""
import itertools

import numpy as np


def gf2_rank(gm):
    """Rank over GF(2) of a 0/1 matrix."""
    m = (np.asarray(gm) != 0).astype(np.uint8).copy()
    rank = 0
    for j in range(m.shape[1]):
        rows = np.nonzero(m[rank:, j])[0]
        if rows.size == 0:
            continue
        p = rank + int(rows[0])
        m[[rank, p]] = m[[p, rank]]
        others = np.nonzero(m[:, j])[0]
        others = others[others != rank]
        m[others] ^= m[rank]
        rank += 1
        if rank == m.shape[0]:
            break
    return rank


def polar_like(k, n):
    """The k rows of highest weight (ties: lower index) of the n x n polar transform, uint8 [k, n]."""
    f = np.array([[1, 0], [1, 1]], dtype=np.int64)
    g = np.array([[1]], dtype=np.int64)
    while g.shape[0] < n:
        g = np.kron(g, f)
    order = np.argsort(-g.sum(1), kind="stable")
    return (g[np.sort(order[:k])] % 2).astype(np.uint8)


def awgn_logits(g, rows, ebno_db, rng):
    """(fp32 logits log P(1)/P(0) [rows, n], the codewords sent uint8 [rows, n]) of random codewords of
    g over BPSK and AWGN at ebno_db; rng is a numpy Generator or a seed."""
    rng = np.random.default_rng(rng)
    k, n = g.shape
    u = rng.integers(0, 2, (rows, k))
    c = (u @ g.astype(np.int64)) % 2
    no = 1.0 / (10 ** (ebno_db / 10) * (k / n))
    y = (1 - 2 * c) + np.sqrt(no / 2) * rng.standard_normal((rows, n))
    return (-2 * y / (no / 2)).astype(np.float32), c.astype(np.uint8)


def patterns(k, t):
    """[(order i, int array [C(k, i), i])] for i = 1 .. t, rows in itertools.combinations order."""
    return [(i, np.array(list(itertools.combinations(range(k), i)), dtype=np.int64).reshape(-1, i))
            for i in range(1, t + 1)]


def most_reliable_basis(gm, llr):
    """Steps 1-4 for a batch.  gm [k, n] 0/1, llr [bs, n] fp32.
    Returns (basis [bs, k, n] uint8 with its columns in the final order, idx [bs, n]: final position ->
    channel index, ls [bs, n] fp32: the clipped LLRs in the final order)."""
    gm = (np.asarray(gm) != 0).astype(np.uint8)
    k, n = gm.shape
    l = np.clip(np.asarray(llr, dtype=np.float32), -100.0, 100.0)
    bs = l.shape[0]
    rows = np.arange(bs)
    order = np.argsort(-np.abs(l), axis=1, kind="stable")
    g = np.ascontiguousarray(gm[:, order].transpose(1, 0, 2))  # [bs, k, n], columns sorted
    piv = np.zeros((bs, k), dtype=np.int64)
    for c in range(k):
        p = np.argmax(g[:, c, :], axis=1)
        piv[:, c] = p
        col = g[rows, :, p].copy()  # [bs, k]: who has a 1 at the pivot
        col[:, c] = 0
        g ^= col[:, :, None] & g[:, c, None, :]
    is_piv = np.zeros((bs, n), dtype=bool)
    is_piv[rows[:, None], piv] = True
    # pivots in row order, then the rest ascending (a stable sort of the flags keeps them ascending)
    rest = np.argsort(is_piv, axis=1, kind="stable")[:, : n - k]
    perm = np.concatenate([piv, rest], axis=1)
    g = np.take_along_axis(g, perm[:, None, :], axis=2)
    idx = np.take_along_axis(order, perm, axis=1)
    ls = np.take_along_axis(l, idx, axis=1)
    return g, idx, ls


def osd_decode(gm, llr, t, chunk_elems=1 << 23):
    """Order-t OSD of llr [bs, n] (fp32 logits) for the generator matrix gm [k, n].
    Returns (codewords uint8 [bs, n] in channel order, dist fp64 [bs]: the metric of the returned word,
    pattern int32 [bs]: -1 for c0 else the pattern index, gap fp64 [bs]: the distance in Delta between
    the winner and the runner-up among c0 (Delta = 0) and all patterns; inf when there is no pattern)."""
    gm = (np.asarray(gm) != 0).astype(np.uint8)
    k, n = gm.shape
    llr = np.asarray(llr, dtype=np.float32).reshape(-1, n)
    bs = llr.shape[0]
    pats = patterns(k, t)
    n_pat = sum(len(p) for _, p in pats)
    out = np.zeros((bs, n), dtype=np.uint8)
    dist = np.zeros(bs, dtype=np.float64)
    pattern = np.full(bs, -1, dtype=np.int32)
    gap = np.full(bs, np.inf, dtype=np.float64)
    step = max(1, int(chunk_elems // max(1, n_pat * n)))
    for lo in range(0, bs, step):
        sl = slice(lo, min(bs, lo + step))
        g, idx, ls = most_reliable_basis(gm, llr[sl])
        m = g.shape[0]
        rows = np.arange(m)
        u = (ls[:, :k] > 0).astype(np.uint8)
        c0 = (u[:, :, None] & g).sum(axis=1, dtype=np.int64).astype(np.uint8) & 1  # [m, n]
        a = ls.astype(np.float64) * (1.0 - 2.0 * c0)
        best = np.zeros(m, dtype=np.float64)
        best_g = np.full(m, -1, dtype=np.int64)
        deltas = [np.zeros((m, 1))]
        base = 0
        for i, p in pats:
            e = g[:, p[:, 0], :]
            for j in range(1, i):
                e = e ^ g[:, p[:, j], :]
            d = -np.einsum("bpn,bn->bp", e.astype(np.float64), a)
            deltas.append(d)
            am = np.argmin(d, axis=1)  # the first minimum
            dm = d[rows, am]
            better = dm < best
            best = np.where(better, dm, best)
            best_g = np.where(better, base + am, best_g)
            base += len(p)
        cw = c0.copy()
        base = 0
        for i, p in pats:
            sel = (best_g >= base) & (best_g < base + len(p))
            if sel.any():
                members = p[best_g[sel] - base]  # [s, i]
                e = np.zeros((int(sel.sum()), n), dtype=np.uint8)
                for j in range(i):
                    e ^= g[np.nonzero(sel)[0], members[:, j], :]
                cw[sel] ^= e
            base += len(p)
        if n_pat:
            alld = np.sort(np.concatenate(deltas, axis=1), axis=1)
            gap[sl] = alld[:, 1] - alld[:, 0]
        z = ls.astype(np.float64) * (1.0 - 2.0 * cw)
        dist[sl] = np.logaddexp(0.0, z).mean(axis=1)
        pattern[sl] = best_g
        o = np.zeros((m, n), dtype=np.uint8)
        np.put_along_axis(o, idx, cw, axis=1)
        out[sl] = o
    return out, dist, pattern, gap
