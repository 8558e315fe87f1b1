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

osd_decode is the statement of the contract: a dense [rows, patterns, n] search.  osd_decode_packed is its
accelerator for the shapes the dense one cannot hold (tests/test_osd.py proves the two equal), and
envelope_case builds the inputs of tests/test_osd_envelope_gpu.py, whose conditions tests/test_osd.py
asserts without a GPU.
"""
import functools
import itertools
import math

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


def random_full_rank(k, n, rng):
    """A uniformly drawn 0/1 matrix [k, n] of rank k (redrawn until it is)."""
    while True:
        g = rng.integers(0, 2, (k, n)).astype(np.uint8)
        if gf2_rank(g) == k:
            return g


def tie_rows(n, rng):
    """Rows that exercise the tie policy; all values are multiples of 2^-6 below 2^7, so every Delta
    is an exact fp64 sum whatever its order."""
    rows = []
    for v in (0.5, 3.0, 100.0):  # all-equal |llr|
        rows += [np.full(n, v) * rng.choice([-1.0, 1.0], n) for _ in range(8)]
    for _ in range(16):  # clipped to +-100 in half the positions
        r = np.round(rng.normal(0, 4, n) * 64) / 64
        half = rng.permutation(n)[: n // 2]
        r[half] = rng.choice([-1.0, 1.0], n // 2) * rng.choice([100.0, 250.0, 1e6], n // 2)
        rows.append(r)
    for _ in range(16):  # exact zeros of either sign: hard decision 0, tie among themselves
        r = np.round(rng.normal(0, 4, n) * 64) / 64
        z = rng.permutation(n)[: n // 3]
        r[z] = rng.choice([0.0, -0.0], z.size)
        rows.append(r)
    for _ in range(16):  # +-Inf is clipped like any large value
        r = np.round(rng.normal(0, 4, n) * 64) / 64
        z = rng.permutation(n)[: n // 4]
        r[z] = rng.choice([-np.inf, np.inf], z.size)
        rows.append(r)
    rows.append(np.zeros(n))
    return np.array(rows, dtype=np.float32)


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


@functools.lru_cache(maxsize=8)
def packed_patterns(k, i):
    """The i-subsets of range(k) in itertools.combinations order as a read-only array [C(k, i), i],
    filled straight from the iterator (no list of tuples); uint8 where the members fit."""
    count = math.comb(k, i)
    flat = np.fromiter(itertools.chain.from_iterable(itertools.combinations(range(k), i)),
                       dtype=np.uint8 if k <= 256 else np.int64, count=count * i)
    p = flat.reshape(count, i)
    p.setflags(write=False)
    return p


_BYTE_BITS = ((np.arange(256)[:, None] >> np.arange(8)) & 1).astype(np.float64)  # [value, bit]


def osd_decode_packed(gm, llr, t, block=1 << 16):
    """osd_decode with a bit-packed search: the same four results, for shapes whose dense
    [rows, patterns, n] candidates do not fit (about 1e-7 s a pattern at n <= 256).
    The basis, c0 and a are the dense function's.  The basis rows are packed eight positions a byte
    (little end first), a candidate is the XOR of packed rows, and its Delta is the fp64 sum, in byte
    order, of one look-up per byte in a table whose entry v of byte b is -sum a[8 b + i] over the bits i
    of v.  First argmin within an order, strict < between orders; the gap is between the two smallest of
    {0} and all Deltas."""
    gm = (np.asarray(gm) != 0).astype(np.uint8)
    k, n = gm.shape
    llr = np.asarray(llr, dtype=np.float32).reshape(-1, n)
    bs = llr.shape[0]
    nb = (n + 7) // 8
    out = np.zeros((bs, n), dtype=np.uint8)
    dist = np.zeros(bs, dtype=np.float64)
    pattern = np.full(bs, -1, dtype=np.int32)
    gap = np.full(bs, np.inf, dtype=np.float64)
    for lo in range(0, bs, 64):
        sl = slice(lo, min(bs, lo + 64))
        g, idx, ls = most_reliable_basis(gm, llr[sl])
        m = g.shape[0]
        u = (ls[:, :k] > 0).astype(np.uint8)
        c0 = (u[:, :, None] & g).sum(axis=1, dtype=np.int64).astype(np.uint8) & 1  # [m, n]
        a = ls.astype(np.float64) * (1.0 - 2.0 * c0)
        packed = np.packbits(g, axis=2, bitorder="little")  # [m, k, nb]
        a8 = np.zeros((m, nb * 8), dtype=np.float64)
        a8[:, :n] = a
        tab = -np.einsum("mbi,vi->mbv", a8.reshape(m, nb, 8), _BYTE_BITS)  # [m, nb, 256]
        cw = c0.copy()
        for r in range(m):
            best, best_g, members = 0.0, -1, ()
            low = [np.zeros(1)]
            base = 0
            for i in range(1, min(t, k) + 1):
                p = packed_patterns(k, i)
                dmin, amin = np.inf, -1
                for s in range(0, len(p), block):
                    q = p[s:s + block]
                    e = packed[r, q[:, 0]]
                    for j in range(1, i):
                        e = e ^ packed[r, q[:, j]]
                    d = tab[r, 0][e[:, 0]]
                    for b in range(1, nb):
                        d += tab[r, b][e[:, b]]
                    am = int(np.argmin(d))  # the first minimum of the block
                    if d[am] < dmin:  # and, by strict <, of the order
                        dmin, amin = float(d[am]), s + am
                    low.append(np.partition(d, 1)[:2] if d.size > 1 else d)
                if dmin < best:
                    best, best_g, members = dmin, base + amin, tuple(int(x) for x in p[amin])
                base += len(p)
            for j in members:
                cw[r] ^= g[r, j]
            pattern[lo + r] = best_g
            if base:
                two = np.partition(np.concatenate(low), 1)[:2]
                gap[lo + r] = two[1] - two[0]
        z = ls.astype(np.float64) * (1.0 - 2.0 * cw)
        dist[sl] = np.logaddexp(0.0, z).mean(axis=1)
        o = np.zeros((m, n), dtype=np.uint8)
        np.put_along_axis(o, idx, cw, axis=1)
        out[sl] = o
    return out, dist, pattern, gap


def structured_g():
    """(16, 40): [I16 | 8 all-zero columns | 16 columns that repeat earlier ones], what shortening and
    repetition produce.  Among the sorted columns the first 16 are dependent, so the pivots skip."""
    rng = np.random.default_rng(1640)
    eye = np.eye(16, dtype=np.uint8)
    return np.concatenate([eye, np.zeros((16, 8), dtype=np.uint8), eye[:, rng.integers(0, 16, 16)]], axis=1)


def planted_rows(g, orders, rng, first_rows=False):
    """One row per order i: a codeword of g with distinct magnitudes in [4, 8] and i signs flipped, so
    that c0 carries i wrong bits where the flipped positions are pivots.  The flipped positions are the i
    most reliable ones, or with first_rows the pivots of the basis rows 0 .. i-1, which makes the
    codeword the first pattern of order i.  What wins is for the reference to say."""
    k, n = g.shape
    rows = []
    for i in orders:
        c = (rng.integers(0, 2, k) @ g.astype(np.int64)) % 2
        mag = rng.uniform(4.0, 8.0, n).astype(np.float32)
        assert len(np.unique(mag)) == n
        r = mag * (2.0 * c - 1.0).astype(np.float32)
        if first_rows:
            flip = most_reliable_basis(g, r[None])[1][0, :i]  # the basis depends on |llr| alone
        else:
            flip = np.argsort(-mag)[:i]
        r[flip] *= -1.0
        rows.append(r)
    return np.array(rows, dtype=np.float32).reshape(-1, n)


def weak_pivot_row(g, i, rng):
    """A row meant to be won by a pattern of order i where the code's rate leaves planted_rows no chance
    (few redundant positions): a codeword whose positions up to the last i pivots of a random order are
    strong (distinct magnitudes in [32, 64]) and from there on weak ([4, 4.4]), with the signs of those i
    pivots flipped.  Only the basis rows of the weak pivots are then worth flipping, and all i of them
    are when every sum of a subset of them outweighs the subset on the weak redundant positions."""
    k, n = g.shape
    order = rng.permutation(n)
    mag = np.empty(n, dtype=np.float32)
    mag[order] = np.linspace(64.0, 32.0, n, dtype=np.float32)
    flip = most_reliable_basis(g, mag[None])[1][0, :k]  # the pivots, as channel indices
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    flip = flip[np.argsort(rank[flip])[k - i:]]  # the i pivots that come last in the order
    weak = order[rank[flip].min():]
    mag[weak] = np.linspace(4.4, 4.0, len(weak), dtype=np.float32)
    c = (rng.integers(0, 2, k) @ g.astype(np.int64)) % 2
    r = mag * (2.0 * c - 1.0).astype(np.float32)
    r[flip] *= -1.0
    return r[None]


# name: (k, n, t, generator matrix, Eb/N0 dB of the AWGN rows, their number, seed, tie rows?, weak-pivot rows
# as (order, seed)).  Every case with tie rows and t >= 2 also gets planted_rows of the orders 1 .. t and,
# with first_rows, of the orders 2 .. t.  Eb/N0 and the seeds were chosen on the CPU for the conditions that
# tests/test_osd.py::test_envelope_inputs_meet_their_conditions asserts.
ENVELOPE_CASES = {
    "k10n20t2": (10, 20, 2, "random", 0.0, 48, 3, True, ()),
    "k8n16t3": (8, 16, 3, "random", 0.0, 48, 1, True, ((3, 1),)),
    "k12n24t4": (12, 24, 4, "random", 0.0, 48, 5, True, ((4, 2),)),
    "k24n33t4": (24, 33, 4, "random", -2.0, 48, 1, True, ((4, 4),)),
    "k40n200t3": (40, 200, 3, "random", 0.0, 48, 1, True, ()),
    "k66n97t3": (66, 97, 3, "random", 0.0, 48, 1, True, ()),
    "k70n130t2": (70, 130, 2, "random", 0.0, 48, 1, True, ()),
    "k128n128t2": (128, 128, 2, "random", 0.0, 48, 1, True, ()),
    "k16n40t2_structured": (16, 40, 2, "structured", 0.0, 48, 1, True, ()),
    "k16n40t2_structured_permuted": (16, 40, 2, "structured_permuted", 0.0, 48, 1, True, ()),
    "k64n128t4": (64, 128, 4, "random", 0.0, 4, 2, False, ()),
    "k128n256t3": (128, 256, 3, "random", 1.0, 4, 1, False, ()),
    "k100n104t4": (100, 104, 4, "random", -2.0, 3, 9, False, ((3, 12),)),
}
ENVELOPE_CORNERS = ("k64n128t4", "k128n256t3", "k100n104t4")


def envelope_case(name):
    """The inputs of an envelope case, rebuilt from its seed: (g uint8 [k, n], t, llr fp32 [rows, n],
    exact bool [rows]).  exact marks the tie rows, whose Deltas are exact in any order; every other row
    must lead its runner-up by more than 1e-9."""
    k, n, t, kind, ebno, rows, seed, ties, weak = ENVELOPE_CASES[name]
    rng = np.random.default_rng([seed, k, n, t])
    if kind == "random":
        g = random_full_rank(k, n, rng)
    else:
        g = structured_g()
        if kind == "structured_permuted":
            g = g[:, np.random.default_rng(4016).permutation(n)]
    llr = [awgn_logits(g, rows, ebno, rng)[0]]
    if t >= 2 and ties:
        llr.append(planted_rows(g, range(1, t + 1), rng))
        llr.append(planted_rows(g, range(2, t + 1), rng, first_rows=True))
    llr += [weak_pivot_row(g, i, np.random.default_rng([s, k, n, i])) for i, s in weak]
    inexact = sum(len(x) for x in llr)
    if ties:
        llr.append(tie_rows(n, rng))
    llr = np.concatenate(llr, axis=0)
    return g, t, llr, np.arange(len(llr)) >= inexact


def winner_orders(pattern, k, t):
    """The order of each winning pattern index (0 for c0, pattern -1)."""
    starts = np.cumsum([0] + [math.comb(k, i) for i in range(1, t + 1)])
    return np.searchsorted(starts, np.asarray(pattern), side="right")
