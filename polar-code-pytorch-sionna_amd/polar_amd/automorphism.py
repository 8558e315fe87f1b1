"""Position permutations for automorphism-ensemble decoding (AE_Dec, pl_ae_decode).

A linear map A in GL(m, 2) on the m index bits of a position, n = 2^m, permutes the n positions:
pi(i) = XOR of A[b] over the set bits b of i, A[b] the image of the b-th unit vector (an m-bit integer).  A
bit-index ("stage") permutation sigma is the case A[b] = 1 << sigma(b).  Every such map is an automorphism of
a Reed-Muller code, which the reference's row-weight frozen sets (froze.py) are whenever k is a sum of
binomials (rm_code); a frozen set that cuts a weight class in the middle keeps only a few of them.  Whether a
permutation is an automorphism of a given code is decided by re-encoding the permuted generator rows
(is_automorphism), not by a rule about its shape.
"""
import math

import numpy as np

DRAW_CAP = 40320        # bit-index permutations one search tests (8!: every one of them up to n = 256)
LINEAR_DRAW_CAP = 512   # invertible GL(m, 2) maps one search tests (each costs a re-encoding of the generator)


def _log2(n):
    n = int(n)
    if n < 2 or n & (n - 1):
        raise ValueError(f"n must be a power of 2, got {n}")
    return n.bit_length() - 1


def perm_table(A, n):
    """pi [n] int64 of the m = log2 n column images A (m-bit integers): pi(i) = XOR of A[b], b the set bits of i.
    A permutation of 0 ... n-1 iff A is invertible over GF(2)."""
    m = _log2(n)
    A = [int(a) for a in A]
    if len(A) != m or any(not 0 <= a < n for a in A):
        raise ValueError(f"A must be {m} integers in [0, {n}), got {A}")
    pi = np.zeros(n, dtype=np.int64)
    idx = np.arange(n)
    for b in range(m):
        pi ^= np.where((idx >> b) & 1, A[b], 0)
    return pi


def _transform(rows):
    """rows [r, n] uint8 times G_n over GF(2) (G_n is its own inverse): the encoder butterfly."""
    b = np.array(rows, dtype=np.uint8, copy=True)
    n = b.shape[1]
    p = np.arange(n)
    h = 1
    while h < n:
        lo = p[(p & h) == 0]
        b[:, lo] ^= b[:, lo + h]
        h <<= 1
    return b


def is_permutation(pi, n):
    pi = np.asarray(pi)
    return pi.shape == (n,) and np.array_equal(np.sort(pi.astype(np.int64)), np.arange(n))


def is_automorphism(pi, frozen_pos, n):
    """True iff the position permutation pi maps the polar code (frozen_pos, n) onto itself: the k generator
    rows (the rows of G_n at the information positions) are permuted, x'[i] = x[pi(i)], and re-encoded
    (u = x' G_n); all frozen positions of every row must be 0.  A permutation preserves a code iff its
    inverse does, so the direction of the table does not matter."""
    _log2(n)
    pi = np.asarray(pi, dtype=np.int64)
    if not is_permutation(pi, n):
        raise ValueError("pi is not a permutation of 0 ... n-1")
    fp = np.asarray(frozen_pos, dtype=np.int64).reshape(-1)
    if len(fp) == 0 or len(fp) == n:
        return True
    info = np.setdiff1d(np.arange(n), fp)
    for i0 in range(0, len(info), 256):  # chunks of generator rows: a bounded footprint at n = 1024
        u = np.zeros((len(info[i0:i0 + 256]), n), dtype=np.uint8)
        u[np.arange(u.shape[0]), info[i0:i0 + 256]] = 1
        if _transform(_transform(u)[:, pi])[:, fp].any():
            return False
    return True


def _invertible(A, m):
    """Gaussian elimination over GF(2) on the m column images."""
    rows = list(A)
    for bit in range(m):
        piv = next((j for j in range(bit, m) if (rows[j] >> bit) & 1), None)
        if piv is None:
            return False
        rows[bit], rows[piv] = rows[piv], rows[bit]
        for j in range(m):
            if j != bit and (rows[j] >> bit) & 1:
                rows[j] ^= rows[bit]
    return True


def _search(frozen_pos, n, num, draws, what, cap, prefilter=None):
    """Identity first, then the distinct maps of `draws` (an iterator of column-image tuples) that pass
    is_automorphism, until num are found; ValueError naming the number found if the draws run out.
    prefilter(pi): a cheap necessary condition tried first."""
    m = _log2(n)
    num = int(num)
    if num < 1:
        raise ValueError(f"num must be at least 1, got {num}")
    ident = tuple(1 << b for b in range(m))
    seen, out = {ident}, [perm_table(ident, n)]
    for A in draws:
        if len(out) >= num:
            break
        if A in seen:
            continue
        seen.add(A)
        pi = perm_table(A, n)
        if (prefilter is None or prefilter(pi)) and is_automorphism(pi, frozen_pos, n):
            out.append(pi)
    if len(out) < num:
        raise ValueError(f"only {len(out)} {what} of this frozen set (n = {n}) found among {len(seen)} tested "
                         f"(cap {cap}), {num} asked for")
    return np.stack(out[:num])


def stage_permutations(frozen_pos, n, num, seed=0):
    """[num, n] int64: the identity, then distinct bit-index permutations that are automorphisms of the code
    (frozen_pos, n), found by seeded rejection sampling.  At most DRAW_CAP permutations are tested; when all m!
    of them are no more than that (n <= 256) they are tested exhaustively, in a seeded random order, so the
    count is exact.  ValueError naming how many were found if fewer than num exist.
    A bit-index permutation keeps the subset order of the indices, so it maps row i of G_n (the indicator of
    the j contained in i) to row pi^-1(i): it is an automorphism iff it maps the information set onto itself.
    That O(n) test runs first; a permutation that passes it is still confirmed by is_automorphism."""
    m = _log2(n)
    rng = np.random.default_rng(seed)
    frozen = np.zeros(n, dtype=bool)
    frozen[np.asarray(frozen_pos, dtype=np.int64).reshape(-1)] = True
    info = np.flatnonzero(~frozen)

    def keeps_info_set(pi):
        return not frozen[pi[info]].any()

    def draws():
        if math.factorial(m) <= DRAW_CAP:
            import itertools
            every = list(itertools.permutations(range(m)))
            for j in rng.permutation(len(every)):
                yield tuple(1 << s for s in every[j])
        else:
            for _ in range(DRAW_CAP):
                yield tuple(1 << int(s) for s in rng.permutation(m))
    return _search(frozen_pos, n, num, draws(), "bit-index permutations", DRAW_CAP, keeps_info_set)


def linear_permutations(frozen_pos, n, num, seed=0):
    """[num, n] int64: the identity, then distinct seeded random invertible maps A in GL(m, 2) whose
    permutation (perm_table) is an automorphism of the code; at most LINEAR_DRAW_CAP invertible draws are tested.
    ValueError naming how many were found if fewer than num are."""
    m = _log2(n)
    rng = np.random.default_rng(seed)

    def draws():
        made = 0
        while made < LINEAR_DRAW_CAP:
            A = tuple(int(a) for a in rng.integers(0, n, size=m))
            if _invertible(A, m):
                made += 1
                yield A
    return _search(frozen_pos, n, num, draws(), "GL(m, 2) maps", LINEAR_DRAW_CAP)


def rm_code(r, m):
    """(k, frozen_pos) of the Reed-Muller code RM(r, m) as a polar code of length 2^m: the information
    positions are the rows of G_n of weight 2^popcount(i) >= 2^(m - r).  For these k it is the set
    get_Kern_frozen_bits(n, n - k, F2) selects (no weight class is cut, so the unstable sort cannot matter)."""
    r, m = int(r), int(m)
    if not 0 <= r <= m or m < 1:
        raise ValueError(f"RM(r, m) needs 0 <= r <= m and m >= 1, got ({r}, {m})")
    n = 1 << m
    w = np.array([bin(i).count("1") for i in range(n)])
    frozen_pos = np.flatnonzero(w < m - r).astype(np.int64)
    return n - len(frozen_pos), frozen_pos
