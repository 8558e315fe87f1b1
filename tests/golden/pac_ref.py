"""numpy restatement of PAC coding (include/polar_mi355x.h: pl_pac_encode, pl_pac_decode).

A PAC code (Arikan 2019) is a rate-1 convolutional precoder in front of the polar transform: the data word v
(the k data bits at the information positions, 0 elsewhere) becomes u_i = XOR_j c_j v_{i-j}, and x = u G_n.  The
decoder is a list decoder over the SC tree of u with a shift register of v per path.  Every decoder value is an
fp32 add, min, negate or compare, so this np.float32 restatement is exact: the kernel must equal it value for
value, ties included (candidates are ordered by (metric, candidate index), +inf metrics among them).
"""
import numpy as np

CONV_133 = (1, 0, 1, 1, 0, 1, 1)  # octal 133, the generator of the PAC(128, 64) example


def conv_mask(conv):
    """(c_0, ..., c_m) -> the uint32 mask with bit j = c_j."""
    conv = tuple(int(c) for c in conv)
    if not 1 <= len(conv) <= 32 or conv[0] != 1 or any(c not in (0, 1) for c in conv):
        raise ValueError(f"conv must be 1 ... 32 bits with c_0 = 1, got {conv}")
    return sum(c << j for j, c in enumerate(conv))


def _parity(x):
    x = x.astype(np.uint32)
    for s in (16, 8, 4, 2, 1):
        x = x ^ (x >> np.uint32(s))
    return (x & np.uint32(1)).astype(np.uint8)


def info_positions(frozen_pos, n):
    m = np.ones(n, bool)
    m[np.asarray(frozen_pos, np.int64)] = False
    return np.flatnonzero(m)


def precode(v_full, conv):
    """[bs, n] data words -> [bs, n] u = v * conv over GF(2) (v at negative indices 0)."""
    v = np.asarray(v_full, np.uint8)
    u = np.zeros_like(v)
    for j, c in enumerate(conv):
        if c and j < v.shape[1]:
            u[:, j:] ^= v[:, : v.shape[1] - j]
    return u


def transform(u):
    """x = u G_n, the bit order of pl_polar_encode: x[p] ^= x[p + h] where bit h of p is clear, h = 1, 2, ..."""
    x = np.array(u, np.uint8)
    n = x.shape[1]
    h = 1
    while h < n:
        y = x.reshape(x.shape[0], n // (2 * h), 2, h)
        y[:, :, 0, :] ^= y[:, :, 1, :]
        h *= 2
    return x


def pac_encode(data, frozen_pos, n, conv=CONV_133):
    """[bs, k] 0/1 data bits -> [bs, n] uint8 codewords."""
    data = np.asarray(data)
    info = info_positions(frozen_pos, n)
    v = np.zeros((data.shape[0], n), np.uint8)
    v[:, info] = data != 0
    return transform(precode(v, conv))


def generator_matrix(frozen_pos, n, conv=CONV_133):
    """[k, n] uint8: row m is the codeword of the m-th unit data word."""
    k = n - len(np.asarray(frozen_pos).reshape(-1))
    return pac_encode(np.eye(k, dtype=np.uint8), frozen_pos, n, conv)


def f_op(x, y, lmax):
    mag = np.minimum(np.minimum(np.abs(x), np.abs(y)), lmax)
    return (np.sign(x) * np.sign(y) * mag).astype(np.float32)


def g_op(x, y, b):
    return (np.where(b != 0, -x, x) + y).astype(np.float32)


def pac_decode(logits, frozen_pos, n, list_size, conv=CONV_133, llr_max=30.0):
    """[bs, n] logits log P(1)/P(0) -> (bits [bs, k] uint8, pm [bs, L] fp32 ascending).  Vectorised over rows,
    one step a leaf; every path keeps its own stage buffers (the kernel's lazy copies hold the same values)."""
    L = int(list_size)
    x = np.asarray(logits, np.float32)
    bs = x.shape[0]
    S = n.bit_length() - 1
    assert 1 << S == n and x.shape[1] == n and L >= 1 and L & (L - 1) == 0
    mask = np.uint32(conv_mask(conv))
    lmax = np.float32(llr_max)
    info = info_positions(frozen_pos, n)
    is_info = np.zeros(n, bool)
    is_info[info] = True
    A = [np.zeros((bs, L, 1 << s), np.float32) for s in range(S)]
    A.append(np.broadcast_to((-x)[:, None, :], (bs, L, n)).copy())  # stage S: the negated channel
    beta = np.zeros((bs, L, n), np.uint8)  # partial sums of u by absolute position
    vdec = np.zeros((bs, L, n), np.uint8)  # decided v
    reg = np.zeros((bs, L), np.uint32)     # v_{i-1} at bit 0, v_{i-2} at bit 1, ...
    pm = np.full((bs, L), np.inf, np.float32)
    pm[:, 0] = 0.0
    rows = np.arange(bs)[:, None]
    for i in range(n):
        if i == 0:
            start = S
        else:
            tz = (i & -i).bit_length() - 1
            for s in range(1, tz + 1):
                pos, h = (i - 1) & ~((1 << s) - 1), 1 << (s - 1)
                beta[:, :, pos:pos + h] ^= beta[:, :, pos + h:pos + 2 * h]
            pos, h = i & ~((1 << (tz + 1)) - 1), 1 << tz
            A[tz] = g_op(A[tz + 1][:, :, :h], A[tz + 1][:, :, h:], beta[:, :, pos:pos + h])
            start = tz
        for s in range(start, 0, -1):
            h = 1 << (s - 1)
            A[s - 1] = f_op(A[s][:, :, :h], A[s][:, :, h:], lmax)
        l = A[0][:, :, 0]
        u0 = _parity((reg << np.uint32(1)) & mask)
        neg = l < 0
        mag = np.abs(l)
        pen0 = np.where((u0 != 0) != neg, mag, np.float32(0)).astype(np.float32)
        if not is_info[i]:
            pm = (pm + pen0).astype(np.float32)
            reg = reg << np.uint32(1)
            beta[:, :, i] = u0
            continue
        pen1 = np.where((u0 == 0) != neg, mag, np.float32(0)).astype(np.float32)
        cand = np.concatenate([pm + pen0, pm + pen1], axis=1).astype(np.float32)  # c < L: v = 0, c >= L: v = 1
        keep = np.argsort(cand, axis=1, kind="stable")[:, :L]                     # (metric, candidate index)
        par, vb = keep % L, (keep // L).astype(np.uint8)
        pm = cand[rows, keep]
        A = [a[rows, par] for a in A[:S]] + [A[S]]
        beta, vdec = beta[rows, par], vdec[rows, par]
        reg = (reg[rows, par] << np.uint32(1)) | vb.astype(np.uint32)
        beta[:, :, i] = u0[rows, par] ^ vb
        vdec[:, :, i] = vb
    best = np.argmin(pm, axis=1)  # first minimum
    bits = vdec[np.arange(bs), best][:, info]
    return bits, np.sort(pm, axis=1, kind="stable")


# ---- seeded inputs ---------------------------------------------------------------------------------------

def special_rows(frozen_pos, n, conv, llr_max, rng):
    """Four rows: all-zero, +-llr_max, beyond llr_max, and the noiseless logits of a random codeword."""
    k = n - len(frozen_pos)
    sign = rng.integers(0, 2, (2, n)) * 2.0 - 1.0
    cw = pac_encode(rng.integers(0, 2, (1, k)), frozen_pos, n, conv)[0]
    return np.stack([np.zeros(n), sign[0] * llr_max, sign[1] * llr_max * 2.5, (2.0 * cw - 1.0) * 8.0]).astype(np.float32)


def awgn_rows(frozen_pos, n, conv, rows, ebno_db, rng, return_data=False):
    """BPSK over AWGN at ebno_db (pick it near the code's waterfall): logits log P(1)/P(0) of random codewords."""
    k = n - len(frozen_pos)
    data = rng.integers(0, 2, (rows, k)).astype(np.uint8)
    cw = pac_encode(data, frozen_pos, n, conv)
    no = 1.0 / (2.0 * (k / n) * 10.0 ** (ebno_db / 10.0))
    y = (1.0 - 2.0 * cw) + rng.standard_normal((rows, n)) * np.sqrt(no)
    logits = (-2.0 * y / no).astype(np.float32)
    return (logits, data) if return_data else logits


def integer_rows(n, rows, rng):
    """Integer LLRs in -3 ... 3: metric ties at almost every fork, zeros among them."""
    return rng.integers(-3, 4, (rows, n)).astype(np.float32)


def make_inputs(frozen_pos, n, conv, llr_max, rows, seed, ebno_db=2.0):
    """`rows` rows of all three kinds: the four special rows first, then AWGN and integer rows in equal parts."""
    rng = np.random.default_rng(seed)
    rest = max(rows - 4, 0)
    parts = [special_rows(frozen_pos, n, conv, llr_max, rng)[:rows],
             awgn_rows(frozen_pos, n, conv, rest // 2, ebno_db, rng),
             integer_rows(n, rest - rest // 2, rng)]
    return np.concatenate(parts, axis=0)
