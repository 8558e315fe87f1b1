"""numpy restatement of parity-constrained list decoding (include/polar_mi355x.h: pl_pcl_table_create,
pl_pcl_decode) and of the 5G downlink DCI chain built on it (polar_amd.dci).

TEST INFRASTRUCTURE ONLY.  The decoder is the list decoder of pac_ref.pac_decode with conv = (1,) plus a table of
constraints u[pos] = rhs ^ parity(mask & u): a FORCE leaf computes the bit of every path, a CHECK leaf forks like an
information leaf and then kills every survivor that violates the relation; a row with no path left after a CHECK
leaf stops there.  Every decoder value is an fp32 add, min, negate or compare and every parity an integer, so this
np.float32 restatement is exact: the kernel must equal it value for value, ties and +inf metrics included.

The DCI part restates the data path of 38.212 section 7.3 from the polynomial: CRC24C by long division, the 24
ones in front of the payload, the RNTI on the last 16 parity bits, the input-bit interleaver gather, u G_n by the
butterfly, the rate-matching gather.  The three index tables (interleaver pattern, information positions, rate
matching) are arguments: the package's are pinned against the reference project elsewhere.
"""
import numpy as np

import pac_ref

CHECK, FORCE = 0, 1
info_positions, transform, f_op, g_op = pac_ref.info_positions, pac_ref.transform, pac_ref.f_op, pac_ref.g_op


# ---- constraint tables -----------------------------------------------------------------------------------

def words_of(n):
    return max(n // 32, 1)


def pack_constraints(n, cons):
    """[(pos, kind, rhs, earlier_positions)] -> (pos int32 [C], kind uint8 [C], rhs uint8 [C], mask uint32 [C, W]),
    sorted by pos; bit (j & 31) of word j >> 5 of a mask row = position j."""
    cons = sorted(cons, key=lambda c: c[0])
    C, W = len(cons), words_of(n)
    pos, kind, rhs = np.zeros(C, np.int32), np.zeros(C, np.uint8), np.zeros(C, np.uint8)
    mask = np.zeros((C, W), np.uint32)
    for c, (p, kd, r, earlier) in enumerate(cons):
        pos[c], kind[c], rhs[c] = p, kd, r
        for j in earlier:
            mask[c, int(j) >> 5] |= np.uint32(1 << (int(j) & 31))
    return pos, kind, rhs, mask


def unpack_mask(mask, n):
    """[C, W] uint32 -> [C, n] uint8."""
    mask = np.asarray(mask, np.uint32).reshape(-1, words_of(n))
    bits = (mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(mask.shape[0], 32 * words_of(n))[:, :n].astype(np.uint8)


def check_table(frozen_pos, n, table):
    """The rules pl_pcl_table_create enforces; returns None or the reason."""
    pos, kind, rhs, mask = table
    frozen = np.zeros(n, bool)
    frozen[np.asarray(frozen_pos, np.int64)] = True
    m = unpack_mask(mask, n).astype(bool)
    for c in range(len(pos)):
        if not 0 <= pos[c] < n or (c and pos[c] <= pos[c - 1]):
            return f"constraint {c}: pos"
        if frozen[pos[c]]:
            return f"constraint {c}: frozen pos"
        if kind[c] not in (CHECK, FORCE) or rhs[c] not in (0, 1):
            return f"constraint {c}: kind / rhs"
        if m[c, pos[c]:].any():
            return f"constraint {c}: not causal"
        if (m[c] & frozen).any():
            return f"constraint {c}: frozen bit in mask"
    return None


def constrained_words(free_bits, frozen_pos, n, table):
    """[bs, k - C] bits for the unconstrained information positions, ascending -> [bs, n] u words that satisfy
    every constraint (a CHECK position of a valid word is as determined as a FORCE position)."""
    pos, _, rhs, mask = table
    info = info_positions(frozen_pos, n)
    m = unpack_mask(mask, n)
    con_at = {int(p): c for c, p in enumerate(pos)}
    free = np.array([i for i in info if int(i) not in con_at], np.int64)
    free_bits = np.asarray(free_bits, np.uint8)
    free_bits = free_bits.reshape(free_bits.shape[0], len(free))
    u = np.zeros((free_bits.shape[0], n), np.uint8)
    u[:, free] = free_bits
    for i in info:  # ascending: a mask only reaches below its position
        c = con_at.get(int(i))
        if c is not None:
            u[:, i] = (rhs[c] + (u.astype(np.int64) @ m[c].astype(np.int64))) & 1
    return u


def satisfies(u, table):
    """[bs, n] u words -> [bs] bool: every constraint holds."""
    pos, _, rhs, mask = table
    if len(pos) == 0:
        return np.ones(u.shape[0], bool)
    m = unpack_mask(mask, u.shape[1]).astype(np.int64)
    par = (u.astype(np.int64) @ m.T) & 1
    return ((u[:, pos] ^ par) == rhs[None, :]).all(1)


# ---- the decoder -----------------------------------------------------------------------------------------

def pcl_decode(logits, frozen_pos, n, list_size, table, llr_max=30.0):
    """[bs, n] logits log P(1)/P(0) -> (bits [bs, k] uint8, pm [bs, L] fp32 ascending, ok [bs] uint8, stop [bs]
    int32).  Vectorised over rows, one step a leaf, the kernel's operation order.  A stopped row is carried along:
    its metrics are all +inf and stay so, so nothing it computes afterwards shows."""
    L = int(list_size)
    x = np.asarray(logits, np.float32)
    bs = x.shape[0]
    S = n.bit_length() - 1
    assert 1 << S == n and x.shape[1] == n and L >= 1 and L & (L - 1) == 0
    assert check_table(frozen_pos, n, table) is None, check_table(frozen_pos, n, table)
    pos, kind, rhs, mask = table
    mbits = unpack_mask(mask, n)
    con_at = {int(p): c for c, p in enumerate(pos)}
    lmax = np.float32(llr_max)
    info = info_positions(frozen_pos, n)
    is_info = np.zeros(n, bool)
    is_info[info] = True
    A = [np.zeros((bs, L, 1 << s), np.float32) for s in range(S)]
    A.append(np.broadcast_to((-x)[:, None, :], (bs, L, n)).copy())  # stage S: the negated channel
    beta = np.zeros((bs, L, n), np.uint8)  # partial sums by absolute position
    udec = np.zeros((bs, L, n), np.uint8)  # decided u
    pm = np.full((bs, L), np.inf, np.float32)
    pm[:, 0] = 0.0
    stop = np.full(bs, n, np.int32)
    rows = np.arange(bs)[:, None]
    zero = np.float32(0)
    for i in range(n):
        if i == 0:
            start = S
        else:
            tz = (i & -i).bit_length() - 1
            for s in range(1, tz + 1):
                p0, h = (i - 1) & ~((1 << s) - 1), 1 << (s - 1)
                beta[:, :, p0:p0 + h] ^= beta[:, :, p0 + h:p0 + 2 * h]
            p0, h = i & ~((1 << (tz + 1)) - 1), 1 << tz
            A[tz] = g_op(A[tz + 1][:, :, :h], A[tz + 1][:, :, h:], beta[:, :, p0:p0 + h])
            start = tz
        for s in range(start, 0, -1):
            h = 1 << (s - 1)
            A[s - 1] = f_op(A[s][:, :, :h], A[s][:, :, h:], lmax)
        l = A[0][:, :, 0]
        neg = l < 0
        mag = np.abs(l)
        c = con_at.get(i)
        if not is_info[i] or (c is not None and kind[c] == FORCE):
            if is_info[i]:
                u = (rhs[c] ^ ((udec.astype(np.int64) @ mbits[c].astype(np.int64)) & 1)).astype(np.uint8)
            else:
                u = np.zeros((bs, L), np.uint8)
            pm = (pm + np.where((u != 0) != neg, mag, zero)).astype(np.float32)
            beta[:, :, i] = u
            udec[:, :, i] = u
            continue
        pen0, pen1 = np.where(neg, mag, zero).astype(np.float32), np.where(neg, zero, mag).astype(np.float32)
        cand = np.concatenate([pm + pen0, pm + pen1], axis=1).astype(np.float32)  # c < L: u = 0, c >= L: u = 1
        keep = np.argsort(cand, axis=1, kind="stable")[:, :L]                     # (metric, candidate index)
        par, ub = keep % L, (keep // L).astype(np.uint8)
        pm = cand[rows, keep]
        A = [a[rows, par] for a in A[:S]] + [A[S]]
        beta, udec = beta[rows, par], udec[rows, par]
        beta[:, :, i] = ub
        udec[:, :, i] = ub
        if c is not None:  # CHECK: after the ranking
            got = (ub ^ ((udec.astype(np.int64) @ mbits[c].astype(np.int64)) & 1)).astype(np.uint8)
            pm = np.where(got != rhs[c], np.float32(np.inf), pm).astype(np.float32)
            dead = ~np.isfinite(pm).any(1)
            stop = np.where(dead & (stop == n), np.int32(i), stop).astype(np.int32)
    best = np.argmin(pm, axis=1)  # first minimum
    ok = np.isfinite(pm[np.arange(bs), best])
    bits = udec[np.arange(bs), best][:, info] * ok[:, None].astype(np.uint8)
    return bits, np.sort(pm, axis=1, kind="stable"), ok.astype(np.uint8), stop


# ---- seeded tables and inputs ----------------------------------------------------------------------------

def random_table(frozen_pos, n, num, seed, kinds=(CHECK, FORCE), density=0.5, sentinel_after=None):
    """`num` constraints at random information positions, random kinds of `kinds`, random rhs, random causal masks
    over the earlier information positions (each with probability `density`).  sentinel_after = r: the first CHECK
    at or after the r-th information position gets an empty mask and rhs = 1 -- the all-zero row, whose ties keep
    the u = 0 children of a full list, dies there."""
    rng = np.random.default_rng(seed)
    info = info_positions(frozen_pos, n)
    where = np.sort(rng.permutation(len(info))[:num])
    cons, planted = [], sentinel_after is None
    for r in where:
        kd = int(kinds[rng.integers(0, len(kinds))])
        earlier = [int(j) for j in info[:r] if rng.random() < density]
        rhs = int(rng.integers(0, 2))
        if not planted and kd == CHECK and r >= sentinel_after:
            earlier, rhs, planted = [], 1, True
        cons.append((int(info[r]), kd, rhs, earlier))
    return pack_constraints(n, cons)


def special_rows(frozen_pos, n, table, llr_max, rng):
    """Four rows: all-zero, +-llr_max, beyond llr_max, and the noiseless logits of a random valid codeword."""
    k_free = n - len(frozen_pos) - len(table[0])
    sign = rng.integers(0, 2, (2, n)) * 2.0 - 1.0
    cw = transform(constrained_words(rng.integers(0, 2, (1, k_free)), frozen_pos, n, table))[0]
    return np.stack([np.zeros(n), sign[0] * llr_max, sign[1] * llr_max * 2.5, (2.0 * cw - 1.0) * 8.0]).astype(np.float32)


def awgn_rows(frozen_pos, n, table, rows, ebno_db, rng, return_words=False):
    """BPSK over AWGN at ebno_db: logits log P(1)/P(0) of random valid codewords."""
    k = n - len(frozen_pos)
    k_free = k - len(table[0])
    u = constrained_words(rng.integers(0, 2, (rows, k_free)), frozen_pos, n, table)
    cw = transform(u)
    no = 1.0 / (2.0 * (max(k, 1) / n) * 10.0 ** (ebno_db / 10.0))
    y = (1.0 - 2.0 * cw) + rng.standard_normal((rows, n)) * np.sqrt(no)
    logits = (-2.0 * y / no).astype(np.float32)
    return (logits, u) if return_words else logits


def noise_rows(n, rows, rng, sigma=4.0):
    """Pure noise: what a blind decoder sees at a candidate that carries nothing."""
    return (rng.standard_normal((rows, n)) * sigma).astype(np.float32)


def make_inputs(frozen_pos, n, table, llr_max, rows, seed, ebno_db=2.0):
    """`rows` rows of all four kinds: the four special rows first, then AWGN, integer (pac_ref.integer_rows: ties
    at almost every fork) and pure-noise rows in equal parts."""
    rng = np.random.default_rng(seed)
    rest = max(rows - 4, 0)
    a, b = rest // 3, rest // 3
    parts = [special_rows(frozen_pos, n, table, llr_max, rng)[:rows], awgn_rows(frozen_pos, n, table, a, ebno_db, rng),
             pac_ref.integer_rows(n, b, rng), noise_rows(n, rest - a - b, rng)]
    return np.concatenate(parts, axis=0)


# ---- the DCI chain (38.212 section 7.3) ------------------------------------------------------------------

# g_CRC24C(D) = D^24 + D^23 + D^21 + D^20 + D^17 + D^15 + D^13 + D^12 + D^8 + D^4 + D^2 + D + 1 (38.212 5.1)
CRC24C_POLY = tuple(1 if d in (24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0) else 0 for d in range(24, -1, -1))


def crc24c(bits):
    """[bs, m] bits, first bit the highest power -> [bs, 24] parity bits: the remainder of bits * D^24 by long
    division, one row at a time."""
    bits = np.asarray(bits, np.uint8)
    pol = np.array(CRC24C_POLY, np.uint8)
    out = np.zeros((bits.shape[0], 24), np.uint8)
    for r in range(bits.shape[0]):
        reg = np.concatenate([bits[r], np.zeros(24, np.uint8)])
        for i in range(bits.shape[1]):
            if reg[i]:
                reg[i:i + 25] ^= pol
        out[r] = reg[-24:]
    return out


def rnti_bits(rnti):
    """16 bits, the most significant first (x_rnti,0 of 38.212 7.3.2)."""
    assert 0 <= int(rnti) < 1 << 16
    return np.array([(int(rnti) >> (15 - i)) & 1 for i in range(16)], np.uint8)


def dci_crc_attach(payload, rnti=0, ones_prefix=True):
    """[bs, A] -> [bs, A + 24]: the CRC24C of (24 ones,) payload, its last 16 bits XORed with the RNTI."""
    a = np.asarray(payload, np.uint8)
    src = np.concatenate([np.ones((a.shape[0], 24), np.uint8), a], axis=1) if ones_prefix else a
    p = crc24c(src)
    p[:, 8:] ^= rnti_bits(rnti)[None, :]
    return np.concatenate([a, p], axis=1)


def dci_encode(payload, info_pos, n_polar, il, idx_rm, rnti=0, ones_prefix=True):
    """[bs, A] payload -> ([bs, E] uint8 code bits, [bs, n_polar] u words).  il: the input-bit interleaver as a
    gather index over the A + 24 bits (c'[m] = c[il[m]]), None = no interleaving; info_pos: the A + 24 information
    positions, ascending; idx_rm: the rate-matching gather index over the mother codeword."""
    c = dci_crc_attach(payload, rnti, ones_prefix)
    if il is not None:
        c = c[:, np.asarray(il, np.int64)]
    u = np.zeros((c.shape[0], n_polar), np.uint8)
    u[:, np.asarray(info_pos, np.int64)] = c
    return transform(u)[:, np.asarray(idx_rm, np.int64)], u


def dci_u_positions(A, info_pos, il):
    """u-position of each of the A + 24 bits of (payload, parity) in their order before the interleaver."""
    K = A + 24
    il = np.arange(K) if il is None else np.asarray(il, np.int64)
    inv = np.empty(K, np.int64)
    inv[il] = np.arange(K)
    return np.asarray(info_pos, np.int64)[inv]


def dci_table(A, info_pos, n_polar, il, rnti=0, ones_prefix=True, n_force=0):
    """The constraint table of the DCI code: one constraint a parity bit, its mask the u-positions of the payload
    bits it depends on, its rhs the parity of the ones prefix and the RNTI bit; the first n_force in decoding order
    are FORCE, the rest CHECK.  The table need not be causal: check_table says."""
    upos = dci_u_positions(A, info_pos, il)
    dep = crc24c(np.eye(A, dtype=np.uint8))                       # [A, 24]: payload bit i -> parity bits
    const = crc24c(np.concatenate([np.ones((1, 24), np.uint8), np.zeros((1, A), np.uint8)], 1))[0] if ones_prefix \
        else np.zeros(24, np.uint8)
    const = const.copy()
    const[8:] ^= rnti_bits(rnti)
    cons = [(int(upos[A + j]), CHECK, int(const[j]), [int(upos[i]) for i in np.flatnonzero(dep[:, j])]) for j in range(24)]
    cons.sort(key=lambda c: c[0])
    cons = [(p, FORCE if r < n_force else CHECK, rhs, e) for r, (p, _, rhs, e) in enumerate(cons)]
    return pack_constraints(n_polar, cons)


def dci_distributed(A, info_pos, il):
    """The number of parity bits placed before the last payload bit."""
    upos = dci_u_positions(A, info_pos, il)
    return int((upos[A:] < upos[:A].max()).sum())


def dci_rate_recover(llr_ch, n_polar, k_polar, idx_rm, llr_max=100.0):
    """[bs, E] channel logits -> [bs, n_polar] mother-code logits: a position sent twice adds its two logits (first
    plus second; a third copy, E > 2 n_polar, is dropped as Polar5GDecoder drops it), punctured positions are 0,
    shortened positions -llr_max (a known zero bit as a logit)."""
    x = np.asarray(llr_ch, np.float32)
    E = x.shape[1]
    out = np.zeros((x.shape[0], n_polar), np.float32)
    seen = np.zeros(n_polar, np.int64)
    for e, j in enumerate(np.asarray(idx_rm, np.int64)):
        if seen[j] == 0:
            out[:, j] = x[:, e]
        elif seen[j] == 1:
            out[:, j] = (out[:, j] + x[:, e]).astype(np.float32)
        seen[j] += 1
    if E < n_polar and k_polar / E > 7 / 16:
        out[:, seen == 0] = -np.float32(llr_max)
    return out


def dci_decode(llr_ch, A, info_pos, n_polar, il, idx_rm, list_size, rnti=0, ones_prefix=True, n_force=0, llr_max=100.0):
    """[bs, E] channel logits -> (payload [bs, A] uint8, ok [bs] uint8, stop [bs] int32, pm)."""
    frozen = np.setdiff1d(np.arange(n_polar), np.asarray(info_pos, np.int64))
    table = dci_table(A, info_pos, n_polar, il, rnti, ones_prefix, n_force)
    x = dci_rate_recover(llr_ch, n_polar, A + 24, idx_rm, llr_max)
    bits, pm, ok, stop = pcl_decode(x, frozen, n_polar, list_size, table, llr_max)
    K = A + 24
    ilx = np.arange(K) if il is None else np.asarray(il, np.int64)
    c = np.zeros_like(bits)
    c[:, ilx] = bits  # c'[m] = c[il[m]]
    return c[:, :A], ok, stop, pm


# ---- the cases of tests/test_pcl_gpu.py (tests/test_pcl_ref.py checks what they contain on the CPU) --------

LLR_MAX = 30.0
# (n, frozen-set kind, list size, table kind)
GPU_CASES = [*[(n, "half", 4, "mixed") for n in (2, 4, 8, 32)],
             *[(n, "half", L, "mixed") for n in (64, 256) for L in (1, 2, 8, 32)],
             (1024, "half", 32, "mixed"), (512, "half", 4, "mixed"),
             (64, "half", 8, "none"), (64, "half", 4, "all"), (64, "half", 1, "all"),
             (64, "half", 8, "force"), (64, "half", 8, "check"), (256, "half", 32, "check"),
             (64, "half", 1, "first"), (64, "half", 4, "first"),
             (64, "edge", 8, "last"), (64, "edge", 8, "straddle"), (256, "edge", 2, "straddle"),
             (64, "half", 1, "kill"), (64, "half", 4, "kill")]
# cases in which no row can stop early, by construction: no CHECK (none, force); every information position
# constrained with L >= 2 (one path is alive throughout, and one of its two children always passes); a list that
# cannot fill before the last CHECK whatever the table (k = 1 and 2 at n = 2 and 4 with L = 4: at most two live
# parents, so all their children are kept; "first" with L >= 2: one alive path at the first leaf)
NEVER_STOPS = {(2, "half", 4, "mixed"), (4, "half", 4, "mixed"), (64, "half", 8, "none"),
               (64, "half", 4, "all"), (64, "half", 8, "force"), (64, "half", 4, "first")}


def case_frozen(n, kind):
    fp = np.sort(np.random.default_rng(n).permutation(n)[: n // 2])
    if kind == "edge":  # 31, 32 and n - 1 are information positions
        fp = np.setdiff1d(fp, [31, 32, n - 1])
    return fp


def case_table(n, kind, L, tkind):
    fp = case_frozen(n, kind)
    info = info_positions(fp, n)
    k, seed, logl = len(info), 7 * n + L, L.bit_length() - 1
    if tkind == "none":
        return pack_constraints(n, [])
    if tkind == "mixed" and n == 8:  # k = 4, L = 4: two free leaves fill the list, then a CHECK that can empty it
        return pack_constraints(n, [(int(info[2]), CHECK, 1, []), (int(info[3]), FORCE, 0, [int(info[0]), int(info[2])])])
    if tkind == "mixed":
        return random_table(fp, n, max(1, k // 3), seed, sentinel_after=min(logl + 2, k - 1))
    if tkind == "all":
        return random_table(fp, n, k, seed)
    if tkind == "force":
        return random_table(fp, n, max(1, k // 3), seed, kinds=(FORCE,))
    if tkind == "check":
        return random_table(fp, n, max(1, k // 3), seed, kinds=(CHECK,), sentinel_after=logl + 2)
    if tkind == "first":  # a CHECK with an empty mask and rhs = 1 at the first information position
        return pack_constraints(n, [(int(info[0]), CHECK, 1, [])])
    if tkind == "last":   # a CHECK at the last position over every other information position, and a FORCE before
        return pack_constraints(n, [(int(info[-2]), FORCE, 1, [int(j) for j in info[:-2:2]]),
                                    (n - 1, CHECK, 0, [int(j) for j in info[:-1]])])
    if tkind == "straddle":  # masks with bits on both sides of a word boundary, and the last bit below n - 1
        return pack_constraints(n, [(32, CHECK, 1, [31]), (int(info[-3]), FORCE, 0, [31, 32]),
                                    (n - 1, CHECK, 1, [31, 32, int(info[-2])])])
    assert tkind == "kill"   # one CHECK, after the list has filled
    return pack_constraints(n, [(int(info[logl + 1]), CHECK, 1, [])])


_CASE_CACHE = {}


def gpu_case(n, kind, L, tkind):
    """(frozen_pos, table, logits, (bits, pm, ok, stop) of the restatement), computed once and read-only.  67 rows,
    9 at n = 1024.  The "kill" cases keep, of a larger seeded draw of all four row kinds, the rows the restatement
    stops at the table's single CHECK: every row of the case dies there."""
    key = (n, kind, L, tkind)
    if key not in _CASE_CACHE:
        fp, table = case_frozen(n, kind), case_table(n, kind, L, tkind)
        rows = 9 if n >= 1024 else 67
        if tkind == "kill":
            x = make_inputs(fp, n, pack_constraints(n, []), LLR_MAX, 40 * rows, seed=1000 * n + L)
            stop = pcl_decode(x, fp, n, L, table, LLR_MAX)[3]
            x = x[stop == table[0][0]][:rows]
            assert x.shape[0] == rows, "the draw holds too few rows that die at the CHECK: draw more"
        else:
            x = make_inputs(fp, n, table, LLR_MAX, rows, seed=1000 * n + L)
        res = pcl_decode(x, fp, n, L, table, LLR_MAX)
        for a in (fp, x, *table, *res):
            a.setflags(write=False)
        _CASE_CACHE[key] = (fp, table, x, res)
    return _CASE_CACHE[key]
