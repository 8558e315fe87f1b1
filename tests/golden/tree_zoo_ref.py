"""The rate-0 zoo of the three register trees that keep only the rate-0 skip: csrc/sc_tree.h (the flip
decodes of pl_scf_decode and every candidate of pl_ae_decode) and its copy in csrc/scq_kernel.hip.

TEST INFRASTRUCTURE ONLY (tests/test_tree_zoo_ref.py audits it on the CPU, tests/test_tree_zoo_gpu.py runs it).

A skip that is missed is invisible (the recursion gives the same zeros); a skip that is falsely taken zeroes
information bits or drops an f pass.  So every code here plants rate-0 nodes NEXT TO nodes that are not
rate-0, and the audit shows that a decoder which skipped the neighbour instead would be caught on the very
rows the GPU test decodes.  A placement is (s, q, sibling): the stage-s node at position q << s is all frozen,
its sibling (s, q ^ 1) is not.

    small   n = 4 ... 32, one placement a code: every stage s = 1 ... log2 n - 1, the first, a middle and the
            last parent position, the rate-0 node once as the left and once as the right child; the sibling is
            a repetition node (all frozen but its last leaf: one flag away from rate-0), everything else the
            general filler of the node zoo (information first, frozen last, in pairs).
    zoo     polar_amd.build.node_zoo() at n = 64 ... 2048: its rate-0 nodes sit beside SPC, rate-1 and filler
            nodes at every stage 1 ... log2 n - 2, on both sides.
    extra   n = 64 ... 2048, two codes a length, for what the zoo lacks: one root half all frozen (the
            half_node flag, flag bits n - 4 and n - 3: the last used flag word), and in the other half pairs
            (rate-0, repetition) at the stages 1 ... log2 G + 1 (G = max(1, n / 128) lanes a decode: the stage
            log2 G is the `bottom` flag, the stages below it are the masks of `inl`), at the front of the half
            with the rate-0 node on one side and at its back with it on the other.  The stage-1 pair at
            position 0 has flag bit 0: the first flag word.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ae_ref  # noqa: E402
import scf_ref  # noqa: E402

SMALL_NS = (4, 8, 16, 32)
BIG_NS = (64, 128, 256, 512, 1024, 2048)
ROWS = 67      # SCQ and SC-Flip rows a code: a wave ends in a partial set at every lane-group width
AE_ROWS = 37   # AE rows a code (each is decoded up to 64 times by the restatement)
SCF_NMAX = AE_NMAX = 1024


def _filler(size):
    return np.tile(np.array([0, 1], np.uint8), size // 2)


def _rep(size):
    return np.r_[np.ones(size - 1, np.uint8), np.uint8(0)]


def plant(n, pairs, r0_half=None):
    """Mask [n] (1 = frozen) of filler with, for every (s, q) of pairs, the stage-s node q all frozen and its
    sibling q ^ 1 a repetition node; r0_half: the root half (0 / 1) that is all frozen.  Returns (mask, placements)."""
    mask = _filler(n)
    used = np.zeros(n, bool)
    out = []
    if r0_half is not None:
        h = n // 2
        mask[r0_half * h: (r0_half + 1) * h] = 1
        used[r0_half * h: (r0_half + 1) * h] = True
        out.append((n.bit_length() - 2, r0_half, "GEN"))
    for s, q in pairs:
        m = 1 << s
        lo = (q >> 1) << (s + 1)
        assert not used[lo: lo + 2 * m].any(), (n, s, q)
        used[lo: lo + 2 * m] = True
        mask[q * m: (q + 1) * m] = 1
        mask[(q ^ 1) * m: ((q ^ 1) + 1) * m] = _rep(m)
        out.append((s, q, "REP"))
    return mask, out


@functools.lru_cache(maxsize=None)
def small_codes():
    out = []
    for n in SMALL_NS:
        log_n = n.bit_length() - 1
        for s in range(1, log_n):
            parents = n >> (s + 1)
            for par in sorted({0, parents // 2, parents - 1}):
                for side in (0, 1):
                    mask, placed = plant(n, [(s, 2 * par + side)])
                    out.append((f"n{n}:s{s}q{2 * par + side}", mask, placed))
    return out


@functools.lru_cache(maxsize=None)
def extra_codes():
    out = []
    for n in BIG_NS:
        log_n, h = n.bit_length() - 1, n // 2
        log_g = max(log_n - 7, 0)
        stages = [s for s in range(1, log_g + 2) if s <= log_n - 4] or [1]
        if log_g == 0:
            stages = [1, 2]
        for r0_half in (1, 0):
            base = (1 - r0_half) * h  # first position of the general half
            pairs = []
            for s in stages:
                front = base + (0 if s == 1 else 2 << s)   # stage-1 pair at the half's first position
                back = base + h - ((2 << s) if s == 1 else (4 << s))
                # r0_half = 1: front pairs have the rate-0 node on the left, back pairs on the right; 0: swapped
                pairs.append((s, (front >> s) + (1 - r0_half)))
                pairs.append((s, (back >> s) + r0_half))
            mask, placed = plant(n, pairs, r0_half)
            out.append((f"n{n}:half{r0_half}R0," + ",".join(f"s{s}q{q}" for s, q in pairs), mask, placed))
    return out


@functools.lru_cache(maxsize=None)
def zoo_codes():
    from polar_amd import build
    out = []
    for name, mask, planted in build.node_zoo():
        placed = []
        for s, q, t in planted:
            if t == "R0":
                sib = np.asarray(mask[(q ^ 1) << s: ((q ^ 1) + 1) << s])
                placed.append((s, q, build.node_type(sib)))
        if placed:  # the zoo codes without a planted rate-0 node have nothing to say here
            out.append((name, np.asarray(mask, np.uint8), placed))
    return out


def all_codes():
    """[(name, mask, placements)]: small, zoo and extra codes, every name unique."""
    return small_codes() + zoo_codes() + extra_codes()


def codes_for(decoder):
    """The codes a decoder takes: SCQ all of them; SC-Flip and AE up to n = 1024, SC-Flip without the codes of
    one information bit (there a flip of the bit and a false skip of its node both decide 0: SC-Flip cannot
    tell them apart, whatever the rows).  That leaves SC-Flip without a zoo code at n = 4 and without the
    stage log2 n - 1 placements of n = 8 ... 32."""
    codes = all_codes()
    if decoder == "scq":
        return codes
    codes = [c for c in codes if len(c[1]) <= SCF_NMAX]
    if decoder == "scf":
        codes = [c for c in codes if int((c[1] == 0).sum()) > 1]
    return codes


def frozen_pos(mask):
    return np.flatnonzero(np.asarray(mask)).astype(np.int64)


def wrong_decoders(mask, placement):
    """The deliberately wrong decoders a placement (s, q, sibling) must be sensitive to, as the switches of
    scf_ref.sc_flip / scq_ref.sc_decode:
      false_r0  the sibling (s, q ^ 1) skipped as if it were rate-0 (a flag index off by one, the wrong plane);
                where the rate-0 node is the right child this is also the left-skip applied to the wrong side
      bl0       the left-skip mistake where it is not the same thing: g computed with bl = 0 although the left
                child is not rate-0, at the nearest node at or above the pair's parent whose two children are
                both not rate-0 (below it the mistake cannot show: one child decides nothing).  Named bl0_rep
                where that node's right child, which the wrong g feeds, is a repetition node."""
    from polar_amd import build
    mask = np.asarray(mask)
    n = len(mask)
    s, q, _ = placement
    out = [("false_r0", {"false_r0": (s, q ^ 1)})]
    ps, pq = s + 1, q >> 1
    while (1 << ps) <= n:
        m = 1 << ps
        lo = pq * m
        if not mask[lo: lo + m // 2].all() and not mask[lo + m // 2: lo + m].all():
            rep = build.node_type(mask[lo + m // 2: lo + m]) == "REP"
            out.append(("bl0_rep" if rep else "bl0", {"bl0": (ps, pq)}))
            break
        ps, pq = ps + 1, pq >> 1
    return out


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


# ---- SCQ ---------------------------------------------------------------------------------------------
SCQ_WIDTHS = (3, 8)


def scq_rows(name, n):
    """Uniform int8 rows over the whole range, -128 included."""
    q = np.random.default_rng([1, _seed(name)]).integers(-128, 128, size=(ROWS, n)).astype(np.int8)
    q[0, 0] = -128
    return q


# ---- SC-Flip -----------------------------------------------------------------------------------------
def scf_crc(k):
    """CRC11 from k = 24, CRC6 from k = 12; below that x^3 + x + 1 (k >= 6) and x^2 + x + 1 of scf_ref.CRC_POLYS.
    pl_plan_set_crc takes no degree above k, and CRC6 on k = 6 ... 11 bits leaves so few codewords (two at
    k = 7) that the bits a wrong g would change are 0 in every passing attempt: the audit cannot hold there."""
    name = "CRC11" if k >= 24 else "CRC6" if k >= 12 else "CRC3" if k >= 6 else "CRC2"
    return scf_ref.crc_params(name)


def scf_max_flips(k):
    return min(k, 16)


SCF_NOISE_ROWS = 12
SCF_RESCUED_ROWS = 40
SCF_CANDIDATES, SCF_TRIED = 330, 130
# per position amplitudes: a g whose operands differ in weight shows a wrong bl even on a row one flip rescues
SCF_AMPLITUDES = (0.4, 1.0, 3.0)
SCF_SIGMA = (0.15, 0.9)
# Draw number per code (default 0): the first draw on which the restatement shows every outcome class and every
# wrong decoder of every placement (tests/test_tree_zoo_ref.py asserts both).  Chosen on the CPU from the
# restatement alone.
SCF_RESEED = {
    'n32:s2q6':
        1,
    'n64:s4q0R1,s4q1R0,s5q1REP':
        2,
    'n128:s5q0R1,s5q1R0,s6q1REP':
        15,
    'n512:s7q0R1,s7q1R0,s8q1REP':
        7,
    'n1024:s9q0R1,s7q4REP,s7q5R1,s6q12R1,s6q13R0,s5q28SPC,s5q29REP,s4q60R0,s4q61SPC,s3q124REP,s3q125R1,s2q252R1,s2q253R0,s1q508R0,s1q511R1':
        1,
    'n1024:s8q0R1,s8q1R0,s9q1REP':
        19,
    'n128:half0R0,s1q33,s1q62,s2q19,s2q28':
        11,
    'n256:half1R0,s1q0,s1q63,s2q2,s2q29':
        9,
    'n256:half0R0,s1q65,s1q126,s2q35,s2q60':
        99,
    'n512:half1R0,s1q0,s1q127,s2q2,s2q61,s3q2,s3q29':
        13,
    'n512:half0R0,s1q129,s1q254,s2q67,s2q124,s3q35,s3q60':
        16,
    'n1024:half1R0,s1q0,s1q255,s2q2,s2q125,s3q2,s3q61,s4q2,s4q29':
        9,
    'n1024:half0R0,s1q257,s1q510,s2q131,s2q252,s3q67,s3q124,s4q35,s4q60':
        4,
}
AE_RESEED = {}


@functools.lru_cache(maxsize=None)
def _scf_rows(name):
    mask = {c[0]: c[1] for c in all_codes()}[name]
    n = len(mask)
    fp = frozen_pos(mask)
    info = np.flatnonzero(np.asarray(mask) == 0)
    k = len(info)
    deg, g = scf_crc(k)
    rng = np.random.default_rng([2, _seed(name), SCF_RESEED.get(name, 0)])
    msg = (rng.random((SCF_CANDIDATES, k - deg)) < 0.5).astype(np.uint8)
    u = np.zeros((SCF_CANDIDATES, n), np.uint8)
    u[:, info] = scf_ref.crc_attach(msg, deg, g)
    sigma = np.linspace(SCF_SIGMA[0], SCF_SIGMA[1], SCF_CANDIDATES)[:, None]
    amp = rng.choice(SCF_AMPLITUDES, size=(SCF_CANDIDATES, n))
    y = amp * (1.0 - 2.0 * scf_ref.encode(u)) + sigma * rng.standard_normal((SCF_CANDIDATES, n))
    x = (-2.0 * amp * y / sigma ** 2).astype(np.float32)
    u0, _, _ = scf_ref.sc_flip(x, fp, n, np.full(SCF_CANDIDATES, -1))
    fail = np.flatnonzero(~scf_ref.crc_ok(u0[:, info], deg, g))[:SCF_TRIED]
    ref = scf_ref.scf_decode(x[fail], fp, n, (deg, g), scf_max_flips(k))
    won = fail[ref["flip_pos"] >= 0][:SCF_RESCUED_ROWS]
    rest = np.setdiff1d(fail, won)[: ROWS - SCF_NOISE_ROWS - len(won)]
    noise = (rng.standard_normal((ROWS - len(won) - len(rest), n)) * 4).astype(np.float32)
    return fp, (deg, g), np.concatenate([x[np.sort(np.r_[won, rest])], noise])


def scf_rows(name, mask):
    """(frozen_pos, (degree, mask), logits [67, n]): noise-dominated rows that fail attempt 0.  Candidates are
    codewords with a valid CRC at +-0.4, +-1 or +-3 (drawn per position) under noise whose deviation climbs from
    0.15 to 0.9 over 330 rows (the zoo
    codes are poor codes, each with a noise level of its own at which one decision is wrong).  The restatement
    decodes the 130 least noisy ones whose plain SC result fails the CRC; kept are up to 40 that one flip
    rescues, then the least noisy of the others up to 55 rows, and rows of noise alone up to 67.  The choice
    looks at the restatement's outcome classes only, never at a device result."""
    assert len(mask) == len(_scf_rows(name)[0]) + int((np.asarray(mask) == 0).sum())
    fp, crc, x = _scf_rows(name)
    return fp.copy(), crc, x.copy()


# ---- AE ----------------------------------------------------------------------------------------------
def ae_num_perms(n):
    """2 C + 1 candidates (C = 64 / G decodes a pass: three passes) where pl_ae_decode takes that many
    (n = 512: 33, n = 1024: 17); its cap of 64 below that (n = 256: two passes, n <= 128: one)."""
    c = 64 // max(1, n // 128)
    return min(2 * c + 1, 64)


@functools.lru_cache(maxsize=None)
def ae_table(n):
    """[M, n]: the identity, distinct seeded bit-index permutations (as many as there are, at most M - 2),
    seeded random permutations for the rest, one of them last.  None need be an automorphism of a zoo code."""
    from polar_amd import automorphism
    m_tot, log_n = ae_num_perms(n), n.bit_length() - 1
    rng = np.random.default_rng([3, n])
    rows, seen = [np.arange(n)], {tuple(range(log_n))}
    for _ in range(4096):
        if len(rows) >= m_tot - 1:
            break
        sigma = tuple(int(v) for v in rng.permutation(log_n))
        if sigma not in seen:
            seen.add(sigma)
            rows.append(automorphism.perm_table([1 << b for b in sigma], n))
    while len(rows) < m_tot:
        rows.append(rng.permutation(n))
    return np.stack(rows).astype(np.int64)


def ae_tables_compared(table):
    """The tables a code is decoded with: all M candidates (the winner hides most of a single wrong decode), and
    candidate 0, the identity, alone (M = 1: every row shows the tree's own decode)."""
    return [table, table[:1]]


def ae_rows(name, mask):
    """Grid logits (integers / 8, magnitude <= 16): 18 rows of ae_ref.exact_grid_llrs (noisy codewords, zeros, a
    row of zeros last) and in front of them 19 rows drawn uniformly from the grid, on which every decision is
    marginal and a wrong g shows."""
    n = len(mask)
    seed = _seed(name) + AE_RESEED.get(name, 0)
    noise = np.random.default_rng([4, seed]).integers(-128, 129, size=(AE_ROWS - 18, n)).astype(np.float32) / np.float32(8)
    return np.concatenate([noise, ae_ref.exact_grid_llrs(seed, 18, n, frozen_pos(mask))])
