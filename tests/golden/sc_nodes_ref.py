"""Instrumented min-sum SC restatement and the channel rows of the node-zoo tests.

TEST INFRASTRUCTURE ONLY (tests/test_sc_nodes_ref.py, tests/test_sc_nodes_gpu.py).

sc_ref       plain numpy SC recursion, vectorised over rows, with NO node shortcut: the root input
             is the negated channel, f is min-sum on inputs clipped at llr_max, g = (1-2u)x + y is
             unclipped, a leaf decides 1 iff its LLR is <= 0, partial sums are [uL^uR, uR] (the
             rules quoted at the top of csrc/sc_static.h).  Returns the information bits and the
             fp32 input vector (alpha) of every requested node (s, q) = stage-s node at q << s.
construct    channel rows that make the alpha of one node exactly a given vector.
classify     which path a shortcut node takes on an alpha: the fast path or one of its escapes.
make_batch   the rows of one zoo code, in aligned 64-row runs of one class per planted node.

The sign of a zero is not part of any contract here: no decision of the decoder observes it, f is
evaluated as sign-xor and minimum, and alphas are compared with == (so -0.0 equals 0.0; every
other value compares bit for bit).
"""
import functools

import numpy as np

LLR_MAX = 30.0
RUN = 64  # rows per run: a wave of either SC kernel holds 64 / G consecutive rows, G = 1 ... 16
SLOTS = (0, 33, 63)  # the escaping row of a mixed run: first, a middle and last slot of a wave


def sc_ref(llr, mask, want=(), llr_max=LLR_MAX, rules=None):
    """(bits float32 [bs, k], {(s, q): alpha float32 [bs, 2^s]}) of min-sum SC, no shortcuts.
    rules = {(s, q): alpha -> beta} replaces the recursion at those nodes (only the tests that show
    a wrong shortcut rule is caught use it)."""
    llr = np.ascontiguousarray(llr, dtype=np.float32)
    frozen = np.asarray(mask).astype(bool)
    bs, n = llr.shape
    log_n = n.bit_length() - 1
    assert 1 << log_n == n == len(frozen)
    lm = np.float32(llr_max)
    want = set(want)
    alphas = {}
    u = np.zeros((bs, n), dtype=np.uint8)

    def rec(a, s, q):
        if (s, q) in want:
            alphas[(s, q)] = a.copy()
        if rules and (s, q) in rules:
            beta = rules[(s, q)](a).astype(np.uint8)
            x = beta.copy()  # u = beta G (the transform is an involution), frozen positions forced to 0
            for t in range(s):
                x = x.reshape(bs, -1, 2, 1 << t)
                x[:, :, 0] ^= x[:, :, 1]
                x = x.reshape(bs, -1)
            u[:, q << s: (q + 1) << s] = x * ~frozen[q << s: (q + 1) << s]
            return beta
        if s == 0:
            if not frozen[q]:
                u[:, q] = a[:, 0] <= 0
            return u[:, q:q + 1].copy()
        h = a.shape[1] // 2
        lo, hi = a[:, :h], a[:, h:]
        m = np.minimum(np.minimum(np.abs(lo), np.abs(hi)), lm)  # min of the clipped magnitudes
        bl = rec(np.where(np.signbit(lo) ^ np.signbit(hi), -m, m), s - 1, 2 * q)
        br = rec(np.where(bl.astype(bool), -lo, lo) + hi, s - 1, 2 * q + 1)
        return np.concatenate([bl ^ br, br], axis=1)

    rec(-llr, log_n, 0)
    return u[:, ~frozen].astype(np.float32), alphas


def path_turns(n, s, q):
    """Turns from the root down to node (s, q), top first: 0 = left child, 1 = right child."""
    log_n = n.bit_length() - 1
    return [(q >> (t - 1 - s)) & 1 for t in range(log_n, s, -1)]


def delivered(n, s, q, alpha, halve=False, llr_max=LLR_MAX):
    """What construct() can deliver of `alpha`: every left turn on the path is an f, which clips at
    llr_max.  With halve the node's own right turn carries alpha / 2 on both sides, so the bound
    above it is 2 llr_max."""
    turns = path_turns(n, s, q)
    if halve:
        assert turns[-1] == 1
        turns = turns[:-1]
    if 0 not in turns:
        return np.asarray(alpha, np.float32)
    b = np.float32(llr_max * (2 if halve else 1))
    return np.clip(np.asarray(alpha, np.float32), -b, b)


def construct(n, s, q, alpha, rng=None, halve=False, llr_max=LLR_MAX):
    """Channel rows [R, n] on which the stage-s node q has input alpha [R, 2^s] (as far as
    delivered() allows).  Walking up from the node: below a left turn the partner (upper half of
    the parent's input) is BIG >= llr_max and positive, so f(v, BIG) = v for |v| <= llr_max; below
    a right turn the lower half is 0, so g = +-0 + v = v whatever the left sibling decided.  The
    root input is the negated channel.  halve (a right child whose left sibling is rate-0, which
    decides u = 0): the parent's halves are alpha / 2 each, g = alpha / 2 + alpha / 2 exactly.
    A whole node vector fixes every entry of the row: the only freedom left is the magnitude of
    the BIG partners, drawn from rng in [llr_max, 4 llr_max]."""
    cur = np.atleast_2d(np.asarray(alpha, np.float32))
    assert cur.shape[1] == 1 << s
    for t, turn in enumerate(reversed(path_turns(n, s, q))):
        if turn == 0:
            big = np.full(cur.shape, llr_max, np.float32)
            if rng is not None:
                big = (big * (1 + 3 * rng.random(cur.shape))).astype(np.float32)
            cur = np.concatenate([cur, big], axis=1)
        elif halve and t == 0:
            cur = np.concatenate([cur * np.float32(0.5)] * 2, axis=1)
        else:
            cur = np.concatenate([np.zeros_like(cur), cur], axis=1)
    assert cur.shape[1] == n
    return -cur


# ---- classes ---------------------------------------------------------------------------------
def rep_sums(a):
    """(SC's pairwise g-order sum, sequential left-to-right sum, reversed sum) of rows, fp32."""
    a = np.asarray(a, np.float32)
    y = a
    while y.shape[1] > 1:
        h = y.shape[1] // 2
        y = y[:, :h] + y[:, h:]
    seq = a[:, 0].copy()
    for j in range(1, a.shape[1]):
        seq = seq + a[:, j]
    rev = a[:, -1].copy()
    for j in range(a.shape[1] - 2, -1, -1):
        rev = rev + a[:, j]
    return y[:, 0], seq, rev


def classes_of(typ, size):
    """The classes that apply to a node type (the first is its plain fast path)."""
    if typ == "SPC":
        return ("fast_even", "fast_odd", "zero", "odd_tie", "odd_clip")
    if typ == "R1":
        return ("fast", "zero")
    if typ == "REP":
        return ("plain", "order") if size >= 8 else ("plain",)
    return ("plain",)


def escapes_of(typ, size):
    """The classes of a type that one row brings into a run of fast-path rows: the escapes of
    rate-1 and SPC, and REP's order-sensitive rows (REP and rate-0 have no escape: a rate-0 node
    and a REP node below size 8 have a single class, so no run of theirs can mix)."""
    return {"SPC": ("zero", "odd_tie", "odd_clip"), "R1": ("zero",),
            "REP": ("order",) if size >= 8 else ()}.get(typ, ())


def classify(alpha, typ, llr_max=LLR_MAX):
    """Class of every row of alpha [R, S] at a node of type typ (array of str)."""
    a = np.asarray(alpha, np.float32)
    out = np.full(a.shape[0], "plain", dtype=object)
    zero = (a == 0).any(axis=1)
    if typ == "R1":
        out[:] = np.where(zero, "zero", "fast")
    elif typ == "SPC":
        mag = np.abs(a)
        mn = mag.min(axis=1)
        odd = (np.signbit(a).sum(axis=1) & 1) == 1
        tie = (mag == mn[:, None]).sum(axis=1) > 1
        out[:] = np.where(zero, "zero", np.where(~odd, "fast_even", np.where(
            mn >= np.float32(llr_max), "odd_clip", np.where(tie, "odd_tie", "fast_odd"))))
    elif typ == "REP" and a.shape[1] >= 8:
        pair, seq, rev = rep_sums(a)
        order = ((seq > 0) == (rev > 0)) & ((seq > 0) != (pair > 0)) & (pair != 0) & (seq != 0) & (rev != 0)
        out[:] = np.where(order, "order", "plain")
    return out


# ---- alpha families --------------------------------------------------------------------------
def _set_parity(a, odd, rng):
    """Flip one sign per row where needed so that the number of negative entries is odd / even."""
    a = a.copy()
    par = (np.signbit(a).sum(axis=1) & 1) == 1
    rows = np.flatnonzero(par != odd)
    cols = rng.integers(0, a.shape[1], len(rows))
    a[rows, cols] = -a[rows, cols]
    return a


@functools.lru_cache(maxsize=None)
def rep_order_rows(size, count=RUN):
    """count REP vectors of `size` >= 8 whose sequential and reversed fp32 sums both have the sign
    opposite to SC's pairwise g-order sum: +-B pairs (B in [16, 30), below llr_max so a left child
    can carry them) across the first pairing level, whose residuals of a few ulp(B) the pairwise
    order adds exactly and the sequential orders round away.  Seeds are searched until found."""
    assert size >= 8
    ulp = np.float32(2.0 ** -19)  # ulp of [16, 32)
    found, seed = [], 0
    while sum(len(f) for f in found) < count:
        rng = np.random.default_rng([size, seed])
        seed += 1
        k, h = 4096, size // 2
        b = (rng.uniform(16.0, 30.0, (k, h)) * rng.choice([-1.0, 1.0], (k, h))).astype(np.float32)
        d = rng.integers(-3, 4, (k, h)).astype(np.float32) * ulp
        a = np.concatenate([b, -b + d], axis=1).astype(np.float32)
        swap = rng.random((k, h)) < 0.5  # which half holds the residual
        lo = np.where(swap, a[:, h:], a[:, :h])
        hi = np.where(swap, a[:, :h], a[:, h:])
        a = np.concatenate([lo, hi], axis=1)
        found.append(a[classify(a, "REP") == "order"])
    return np.concatenate(found)[:count]


def family(typ, side, cls, size, rows, rng, llr_max=LLR_MAX):
    """rows alpha vectors [rows, size] meant for class cls of a type-typ node that is a left
    (side 0) or right (side 1) child."""
    a = (rng.standard_normal((rows, size)) * 2.5).astype(np.float32)
    r = np.arange(rows)
    if cls in ("plain", "fast"):
        return a
    if cls == "order":
        return rep_order_rows(size)[r % RUN]
    if cls == "zero":  # one planted zero, every other row a -0.0
        a[r, rng.integers(0, size, rows)] = np.where(r & 1, np.float32(-0.0), np.float32(0.0))
        return a
    if cls == "fast_even":
        return _set_parity(a, False, rng)
    if cls == "fast_odd":
        return _set_parity(a, True, rng)
    if cls == "odd_tie":  # the minimum magnitude duplicated once, with a random sign
        mag = np.abs(a)
        i = mag.argmin(axis=1)
        j = (i + rng.integers(1, size, rows)) % size
        a[r, j] = mag[r, i] * rng.choice([-1.0, 1.0], rows).astype(np.float32)
        return _set_parity(a, True, rng)
    assert cls == "odd_clip"
    if side == 0:  # a left child's input is an f output: the minimum can only equal llr_max
        mag = np.full((rows, size), llr_max, np.float32)
    else:
        mag = rng.uniform(1.05 * llr_max, 1.9 * llr_max, (rows, size)).astype(np.float32)
    return _set_parity(mag * rng.choice([-1.0, 1.0], (rows, size)).astype(np.float32), True, rng)


def unconstructed(n, rows, rng):
    """Rows no construction touched: continuous, the half-integer grid with zeros, x40 saturated."""
    a = (rng.standard_normal((rows, n)) * 2.5).astype(np.float32)
    third = rows // 3
    a[third:2 * third] = (np.round(rng.standard_normal((third, n)) * 2) * 0.5).astype(np.float32)
    a[2 * third:] *= np.float32(40.0)
    return a


def run_plan(s, q, typ):
    """(class, kind, slot) of the runs of a planted node: the slot rotates with the stage, the side
    and the class, so over the stages of one n every escape class sits at every slot."""
    plan = [(c, "aligned", -1) for c in classes_of(typ, 1 << s)]
    return plan + [(c, "mixed", SLOTS[(s + (q & 1) + j) % 3]) for j, c in enumerate(escapes_of(typ, 1 << s))]


def make_batch(n, mask, planted, seed=0, tail=37, llr_max=LLR_MAX):
    """The rows of one zoo code.  Per planted node (s, q, type): one aligned run of RUN rows per
    class of the type, then one mixed run per escape class -- fast-path rows with a single row of
    that class at a first / middle / last slot (SLOTS, see run_plan) -- and
    after all runs as many unconstructed rows plus a ragged tail.
    Returns dict(llr, alpha = intended alpha of every constructed row (list per run),
    runs = [dict(node, cls, kind, slot, start)], row_node = planted index per row or -1)."""
    mask = np.asarray(mask)
    llrs, alphas, runs = [], [], []
    for i, (s, q, typ) in enumerate(planted):
        size, side = 1 << s, q & 1
        rng = np.random.default_rng([seed, n, s, q])
        # a right child next to a rate-0 sibling sees x + y of its parent's halves
        halve = side == 1 and bool(mask[(q - 1) << s: q << s].all())
        for cls, kind, slot in run_plan(s, q, typ):
            if kind == "aligned":
                a = family(typ, side, cls, size, RUN, rng, llr_max)
            else:
                a = family(typ, side, classes_of(typ, size)[0], size, RUN, rng, llr_max)
                if typ == "SPC":  # both parities among the fast rows
                    a = _set_parity(a, np.arange(RUN) % 2 == 1, rng)
                a[slot] = family(typ, side, cls, size, RUN, rng, llr_max)[slot]
            a = delivered(n, s, q, a, halve, llr_max)
            runs.append(dict(node=i, cls=cls, kind=kind, slot=slot, start=RUN * len(runs)))
            alphas.append(a)
            llrs.append(construct(n, s, q, a, rng, halve, llr_max))
    built = RUN * len(runs)
    llrs.append(unconstructed(n, built + tail, np.random.default_rng([seed, n, 1 << 20])))
    row_node = np.full(2 * built + tail, -1)
    for r in runs:
        row_node[r["start"]: r["start"] + RUN] = r["node"]
    return dict(llr=np.concatenate(llrs).astype(np.float32), alpha=alphas, runs=runs, row_node=row_node)
