"""Soft-cancellation (SCAN) polar decoding in plain numpy: the contract pl_scan_decode is pinned to.

TEST INFRASTRUCTURE ONLY.  A restatement of include/polar_mi355x.h (pl_scan_decode), every operation fp32
in the stated order.  Messages, initial values, f, clip and the outputs are pl_bp_decode's (bp_ref.py);
only the schedule differs.  One iteration is node(S, 0); node(0, .) does nothing; node(s, b), h = 2^(s-1),
for every i in [b, b+h):

    L[s-1][i]   = clip(f(L[s][i], L[s][i+h] + R[s-1][i+h]))      R[s-1][i+h] of the previous iteration
    node(s-1, b)
    L[s-1][i+h] = clip(f(L[s][i], R[s-1][i]) + L[s][i+h])        R[s-1][i] just written by the left child
    node(s-1, b+h)
    R[s][i]     = clip(f(R[s-1][i], L[s][i+h] + R[s-1][i+h]))
    R[s][i+h]   = clip(f(R[s-1][i], L[s][i]) + R[s-1][i+h])

With the exact f a row is FRAGILE when any f it evaluated lay so near a rounding midpoint that a correct
device form may round the other way (exactf_cr.f_cr); a comparison leaves such rows out.
"""
import numpy as np

from bp_ref import (EXACT_CASES, FRAGILE_CAP, F32, awgn_logits, clip, early_stop_inputs, encode,  # noqa: F401
                    f_minsum, make_inputs, noiseless_logits, rate_half_frozen)


def scan_decode(llr_logits, frozen_pos, n, num_iter, llr_max=19.3, exact=False, scale=1.0, early_stop=False):
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

    # [stage, position, row]: a node's positions are a contiguous slab
    L = np.zeros((s_tot + 1, n, rows), dtype=F32)
    R = np.zeros((s_tot + 1, n, rows), dtype=F32)
    L[s_tot] = clip(-x, llr_max).T
    R[0][frozen, :] = F32(llr_max)
    fragile = np.zeros(rows, dtype=bool)
    iters = np.full(rows, num_iter, dtype=np.int32)
    state = {"act": np.ones(rows, dtype=bool)}  # the rows still iterating

    def f(a, b):
        if exact:
            o, fr = f_cr(np.ascontiguousarray(a), np.ascontiguousarray(b), llr_max)
            fragile[state["act"]] |= fr.any(axis=0)
            return o
        return f_minsum(np.ascontiguousarray(a), np.ascontiguousarray(b), llr_max, scale)

    def node(s, b):
        if s == 0:
            return
        a = state["act"]
        h = 1 << (s - 1)
        lo, hi = slice(b, b + h), slice(b + h, b + 2 * h)
        L[s - 1][lo, a] = clip(f(L[s][lo, a], (L[s][hi, a] + R[s - 1][hi, a]).astype(F32)), llr_max)
        node(s - 1, b)
        L[s - 1][hi, a] = clip((f(L[s][lo, a], R[s - 1][lo, a]) + L[s][hi, a]).astype(F32), llr_max)
        node(s - 1, b + h)
        r_lo = clip(f(R[s - 1][lo, a], (L[s][hi, a] + R[s - 1][hi, a]).astype(F32)), llr_max)
        r_hi = clip((f(R[s - 1][lo, a], L[s][lo, a]) + R[s - 1][hi, a]).astype(F32), llr_max)
        R[s][lo, a], R[s][hi, a] = r_lo, r_hi

    with np.errstate(over="ignore", invalid="ignore"):
        for it in range(num_iter):
            a = state["act"]
            if not a.any():
                break
            node(s_tot, 0)
            if early_stop:
                idx = np.flatnonzero(a)
                uh = (~(L[0][:, a].T > 0)) & ~frozen[None, :]
                xh = ~((L[s_tot][:, a] + R[s_tot][:, a]).astype(F32).T > 0)
                stop = (encode(uh) == xh.astype(np.uint8)).all(axis=1)
                iters[idx[stop]] = it + 1
                a = a.copy()
                a[idx[stop]] = False
                state["act"] = a

    info = ~frozen
    l0 = L[0].T
    return {"bits": (~(l0[:, info] > 0)).astype(np.uint8), "soft_u": (-l0[:, info]).astype(F32),
            "ext_x": np.ascontiguousarray((-R[s_tot]).T.astype(F32)), "iters": iters, "fragile": fragile}


# ---- the cases tests/test_scan_gpu.py compares on (tests/test_scan_ref.py checks what they assume) ----
MINSUM_CODES = [(n, None) for n in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)] + [(64, 64), (64, 1)]
MINSUM_ROWS, MINSUM_ITERS = 67, (1, 2, 3)
SCALED_SIZES, SCALE = (8, 256), 0.9375

# exact f: bp_ref.EXACT_CASES plus n = 2048 (one iteration; 32 rows there, EXACT_ROWS elsewhere)
SCAN_EXACT_CASES = list(EXACT_CASES) + [(2048, 1, 19.3)]
EXACT_ROWS = 128


def exact_case_inputs(n, num_iter, llr_max):
    """(frozen_pos, logits) of one exact-f case."""
    fp = rate_half_frozen(n, 7000 + n)
    _, x = make_inputs(7100 + n + num_iter + int(llr_max), n, fp, 32 if n == 2048 else EXACT_ROWS, llr_max)
    return fp, x


# early stop: early_stop_inputs with rate_half_frozen(n, 0), EARLY_STOP_ITERS iterations.  n = 4 ... 512 show rows
# stopping after 1 iteration, after 2 ... 5 and never; at n = 2 every row stops after 1; at n = 1024 and 2048 the
# inputs show "1" and "never" only (tests/test_scan_ref.py asserts each of these).
EARLY_STOP_SIZES = (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
EARLY_STOP_FROZEN_SEED = 0
EARLY_STOP_ITERS = 6


def early_stop_classes(n):
    """(after one, after 2 .. 5, never): the classes the early-stop inputs of size n must show."""
    if n == 2:
        return (True, False, False)
    return (True, n <= 512, True)
