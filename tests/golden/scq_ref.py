"""Fixed-point SC decoding on int8 LLRs in plain numpy: the rule pl_scq_decode / pl_llr_quantize are pinned to.

TEST INFRASTRUCTURE ONLY.  The contract is that of include/polar_mi355x.h, all in integers:

    Imax = 2^(q_internal-1) - 1, Cmax = 2^(q_channel-1) - 1
    quantize    t = float32(logit) * float32(inv_step) (one fp32 rounding), q = rint(clip(t, -Cmax, Cmax)),
                ties to even, int8; +-Inf saturates
    load        a_i = -clip(llr_q_i, -Imax, Imax)
    f(x, y)     sgn(x) sgn(y) min(|x|, |y|), sgn(0) = 0
    g(x, y, b)  clip(y + (1 - 2b) x, -Imax, Imax)
    leaf        frozen -> 0, else HD(a) = !(a > 0)   (0 decides 1)

sc_decode() is the plain recursion (left child on f, right child on g with the left child's re-encoded bits),
vectorised over rows on int32, without any shortcut.  It also counts what saturated, so that a test can assert
that its inputs exercise the clamps.
"""
import numpy as np


def imax(q):
    return (1 << (int(q) - 1)) - 1


def quantize(logits, inv_step, q_channel):
    """int8 levels of fp32 logits (any shape)."""
    c = np.float32(imax(q_channel))
    with np.errstate(over="ignore", under="ignore"):
        t = np.asarray(logits, dtype=np.float32) * np.float32(inv_step)
    assert t.dtype == np.float32
    return np.rint(np.clip(t, -c, c)).astype(np.int8)


def quantizer_vectors():
    """(logits fp32, inv_step, q_channel, expected int8): exact ties at a power-of-two step, signed zeros, Inf,
    a finite value whose product overflows, denormals, and the whole range."""
    step = np.float32(0.25)
    inv = np.float32(4.0)
    j = np.arange(-40, 40, dtype=np.float32)
    ties = (j + np.float32(0.5)) * step  # t = j + 1/2 exactly: ties go to the even neighbour
    want_ties = np.clip(np.where(np.floor(j) % 2 == 0, j, j + 1), -31, 31)
    x = np.concatenate([ties, np.array([0.0, -0.0, np.inf, -np.inf, 1e30, -1e30, 3e38, -3e38, 1e-45, -1e-45, 1e-39,
                                        7.74, 7.76, -7.74, -7.76, 100.0, -100.0], dtype=np.float32)])
    want = np.concatenate([want_ties, [0, 0, 31, -31, 31, -31, 31, -31, 0, 0, 0, 31, 31, -31, -31, 31, -31]])
    return x.astype(np.float32), float(inv), 6, want.astype(np.int8)


def _node(a, frozen, im, stats, pos=0, wrong=None):
    """a [rows, m] int32, frozen [m] bool -> the node's partial sums [rows, m] (uint8) and its u [rows, m].
    pos: the node's first position; wrong: sc_decode's false_r0 / bl0 switches."""
    m = a.shape[1]
    here = (m.bit_length() - 1, pos // m)
    if wrong and wrong.get("false_r0") == here:
        return np.zeros(a.shape, np.uint8), np.zeros(a.shape, np.uint8)
    if m == 1:
        u = np.zeros(a.shape, np.uint8) if frozen[0] else (~(a > 0)).astype(np.uint8)
        return u, u
    h = m // 2
    x, y = a[:, :h], a[:, h:]
    fl = np.sign(x) * np.sign(y) * np.minimum(np.abs(x), np.abs(y))
    bl, ul = _node(fl, frozen[:h], im, stats, pos, wrong)
    bg = np.zeros_like(bl) if wrong and wrong.get("bl0") == here else bl
    s = y + (1 - 2 * bg.astype(np.int32)) * x
    gr = np.clip(s, -im, im)
    stats["g_total"] += s.size
    stats["g_clamped"] += int((gr != s).sum())
    br, ur = _node(gr, frozen[h:], im, stats, pos + h, wrong)
    return np.concatenate([bl ^ br, br], axis=1), np.concatenate([ul, ur], axis=1)


def sc_decode(llr_q, frozen_pos, q_internal, return_stats=False, wrong=None):
    """llr_q [rows, n] int8 (logit sign, any value) -> [rows, k] uint8 bits at the information positions,
    ascending.  return_stats: also {"load_clamped", "g_clamped", "g_total"}, counts over the whole call.
    wrong = {"false_r0": (s, q)} or {"bl0": (s, q)} models a deliberately WRONG decoder at the stage-s node at
    position q << s (tests/test_tree_zoo_ref.py only): the node is treated as all frozen although it is not, or
    its g is computed with the left child's partial sums taken as 0 although the left child was decoded."""
    q = np.asarray(llr_q)
    assert q.dtype == np.int8 and q.ndim == 2
    n = q.shape[1]
    assert n >= 2 and n & (n - 1) == 0 and 2 <= q_internal <= 8
    im = imax(q_internal)
    frozen = np.zeros(n, bool)
    frozen[np.asarray(frozen_pos, dtype=np.int64)] = True
    q32 = q.astype(np.int32)
    a = -np.clip(q32, -im, im)
    stats = {"load_clamped": int((np.abs(q32) > im).sum()), "g_clamped": 0, "g_total": 0}
    _, u = _node(a, frozen, im, stats, 0, wrong)
    bits = np.ascontiguousarray(u[:, ~frozen])
    return (bits, stats) if return_stats else bits


def random_frozen(n, k, seed):
    """A seeded random frozen set of n - k positions (ascending)."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.permutation(n)[: n - k]).astype(np.int64)


def rm_frozen(n):
    """The pinned RM-weight set of the largest rate <= 1/2 code of length n in frozen_sets.npz, or None."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "polar-code-pytorch-sionna_amd",
                        "polar_amd", "data", "frozen_sets.npz")
    with np.load(path) as d:
        ks = sorted(int(key.split("_")[0][1:]) for key in d.files if int(key.split("_")[1][1:]) == n)
        ks = [k for k in ks if 2 * k <= n] or ks
        return d[f"k{ks[-1]}_n{n}"].astype(np.int64) if ks else None
