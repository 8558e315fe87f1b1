"""Frozen-set design on the GPU: genie-aided Monte-Carlo SC construction.

The classical construction (Arikan 2009, section IX): run SC with the true bits fed back, count
the decision errors of each of the n bit channels over many noisy codewords, freeze the worst
n - k.  The codewords come from the fused link producer (ops.awgn_qam_llr) over a plan with no
frozen position, so every position carries a random bit -- which also averages over the unequal
bit levels of 16/64/256-QAM, where an all-zero codeword would not -- at the noise variance of the
design rate k/n; the bit-channel leaves and their error counts are one kernel (ops.genie_count,
csrc/genie_kernel.hip).  Philox is keyed, so a design is reproducible bit for bit.

    fp = design_frozen_pos(512, 1024, ebno_db=2.5)          # sorted int64 tensor, as reference_frozen_pos
"""
import numpy as np
import torch as tc


def bit_channel_errors(n, k, ebno_db, rows, num_bits_per_symbol=2, f_mode=0, llr_max=30.0, seed=0, batch=65536,
                       device=None):
    """(counts int64[n] numpy, rows_done): counts[i] = the codewords, of rows_done drawn at ebno_db
    for the rate k/n over 2^m-QAM, whose genie-aided SC decision of position i is wrong.  One Philox
    iteration per batch of `batch` rows (the last one shorter), all into one device counter vector."""
    from . import _lib, ops
    from .channel import ebnodb2no
    n, k, rows, batch = int(n), int(k), int(rows), int(batch)
    if not 1 <= k <= n:
        raise ValueError(f"the design rate needs 1 <= k <= n, got k = {k}, n = {n}")
    if rows < 0 or batch < 1:
        raise ValueError(f"rows must be >= 0 and batch >= 1, got {rows}, {batch}")
    m = ops.check_bits_per_symbol(num_bits_per_symbol, n, "the code length n")
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    no = float(ebnodb2no(float(ebno_db), m, k / n))
    plan = _lib.Plan(n, np.zeros(n, dtype=np.uint8), 1, flags=_lib.PL_PLAN_GENERIC, device=dev)  # k_plan = n
    counts = tc.zeros(n, dtype=tc.int64, device=dev)
    done, it = 0, 0
    while done < rows:
        bs = min(batch, rows - done)
        _, ubits, _, llr = ops.awgn_qam_llr(plan, m, bs, no, seed, it, with_u=False, with_ubits=True)
        ops.genie_count(n, llr, ubits, f_mode=f_mode, llr_max=llr_max, counts=counts)
        done += bs
        it += 1
    return counts.cpu().numpy(), done


def select_frozen(counts, k):
    """Sorted int64 frozen positions (torch tensor) of the (k, n) code designed from per-position
    error counts: the information set is the k positions smallest under the key (count ascending,
    popcount(i) descending, i descending) -- deterministic; ties (the zero counts of the good
    channels above all) fall back to the RM weight, then to the later position."""
    c = np.asarray(counts.cpu() if isinstance(counts, tc.Tensor) else counts).astype(np.int64).reshape(-1)
    n, k = len(c), int(k)
    if not 0 <= k <= n:
        raise ValueError(f"k must be in [0, {n}], got {k}")
    i = np.arange(n, dtype=np.int64)
    pop = np.array([bin(int(v)).count("1") for v in i], dtype=np.int64)
    order = np.lexsort((-i, -pop, c))  # last key first: count, then popcount descending, then i descending
    return tc.from_numpy(np.sort(order[k:]).astype(np.int64))


def union_bound(counts, rows, frozen_pos):
    """The estimated union bound on the SC block error rate of the designed code: the sum over its
    information positions of counts / rows."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    info = np.ones(len(c), dtype=bool)
    info[np.asarray(frozen_pos, dtype=np.int64)] = False
    return float(c[info].sum() / max(int(rows), 1))


def design_frozen_pos(k, n, ebno_db, rows=2 ** 20, **kw):
    """select_frozen(bit_channel_errors(n, k, ebno_db, rows, **kw), k): the frozen positions of the
    (k, n) code matched to ebno_db (and to the modulation, num_bits_per_symbol)."""
    counts, _ = bit_channel_errors(n, k, ebno_db, rows, **kw)
    return select_frozen(counts, k)
