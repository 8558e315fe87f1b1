"""Drop-in ordered-statistics decoder: OSDecoder <-> my_sn/fec/osd/dec.py:8-192.

Order-t OSD estimates the maximum-likelihood performance of a short code, the curve a list decoder
is measured against.  The constructor takes the reference's arguments and makes its checks; the
generator matrix is built as the reference builds it, by encoding the identity, so any encoder with
`.k` that maps [k, k] -> [k, n] works (channel.GpuEncoder, a dense u @ G encoder, Polar5GEncoder).
Decoding runs in libpolar_mi355x.so (csrc/osd_kernel.hip, one wave per codeword); CPU inputs are
copied over and back as SC_Dec does, and without a GPU forward raises.

Among equal |llr| the lower index is the more reliable one (the reference's argsort leaves that
order open).  The envelope is 1 <= k <= 128, k <= n <= 256, 0 <= t <= min(k, 4) and at most 2^22
error patterns; a code outside it is a ValueError at construction.
"""
import math

import numpy as np
import torch as tc
from torch import nn

from . import _lib, ops
from .decoders import _gpu_for

MAX_K, MAX_N, MAX_T, MAX_PATTERNS = 128, 256, 4, 1 << 22


def num_patterns(k, t):
    """The candidates an order-t search over k basis rows tries: sum of C(k, i), i = 1 .. t."""
    return sum(math.comb(int(k), i) for i in range(1, int(t) + 1))


def check_supported(k, n, t):
    """ValueError for a code or an order outside the kernel's envelope (include/polar_mi355x.h)."""
    k, n, t = int(k), int(n), int(t)
    limits = (f"the MI355X OSD kernel takes 1 <= k <= {MAX_K}, k <= n <= {MAX_N}, 0 <= t <= min(k, {MAX_T}) "
              f"and at most 2^22 error patterns")
    if not (1 <= k <= MAX_K and k <= n <= MAX_N and 0 <= t <= min(k, MAX_T)):
        raise ValueError(f"OSD of k = {k}, n = {n} at order t = {t} is not supported: {limits}")
    if num_patterns(k, t) > MAX_PATTERNS:
        raise ValueError(f"OSD of k = {k} at order t = {t} needs {num_patterns(k, t)} error patterns: {limits}")


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


class OSDecoder(nn.Module):
    """Ordered-statistics decoder of order t for the code of `encoder` (reference:
    my_sn/fec/osd/dec.py:8-192).  forward(logits [..., n]) -> codeword bits [..., n] in `dtype`;
    afterwards `last_dist` holds the fp64 metric of every returned word, [...]."""

    def __init__(self, t=0, encoder=None, dtype=tc.float32, device='cpu'):
        super().__init__()
        self.device = device
        self.dtype = dtype
        self._llr_max = 100.
        if dtype not in (tc.float16, tc.float32, tc.float64):
            raise ValueError('dtype must be {tf.float16, tf.float32, tf.float64}.')
        assert (int(t) == t), "t must be int."
        self._t = int(t)
        if encoder.k is None:
            raise AttributeError("It seems as if encoder is not init or has no attribute k.")
        u = tc.eye(encoder.k, device=device)
        gm = encoder(u)
        gm = gm.detach().cpu().numpy() if isinstance(gm, tc.Tensor) else np.asarray(gm)
        if gm.ndim != 2 or gm.shape[0] != encoder.k:
            raise ValueError(f"the encoder must map [k, k] to [k, n]; got {gm.shape} for k = {encoder.k}")
        self._gm_u8 = np.ascontiguousarray(gm != 0, dtype=np.uint8)
        self._gm = tc.from_numpy(self._gm_u8.copy()).to(dtype)
        self._k, self._n = self._gm_u8.shape
        check_supported(self._k, self._n, self._t)
        if gf2_rank(self._gm_u8) != self._k:
            raise ValueError(f"the generator matrix of the encoder is not of rank k = {self._k}")
        self.n_patterns = num_patterns(self._k, self._t)
        self.last_dist = None
        self._plans = _lib.PlanSet()

    @property
    def k(self):
        return self._k

    @property
    def n(self):
        return self._n

    @property
    def t(self):
        return self._t

    @property
    def gm(self):
        """The generator matrix, [k, n] in `dtype` (on the CPU)."""
        return self._gm

    def plan(self, device=None):
        """The decoding plan on `device` (default: the current GPU); plans are device-bound."""
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        return _lib.OsdPlan(self._gm_u8, self._t, device=dev)

    def forward(self, inputs):
        assert inputs.shape[-1] == self._n, "Last input dim must be of len n."
        input_shape = inputs.shape
        llr = inputs.reshape(-1, self._n).to(tc.float32)
        dev = _gpu_for(llr, self.device)
        c_hat, dist = ops.osd_decode(self.plan(dev), llr.to(dev, non_blocking=True), return_dist=True)
        self.last_dist = dist.reshape(input_shape[:-1]).to(inputs.device)
        return c_hat.reshape(input_shape).to(device=inputs.device, dtype=self.dtype)
