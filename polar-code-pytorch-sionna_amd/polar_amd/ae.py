"""AE_Dec: automorphism-ensemble SC decoding (pl_ae_decode).

AED (Geiselhart, Elkelesh, Ebada, Cammerer, ten Brink 2021) decodes M permuted copies of the received word
with plain SC, un-permutes the M candidate codewords and keeps the one closest to the received word: no CRC,
no sorting, no path metrics.  It suits codes with a large automorphism group that SC is not invariant under,
which the reference's row-weight frozen sets are whenever they are Reed-Muller codes (automorphism.rm_code).
The reference has no such decoder; the rule, the metric and the tie order are stated in
include/polar_mi355x.h.  forward() is SC_Dec's contract: [..., n] logits log P(1)/P(0) in, [..., k] bits out,
CPU tensors copied to the GPU and back.
"""
import warnings

import numpy as np
import torch as tc
from torch import nn

from . import _lib, automorphism, ops
from .decoders import _frozen_mask, _gpu_for

AE_MAX_N = 1024     # the kernel's register tree is built for n <= 1024
AE_MAX_PERMS = 64   # candidates a row


class AE_Dec(nn.Module):
    """Automorphism-ensemble SC decoder of the polar code (frozen_pos, n), n <= 1024.

    num_perms (1 ... 64) permutations are made by automorphism.stage_permutations (kind='stage': bit-index
    permutations) or linear_permutations (kind='linear': GL(m, 2) maps) with `seed`; the identity is the
    first, so num_perms=1 is plain leaf-by-leaf SC.  A frozen set that admits fewer raises ValueError.
    perms: an [M, n] integer array of the caller's own permutations instead (each row validated as a
    permutation; one that is no automorphism of the code gets a warning, not an error: the decoder is then
    merely poor).  f: 'minsum' or 'exact' (the boxplus of the my_sn decoders); llr_max: the clipping bound of f.
    return_metric: forward() returns (u_hat, metric), metric fp32 [...].
    After forward(): last_best_idx (int32 [...]) is the winning candidate of each row and last_metric (fp32
    [...]) its distance sum |a_i| [x_i != HD(a_i)], both on the input's device.
    """

    def __init__(self, frozen_pos, n, num_perms=8, kind='stage', perms=None, seed=0, f='minsum', llr_max=30.,
                 return_metric=False, output_dtype=tc.float32, device='cpu'):
        super().__init__()
        n = int(n)
        if n < 2 or n & (n - 1):
            raise ValueError(f"n must be a power of 2, got {n}")
        if n > AE_MAX_N:
            raise ValueError(f"automorphism-ensemble decoding of n = {n} is not supported by the MI355X kernel "
                             f"(n <= {AE_MAX_N})")
        if f not in ("exact", "minsum"):
            raise ValueError(f"f must be 'exact' or 'minsum', got {f!r}")
        if kind not in ("stage", "linear"):
            raise ValueError(f"kind must be 'stage' or 'linear', got {kind!r}")
        if not float(llr_max) > 0.0:
            raise ValueError(f"llr_max must be positive, got {llr_max}")
        if output_dtype not in (tc.float16, tc.float32, tc.float64):
            raise ValueError('output_dtype must be {tf.float16, tf.float32, tf.float64}.')
        self.n = n
        self.frozen_pos = frozen_pos
        fp, mask = _frozen_mask(frozen_pos, n)
        self.k = n - len(fp)
        self.info_pos = np.setdiff1d(np.arange(n), fp)
        assert self.k == len(self.info_pos), "Internal error: invalid info_pos generated."
        if perms is None:
            if not isinstance(num_perms, (int, np.integer)) or not 1 <= int(num_perms) <= AE_MAX_PERMS:
                raise ValueError(f"num_perms must be an integer in [1, {AE_MAX_PERMS}], got {num_perms!r}")
            make = automorphism.stage_permutations if kind == "stage" else automorphism.linear_permutations
            table = make(np.asarray(fp, dtype=np.int64), n, int(num_perms), seed=seed)
        else:
            table = np.asarray(perms.cpu() if isinstance(perms, tc.Tensor) else perms)
            if table.ndim != 2 or table.shape[1] != n or table.dtype.kind not in "iu" or \
                    not 1 <= table.shape[0] <= AE_MAX_PERMS:
                raise ValueError(f"perms must be an [M, {n}] integer array with 1 <= M <= {AE_MAX_PERMS}")
            table = table.astype(np.int64)
            for t, pi in enumerate(table):
                if not automorphism.is_permutation(pi, n):
                    raise ValueError(f"perms[{t}] is not a permutation of 0 ... {n - 1}")
                if not automorphism.is_automorphism(pi, np.asarray(fp, dtype=np.int64), n):
                    warnings.warn(f"AE_Dec: perms[{t}] is not an automorphism of the code; its candidate is "
                                  "decoded all the same and will rarely win")
        self.perms = table
        self.num_perms = int(table.shape[0])
        self.kind, self.f, self.llr_max = kind, f, float(llr_max)
        self.output_dtype, self.device = output_dtype, device
        self._return_metric = bool(return_metric)
        self.last_best_idx = self.last_metric = None
        self._mask = mask
        self._plans = _lib.PlanSet()

    def plan(self, device=None):
        """(the SC plan, the permutation table) on `device` (default: the current GPU); both are device-bound."""
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        f_mode = _lib.PL_F_EXACT if self.f == "exact" else _lib.PL_F_MINSUM
        # only the plan's tables are used: no specialised SC kernel is looked up or compiled
        p = _lib.Plan(self.n, self._mask, 1, f_mode, self.llr_max, flags=_lib.PL_PLAN_GENERIC, device=dev)
        return p, ops.ae_perm_table(self.perms, tc.device("cuda", dev))

    def forward(self, inputs):
        inputs = inputs.to(dtype=tc.float32)
        assert inputs.shape[-1] == self.n, "Last input dim must be of len n."
        assert len(inputs.shape) > 1
        lead = list(inputs.shape[:-1])
        llr = inputs.reshape([-1, self.n])
        dev = _gpu_for(llr, self.device)
        plan, table = self.plan(dev)
        u_hat, idx, met = ops.ae_decode(plan, llr.to(dev, non_blocking=True), table, return_info=True)
        self.last_best_idx = idx.reshape(lead).to(inputs.device)
        self.last_metric = met.reshape(lead).to(inputs.device)
        u_hat = u_hat.reshape(lead + [self.k]).to(device=inputs.device, dtype=self.output_dtype)
        return (u_hat, self.last_metric) if self._return_metric else u_hat
