"""SCF_Dec: CRC-aided successive-cancellation flip decoding (pl_scf_decode).

SC-Flip (Afisiadis, Balatsoukas-Stimming, Burg 2014) is the other standard way to use an outer CRC
next to the list decoder: SC first; a row whose SC result fails the CRC is decoded again, up to
max_flips times, each time with the decision at one more of its least reliable information
positions inverted, until the CRC passes.  The reference has no such decoder; the rule, the tie
order of the candidates and the outputs are stated in include/polar_mi355x.h.  The constructor is
written in the manner of mysn.SCL_Dec, forward() is SC_Dec's contract: [..., n] logits
log P(1)/P(0) in, [..., k] bits out (the CRC bits included), CPU tensors copied to the GPU and back.
"""
import numpy as np
import torch as tc
from torch import nn

from . import _lib, ops
from .decoders import _frozen_mask, _gpu_for
from .mysn import crc_params

SCF_MAX_N = 1024     # the flip kernel's register tree and LDS tables are built for n <= 1024
SCF_MAX_FLIPS = 64   # candidate positions a row


class SCF_Dec(nn.Module):
    """SC-Flip decoder of the polar code (frozen_pos, n), n <= 1024, with the outer CRC crc_degree
    ('CRC24A', 'CRC24B', 'CRC24C', 'CRC16', 'CRC11', 'CRC6': the last bits of the k are its parity).

    max_flips: candidate positions a failing row may try (0 ... 64; 0 is SC plus the CRC status).
    f: 'exact' (the boxplus of the my_sn decoders) or 'minsum'.  llr_max: the clipping bound of f.
    return_crc_status: forward() returns (u_hat, crc_status), crc_status torch.bool [...].
    After forward(): last_attempts (int32 [...]) holds the SC decodes the sequential algorithm runs
    on each row, last_flip_pos (int32 [...]) the inverted position (0 ... n-1) or -1, last_crc_ok the
    CRC status, all on the input's device.
    """

    def __init__(self, frozen_pos, n, crc_degree, max_flips=16, f='exact', return_crc_status=False,
                 output_dtype=tc.float32, device='cpu', llr_max=30.):
        super().__init__()
        n = int(n)
        if n < 2 or n & (n - 1):
            raise ValueError(f"n must be a power of 2, got {n}")
        if n > SCF_MAX_N:
            raise ValueError(f"SC-Flip decoding of n = {n} is not supported by the MI355X kernel (n <= {SCF_MAX_N})")
        if crc_degree is None:
            raise ValueError("SC-Flip requires an outer CRC (crc_degree).")
        if f not in ("exact", "minsum"):
            raise ValueError(f"f must be 'exact' or 'minsum', got {f!r}")
        if not isinstance(max_flips, (int, np.integer)) or not 0 <= int(max_flips) <= SCF_MAX_FLIPS:
            raise ValueError(f"max_flips must be an integer in [0, {SCF_MAX_FLIPS}], got {max_flips!r}")
        if not float(llr_max) > 0.0:
            raise ValueError(f"llr_max must be positive, got {llr_max}")
        if output_dtype not in (tc.float16, tc.float32, tc.float64):
            raise ValueError('output_dtype must be {tf.float16, tf.float32, tf.float64}.')
        self._crc = crc_params(crc_degree)  # ValueError for an unknown name
        self.n = n
        self.frozen_pos = frozen_pos
        fp, mask = _frozen_mask(frozen_pos, n)
        self.k = n - len(fp)
        self.info_pos = np.setdiff1d(np.arange(n), fp)
        assert self.k == len(self.info_pos), "Internal error: invalid info_pos generated."
        if self.k < self._crc[0]:
            raise ValueError("Value of k is too small for given CRC_degree.")
        self.k_crc = self._crc[0]
        self.max_flips, self.f, self.llr_max = int(max_flips), f, float(llr_max)
        self.output_dtype, self.device = output_dtype, device
        self._return_crc_status = bool(return_crc_status)
        self.last_attempts = self.last_flip_pos = self.last_crc_ok = None
        self._mask = mask
        self._plans = _lib.PlanSet()

    def plan(self, device=None):
        """The SC plan with the CRC on `device` (default: the current GPU); plans are device-bound."""
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        f_mode = _lib.PL_F_EXACT if self.f == "exact" else _lib.PL_F_MINSUM
        p = _lib.Plan(self.n, self._mask, 1, f_mode, self.llr_max, device=dev)
        p.set_crc(*self._crc)
        return p

    def forward(self, inputs):
        inputs = inputs.to(dtype=tc.float32)
        assert inputs.shape[-1] == self.n, "Last input dim must be of len n."
        assert len(inputs.shape) > 1
        lead = list(inputs.shape[:-1])
        llr = inputs.reshape([-1, self.n])
        dev = _gpu_for(llr, self.device)
        u_hat, ok, pos, att = ops.scf_decode(self.plan(dev), llr.to(dev, non_blocking=True), self.max_flips,
                                             return_info=True)
        self.last_crc_ok = ok.reshape(lead).to(inputs.device)
        self.last_flip_pos = pos.reshape(lead).to(inputs.device)
        self.last_attempts = att.reshape(lead).to(inputs.device)
        u_hat = u_hat.reshape(lead + [self.k]).to(device=inputs.device, dtype=self.output_dtype)
        return (u_hat, self.last_crc_ok) if self._return_crc_status else u_hat
