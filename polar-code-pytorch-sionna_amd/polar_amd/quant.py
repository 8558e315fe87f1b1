"""SCQ_Dec: fixed-point successive-cancellation decoding on quantised LLRs (pl_llr_quantize, pl_scq_decode).

Every other decoder of the package computes in fp32 or fp64, so its BLER curve is that of an ideal decoder.
SCQ_Dec answers the hardware question: how many LLR bits does an SC decoder need?  The channel logits are
quantised to q_channel bits (a uniform mid-tread quantiser of step llr_max / Cmax, Cmax = 2^(q_channel-1) - 1,
saturating at +-llr_max) and decoded in integers that saturate at +-Imax = 2^(q_internal-1) - 1 after every g.
The reference has no such decoder; the arithmetic is stated in include/polar_mi355x.h and restated in numpy in
tests/golden/scq_ref.py, which the kernel equals bit for bit.  forward() is SC_Dec's contract: [..., n] logits
log P(1)/P(0) in, [..., k] bits out, CPU tensors copied to the GPU and back.
"""
import numpy as np
import torch as tc
from torch import nn

from . import _lib, ops
from .decoders import _frozen_mask, _gpu_for, check_supported


class SCQ_Dec(nn.Module):
    """Fixed-point SC decoder of the polar code (frozen_pos, n), 2 <= n <= 2048.

    q_channel, q_internal: bits of the channel LLRs and of the decoder's internal LLRs, sign included,
    2 <= q_channel <= q_internal <= 8.  llr_max: the logit magnitude the largest channel level stands for.
    Attributes: cmax, imax (the largest levels), step = llr_max / cmax, inv_step = float32(1 / step), the
    factor pl_llr_quantize multiplies by.
    forward(inputs): float logits, quantised then decoded.  forward_q(q): int8 rows decoded as they are
    (any value; the decoder clamps what it loads to +-imax).  quantize(inputs): the int8 rows forward() decodes.
    """

    def __init__(self, frozen_pos, n, q_channel=6, q_internal=6, llr_max=30., output_dtype=tc.float32, device='cpu'):
        super().__init__()
        n = int(n)
        if n < 2 or n & (n - 1):
            raise ValueError(f"n must be a power of 2, got {n}")
        check_supported(n)
        for name, q in (("q_channel", q_channel), ("q_internal", q_internal)):
            if not isinstance(q, (int, np.integer)) or isinstance(q, bool) or not 2 <= int(q) <= 8:
                raise ValueError(f"{name} must be an integer in [2, 8], got {q!r}")
        if int(q_channel) > int(q_internal):
            raise ValueError(f"q_channel ({q_channel}) must not exceed q_internal ({q_internal})")
        if not (float(llr_max) > 0.0 and np.isfinite(float(llr_max))):
            raise ValueError(f"llr_max must be positive and finite, got {llr_max}")
        if output_dtype not in (tc.float16, tc.float32, tc.float64):
            raise ValueError('output_dtype must be {tf.float16, tf.float32, tf.float64}.')
        self.n = n
        self.frozen_pos = frozen_pos
        fp, mask = _frozen_mask(frozen_pos, n)
        self.k = n - len(fp)
        self.info_pos = np.setdiff1d(np.arange(n), fp)
        if self.k != len(self.info_pos):
            raise ValueError("frozen_pos must hold distinct positions in [0, n)")
        self.q_channel, self.q_internal, self.llr_max = int(q_channel), int(q_internal), float(llr_max)
        self.cmax = (1 << (self.q_channel - 1)) - 1
        self.imax = (1 << (self.q_internal - 1)) - 1
        self.step = self.llr_max / self.cmax
        self.inv_step = float(np.float32(1.0 / self.step))
        if not (self.inv_step > 0.0 and np.isfinite(self.inv_step)):
            raise ValueError(f"llr_max = {llr_max} gives no usable fp32 step")
        self.output_dtype, self.device = output_dtype, device
        self._mask = mask
        self._plans = _lib.PlanSet()

    def plan(self, device=None):
        """The plan on `device` (default: the current GPU).  Only its n and frozen set are used, so it is a
        generic plan: no specialised SC kernel is looked up or compiled for it."""
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        return _lib.Plan(self.n, self._mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC, device=dev)

    def _rows(self, inputs):
        assert inputs.shape[-1] == self.n, "Last input dim must be of len n."
        assert len(inputs.shape) > 1
        rows = inputs.reshape([-1, self.n])
        dev = _gpu_for(rows, self.device)
        return rows.to(dev, non_blocking=True), dev, list(inputs.shape[:-1])

    def quantize(self, inputs):
        """[..., n] float logits -> [..., n] int8 levels in [-cmax, cmax], on the input's device."""
        rows, _, lead = self._rows(inputs.to(dtype=tc.float32))
        return ops.llr_quantize(rows, self.inv_step, self.q_channel).reshape(lead + [self.n]).to(inputs.device)

    def forward_q(self, q):
        """[..., n] int8 LLRs (logit sign) -> [..., k] bits."""
        if q.dtype != tc.int8:
            raise ValueError(f"forward_q takes int8 LLRs, got {q.dtype}")
        rows, dev, lead = self._rows(q)
        u_hat = ops.scq_decode(self.plan(dev), rows, self.q_internal)
        return u_hat.reshape(lead + [self.k]).to(device=q.device, dtype=self.output_dtype)

    def forward(self, inputs):
        rows, dev, lead = self._rows(inputs.to(dtype=tc.float32))
        q = ops.llr_quantize(rows, self.inv_step, self.q_channel)
        u_hat = ops.scq_decode(self.plan(dev), q, self.q_internal)
        return u_hat.reshape(lead + [self.k]).to(device=inputs.device, dtype=self.output_dtype)
