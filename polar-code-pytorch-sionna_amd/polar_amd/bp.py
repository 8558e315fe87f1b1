"""BP_Dec: iterative belief-propagation polar decoding with soft output (pl_bp_decode).

The reference names the decoder (my_sn/fec/polar/dec.py:1, "SC, SCL and iterative BP decoding";
Polar5GDecoder's dec_type "BP") and does not contain it.  The message-passing rules, the initial
values and the outputs are stated in include/polar_mi355x.h; the constructor follows the my_sn
decoders' (frozen_pos, n, output_dtype, device), forward() is SC_Dec's contract: [..., n] logits
log P(1)/P(0) in, [..., k] out, CPU tensors copied to the GPU and back.
"""
import numpy as np
import torch as tc
from torch import nn

from . import _lib, ops
from .decoders import _frozen_mask, _gpu_for

BP_MAX_N = 1024  # the messages of a codeword, (2 log2 n + 1) n fp32, live in one CU's LDS


class BP_Dec(nn.Module):
    """Belief-propagation decoder of the polar code (frozen_pos, n), n <= 1024.

    num_iter: iterations (each an R pass and an L pass over the log2 n stages).
    hard_out: True returns the decided information bits (0/1), False their logits log P(1)/P(0).
    f: 'exact' (the boxplus of the my_sn decoders) or 'minsum'; scale in (0, 1] multiplies the
    min-sum magnitude (scaled min-sum; 1 with the exact f).
    early_stop: a row ends once its hard decisions re-encode to the hard decisions on the code bits.
    llr_max: clipping bound of every message.
    After forward(): last_iters holds the iterations each row ran (int32, [...]), and with
    return_ext, last_ext the extrinsic logits of the code bits ([..., n]), on the input's device.
    """
    # what SCAN_Dec (scan.py), the same module on another schedule, replaces
    _NAME, _MAX_N, _decode = "BP", BP_MAX_N, staticmethod(ops.bp_decode)

    def __init__(self, frozen_pos, n, num_iter=20, hard_out=True, output_dtype=tc.float32, device='cpu', f='exact',
                 scale=1.0, early_stop=False, llr_max=19.3, return_ext=False):
        super().__init__()
        n = int(n)
        if n < 2 or n & (n - 1):
            raise ValueError(f"n must be a power of 2, got {n}")
        if n > self._MAX_N:
            raise ValueError(f"{self._NAME} decoding of n = {n} is not supported by the MI355X kernel (n <= {self._MAX_N})")
        if f not in ("exact", "minsum"):
            raise ValueError(f"f must be 'exact' or 'minsum', got {f!r}")
        if int(num_iter) < 1:
            raise ValueError(f"num_iter must be >= 1, got {num_iter}")
        if not 0.0 < float(scale) <= 1.0:
            raise ValueError(f"scale must be in (0, 1], got {scale}")
        if f == "exact" and float(scale) != 1.0:
            raise ValueError("scale != 1 needs f='minsum' (the exact f is not scaled)")
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
        self.num_iter, self.hard_out, self.output_dtype, self.device = int(num_iter), bool(hard_out), output_dtype, device
        self.f, self.scale, self.early_stop = f, float(scale), bool(early_stop)
        self.llr_max, self.return_ext = float(llr_max), bool(return_ext)
        self.last_iters = self.last_ext = None
        self._mask = mask
        self._plans = _lib.PlanSet()

    def plan(self, device=None):
        """The plan on `device` (default: the current GPU): PL_PLAN_GENERIC, only its tables are used."""
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        f_mode = _lib.PL_F_EXACT if self.f == "exact" else _lib.PL_F_MINSUM
        return _lib.Plan(self.n, self._mask, 1, f_mode, self.llr_max, flags=_lib.PL_PLAN_GENERIC, device=dev)

    def forward(self, inputs):
        inputs = inputs.to(dtype=tc.float32)
        assert inputs.shape[-1] == self.n, "Last input dim must be of len n."
        assert len(inputs.shape) > 1
        lead = list(inputs.shape[:-1])
        llr = inputs.reshape([-1, self.n])
        dev = _gpu_for(llr, self.device)
        res = self._decode(self.plan(dev), llr.to(dev, non_blocking=True), self.num_iter, self.scale, self.early_stop,
                           hard=self.hard_out, soft=not self.hard_out, ext=self.return_ext, iters=True)
        self.last_iters = res["iters"].reshape(lead).to(inputs.device)
        self.last_ext = res["ext_x"].reshape(lead + [self.n]).to(inputs.device) if self.return_ext else None
        out = res["bits"] if self.hard_out else res["soft_u"]
        return out.reshape(lead + [self.k]).to(device=inputs.device, dtype=self.output_dtype)
