"""PAC codes: PACEncoder and PAC_Dec (pl_pac_encode, pl_pac_decode; Arikan 2019).

A polarization-adjusted convolutional code is a rate-1 convolutional precoder in front of the polar transform,
with the frozen set as rate profile -- for the Reed-Muller profile, the row-weight sets of
reference_frozen_pos, which plain SC-type decoders handle poorly -- and a list decoder that carries the
precoder's shift register on every path.  PAC(128, 64) with the generator 0o133 is the standard example:

    fp = reference_frozen_pos(64, 128)
    enc, dec = PACEncoder(fp, 128), PAC_Dec(fp, 128, list_size=32, device="cuda")

The reference has no PAC code; the contract is stated in include/polar_mi355x.h.  conv = (c_0, ..., c_m), c_0 = 1,
m <= 31: u_i = XOR_j c_j v_{i-j}.  conv = (1,) is the plain polar code.
"""
import numpy as np
import torch as tc
from torch import nn

from . import _lib, ops
from .decoders import _frozen_mask, _gpu_for

PAC_MAX_N = 1024   # the list state of a codeword lives in one work-group's LDS
PAC_MAX_LIST = 32  # the 2L candidates of a fork sit one a lane of a wave
CONV_133 = (1, 0, 1, 1, 0, 1, 1)


def conv_from_octal(octal):
    """'133' (or 0o133 as an int's octal digits: 133) -> (1, 0, 1, 1, 0, 1, 1): the binary digits of the octal
    number, most significant first, as c_0 ... c_m."""
    value = int(str(octal), 8)
    if value < 1:
        raise ValueError(f"the generator must be a positive octal number, got {octal!r}")
    return tuple(int(b) for b in bin(value)[2:])


def conv_to_mask(conv):
    """(c_0, ..., c_m) -> the uint32 mask of the C ABI, bit j = c_j."""
    conv = tuple(int(c) for c in conv)
    if not 1 <= len(conv) <= 32 or any(c not in (0, 1) for c in conv) or conv[0] != 1:
        raise ValueError(f"conv must be 1 ... 32 bits (c_0, ..., c_m) with c_0 = 1, got {conv}")
    return sum(c << j for j, c in enumerate(conv))


def _check_n(n, what):
    n = int(n)
    if n < 2 or n & (n - 1):
        raise ValueError(f"n must be a power of 2, got {n}")
    if n > PAC_MAX_N:
        raise ValueError(f"PAC {what} of n = {n} is not supported by the MI355X kernel (n <= {PAC_MAX_N})")
    return n


class PACEncoder(nn.Module):
    """Encoder of the PAC code (frozen_pos as rate profile, n <= 1024, generator conv): forward([..., k] 0/1) ->
    [..., n] fp32 codewords.  .k and .n are what OSDecoder and System_AWGN_model ask of an encoder; CPU tensors
    are copied to the GPU and back."""

    def __init__(self, frozen_pos, n, conv=CONV_133, device='cpu'):
        super().__init__()
        self.n = _check_n(n, "encoding")
        self.frozen_pos = frozen_pos
        self.conv = tuple(int(c) for c in conv)
        self.conv_mask = conv_to_mask(conv)
        fp, self._mask = _frozen_mask(frozen_pos, self.n)
        self.k = self.n - len(fp)
        self.device = device
        self._plans = _lib.PlanSet()

    def _make_plan(self, dev):
        return _lib.Plan(self.n, self._mask, 1, flags=_lib.PL_PLAN_GENERIC, device=dev)

    def forward(self, u):
        assert u.shape[-1] == self.k, "Last input dim must be of len k."
        lead = list(u.shape[:-1])
        bits = u.reshape([-1, self.k])
        dev = _gpu_for(bits, self.device)
        cw = ops.pac_encode(self._plans.get(dev, self._make_plan), self.conv_mask, bits.to(dev, non_blocking=True))
        return cw.reshape(lead + [self.n]).to(u.device)

    def generator_matrix(self):
        """[k, n] uint8 numpy array: row m is the codeword of the m-th unit data word."""
        gm = self.forward(tc.eye(self.k, dtype=tc.float32))
        return np.ascontiguousarray(gm.cpu().numpy() != 0, dtype=np.uint8)


class PAC_Dec(nn.Module):
    """List decoder of the PAC code (frozen_pos, n <= 1024, generator conv) with list_size paths, a power of two
    in 1 ... 32, the min-sum f clipped at llr_max and fp32 path metrics.  forward() is SC_Dec's contract:
    [..., n] logits log P(1)/P(0) in, [..., k] data bits out, CPU tensors copied to the GPU and back.
    After forward(): last_pm (fp32 [..., list_size]) holds the final path metrics, ascending."""

    def __init__(self, frozen_pos, n, list_size=32, conv=CONV_133, llr_max=30., output_dtype=tc.float32, device='cpu'):
        super().__init__()
        self.n = _check_n(n, "decoding")
        list_size = int(list_size)
        if not 1 <= list_size <= PAC_MAX_LIST or list_size & (list_size - 1):
            raise ValueError(f"list_size must be a power of two in [1, {PAC_MAX_LIST}], got {list_size}")
        if not float(llr_max) > 0.0:
            raise ValueError(f"llr_max must be positive, got {llr_max}")
        if output_dtype not in (tc.float16, tc.float32, tc.float64):
            raise ValueError('output_dtype must be {tf.float16, tf.float32, tf.float64}.')
        self.frozen_pos = frozen_pos
        self.conv = tuple(int(c) for c in conv)
        self.conv_mask = conv_to_mask(conv)
        fp, self._mask = _frozen_mask(frozen_pos, self.n)
        self.k = self.n - len(fp)
        self.info_pos = np.setdiff1d(np.arange(self.n), fp)
        assert self.k == len(self.info_pos), "Internal error: invalid info_pos generated."
        self.list_size, self.llr_max = list_size, float(llr_max)
        self.output_dtype, self.device = output_dtype, device
        self.last_pm = None
        self._plans = _lib.PlanSet()

    def plan(self, device=None):
        """The plan on `device` (default: the current GPU): it supplies n, the frozen set and llr_max."""
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        # only the plan's tables are used: no specialised SC kernel is looked up or compiled
        return _lib.Plan(self.n, self._mask, 1, _lib.PL_F_MINSUM, self.llr_max, flags=_lib.PL_PLAN_GENERIC, device=dev)

    def forward(self, inputs):
        inputs = inputs.to(dtype=tc.float32)
        assert inputs.shape[-1] == self.n, "Last input dim must be of len n."
        assert len(inputs.shape) > 1
        lead = list(inputs.shape[:-1])
        llr = inputs.reshape([-1, self.n])
        dev = _gpu_for(llr, self.device)
        v_hat, pm = ops.pac_decode(self.plan(dev), self.conv_mask, self.list_size, llr.to(dev, non_blocking=True),
                                   return_pm=True)
        self.last_pm = pm.reshape(lead + [self.list_size]).to(inputs.device)
        return v_hat.reshape(lead + [self.k]).to(device=inputs.device, dtype=self.output_dtype)
