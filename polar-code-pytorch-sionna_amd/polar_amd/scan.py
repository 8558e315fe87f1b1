"""SCAN_Dec: soft-cancellation polar decoding with soft output (pl_scan_decode; Fayyaz and Barry 2014).

The reference has no such decoder.  The messages, the unit equations, the initial values and the outputs
are BP_Dec's; the units are visited in the order of the SC tree walk (include/polar_mi355x.h), so a
decided or frozen leaf reaches the rest of the tree within one iteration.  The module is BP_Dec with
another entry point, default num_iter and length limit: the same constructor checks, forward() contract,
last_iters and last_ext.
"""
import torch as tc

from . import ops
from .bp import BP_Dec

SCAN_MAX_N = 2048  # the messages of a codeword, (log2 n + 1/2) n - 64 fp32, live in LDS


class SCAN_Dec(BP_Dec):
    """Soft-cancellation decoder of the polar code (frozen_pos, n), n <= 2048.

    num_iter: iterations (each one SC tree walk that updates every L and R message once).
    Every other argument, forward(), last_iters and last_ext are BP_Dec's.
    """
    _NAME, _MAX_N, _decode = "SCAN", SCAN_MAX_N, staticmethod(ops.scan_decode)

    def __init__(self, frozen_pos, n, num_iter=2, hard_out=True, output_dtype=tc.float32, device='cpu', f='exact',
                 scale=1.0, early_stop=False, llr_max=19.3, return_ext=False):
        super().__init__(frozen_pos, n, num_iter, hard_out, output_dtype, device, f, scale, early_stop, llr_max,
                         return_ext)
