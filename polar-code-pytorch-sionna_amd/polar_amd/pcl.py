"""Parity-constrained list decoding: PCL_Dec (pl_pcl_table_create, pl_pcl_decode).

A list decoder in which a u-bit may be tied to earlier u-bits by an affine parity relation
u[pos] = rhs ^ parity(u[earlier positions]) -- "dynamic frozen bits".  A FORCE constraint is computed by the
decoder on every path (no fork); a CHECK constraint forks like an information bit and then kills the paths that
violate it, and a row with no path left stops decoding: a distributed CRC (polar_amd.dci), parity-check polar
codes, RM-polar codes with dynamic frozen bits.  PAC_Dec is the special case of one convolution at every position.

    cons = [(5, CHECK, 0, [3]), (7, FORCE, 1, [3, 5, 6])]      # (pos, kind, rhs, earlier_positions)
    dec = PCL_Dec(frozen_pos, 8, cons, list_size=8, return_status=True, device="cuda")
    u_hat, ok, stop = dec(llr)

The reference has no such decoder; the contract is stated in include/polar_mi355x.h.
"""
import numpy as np
import torch as tc
from torch import nn

from . import _lib, ops
from ._lib import PL_PCL_CHECK as CHECK, PL_PCL_FORCE as FORCE  # noqa: F401
from .decoders import _frozen_mask, _gpu_for

PCL_MAX_N = 1024   # the list state of a codeword lives in one work-group's LDS
PCL_MAX_LIST = 32  # the 2L candidates of a fork sit one a lane of a wave


def pack_constraints(n, constraints):
    """[(pos, kind, rhs, earlier_positions)] -> (pos int32 [C], kind uint8 [C], rhs uint8 [C], mask uint32 [C, W]),
    the arrays of pl_pcl_table_create, sorted by pos; W = max(n / 32, 1), bit (j & 31) of word j >> 5 of a mask row
    = u-position j.  kind is CHECK or FORCE.  Only the shape of the entries is checked here; the library validates
    the table against the frozen set (positions not frozen, masks causal)."""
    n = int(n)
    cons = sorted(((int(p), int(kd), int(r), [int(j) for j in e]) for p, kd, r, e in constraints), key=lambda c: c[0])
    C, W = len(cons), max(n // 32, 1)
    pos, kind, rhs = np.zeros(C, np.int32), np.zeros(C, np.uint8), np.zeros(C, np.uint8)
    mask = np.zeros((C, W), np.uint32)
    for c, (p, kd, r, earlier) in enumerate(cons):
        if kd not in (CHECK, FORCE) or r not in (0, 1):
            raise ValueError(f"constraint at {p}: kind must be CHECK or FORCE and rhs 0 or 1, got {kd}, {r}")
        if not 0 <= p < n or any(not 0 <= j < n for j in earlier):
            raise ValueError(f"constraint at {p}: positions must lie in [0, {n})")
        pos[c], kind[c], rhs[c] = p, kd, r
        for j in earlier:
            mask[c, j >> 5] |= np.uint32(1 << (j & 31))
    return pos, kind, rhs, mask


class PCL_Dec(nn.Module):
    """List decoder of the polar code (frozen_pos, n <= 1024) under `constraints`, a list of
    (pos, kind, rhs, earlier_positions) or the packed arrays of pack_constraints, with list_size paths, a power of
    two in 1 ... 32, the min-sum f clipped at llr_max and fp32 path metrics.  forward() is SC_Dec's contract:
    [..., n] logits log P(1)/P(0) in, [..., k] u-bits at the non-frozen positions out (constrained positions
    included; all zero where no path survived), CPU tensors copied to the GPU and back.  return_status adds
    ok [...] (1 = a live path was output) and stop [...] int32 (the leaf at which the row stopped, n = ran to the
    end).  After forward(): last_pm (fp32 [..., list_size]) holds the final path metrics, ascending, +inf = dead."""

    def __init__(self, frozen_pos, n, constraints, list_size=8, return_status=False, llr_max=30.,
                 output_dtype=tc.float32, device='cpu'):
        super().__init__()
        n = int(n)
        if n < 2 or n & (n - 1):
            raise ValueError(f"n must be a power of 2, got {n}")
        if n > PCL_MAX_N:
            raise ValueError(f"parity-constrained list decoding of n = {n} is not supported by the MI355X kernel "
                             f"(n <= {PCL_MAX_N})")
        list_size = int(list_size)
        if not 1 <= list_size <= PCL_MAX_LIST or list_size & (list_size - 1):
            raise ValueError(f"list_size must be a power of two in [1, {PCL_MAX_LIST}], got {list_size}")
        if not float(llr_max) > 0.0:
            raise ValueError(f"llr_max must be positive, got {llr_max}")
        if output_dtype not in (tc.float16, tc.float32, tc.float64):
            raise ValueError('output_dtype must be {tf.float16, tf.float32, tf.float64}.')
        self.n = n
        self.frozen_pos = frozen_pos
        fp, self._mask = _frozen_mask(frozen_pos, n)
        self.k = n - len(fp)
        self.info_pos = np.setdiff1d(np.arange(n), fp)
        assert self.k == len(self.info_pos), "Internal error: invalid info_pos generated."
        if isinstance(constraints, tuple) and len(constraints) == 4 and isinstance(constraints[0], np.ndarray):
            self.constraints = tuple(np.array(a) for a in constraints)
        else:
            self.constraints = pack_constraints(n, constraints)
        self.list_size, self.llr_max = list_size, float(llr_max)
        self.return_status = bool(return_status)
        self.output_dtype, self.device = output_dtype, device
        self.last_pm = None
        self._plans = _lib.PlanSet()

    def plan(self, device=None):
        """(plan, table) on `device` (default: the current GPU)."""
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        # only the plan's tables are used: no specialised SC kernel is looked up or compiled
        plan = _lib.Plan(self.n, self._mask, 1, _lib.PL_F_MINSUM, self.llr_max, flags=_lib.PL_PLAN_GENERIC, device=dev)
        return plan, _lib.PclTable(plan, *self.constraints)

    def decode(self, llr):
        """[bs, n] fp32 logits on the GPU -> (bits [bs, k] fp32, pm, ok uint8, stop int32), all on the GPU."""
        plan, table = self.plan(llr.device)
        return ops.pcl_decode(plan, table, self.list_size, llr, return_pm=True, return_status=True)

    def forward(self, inputs):
        inputs = inputs.to(dtype=tc.float32)
        assert inputs.shape[-1] == self.n, "Last input dim must be of len n."
        assert len(inputs.shape) > 1
        lead = list(inputs.shape[:-1])
        llr = inputs.reshape([-1, self.n])
        dev = _gpu_for(llr, self.device)
        u_hat, pm, ok, stop = self.decode(llr.to(dev, non_blocking=True))
        self.last_pm = pm.reshape(lead + [self.list_size]).to(inputs.device)
        u_hat = u_hat.reshape(lead + [self.k]).to(device=inputs.device, dtype=self.output_dtype)
        if not self.return_status:
            return u_hat
        return u_hat, ok.reshape(lead).to(inputs.device), stop.reshape(lead).to(inputs.device)
