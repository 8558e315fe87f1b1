"""The 5G NR downlink polar chain (PDCCH / PBCH style, 3GPP TS 38.212 sections 5.3.1, 5.4.1, 7.3): DCIEncoder and
DCIDecoder.

    enc = DCIEncoder(40, 216, rnti=0xBEEF, device="cuda")
    dec = DCIDecoder(enc, list_size=8, return_crc_status=True)
    a_hat, ok = dec(llr)             # dec.last_stop: the leaf at which each row stopped (n_polar = ran to the end)

Encoder: CRC24C over the payload (with ones_prefix, over 24 ones followed by the payload), the last 16 parity bits
XORed with the RNTI, the input-bit interleaver that distributes parity bits into the information word, the polar
transform, sub-block interleaving and bit selection (no channel interleaver on the downlink).  The tables are those
of Polar5GEncoder(channel_type="downlink"), whose own forward() raises as the reference's does.
ones_prefix=False with rnti=0 is Sionna's simplified scheme; interleave=False leaves all 24 parity bits at the tail.

Decoder: every parity bit is one constraint of the parity-constrained list decoder (polar_amd.pcl, pl_pcl_decode):
its mask the u-positions of the payload bits it depends on, its rhs the contribution of the ones prefix and the
RNTI.  A path that fails a parity bit dies where the bit is decoded, not after the whole word, and a row in which no
path is left stops: blind decoding of a candidate that carries nothing.  The reference has no downlink decoder.
"""
import ctypes

import numpy as np
import torch as tc
from torch import nn

from . import _lib, ops
from .decoders import _gpu_for
from .pcl import CHECK, FORCE, pack_constraints
from .polar5g import (Polar5GDecoder, _rate_match_tables, _to_dev_i32, crc_generator_rows, subblock_interleaving)

K_CRC = 24


def _rnti_bits(rnti):
    rnti = int(rnti)
    if not 0 <= rnti < 1 << 16:
        raise ValueError(f"rnti must be a 16-bit value, got {rnti}")
    return np.array([(rnti >> (15 - i)) & 1 for i in range(16)], np.uint8)  # x_rnti,0 is the most significant bit


def _gather(x, idx, n_out):
    out = tc.empty((x.shape[0], n_out), dtype=tc.float32, device=x.device)
    with tc.cuda.device(x.device):
        _lib.check(_lib.lib().pl_gather_rows(ctypes.c_void_p(x.data_ptr()), x.shape[0], x.shape[1],
                                             ctypes.c_void_p(idx.data_ptr()), n_out, ctypes.c_void_p(out.data_ptr()),
                                             _lib.current_stream_ptr(x.device)), "pl_gather_rows")
    return out


class DCIEncoder(nn.Module):
    """forward([..., k] 0/1 payload) -> [..., n] fp32 code bits.  k <= 140 payload bits, 25 <= n <= 576 code bits
    (the limits of the downlink configuration).  .k / .n are what System_AWGN_model asks of an encoder."""

    def __init__(self, k, n, rnti=0, ones_prefix=True, interleave=True, dtype=tc.float32, device='cpu'):
        super().__init__()
        k, n = int(k), int(n)
        if not 1 <= k <= 140 or not 25 <= n <= 576 or k + K_CRC > n:
            raise ValueError(f"the downlink chain needs 1 <= k <= 140, 25 <= n <= 576 and k + 24 <= n, got k = {k}, n = {n}")
        crc_pol, n_polar, frozen_pos, idx_rm, idx_input = _rate_match_tables(k, n, "downlink")
        assert crc_pol == "CRC24C"
        self.k, self.n = k, n
        self.k_polar, self.n_polar = k + K_CRC, int(n_polar)
        self.rnti, self.ones_prefix, self.interleave = int(rnti), bool(ones_prefix), bool(interleave)
        self.dtype, self.device = dtype, device
        self.frozen_pos = np.asarray(frozen_pos, np.int64)
        self.info_pos = np.setdiff1d(np.arange(self.n_polar), self.frozen_pos)
        self.ind_rate_matching = np.asarray(idx_rm, np.int64)
        # c'[m] = c[ind_input_int[m]]: the interleaver as a gather index over (payload, parity)
        self.ind_input_int = np.asarray(idx_input, np.int64) if self.interleave else np.arange(self.k_polar)
        self.g_rows = crc_generator_rows(crc_pol, k)  # row m: the parity of the m-th unit payload, bit c = column c
        # what the ones prefix and the RNTI add to the parity bits: a constant of the code
        const = np.zeros(K_CRC, np.uint8)
        if self.ones_prefix:
            lead = np.bitwise_xor.reduce(crc_generator_rows(crc_pol, k + K_CRC)[:K_CRC])
            const = np.array([(int(lead) >> c) & 1 for c in range(K_CRC)], np.uint8)
        const[8:] ^= _rnti_bits(self.rnti)
        self.parity_const = const
        self._mask = np.zeros(self.n_polar, np.uint8)
        self._mask[self.frozen_pos] = 1
        self._plans = _lib.PlanSet()
        self._dev_tables = {}

    def plan(self, device=None):
        return self._plans.get(device, self._make_plan)

    def _make_plan(self, dev):
        return _lib.Plan(self.n_polar, self._mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC, device=dev)

    def tables(self, dev):
        key = str(dev)
        if key not in self._dev_tables:
            self._dev_tables[key] = (tc.as_tensor(self.g_rows.view(np.int32), device=dev),
                                     tc.as_tensor(self.parity_const.astype(np.float32), device=dev),
                                     _to_dev_i32(self.ind_input_int, dev), _to_dev_i32(self.ind_rate_matching, dev))
        return self._dev_tables[key]

    def crc_attach(self, a):
        """[bs, k] fp32 on the GPU -> [bs, k + 24]: payload, then the parity bits with prefix and RNTI applied."""
        ops._require_cuda(a, "a")
        a = a.to(tc.float32).contiguous()
        g, const, _, _ = self.tables(a.device)
        out = tc.empty((a.shape[0], self.k_polar), dtype=tc.float32, device=a.device)
        with tc.cuda.device(a.device):
            _lib.check(_lib.lib().pl_crc_attach(ctypes.c_void_p(a.data_ptr()), a.shape[0], self.k,
                                                ctypes.c_void_p(g.data_ptr()), K_CRC, ctypes.c_void_p(out.data_ptr()),
                                                _lib.current_stream_ptr(a.device)), "pl_crc_attach")
        out[:, self.k:] = (out[:, self.k:] != const).to(tc.float32)  # XOR with the code's constant
        return out

    def mother_input(self, a):
        """[bs, k] on the GPU -> [bs, k + 24] bits at the information positions of the mother code, ascending."""
        _, _, il, _ = self.tables(a.device)
        return _gather(self.crc_attach(a), il, self.k_polar)

    def forward(self, u):
        assert u.shape[-1] == self.k, "Last dim must be len k."
        dev = _gpu_for(u, self.device)
        a = u.reshape(-1, self.k).to(dev, tc.float32)
        x = ops.polar_encode(self.plan(dev), self.mother_input(a))
        _, _, _, rm = self.tables(dev)
        out = _gather(x, rm, self.n)
        return out.reshape(list(u.shape[:-1]) + [self.n]).to(device=u.device, dtype=self.dtype)


def dci_constraints(enc, n_force=0):
    """The constraint list [(pos, kind, rhs, earlier_positions)] of a DCIEncoder's code, in decoding order: parity
    bit j sits at the u-position the interleaver gives it, depends on the payload bits m with bit j of g_rows[m] set,
    and has rhs = parity_const[j].  The first n_force are FORCE, the rest CHECK."""
    inv = np.empty(enc.k_polar, np.int64)
    inv[enc.ind_input_int] = np.arange(enc.k_polar)
    upos = enc.info_pos[inv]  # u-position of each bit of (payload, parity)
    cons = []
    for j in range(K_CRC):
        dep = np.flatnonzero((enc.g_rows >> np.uint32(j)) & np.uint32(1))
        cons.append((int(upos[enc.k + j]), CHECK, int(enc.parity_const[j]), [int(upos[m]) for m in dep]))
    cons.sort(key=lambda c: c[0])
    return [(p, FORCE if r < int(n_force) else CHECK, rhs, e) for r, (p, _, rhs, e) in enumerate(cons)]


def distributed_parity_bits(enc):
    """How many parity bits are decoded before the last payload bit (3 or 7 with the interleaver, 0 without)."""
    inv = np.empty(enc.k_polar, np.int64)
    inv[enc.ind_input_int] = np.arange(enc.k_polar)
    upos = enc.info_pos[inv]
    return int((upos[enc.k:] < upos[:enc.k].max()).sum())


class DCIDecoder(nn.Module):
    """forward([..., n] logits log P(1)/P(0)) -> [..., k] payload bits (+ ok [...] with return_crc_status: 1 = a
    path that satisfies all 24 parity bits, RNTI included, was found).  list_size: a power of two in 1 ... 32.
    n_force: the first n_force parity bits in decoding order are FORCE constraints (used to correct), the rest CHECK
    (used to detect).  After forward(): last_stop [...] int32 (the leaf at which a row stopped; n_polar = it ran to
    the end) and last_pm.  Rows without a surviving path return an all-zero payload."""

    def __init__(self, enc, list_size=8, n_force=0, return_crc_status=False, output_dtype=tc.float32):
        super().__init__()
        if not isinstance(enc, DCIEncoder):
            raise ValueError("enc must be a DCIEncoder")
        if not 0 <= int(n_force) <= K_CRC:
            raise ValueError(f"n_force must lie in [0, {K_CRC}], got {n_force}")
        assert isinstance(return_crc_status, bool), "return_crc_status must be bool."
        from .pcl import PCL_Dec
        self._enc = enc
        self._n_target, self._k_target = enc.n, enc.k
        self._n_polar, self._k_polar = enc.n_polar, enc.k_polar
        self._bil = False   # no channel interleaver on the downlink
        self._llr_max = 100  # Polar5GDecoder's internal maximum (shortened positions)
        self.ind_ch_int_inv = None
        self.ind_sub_int_inv = np.argsort(subblock_interleaving(np.arange(self._n_polar)))
        self._build_recovery()
        self._dev_tables = {}
        self.n_force = int(n_force)
        self.constraints = dci_constraints(enc, self.n_force)
        self._pcl = PCL_Dec(enc.frozen_pos, enc.n_polar, pack_constraints(enc.n_polar, self.constraints),
                            list_size=list_size, return_status=True, llr_max=float(self._llr_max), device=enc.device)
        inv = np.empty(enc.k_polar, np.int64)
        inv[enc.ind_input_int] = np.arange(enc.k_polar)
        self._deint = inv[:enc.k]  # payload bit m is bit _deint[m] of the decoder's output
        self._return_crc_status = return_crc_status
        self._output_dtype = output_dtype
        self.list_size = self._pcl.list_size
        self.last_stop = self.last_pm = self.last_ok = None

    # Rate recovery: Polar5GDecoder's table logic, without the channel de-interleaver (_bil False).  polar5g.py is
    # left as it is (its behaviour is pinned to the reference), so its three methods are borrowed as plain functions
    # and this class supplies what they read: _build_recovery reads _n_polar, _n_target, _k_polar, _bil,
    # ind_ch_int_inv (only when _bil), ind_sub_int_inv and _llr_max and writes _rec; tables reads _rec and
    # _dev_tables (keyed by str(device); forward() adds its own "deint" + str(device) keys to the same dict);
    # rate_recover reads _n_target, _n_polar and tables().  A rename of any of these in Polar5GDecoder must be
    # followed here; tests/test_dci_gpu.py holds the result to the restatement's own rate recovery.
    _build_recovery = Polar5GDecoder._build_recovery
    tables = Polar5GDecoder.tables
    rate_recover = Polar5GDecoder.rate_recover

    @property
    def k(self):
        return self._k_target

    @property
    def n(self):
        return self._n_target

    @property
    def polar_dec(self):
        return self._pcl

    def decode_mother(self, llr_dec):
        """[bs, n_polar] mother-code logits on the GPU -> (bits [bs, k + 24] at the information positions, pm, ok,
        stop), all on the GPU."""
        return self._pcl.decode(llr_dec)

    def forward(self, inputs):
        inputs = inputs.to(tc.float32)
        assert inputs.shape[-1] == self._n_target, "Last input dim must be of len n."
        assert len(inputs.shape) > 1
        lead = list(inputs.shape[:-1])
        llr_ch = inputs.reshape([-1, self._n_target])
        dev = _gpu_for(llr_ch, self._enc.device)
        bits, pm, ok, stop = self.decode_mother(self.rate_recover(llr_ch.to(dev)))
        key = "deint" + str(dev)
        if key not in self._dev_tables:
            self._dev_tables[key] = _to_dev_i32(self._deint, dev)
        a_hat = _gather(bits, self._dev_tables[key], self._k_target)
        self.last_pm = pm.reshape(lead + [self.list_size]).to(inputs.device)
        self.last_stop = stop.reshape(lead).to(inputs.device)
        self.last_ok = ok.reshape(lead).to(inputs.device)
        a_hat = a_hat.reshape(lead + [self._k_target]).to(device=inputs.device, dtype=self._output_dtype)
        if not self._return_crc_status:
            return a_hat
        return a_hat, self.last_ok.to(self._output_dtype)
