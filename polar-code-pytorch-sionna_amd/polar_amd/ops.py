"""Tensor-level entry points over the C ABI (device tensors in, device tensors out).

Every function here launches a hand-written gfx950 kernel from libpolar_mi355x.so on the
current torch stream of the tensor's device; nothing runs on the CPU and there is no fallback.
"""
import ctypes

import torch

from . import _lib


def _require_cuda(t, name):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{name} must be a tensor on a ROCm GPU (got "
                           f"{getattr(t, 'device', type(t))}); the MI355X decoder has no CPU path")


def _counts(counts, device):
    """The int64 device counters a counting kernel accumulates into with 64-bit atomics: created
    if None, else checked (contiguous int64 with >= 2 elements on `device`), so a host, narrower
    or foreign-device tensor never reaches the kernel as a raw pointer."""
    if counts is None:
        return torch.zeros(2, dtype=torch.int64, device=device)
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or not counts.is_contiguous() \
            or counts.numel() < 2 or counts.device != torch.device(device):
        raise ValueError(f"counts must be a contiguous int64 tensor of >= 2 elements on {device}, got "
                         f"{getattr(counts, 'dtype', type(counts))} {tuple(getattr(counts, 'shape', ()))} on "
                         f"{getattr(counts, 'device', None)}")
    return counts


def _out_kind(dtype):
    if dtype == torch.float32:
        return _lib.PL_OUT_F32
    if dtype == torch.uint8:
        return _lib.PL_OUT_U8
    raise ValueError(f"unsupported decoder output dtype {dtype}")


def sc_decode(plan, llr_logits, out=None, out_dtype=torch.float32):
    """SC-decode [bs, n] fp32 logits on the GPU -> [bs, k] bits (polar_sc.py:113-133 semantics)."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    elif out.shape != (bs, plan.k) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)
    with torch.cuda.device(x.device):
        st = _lib.current_stream_ptr(x.device)
        _lib.check(_lib.lib().pl_sc_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), bs,
                                           ctypes.c_void_p(out.data_ptr()), kind, st), "pl_sc_decode")
    return out


def scl_workspace(plan, bs, device):
    """A device workspace of pl_scl_workspace_size(plan, bs) bytes (reusable across calls)."""
    ws_bytes = int(_lib.lib().pl_scl_workspace_size(plan.handle, bs))
    return torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=device)


def scl_decode(plan, llr_logits, out=None, out_dtype=torch.float32, return_pm=False, workspace=None):
    """SCL-decode [bs, n] fp32 logits -> [bs, k] bits (+ sorted path metrics [bs, 2L] fp64).
    workspace: optional uint8 device tensor from scl_workspace() (allocated per call if None)."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    elif out.shape != (bs, plan.k) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)
    L = _lib.lib()
    ws_bytes = int(L.pl_scl_workspace_size(plan.handle, bs))
    ws = workspace if workspace is not None else scl_workspace(plan, bs, x.device)
    # the kernel lays fp64 tables over the workspace's first ws_bytes bytes: a wider dtype, a strided
    # view or an address off 8 bytes would reach it as a raw pointer all the same
    if not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or not ws.is_contiguous() \
            or ws.device != x.device or ws.numel() < ws_bytes or (ws_bytes and ws.data_ptr() % 8):
        raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {ws_bytes} elements on {x.device}, "
                         "8-byte aligned (scl_workspace)")
    pm = torch.empty((bs, 2 * plan.list_size), dtype=torch.float64, device=x.device) if return_pm else None
    with torch.cuda.device(x.device):
        st = _lib.current_stream_ptr(x.device)
        _lib.check(L.pl_scl_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), bs, ctypes.c_void_p(out.data_ptr()),
                                   kind, ctypes.c_void_p(pm.data_ptr() if pm is not None else 0),
                                   ctypes.c_void_p(ws.data_ptr()), ws_bytes, st), "pl_scl_decode")
    return (out, pm) if return_pm else out


_hybrid_ws = {}  # (device, stream) -> the last hybrid workspace used there (grown, never shrunk)


def hybrid_workspace(sc_plan, scl_plan, bs, device):
    """A device workspace of pl_hybrid_workspace_size(sc_plan, scl_plan, bs) bytes, cached per
    device and stream and by size: one call after another on a stream reuses it (stream order
    keeps them apart), and a larger batch replaces it."""
    ws_bytes = int(_lib.lib().pl_hybrid_workspace_size(sc_plan.handle, scl_plan.handle, bs))
    device = torch.device(device)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _hybrid_ws.get(key)
    if ws is None or ws.numel() < ws_bytes:
        ws = _hybrid_ws[key] = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=device)
    return ws


def hybrid_decode(sc_plan, scl_plan, llr_logits, out=None, out_dtype=torch.float32, return_info=False):
    """Hybrid SC / SC-list decode (pl_hybrid_decode) of [bs, n] fp32 logits -> [bs, k] bits:
    sc_plan decodes every row, scl_plan (a list plan with a CRC, of the same code) decodes again
    the rows whose SC result fails the CRC.  return_info: also (crc_ok bool [bs]: the CRC of the
    row's output; list_rows int32 [n_list]: the rows that were list-decoded, ascending; n_list).
    The call synchronises the current stream once (the count of failing rows is read back)."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != scl_plan.n:
        raise ValueError(f"llr_logits must be [bs, {scl_plan.n}], got {tuple(x.shape)}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, scl_plan.k), dtype=out_dtype, device=x.device)
    elif out.shape != (bs, scl_plan.k) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)
    ok = torch.empty((bs,), dtype=torch.uint8, device=x.device) if return_info else None
    rows = torch.empty((bs,), dtype=torch.int32, device=x.device) if return_info else None
    n_list = ctypes.c_int64(0)
    L = _lib.lib()
    with torch.cuda.device(x.device):
        ws = hybrid_workspace(sc_plan, scl_plan, bs, x.device)
        ws_bytes = int(L.pl_hybrid_workspace_size(sc_plan.handle, scl_plan.handle, bs))
        _lib.check(L.pl_hybrid_decode(sc_plan.handle, scl_plan.handle, ctypes.c_void_p(x.data_ptr()), bs,
                                      ctypes.c_void_p(out.data_ptr()), kind,
                                      ctypes.c_void_p(ok.data_ptr() if return_info else 0),
                                      ctypes.c_void_p(rows.data_ptr() if return_info else 0), ctypes.byref(n_list),
                                      ctypes.c_void_p(ws.data_ptr()), ws_bytes, _lib.current_stream_ptr(x.device)),
                   "pl_hybrid_decode")
    if not return_info:
        return out
    return out, ok != 0, rows[: n_list.value], int(n_list.value)


_scf_ws = {}  # (device, stream) -> the last SC-Flip workspace used there (grown, never shrunk)


def scf_workspace(plan, bs, max_flips, device):
    """A device workspace of pl_scf_workspace_size(plan, bs, max_flips) bytes, cached per device and
    stream like hybrid_workspace: calls on one stream reuse it, a larger batch replaces it."""
    ws_bytes = int(_lib.lib().pl_scf_workspace_size(plan.handle, bs, int(max_flips)))
    device = torch.device(device)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _scf_ws.get(key)
    if ws is None or ws.numel() < ws_bytes:
        ws = _scf_ws[key] = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=device)
    return ws


def scf_decode(plan, llr_logits, max_flips, out=None, out_dtype=torch.float32, return_info=False):
    """CRC-aided SC-Flip decode (pl_scf_decode) of [bs, n] fp32 logits -> [bs, k] bits: SC, then a row
    whose result fails the plan's CRC (Plan.set_crc) is decoded again with the decision at each of its
    max_flips (0 ... 64) least reliable information positions inverted in turn, until the CRC passes.
    return_info: also (crc_ok bool [bs]; flip_pos int32 [bs], the inverted position 0 ... n-1 or -1;
    attempts int32 [bs], the SC decodes the sequential algorithm runs).  No host synchronisation: with
    `out` given and return_info False the call allocates nothing and can be captured (LaunchGraph)."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    max_flips = int(max_flips)
    if not 0 <= max_flips <= 64:
        raise ValueError(f"max_flips must be in [0, 64], got {max_flips}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    elif out.shape != (bs, plan.k) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)
    ok = torch.empty((bs,), dtype=torch.uint8, device=x.device) if return_info else None
    pos = torch.empty((bs,), dtype=torch.int32, device=x.device) if return_info else None
    att = torch.empty((bs,), dtype=torch.int32, device=x.device) if return_info else None
    L = _lib.lib()

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None and bs > 0 else 0)
    with torch.cuda.device(x.device):
        ws = scf_workspace(plan, bs, max_flips, x.device)
        ws_bytes = int(L.pl_scf_workspace_size(plan.handle, bs, max_flips))
        _lib.check(L.pl_scf_decode(plan.handle, ptr(x), bs, max_flips, ptr(out), kind, ptr(ok), ptr(pos), ptr(att),
                                   ctypes.c_void_p(ws.data_ptr()), ws_bytes, _lib.current_stream_ptr(x.device)),
                   "pl_scf_decode")
    if not return_info:
        return out
    return out, ok != 0, pos, att


def _width(q, name):
    try:
        v = q.__index__()  # Python and numpy integers, no floats
    except (AttributeError, TypeError):
        v = None
    if v is None or isinstance(q, bool) or not 2 <= v <= 8:
        raise ValueError(f"{name} must be an integer in [2, 8], got {q!r}")
    return v


def llr_quantize(llr_logits, inv_step, q_channel, out=None):
    """Quantise fp32 logits of any shape to int8 (pl_llr_quantize): q = rint(clamp(logit * inv_step, -Cmax, Cmax)),
    ties to even, Cmax = 2^(q_channel-1) - 1; +-Inf saturates.  The sign is kept (the decoder negates).  `out`:
    a contiguous int8 tensor of the input's shape on its device (then nothing is allocated)."""
    _require_cuda(llr_logits, "llr_logits")
    q_channel = _width(q_channel, "q_channel")
    inv_step = float(inv_step)
    if not (inv_step > 0.0 and inv_step != float("inf")):
        raise ValueError(f"inv_step must be positive and finite, got {inv_step}")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    elif out.dtype != torch.int8 or out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous int8 tensor of the input's shape on the input's device")
    count = x.numel()
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_llr_quantize(ctypes.c_void_p(x.data_ptr() if count else 0), count, inv_step, q_channel,
                                              ctypes.c_void_p(out.data_ptr() if count else 0),
                                              _lib.current_stream_ptr(x.device)), "pl_llr_quantize")
    return out


def scq_decode(plan, llr_q, q_internal, out=None, out_dtype=torch.float32):
    """Fixed-point SC decode (pl_scq_decode) of [bs, n] int8 LLRs (logit sign, any value) -> [bs, k] bits, all
    node values integers clamped to +-(2^(q_internal-1) - 1).  Only the plan's n and frozen set are used.  With
    `out` given nothing is allocated and the call can be captured (LaunchGraph)."""
    _require_cuda(llr_q, "llr_q")
    q_internal = _width(q_internal, "q_internal")
    x = llr_q
    if x.dtype != torch.int8:
        raise ValueError(f"llr_q must be an int8 tensor (llr_quantize), got {x.dtype}")
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_q must be [bs, {plan.n}], got {tuple(x.shape)}")
    if not x.is_contiguous() or x.data_ptr() % 16:  # the kernel reads a row 16 bytes at a time
        x = x.clone(memory_format=torch.contiguous_format)
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    elif out.shape != (bs, plan.k) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_scq_decode(plan.handle, ctypes.c_void_p(x.data_ptr() if bs else 0), bs, q_internal,
                                            ctypes.c_void_p(out.data_ptr() if bs else 0), kind,
                                            _lib.current_stream_ptr(x.device)), "pl_scq_decode")
    return out


def ae_perm_table(perms, device):
    """[M, n] integer permutations (rows) -> the contiguous device table pl_ae_decode reads: uint16 values
    carried in an int16 tensor (1 <= M <= 64, entries in [0, n), n <= 1024)."""
    import numpy as np
    p = np.asarray(perms.cpu() if isinstance(perms, torch.Tensor) else perms)
    if p.ndim != 2 or not 1 <= p.shape[0] <= 64 or p.dtype.kind not in "iu":
        raise ValueError(f"perms must be an [M, n] integer array with 1 <= M <= 64, got {p.dtype} {p.shape}")
    if p.min() < 0 or p.max() >= p.shape[1]:
        raise ValueError("perms: entries must be in [0, n)")
    return torch.from_numpy(np.ascontiguousarray(p.astype(np.uint16)).view(np.int16)).to(device)


def ae_decode(plan, llr_logits, perm_table, out=None, out_dtype=torch.float32, return_info=False):
    """Automorphism-ensemble SC decode (pl_ae_decode) of [bs, n] fp32 logits -> [bs, k] bits: every row is
    decoded by plain SC through each of the M permutations of perm_table (ae_perm_table: [M, n] on the
    input's device) and the candidate codeword closest to the row is kept.  return_info: also (best_idx
    int32 [bs], the winning candidate; best_metric fp32 [bs], its distance sum |a_i| [x_i != HD(a_i)]).
    One launch, no workspace, no host synchronisation: with `out` given and return_info False the call
    allocates nothing and can be captured (LaunchGraph)."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    t = perm_table
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int16 or t.dim() != 2 or t.shape[1] != plan.n or \
            not t.is_contiguous() or t.device != x.device:
        raise ValueError("perm_table must be a contiguous int16 [M, n] tensor on the input's device (ae_perm_table)")
    if not 1 <= t.shape[0] <= 64:
        raise ValueError(f"perm_table must hold 1 ... 64 permutations, got {t.shape[0]}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    elif out.shape != (bs, plan.k) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)
    idx = torch.empty((bs,), dtype=torch.int32, device=x.device) if return_info else None
    met = torch.empty((bs,), dtype=torch.float32, device=x.device) if return_info else None

    def ptr(v):
        return ctypes.c_void_p(v.data_ptr() if v is not None and bs > 0 else 0)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_ae_decode(plan.handle, ptr(x), bs, ctypes.c_void_p(t.data_ptr()), t.shape[0], ptr(out),
                                           kind, ptr(idx), ptr(met), _lib.current_stream_ptr(x.device)),
                   "pl_ae_decode")
    if not return_info:
        return out
    return out, idx, met


def crc_status(plan, bits):
    """pl_crc_status: [bs, k] decoded bits (fp32 0/1 or uint8) -> bool [bs], True where the row
    passes the CRC of the plan (pl_plan_set_crc; the last `degree` bits are the parity)."""
    _require_cuda(bits, "bits")
    b = bits
    if b.dtype not in (torch.float32, torch.uint8):
        b = b.to(torch.float32)
    b = b.contiguous()
    if b.dim() != 2 or b.shape[1] != plan.k:
        raise ValueError(f"bits must be [bs, {plan.k}], got {tuple(b.shape)}")
    valid = torch.empty((b.shape[0],), dtype=torch.uint8, device=b.device)
    with torch.cuda.device(b.device):
        _lib.check(_lib.lib().pl_crc_status(plan.handle, ctypes.c_void_p(b.data_ptr()), _out_kind(b.dtype), b.shape[0],
                                            ctypes.c_void_p(valid.data_ptr()), _lib.current_stream_ptr(b.device)),
                   "pl_crc_status")
    return valid != 0


def osd_decode(plan, llr_logits, out=None, out_dtype=torch.float32, return_dist=False, return_pattern=False):
    """Ordered-statistics decode (pl_osd_decode, plan: _lib.OsdPlan) of [bs, n] fp32 logits
    log P(1)/P(0) -> [bs, n] codeword bits in channel order (my_sn/fec/osd/dec.py:148-192).
    return_dist: also the fp64 metric [bs] of each returned word (the mean softplus of dec.py:68-81);
    return_pattern: also int32 [bs], -1 where the re-encoded hard decision c0 won, else the index of
    the winning error pattern (orders 1 .. t in turn, each in itertools.combinations order)."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.n), dtype=out_dtype, device=x.device)
    elif out.shape != (bs, plan.n) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, n] tensor on the input's device")
    kind = _out_kind(out.dtype)
    dist = torch.empty((bs,), dtype=torch.float64, device=x.device) if return_dist else None
    pat = torch.empty((bs,), dtype=torch.int32, device=x.device) if return_pattern else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_osd_decode(plan.handle, ctypes.c_void_p(x.data_ptr()), bs,
                                            ctypes.c_void_p(out.data_ptr()), kind,
                                            ctypes.c_void_p(dist.data_ptr() if return_dist else 0),
                                            ctypes.c_void_p(pat.data_ptr() if return_pattern else 0),
                                            _lib.current_stream_ptr(x.device)), "pl_osd_decode")
    res = (out,) + ((dist,) if return_dist else ()) + ((pat,) if return_pattern else ())
    return res if len(res) > 1 else out


def polar_encode(plan, u_bits, out=None):
    """Encode [bs, k] 0/1 fp32 information bits -> [bs, n] fp32 codewords (enc.py:30-43)."""
    _require_cuda(u_bits, "u_bits")
    u = u_bits
    if u.dtype != torch.float32 or not u.is_contiguous():
        u = u.to(torch.float32).contiguous()
    if u.dim() != 2 or u.shape[1] != plan.k:
        raise ValueError(f"u_bits must be [bs, {plan.k}], got {tuple(u.shape)}")
    bs = u.shape[0]
    if out is None:
        out = torch.empty((bs, plan.n), dtype=torch.float32, device=u.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != (bs, plan.n) \
            or not out.is_contiguous() or out.device != u.device:
        raise ValueError("out must be a contiguous float32 [bs, n] tensor on the input's device")
    with torch.cuda.device(u.device):
        st = _lib.current_stream_ptr(u.device)
        _lib.check(_lib.lib().pl_polar_encode(plan.handle, ctypes.c_void_p(u.data_ptr()), bs,
                                              ctypes.c_void_p(out.data_ptr()), st), "pl_polar_encode")
    return out


def awgn_qpsk_llr(plan, bs, no, seed, iteration, row0=0, with_bits=True):
    """The fused System_AWGN_model producer (pl_awgn_qpsk_llr) on the plan's device: returns
    (u [bs, k] fp32 0/1 or None, logits [bs, n] fp32) for rows row0.. of the (seed, iteration)
    stream."""
    dev = plan.device
    no = float(no)
    if not no > 0.0:
        raise ValueError(f"noise variance must be positive, got {no}")
    if not 0 <= int(iteration) < 2 ** 32:
        raise ValueError(f"iteration must be in [0, 2^32) (the Philox counter word), got {iteration}")
    llr = torch.empty((bs, plan.n), dtype=torch.float32, device=dev)
    u = torch.empty((bs, plan.k), dtype=torch.float32, device=dev) if with_bits else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pl_awgn_qpsk_llr(plan.handle, int(seed) & (2 ** 64 - 1), int(iteration) & (2 ** 64 - 1),
                                               int(row0), int(bs), no,
                                               ctypes.c_void_p(u.data_ptr() if u is not None else 0),
                                               ctypes.c_void_p(llr.data_ptr()), _lib.current_stream_ptr(dev)),
                   "pl_awgn_qpsk_llr")
    return u, llr


def awgn_qpsk_llr_bits(plan, bs, no, seed, iteration, row0=0):
    """pl_awgn_qpsk_llr_bits: the fused producer with the information bits packed -- returns
    (ubits [bs, ceil(k/32)] int32 words, bit m % 32 of word m // 32 = bit m; logits [bs, n] fp32).
    Same stream and logits as awgn_qpsk_llr."""
    dev = plan.device
    no = float(no)
    if not no > 0.0:
        raise ValueError(f"noise variance must be positive, got {no}")
    if not 0 <= int(iteration) < 2 ** 32:
        raise ValueError(f"iteration must be in [0, 2^32) (the Philox counter word), got {iteration}")
    llr = torch.empty((bs, plan.n), dtype=torch.float32, device=dev)
    ubits = torch.empty((bs, (plan.k + 31) // 32), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pl_awgn_qpsk_llr_bits(plan.handle, int(seed) & (2 ** 64 - 1),
                                                    int(iteration) & (2 ** 64 - 1), int(row0), int(bs), no,
                                                    ctypes.c_void_p(ubits.data_ptr()), ctypes.c_void_p(llr.data_ptr()),
                                                    _lib.current_stream_ptr(dev)),
                   "pl_awgn_qpsk_llr_bits")
    return ubits, llr


def _table(t, dtype, numel, name, device, optional=False):
    """A device table handed to a kernel as a raw pointer: contiguous, of this dtype, length and device."""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.numel() != numel \
            or t.device != torch.device(device):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of {numel} elements on {device}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on "
                         f"{getattr(t, 'device', None)}")
    return t


def nr_awgn_qpsk_llr(plan, k_target, g_rows, crc_degree, rm_idx, src_a, src_b, fill, bs, no, seed, iteration, row0=0,
                     with_u=True, with_ubits=True, with_ch=False):
    """The fused 5G NR link producer (pl_nr_awgn_qpsk_llr) on the mother-code plan's device: for rows
    row0.. of the (seed, iteration) stream, information bits -> CRC attach -> polar encode -> rate
    matching -> QPSK -> AWGN of variance `no` -> demapper -> rate recovery, one launch.
    g_rows int32 [k_target] and crc_degree (bits): Polar5GEncoder.tables()[0] / crc_length; rm_idx
    int32 [E]: tables()[1]; src_a, src_b (or None), fill (or None): Polar5GDecoder.tables().
    Returns (u [bs, k_target] fp32 or None, ubits [bs, ceil(k_target/32)] int32 or None,
    llr_ch [bs, E] fp32 or None, llr [bs, n] fp32), the optional ones as with_u / with_ubits / with_ch
    say.  Bad values (odd E, no <= 0, a plan whose k is not k_target + crc_degree, an iteration outside
    [0, 2^32)) raise PolarArgumentError from the library."""
    dev = plan.device
    k_target, bs = int(k_target), int(bs)
    if k_target < 0 or bs < 0:
        raise ValueError(f"k_target and bs must be >= 0, got {k_target}, {bs}")
    if not isinstance(rm_idx, torch.Tensor) or rm_idx.dim() != 1:
        raise ValueError("rm_idx must be a 1-D int32 tensor (the rate-matching gather index)")
    e = int(rm_idx.numel())
    g_rows = _table(g_rows, torch.int32, k_target, "g_rows", dev)
    rm_idx = _table(rm_idx, torch.int32, e, "rm_idx", dev)
    src_a = _table(src_a, torch.int32, plan.n, "src_a", dev)
    src_b = _table(src_b, torch.int32, plan.n, "src_b", dev, optional=True)
    fill = _table(fill, torch.float32, plan.n, "fill", dev, optional=True)
    nq = (k_target + 31) // 32
    llr = torch.empty((bs, plan.n), dtype=torch.float32, device=dev)
    u = torch.empty((bs, k_target), dtype=torch.float32, device=dev) if with_u else None
    ubits = torch.empty((bs, nq), dtype=torch.int32, device=dev) if with_ubits else None
    ch = torch.empty((bs, e), dtype=torch.float32, device=dev) if with_ch else None

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pl_nr_awgn_qpsk_llr(plan.handle, k_target, ptr(g_rows), int(crc_degree), ptr(rm_idx), e,
                                                  ptr(src_a), ptr(src_b), ptr(fill), int(seed) & (2 ** 64 - 1),
                                                  int(iteration) & (2 ** 64 - 1), int(row0), bs, float(no),
                                                  ptr(ubits), ptr(u), ptr(ch), ptr(llr),
                                                  _lib.current_stream_ptr(dev)), "pl_nr_awgn_qpsk_llr")
    return u, ubits, ch, llr


QAM_BITS_PER_SYMBOL = (2, 4, 6, 8)  # what the fused producers modulate: QPSK, 16-, 64-, 256-QAM


def check_bits_per_symbol(m, positions, what):
    """ValueError unless m is one of QAM_BITS_PER_SYMBOL and divides the row's `positions` (`what`
    names them: the code length n, or the transmitted length E)."""
    if m not in QAM_BITS_PER_SYMBOL:
        raise ValueError(f"num_bits_per_symbol must be one of {QAM_BITS_PER_SYMBOL}, got {m}")
    if int(positions) % m != 0:
        raise ValueError(f"num_bits_per_symbol {m} must divide {what} = {positions} (whole symbols)")
    return int(m)


def awgn_qam_llr(plan, bits_per_symbol, bs, no, seed, iteration, row0=0, with_u=True, with_ubits=False, with_y=False):
    """The fused System_AWGN_model producer over 2^m-QAM (pl_awgn_qam_llr), m = bits_per_symbol in
    {2, 4, 6, 8} dividing plan.n, on the plan's device: returns (u [bs, k] fp32 0/1 or None, ubits
    [bs, ceil(k/32)] int32 or None, y [bs, n/m, 2] fp32 received symbols or None, logits [bs, n]
    fp32) for rows row0.. of the (seed, iteration) stream, the optional ones as with_u / with_ubits
    / with_y say (with_y needs m > 2).  The information bits are awgn_qpsk_llr's for the same key."""
    dev = plan.device
    no, bs = float(no), int(bs)
    m = check_bits_per_symbol(bits_per_symbol, plan.n, "the code length n")
    if not no > 0.0:
        raise ValueError(f"noise variance must be positive, got {no}")
    if not 0 <= int(iteration) < 2 ** 32:
        raise ValueError(f"iteration must be in [0, 2^32) (the Philox counter word), got {iteration}")
    if bs < 0:
        raise ValueError(f"bs must be >= 0, got {bs}")
    if with_y and m == 2:
        raise ValueError("with_y needs num_bits_per_symbol > 2 (the QPSK kernel does not write the symbols)")
    llr = torch.empty((bs, plan.n), dtype=torch.float32, device=dev)
    u = torch.empty((bs, plan.k), dtype=torch.float32, device=dev) if with_u else None
    ubits = torch.empty((bs, (plan.k + 31) // 32), dtype=torch.int32, device=dev) if with_ubits else None
    y = torch.empty((bs, plan.n // m, 2), dtype=torch.float32, device=dev) if with_y else None

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pl_awgn_qam_llr(plan.handle, m, int(seed) & (2 ** 64 - 1), int(iteration) & (2 ** 64 - 1),
                                              int(row0), bs, no, ptr(u), ptr(ubits), ptr(y), ptr(llr),
                                              _lib.current_stream_ptr(dev)), "pl_awgn_qam_llr")
    return u, ubits, y, llr


def nr_awgn_qam_llr(plan, bits_per_symbol, k_target, g_rows, crc_degree, rm_idx, src_a, src_b, fill, bs, no, seed,
                    iteration, row0=0, with_u=True, with_ubits=True, with_ch=False, with_y=False):
    """The fused 5G NR link producer over 2^m-QAM (pl_nr_awgn_qam_llr), m = bits_per_symbol in
    {2, 4, 6, 8} dividing E = len(rm_idx): nr_awgn_qpsk_llr's arguments and outputs, plus y [bs, E/m, 2]
    fp32 received symbols (with_y, m > 2).  Returns (u, ubits, llr_ch, y, llr)."""
    dev = plan.device
    k_target, bs = int(k_target), int(bs)
    if k_target < 0 or bs < 0:
        raise ValueError(f"k_target and bs must be >= 0, got {k_target}, {bs}")
    if not isinstance(rm_idx, torch.Tensor) or rm_idx.dim() != 1:
        raise ValueError("rm_idx must be a 1-D int32 tensor (the rate-matching gather index)")
    e = int(rm_idx.numel())
    m = check_bits_per_symbol(bits_per_symbol, e, "the transmitted length E")
    if with_y and m == 2:
        raise ValueError("with_y needs num_bits_per_symbol > 2 (the QPSK kernel does not write the symbols)")
    g_rows = _table(g_rows, torch.int32, k_target, "g_rows", dev)
    rm_idx = _table(rm_idx, torch.int32, e, "rm_idx", dev)
    src_a = _table(src_a, torch.int32, plan.n, "src_a", dev)
    src_b = _table(src_b, torch.int32, plan.n, "src_b", dev, optional=True)
    fill = _table(fill, torch.float32, plan.n, "fill", dev, optional=True)
    nq = (k_target + 31) // 32
    llr = torch.empty((bs, plan.n), dtype=torch.float32, device=dev)
    u = torch.empty((bs, k_target), dtype=torch.float32, device=dev) if with_u else None
    ubits = torch.empty((bs, nq), dtype=torch.int32, device=dev) if with_ubits else None
    ch = torch.empty((bs, e), dtype=torch.float32, device=dev) if with_ch else None
    y = torch.empty((bs, e // m, 2), dtype=torch.float32, device=dev) if with_y else None

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pl_nr_awgn_qam_llr(plan.handle, m, k_target, ptr(g_rows), int(crc_degree), ptr(rm_idx), e,
                                                 ptr(src_a), ptr(src_b), ptr(fill), int(seed) & (2 ** 64 - 1),
                                                 int(iteration) & (2 ** 64 - 1), int(row0), bs, float(no),
                                                 ptr(ubits), ptr(u), ptr(y), ptr(ch), ptr(llr),
                                                 _lib.current_stream_ptr(dev)), "pl_nr_awgn_qam_llr")
    return u, ubits, ch, y, llr


def count_errors_packed(bits, ref_bits, k_cmp=None, counts=None):
    """pl_count_errors_packed: [bit errors, block errors] (int64, on the device) of the first k_cmp
    columns (default: all) of `bits` ([bs, row_len] fp32 0/1 or uint8, e.g. a decoder's k_polar-wide
    output) against `ref_bits` ([bs, ceil(k_cmp/32)] int32 words, nr_awgn_qpsk_llr's / pack_bits'
    layout); accumulates into counts (created if None) and returns it."""
    _require_cuda(bits, "bits")
    b = bits
    if b.dtype not in (torch.float32, torch.uint8):
        b = b.to(torch.float32)
    b = b.contiguous()
    if b.dim() != 2:
        raise ValueError(f"bits must be [bs, row_len], got {tuple(b.shape)}")
    bs, row_len = b.shape
    k_cmp = row_len if k_cmp is None else int(k_cmp)
    if not 0 <= k_cmp <= row_len:
        raise ValueError(f"k_cmp must be in [0, {row_len}], got {k_cmp}")
    nq = (k_cmp + 31) // 32
    if not isinstance(ref_bits, torch.Tensor) or ref_bits.shape != (bs, nq) or ref_bits.dtype != torch.int32 \
            or ref_bits.device != b.device:
        raise ValueError(f"ref_bits must be int32 [{bs}, {nq}] on the input's device")
    ref = ref_bits.contiguous()
    counts = _counts(counts, b.device)
    with torch.cuda.device(b.device):
        _lib.check(_lib.lib().pl_count_errors_packed(ctypes.c_void_p(b.data_ptr()), _out_kind(b.dtype), bs, row_len,
                                                     k_cmp, ctypes.c_void_p(ref.data_ptr()),
                                                     ctypes.c_void_p(counts.data_ptr()),
                                                     _lib.current_stream_ptr(b.device)), "pl_count_errors_packed")
    return counts


def genie_count(n, llr_logits, u_bits, f_mode=0, llr_max=30.0, counts=None, return_leaf=False):
    """pl_genie_count: genie-aided SC of [bs, n] fp32 logits whose u-domain words are u_bits ([bs,
    ceil(n/32)] int32, ALL n positions packed as pack_bits does): counts[i] += the rows whose leaf
    LLR at position i decides against u[i] when every earlier bit is fed back correctly.  counts:
    int64 [n] on the input's device, accumulated into (created if None; False: no counting, with
    return_leaf).  Returns counts, or (counts, leaf [bs, n] fp32: positive favours 0) with return_leaf."""
    _require_cuda(llr_logits, "llr_logits")
    n = int(n)
    if n < 2 or n > 2048 or n & (n - 1):
        raise ValueError(f"n must be a power of two in [2, 2048], got {n}")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != n:
        raise ValueError(f"llr_logits must be [bs, {n}], got {tuple(x.shape)}")
    bs, nq = x.shape[0], (n + 31) // 32
    if not isinstance(u_bits, torch.Tensor) or u_bits.shape != (bs, nq) or u_bits.dtype != torch.int32 \
            or u_bits.device != x.device:
        raise ValueError(f"u_bits must be int32 [{bs}, {nq}] on the input's device")
    u = u_bits.contiguous()
    if counts is False:
        if not return_leaf:
            raise ValueError("counts=False needs return_leaf=True: nothing to compute")
        counts = None
    elif counts is None:
        counts = torch.zeros(n, dtype=torch.int64, device=x.device)
    elif not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or not counts.is_contiguous() \
            or counts.shape != (n,) or counts.device != x.device:
        raise ValueError(f"counts must be a contiguous int64 [{n}] tensor on {x.device}")
    leaf = torch.empty((bs, n), dtype=torch.float32, device=x.device) if return_leaf else None

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_genie_count(n, int(f_mode), float(llr_max), ptr(x), ptr(u), bs, ptr(counts), ptr(leaf),
                                             _lib.current_stream_ptr(x.device)), "pl_genie_count")
    return (counts, leaf) if return_leaf else counts


def _soft_decode(entry, what, flag, plan, llr_logits, num_iter, scale, early_stop, out_dtype, hard, soft, ext, iters):
    """The tensor side shared by bp_decode and scan_decode (one C signature): checks, the requested outputs,
    the call of `entry` (a name in the library) on the input's device and current stream."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    bs = x.shape[0]
    out = {}
    if hard:
        out["bits"] = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    if soft:
        out["soft_u"] = torch.empty((bs, plan.k), dtype=torch.float32, device=x.device)
    if ext:
        out["ext_x"] = torch.empty((bs, plan.n), dtype=torch.float32, device=x.device)
    if iters:
        out["iters"] = torch.empty((bs,), dtype=torch.int32, device=x.device)
    kind = _out_kind(out_dtype) if hard else _lib.PL_OUT_F32
    if not out:
        raise ValueError(f"{what}: no output requested (hard, soft, ext, iters)")
    if bs == 0:  # empty tensors have no address to hand over
        return out

    def ptr(name):
        return ctypes.c_void_p(out[name].data_ptr() if name in out else 0)
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.lib(), entry)(plan.handle, ctypes.c_void_p(x.data_ptr()), bs, int(num_iter), float(scale),
                                              flag if early_stop else 0, ptr("bits"), kind, ptr("soft_u"), ptr("ext_x"),
                                              ptr("iters"), _lib.current_stream_ptr(x.device)), entry)
    return out


def bp_decode(plan, llr_logits, num_iter=20, scale=1.0, early_stop=False, out_dtype=torch.float32, hard=True,
              soft=False, ext=False, iters=False):
    """pl_bp_decode: belief-propagation decode of [bs, n] fp32 logits with the list-size-1 `plan`
    (its n <= 1024, frozen set, f mode and llr_max).  Returns a dict with the requested outputs:
    'bits' [bs, k] (hard), 'soft_u' [bs, k] fp32 logits of the information bits (soft), 'ext_x' [bs, n]
    fp32 extrinsic logits of the code bits (ext), 'iters' [bs] int32 iterations run (iters).  scale in
    (0, 1] multiplies the min-sum magnitude; early_stop ends a row once its hard decisions re-encode
    to the hard decisions on the code bits.  Nothing is synchronised: the call can be graph-captured."""
    return _soft_decode("pl_bp_decode", "bp_decode", _lib.PL_BP_EARLY_STOP, plan, llr_logits, num_iter, scale,
                        early_stop, out_dtype, hard, soft, ext, iters)


def scan_decode(plan, llr_logits, num_iter=2, scale=1.0, early_stop=False, out_dtype=torch.float32, hard=True,
                soft=False, ext=False, iters=False):
    """pl_scan_decode: soft-cancellation (SCAN) decode of [bs, n] fp32 logits with the list-size-1 `plan`
    (its n <= 2048, frozen set, f mode and llr_max): bp_decode's messages, arguments and outputs on the
    schedule of the SC tree walk.  Nothing is synchronised: the call can be graph-captured."""
    return _soft_decode("pl_scan_decode", "scan_decode", _lib.PL_SCAN_EARLY_STOP, plan, llr_logits, num_iter, scale,
                        early_stop, out_dtype, hard, soft, ext, iters)


def _conv_mask(conv_mask):
    """The uint32 generator mask of a PAC code (bit j = c_j) as a Python int; c_0 must be set."""
    try:
        m = conv_mask.__index__()
    except (AttributeError, TypeError):
        m = None
    if m is None or isinstance(conv_mask, bool) or not 0 < m < 2 ** 32 or not m & 1:
        raise ValueError(f"conv_mask must be an integer in [1, 2^32) with bit 0 (c_0) set, got {conv_mask!r}")
    return m


def pac_encode(plan, conv_mask, data_bits, out=None):
    """pl_pac_encode: [bs, k] 0/1 data bits -> [bs, n] fp32 codewords of the PAC code (the plan's n <= 1024 and
    frozen set as rate profile, the generator conv_mask: bit j = c_j): rate-profile scatter, convolutional
    precoder u_i = XOR_j c_j v_{i-j}, polar transform.  conv_mask = 1 is polar_encode."""
    _require_cuda(data_bits, "data_bits")
    m = _conv_mask(conv_mask)
    u = data_bits
    if u.dtype != torch.float32 or not u.is_contiguous():
        u = u.to(torch.float32).contiguous()
    if u.dim() != 2 or u.shape[1] != plan.k:
        raise ValueError(f"data_bits must be [bs, {plan.k}], got {tuple(u.shape)}")
    bs = u.shape[0]
    if out is None:
        out = torch.empty((bs, plan.n), dtype=torch.float32, device=u.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != (bs, plan.n) \
            or not out.is_contiguous() or out.device != u.device:
        raise ValueError("out must be a contiguous float32 [bs, n] tensor on the input's device")
    with torch.cuda.device(u.device):
        _lib.check(_lib.lib().pl_pac_encode(plan.handle, m, ctypes.c_void_p(u.data_ptr() if u.numel() else 0), bs,
                                            ctypes.c_void_p(out.data_ptr() if bs else 0),
                                            _lib.current_stream_ptr(u.device)), "pl_pac_encode")
    return out


def pac_decode(plan, conv_mask, list_size, llr_logits, out=None, out_dtype=torch.float32, return_pm=False):
    """pl_pac_decode: list-decode [bs, n] fp32 logits of the PAC code (plan: a min-sum plan without a CRC; its
    n <= 1024, frozen set and llr_max are used; conv_mask: bit j = c_j) with list_size paths, a power of two in
    1 ... 32 -> [bs, k] data bits (+ the final path metrics [bs, list_size] fp32, ascending, with return_pm).
    One launch, no workspace, no host synchronisation: with `out` given and return_pm False the call
    allocates nothing and can be captured (LaunchGraph)."""
    _require_cuda(llr_logits, "llr_logits")
    m = _conv_mask(conv_mask)
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    list_size = int(list_size)
    if not 1 <= list_size <= 32 or list_size & (list_size - 1):
        raise ValueError(f"list_size must be a power of two in [1, 32], got {list_size}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.shape != (bs, plan.k) or not out.is_contiguous() \
            or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)
    pm = torch.empty((bs, list_size), dtype=torch.float32, device=x.device) if return_pm else None

    def ptr(v):
        return ctypes.c_void_p(v.data_ptr() if v is not None and v.numel() > 0 else 0)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_pac_decode(plan.handle, m, list_size, ptr(x), bs, ptr(out), kind, ptr(pm),
                                            _lib.current_stream_ptr(x.device)), "pl_pac_decode")
    return (out, pm) if return_pm else out


def pcl_decode(plan, table, list_size, llr_logits, out=None, out_dtype=torch.float32, return_pm=False,
               return_status=False, pm=None, ok=None, stop=None):
    """pl_pcl_decode: list-decode [bs, n] fp32 logits under the parity constraints of `table` (_lib.PclTable, made
    for `plan`: a min-sum plan without a CRC; its n <= 1024, frozen set and llr_max are used) with list_size paths, a
    power of two in 1 ... 32 -> [bs, k] u-bits at the information positions, constrained positions included, all
    zero for a row with no path left.  return_pm adds the final metrics [bs, list_size] fp32, ascending, +inf for
    dead paths; return_status adds ok [bs] uint8 (1 = a live path was output) and stop [bs] int32 (the leaf at which
    the row stopped, n if it ran to the end).  The returned tuple is (bits[, pm][, ok, stop]).  pm / ok / stop may be
    given as preallocated tensors.  One launch, no workspace, no host synchronisation: with every requested output
    given the call allocates nothing and can be captured (LaunchGraph)."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    list_size = int(list_size)
    if not 1 <= list_size <= 32 or list_size & (list_size - 1):
        raise ValueError(f"list_size must be a power of two in [1, 32], got {list_size}")
    bs = x.shape[0]
    if out is None:
        out = torch.empty((bs, plan.k), dtype=out_dtype, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.shape != (bs, plan.k) or not out.is_contiguous() \
            or out.device != x.device:
        raise ValueError("out must be a contiguous [bs, k] tensor on the input's device")
    kind = _out_kind(out.dtype)

    def side(t, want, shape, dtype, name):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=x.device) if want else None
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.shape != shape or not t.is_contiguous() \
                or t.device != x.device:
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the input's device")
        return t
    pm = side(pm, return_pm, (bs, list_size), torch.float32, "pm")
    ok = side(ok, return_status, (bs,), torch.uint8, "ok")
    stop = side(stop, return_status, (bs,), torch.int32, "stop")

    def ptr(v):
        return ctypes.c_void_p(v.data_ptr() if v is not None and v.numel() > 0 else 0)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_pcl_decode(plan.handle, table.handle, list_size, ptr(x), bs, ptr(out), kind, ptr(pm),
                                            ptr(ok), ptr(stop), _lib.current_stream_ptr(x.device)), "pl_pcl_decode")
    res = (out,) + ((pm,) if return_pm else ()) + ((ok, stop) if return_status else ())
    return res if len(res) > 1 else out


def pack_bits(bits):
    """[..., k] 0/1 tensor -> [rows, ceil(k/32)] int32 words in pl_sc_decode_count's layout."""
    k = bits.shape[-1]
    b = (bits.reshape(-1, k) != 0).to(torch.int64)
    nq = (k + 31) // 32
    b = torch.nn.functional.pad(b, (0, nq * 32 - k)).reshape(-1, nq, 32)
    w = (b << torch.arange(32, device=b.device, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)



def sc_decode_count(plan, llr_logits, ref_bits, counts=None):
    """pl_sc_decode_count: SC decode fused with count_errors / count_block_errors (my_sn/sim.py:7-18)
    against packed reference bits (awgn_qpsk_llr_bits / pack_bits); accumulates [bit errors, block
    errors] into counts (int64 [2] on the device, created if None) and returns it.  Raises
    PolarLibError (PL_ENOTSUP) for a plan on the generic SC kernel."""
    _require_cuda(llr_logits, "llr_logits")
    x = llr_logits
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != plan.n:
        raise ValueError(f"llr_logits must be [bs, {plan.n}], got {tuple(x.shape)}")
    bs = x.shape[0]
    nq = (plan.k + 31) // 32
    if not isinstance(ref_bits, torch.Tensor) or ref_bits.shape != (bs, nq) or ref_bits.dtype != torch.int32 \
            or ref_bits.device != x.device:
        raise ValueError(f"ref_bits must be int32 [{bs}, {nq}] on the input's device")
    ref = ref_bits.contiguous()
    counts = _counts(counts, x.device)
    ws_bytes = int(_lib.lib().pl_sc_count_workspace_size(plan.handle, bs))
    ws = torch.empty((max(ws_bytes, 4),), dtype=torch.uint8, device=x.device)  # per call: stream-safe
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().pl_sc_decode_count(plan.handle, ctypes.c_void_p(x.data_ptr()), bs,
                                                 ctypes.c_void_p(ref.data_ptr()), ctypes.c_void_p(counts.data_ptr()),
                                                 ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                                                 _lib.current_stream_ptr(x.device)), "pl_sc_decode_count")
    return counts


def sc_sim_count(plan, bs, no, seed, iteration, row0=0, counts=None, dump=False):
    """pl_sc_sim_count: one Monte-Carlo iteration inside the specialised SC kernel -- information
    bits, encoder, QPSK, AWGN and logits generated in the decoder's registers, decoded and counted
    (System_AWGN_model.forward + my_sn/sim.py:84-100).  Accumulates [bit errors, block errors] into
    counts (int64 [2] on the plan's device, created if None) and returns it; with dump=True returns
    (counts, u [bs, k] fp32, logits [bs, n] fp32) as generated.  Raises PolarLibError (PL_ENOTSUP)
    for plans without the fused entry (generic kernel, or not 64 channel slots per lane)."""
    dev = plan.device
    no = float(no)
    if not no > 0.0:
        raise ValueError(f"noise variance must be positive, got {no}")
    bs = int(bs)
    if not 0 <= int(iteration) < 2 ** 32:
        raise ValueError(f"iteration must be in [0, 2^32) (the Philox counter word), got {iteration}")
    counts = _counts(counts, dev)
    u = llr = None
    if dump:
        u = torch.empty((bs, plan.k), dtype=torch.float32, device=dev)
        llr = torch.empty((bs, plan.n), dtype=torch.float32, device=dev)
    ws_bytes = int(_lib.lib().pl_sc_count_workspace_size(plan.handle, bs))
    ws = torch.empty((max(ws_bytes, 4),), dtype=torch.uint8, device=dev)  # per call: stream-safe
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pl_sc_sim_count(plan.handle, int(seed) & (2 ** 64 - 1), int(iteration) & (2 ** 64 - 1),
                                              int(row0), bs, no, ctypes.c_void_p(counts.data_ptr()),
                                              ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                                              ctypes.c_void_p(llr.data_ptr() if dump else None),
                                              ctypes.c_void_p(u.data_ptr() if dump else None),
                                              _lib.current_stream_ptr(dev)), "pl_sc_sim_count")
    return (counts, u, llr) if dump else counts


def count_errors(a, b, counts=None):
    """[bit errors, block errors] (int64, on the device) of two [..., k] 0/1 fp32 tensors
    (my_sn/sim.py:7-18 count_errors / count_block_errors in one pass); accumulates into counts."""
    _require_cuda(a, "a")
    _require_cuda(b, "b")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("count_errors: tensors must have the same shape and device")
    k = a.shape[-1] if a.dim() else 1
    x = a.to(torch.float32).contiguous()
    y = b.to(torch.float32).contiguous()
    rows = x.numel() // k if k else 0
    counts = _counts(counts, a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().pl_count_errors(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), rows, k,
                                              ctypes.c_void_p(counts.data_ptr()), _lib.current_stream_ptr(a.device)),
                   "pl_count_errors")
    return counts


class LaunchGraph:
    """`launches` back-to-back calls of fn() (decodes of resident batches: ops.sc_decode /
    scl_decode with `out` -- and for SCL `workspace` -- given, so nothing is allocated) captured
    once into a HIP graph and replayed as one submission.  Small batches are launch-bound: at
    (128,256) x 4096 a decode is ~7.5 us per launch issued one by one and ~6.5 us per launch
    replayed (profiles/r05i_graph_time.txt; an empty kernel: ~3 us vs ~1.7 us).  The graph
    holds the buffers' addresses: refill the same tensors in place between replays.  The graph
    also keeps fn -- and with it the plan, tensors and workspace its closure holds -- alive for as
    long as it exists: a plan destroyed under a captured graph would unload the code object its
    kernel launches come from, and freed tensors would be replayed into."""

    def __init__(self, fn, launches, device=None):
        if launches < 1:
            raise ValueError("launches must be >= 1")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.launches = int(launches)
        self.fn = fn  # keep-alive of everything the captured launches point at (see above)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # one eager call first: plans load their code object lazily
            fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.device(dev), torch.cuda.graph(self.graph):
            for _ in range(self.launches):
                fn()

    def replay(self):
        self.graph.replay()


def shader_clock_ghz(device=None, iters=16384):
    """The shader clock of one CU now (pl_clock_probe: one wave's dependent VALU chain timed by
    s_memtime against the 100 MHz s_memrealtime), in GHz, measured on the current stream of
    `device` -- so it runs right after whatever was queued before it.  Diagnostics for bench.py."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    ticks = torch.zeros(3, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pl_clock_probe(ctypes.c_void_p(ticks.data_ptr()), int(iters),
                                             _lib.current_stream_ptr(dev)), "pl_clock_probe")
    t = ticks.cpu()
    return 0.1 * float(t[0]) / max(float(t[1]), 1.0)
