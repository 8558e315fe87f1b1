"""BER/BLER simulation driver with the flags of x_run_sn_polar/main.py + config.py.

    python -m polar_amd.cli --k 32 --n 64 --algos [scl] --bs 100 --mc_iter 1
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m polar_amd.cli \\
        --k 512 --n 1024 --bs 65536 --mc_iter 10 --snr_end 4.5
    python -m polar_amd.cli --code 5g --k 500 --n 1024 --algos [scl] --hybrid_sc --bs 8192 --mc_iter 10

Reference: main.py:32-76 (gen_code, seed 42 per code, SNR grid arange(0, snr_end, 0.5), SC always,
SCL when 'scl' in algos, PlotBER.simulate with target_block_errs=1000) and config.py:5-26.
--llr_device cpu reproduces the reference run bit for bit (LLRs generated on the CPU with the
reference's RNG call order, decoded on the GPU); the default generates LLRs on the GPU.  With
several ranks (torchrun, one per GPU) every rank simulates --bs codewords per iteration with its
own RNG stream (seed 42 + rank) and the error counters are summed with one RCCL all_reduce.
--code 5g simulates the rate-matched, CRC-aided 5G NR uplink code (Polar5GEncoder / Polar5GDecoder
with --k, --n as k_target, n_target; no counterpart in main.py): the SC leg is dec_type="SC", the
scl leg dec_type="SCL" with --list_size (and --hybrid_sc), the LLRs from the fused 5G producer
(channel.FusedAWGN5G) or, with --llr_producer ops, from the op-by-op chain (System5G_AWGN_model).
--num_bits_per_symbol 4 / 6 / 8 runs either code over 16-, 64- or 256-QAM (main.py fixes QPSK).
'osd' in --algos adds the ordered-statistics decoder of order --osd_t (OSDecoder, my_sn/fec/osd/dec.py), the
estimate of the maximum-likelihood curve: its BLER is comparable with SC / SCL (the encoder is injective), its
BER counts codeword bits.
'bp' in --algos adds the belief-propagation decoder (BP_Dec, pl_bp_decode): --bp_iter iterations of --bp_f
(exact or minsum, the latter scaled by --bp_scale), --bp_early_stop ends a row once its decisions re-encode.
'scan' in --algos adds the soft-cancellation decoder (SCAN_Dec, pl_scan_decode): --scan_iter iterations (default 2)
of --scan_f (exact or minsum); --code plain, n <= 2048.
'pac' in --algos adds the PAC code on the same rate profile (PACEncoder + PAC_Dec, pl_pac_encode / pl_pac_decode):
the convolutional precoder --pac_conv (octal, default 133) in front of the polar transform, list-decoded with
--pac_list paths (default 32); --code plain, n <= 1024; the leg runs the op-by-op model (System_AWGN_model), as its
codewords are not the plain code's.  With 'osd' also in --algos a second OSD leg, "OSD-t of the PAC code", decodes
the PAC code's own generator matrix: the maximum-likelihood yardstick of that code.
'scf' in --algos adds the CRC-aided SC-Flip decoder (SCF_Dec, pl_scf_decode) with --scf_flips candidate
positions a row and the f of --scf_f; it needs --code 5g, the only code here with a CRC.
'ae' in --algos adds the automorphism-ensemble SC decoder (AE_Dec, pl_ae_decode): --ae_perms permuted SC
decodes a row through bit-index (--ae_kind stage) or GL(m, 2) (--ae_kind linear) automorphisms of the code,
with the f of --ae_f.  It pays on the Reed-Muller sets (k a sum of binomials, e.g. --k 64 --n 128); a frozen
set that admits fewer than --ae_perms such permutations is an argument error.
'scq' in --algos adds the fixed-point SC decoder (SCQ_Dec, pl_llr_quantize + pl_scq_decode): channel LLRs of
--scq_qc bits with the largest level at --scq_llr_max, internal LLRs of --scq_qi bits; --code plain only.
'--code dci simulates the 5G NR downlink chain (polar_amd.dci: DCIEncoder / DCIDecoder with --k, --n as payload and
code bits, k <= 140, 25 <= n <= 576): CRC24C with the ones prefix and --dci_rnti, the input-bit interleaver (off
with --dci_tail_crc), downlink rate matching, decoded by the parity-constrained list decoder (pl_pcl_decode) with
--dci_n_force of the parity bits as FORCE constraints.  The SC leg is list size 1, the scl leg --list_size; a row
without a surviving path counts as a block error.  The legs run the op-by-op model (System_AWGN_model): the fused
producer is uplink-only.
"""
import argparse
import math
import os
import random

import numpy as np
import torch as tc


def _list_arg(s):
    s = s.strip()
    if s.startswith("[") and s.endswith("]"):
        s = s[1:-1]
    return [x.strip().strip("'\"") for x in s.split(",") if x.strip()]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--algos", type=_list_arg, default=["scl"])
    ap.add_argument("--kern", default="F2")
    ap.add_argument("--verbose", type=lambda s: s.lower() in ("1", "true", "yes"), default=False)
    ap.add_argument("--bs", type=int, default=3)
    ap.add_argument("--snr_end", type=float, default=5)
    ap.add_argument("--mc_iter", type=int, default=10)
    ap.add_argument("--list_size", type=int, default=8)
    ap.add_argument("--mode", default="max")
    ap.add_argument("--spec", default=False)
    ap.add_argument("--llr_device", choices=["cuda", "cpu"], default="cuda")
    ap.add_argument("--llr_producer", choices=["fused", "ops"], default="fused",
                    help="cuda LLRs: one fused HIP kernel (Philox; default) or the op-by-op torch port")
    ap.add_argument("--num_bits_per_symbol", type=int, choices=[2, 4, 6, 8], default=2,
                    help="modulation: QPSK (default; main.py's), 16-, 64- or 256-QAM; must divide --n")
    ap.add_argument("--target_block_errs", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--plot", default=None, help="save the BLER plot here (matplotlib)")
    ap.add_argument("--code", choices=["plain", "5g", "dci"], default="plain",
                    help="plain: the (k, n) polar code of main.py; 5g: the 5G NR uplink code with --k, --n as "
                         "k_target, n_target (CRC, rate matching); dci: the 5G NR downlink chain (distributed CRC24C)")
    ap.add_argument("--dci_rnti", type=lambda v: int(v, 0), default=0, help="--code dci: the 16-bit RNTI (e.g. 0xBEEF)")
    ap.add_argument("--dci_n_force", type=int, default=0,
                    help="--code dci: the first parity bits in decoding order that are FORCE constraints, 0 ... 24")
    ap.add_argument("--dci_tail_crc", action="store_true",
                    help="--code dci: no input-bit interleaver, all 24 parity bits at the tail")
    ap.add_argument("--hybrid_sc", action="store_true",
                    help="--code 5g, scl leg: SC first, the list decoder only on rows whose CRC fails")
    ap.add_argument("--frozen", choices=["reference", "recompute", "design"], default="reference",
                    help="reference: the pinned sets froze.py produced; recompute: re-run froze.py's recipe; design: "
                         "genie-aided Monte-Carlo SC construction at --design_ebno (polar_amd.design; --code plain, GPU)")
    ap.add_argument("--design_ebno", type=float, default=None, help="--frozen design: the Eb/N0 (dB) to design for")
    ap.add_argument("--design_rows", type=int, default=2 ** 20, help="--frozen design: codewords of the design run")
    ap.add_argument("--osd_t", type=int, default=2,
                    help="order of the OSD leg ('osd' in --algos): 0 <= t <= min(k, 4), at most 2^22 patterns")
    ap.add_argument("--bp_iter", type=int, default=20, help="iterations of the BP leg ('bp' in --algos)")
    ap.add_argument("--bp_f", choices=["exact", "minsum"], default="exact", help="f of the BP leg")
    ap.add_argument("--bp_scale", type=float, default=1.0, help="BP leg, --bp_f minsum: the magnitude scale in (0, 1]")
    ap.add_argument("--bp_early_stop", action="store_true",
                    help="BP leg: a row stops once its hard decisions re-encode to those on the code bits")
    ap.add_argument("--scan_iter", type=int, default=2, help="iterations of the SCAN leg ('scan' in --algos)")
    ap.add_argument("--scan_f", choices=["exact", "minsum"], default="exact", help="f of the SCAN leg")
    ap.add_argument("--pac_list", type=int, default=32, help="list size of the PAC leg ('pac' in --algos): 1, 2, ... 32")
    ap.add_argument("--pac_conv", default="133", help="PAC leg: the precoder's generator in octal (c_0 first)")
    ap.add_argument("--scf_flips", type=int, default=16,
                    help="SC-Flip leg ('scf' in --algos): candidate positions a row, 0 ... 64")
    ap.add_argument("--scf_f", choices=["exact", "minsum"], default="exact", help="f of the SC-Flip leg")
    ap.add_argument("--ae_perms", type=int, default=8,
                    help="automorphism-ensemble leg ('ae' in --algos): permuted SC decodes a row, 1 ... 64")
    ap.add_argument("--ae_kind", choices=["stage", "linear"], default="stage",
                    help="automorphism-ensemble leg: bit-index permutations or GL(m, 2) maps")
    ap.add_argument("--ae_f", choices=["minsum", "exact"], default="minsum", help="f of the automorphism-ensemble leg")
    ap.add_argument("--scq_qc", type=int, default=6, help="fixed-point SC leg ('scq' in --algos): channel LLR bits, 2 ... 8")
    ap.add_argument("--scq_qi", type=int, default=6,
                    help="fixed-point SC leg: internal LLR bits, --scq_qc ... 8")
    ap.add_argument("--scq_llr_max", type=float, default=30.0,
                    help="fixed-point SC leg: the logit magnitude of the largest channel level")
    c = ap.parse_args(argv)
    c._error = ap.error
    if c.code == "dci":
        extra = [a for a in c.algos if a != "scl"]
        if extra:
            ap.error(f"--code dci has an SC and an scl leg only, got {extra} in --algos")
        if not 1 <= c.k <= 140 or not 25 <= c.n <= 576 or c.k + 24 > c.n:
            ap.error("--code dci needs 1 <= --k <= 140, 25 <= --n <= 576 and k + 24 <= n")
        if not 0 <= c.dci_rnti < 1 << 16:
            ap.error("--dci_rnti must be a 16-bit value")
        if not 0 <= c.dci_n_force <= 24:
            ap.error("--dci_n_force must be in [0, 24]")
        if c.list_size < 1 or c.list_size > 32 or c.list_size & (c.list_size - 1):
            ap.error("--code dci: --list_size must be a power of two in [1, 32]")
        if c.llr_device != "cuda":
            ap.error("--code dci runs on the GPU (--llr_device cuda)")
    if "ae" in c.algos:
        from .ae import AE_MAX_N, AE_MAX_PERMS
        if c.code != "plain":
            ap.error("'ae' in --algos needs --code plain")
        if c.n > AE_MAX_N:
            ap.error(f"'ae' in --algos needs --n <= {AE_MAX_N}")
        if not 1 <= c.ae_perms <= AE_MAX_PERMS:
            ap.error(f"--ae_perms must be in [1, {AE_MAX_PERMS}]")
    if "scq" in c.algos:
        if c.code != "plain":
            ap.error("'scq' in --algos needs --code plain")
        if not 2 <= c.scq_qc <= c.scq_qi <= 8:
            ap.error("--scq_qc and --scq_qi must satisfy 2 <= scq_qc <= scq_qi <= 8")
        if not (c.scq_llr_max > 0.0 and math.isfinite(c.scq_llr_max)):
            ap.error("--scq_llr_max must be positive and finite")
    if "scf" in c.algos:
        from .scf import SCF_MAX_FLIPS
        if c.code != "5g":
            ap.error("'scf' in --algos needs --code 5g (the SC-Flip decoder needs the CRC)")
        if not 0 <= c.scf_flips <= SCF_MAX_FLIPS:
            ap.error(f"--scf_flips must be in [0, {SCF_MAX_FLIPS}]")
    if "bp" in c.algos:
        from .bp import BP_MAX_N
        if c.code != "plain":
            ap.error("'bp' in --algos needs --code plain")
        if c.n > BP_MAX_N:
            ap.error(f"'bp' in --algos needs --n <= {BP_MAX_N}")
        if c.bp_iter < 1:
            ap.error("--bp_iter must be >= 1")
        if not 0.0 < c.bp_scale <= 1.0 or (c.bp_f == "exact" and c.bp_scale != 1.0):
            ap.error("--bp_scale must be in (0, 1], and 1 with --bp_f exact")
    if "scan" in c.algos:
        from .scan import SCAN_MAX_N
        if c.code != "plain":
            ap.error("'scan' in --algos needs --code plain")
        if c.n > SCAN_MAX_N:
            ap.error(f"'scan' in --algos needs --n <= {SCAN_MAX_N}")
        if c.scan_iter < 1:
            ap.error("--scan_iter must be >= 1")
    if "pac" in c.algos:
        from .pac import PAC_MAX_LIST, PAC_MAX_N, conv_from_octal, conv_to_mask
        if c.code != "plain":
            ap.error("'pac' in --algos needs --code plain")
        if c.n > PAC_MAX_N:
            ap.error(f"'pac' in --algos needs --n <= {PAC_MAX_N}")
        if not 1 <= c.pac_list <= PAC_MAX_LIST or c.pac_list & (c.pac_list - 1):
            ap.error(f"--pac_list must be a power of two in [1, {PAC_MAX_LIST}]")
        try:
            conv_to_mask(conv_from_octal(c.pac_conv))
        except ValueError as e:
            ap.error(f"--pac_conv: {e}")
    if "osd" in c.algos:
        from .osd import check_supported
        if c.code != "plain":
            ap.error("'osd' in --algos needs --code plain")
        try:
            check_supported(c.k, c.n, c.osd_t)
        except ValueError as e:
            ap.error(str(e))
    if c.frozen == "design":
        if c.design_ebno is None:
            ap.error("--frozen design needs --design_ebno")
        if c.code != "plain":
            ap.error("--frozen design needs --code plain")
        if c.llr_device != "cuda":
            ap.error("--frozen design runs on the GPU (--llr_device cuda)")
        if c.design_rows < 1:
            ap.error("--design_rows must be >= 1")
    return c


def designed_frozen_pos(c, device):
    """--frozen design: the set designed once per run (kept on the parsed arguments), so every leg
    decodes the same code; returns (frozen_pos, hash, union bound estimate)."""
    if getattr(c, "_designed", None) is None:
        import hashlib
        from . import design
        counts, rows = design.bit_channel_errors(c.n, c.k, c.design_ebno, c.design_rows,
                                                 num_bits_per_symbol=getattr(c, "num_bits_per_symbol", 2),
                                                 seed=c.seed, device=device)
        fp = design.select_frozen(counts, c.k)
        digest = hashlib.sha256(fp.numpy().astype("<i8").tobytes()).hexdigest()[:16]
        c._designed = (fp, digest, design.union_bound(counts, rows, fp))
    return c._designed


def set_seed(seed):  # main.py:24-29
    np.random.seed(seed)
    random.seed(seed)
    tc.manual_seed(seed)


def gen_code_5g(c, name, mode, device, generator=None):
    """[model, name] of the 5G NR uplink code (k_target, n_target) = (--k, --n) on a GPU."""
    from . import channel
    from .polar5g import Polar5GDecoder, Polar5GEncoder
    if device.type != "cuda":
        raise ValueError("--code 5g runs on the GPU (--llr_device cuda)")
    enc = Polar5GEncoder(c.k, c.n)
    m = getattr(c, "num_bits_per_symbol", 2)
    if mode == "sc":
        dec = Polar5GDecoder(enc, dec_type="SC")
    elif mode == "scl":
        dec = Polar5GDecoder(enc, dec_type="SCL", list_size=c.list_size, hybrid_sc=c.hybrid_sc)
    elif mode == "scf":
        dec = Polar5GDecoder(enc, dec_type="SCF", list_size=c.scf_flips, scf_f=c.scf_f)
    else:
        raise Exception('error...')
    if c.llr_producer == "fused":
        rank = int(os.environ.get("RANK", "0"))  # rank r draws stream rows [r*bs, (r+1)*bs)
        model = channel.FusedAWGN5G(enc, dec, device=device, seed=c.seed, row0=rank * c.bs, num_bits_per_symbol=m)
    else:
        model = channel.System5G_AWGN_model(enc, dec, device=device, generator=generator, num_bits_per_symbol=m)
    return [model, name]


def gen_code_dci(c, name, mode, device, generator=None):
    """[model, name] of the 5G NR downlink chain (payload, code bits) = (--k, --n) on a GPU, op by op."""
    from . import channel
    from .dci import DCIDecoder, DCIEncoder
    if device.type != "cuda":
        raise ValueError("--code dci runs on the GPU (--llr_device cuda)")
    enc = DCIEncoder(c.k, c.n, rnti=c.dci_rnti, interleave=not c.dci_tail_crc, device=str(device))
    dec = DCIDecoder(enc, list_size=1 if mode == "sc" else c.list_size, n_force=c.dci_n_force)
    model = channel.System_AWGN_model(c.n, c.k, enc, dec, device=device, generator=generator,
                                      num_bits_per_symbol=getattr(c, "num_bits_per_symbol", 2))
    return [model, name]


def gen_code(c, name, mode, device, generator=None):  # main.py:32-41
    from . import channel, frozen
    from .decoders import SC_Dec, SCL_Dec
    if getattr(c, "code", "plain") == "5g":
        return gen_code_5g(c, name, mode, device, generator)
    if getattr(c, "code", "plain") == "dci":
        return gen_code_dci(c, name, mode, device, generator)
    assert math.log(c.n, 2).is_integer()
    G, _, fp = frozen.get_Kern_frozen_bits(c.n, c.n - c.k, frozen.F2)
    if c.frozen == "reference":
        try:
            fp = frozen.reference_frozen_pos(c.k, c.n)
        except KeyError:
            pass
    elif c.frozen == "design":
        fp, digest, ub = designed_frozen_pos(c, device)
        if int(os.environ.get("RANK", "0")) == 0:
            print(f"{name}: frozen set designed at {c.design_ebno} dB over {c.design_rows} rows, hash {digest}, "
                  f"union bound {ub:.3e}")
    if device.type == "cuda":
        enc = channel.GpuEncoder(fp, c.n)
    else:
        enc = channel.DenseEncoder(fp, c.n, G, device=device)
    dev_str = str(device) if device.type == "cuda" else "cpu"
    if mode in ("pac", "osd_pac"):  # the PAC code on this rate profile: its own encoder, the op-by-op model
        from .pac import PAC_Dec, PACEncoder, conv_from_octal
        conv = conv_from_octal(c.pac_conv)
        enc = PACEncoder(fp, c.n, conv, device=dev_str)
    if mode == "sc":
        dec = SC_Dec(fp, c.n, device=dev_str)
    elif mode == "scl":
        dec = SCL_Dec(fp, c.n, c.list_size, device=dev_str)
    elif mode in ("osd", "osd_pac"):  # decides codewords: the model compares them with the transmitted ones
        from .osd import OSDecoder
        dec = OSDecoder(c.osd_t, enc, device=dev_str)
    elif mode == "pac":
        dec = PAC_Dec(fp, c.n, list_size=c.pac_list, conv=conv, device=dev_str)
    elif mode == "bp":
        from .bp import BP_Dec
        dec = BP_Dec(fp, c.n, num_iter=c.bp_iter, device=dev_str, f=c.bp_f, scale=c.bp_scale,
                     early_stop=c.bp_early_stop)
    elif mode == "scan":
        from .scan import SCAN_Dec
        dec = SCAN_Dec(fp, c.n, num_iter=c.scan_iter, device=dev_str, f=c.scan_f)
    elif mode == "ae":
        from .ae import AE_Dec
        try:  # the frozen set is known only here (--frozen design makes it on the GPU)
            dec = AE_Dec(fp, c.n, num_perms=c.ae_perms, kind=c.ae_kind, seed=c.seed, f=c.ae_f, device=dev_str)
        except ValueError as e:
            c._error(f"'ae' in --algos: {e}")
    elif mode == "scq":
        from .quant import SCQ_Dec
        dec = SCQ_Dec(fp, c.n, q_channel=c.scq_qc, q_internal=c.scq_qi, llr_max=c.scq_llr_max, device=dev_str)
    else:
        raise Exception('error...')
    cw = mode in ("osd", "osd_pac")
    if device.type == "cuda" and getattr(c, "llr_producer", "fused") == "fused" and mode not in ("pac", "osd_pac"):
        # one HIP launch for bits/encoder/mapper/channel/demapper; rank r draws stream rows
        # [r*bs, (r+1)*bs) of the seed's stream
        rank = int(os.environ.get("RANK", "0"))
        model = channel.FusedAWGN(c.n, c.k, fp, dec, device=device, seed=c.seed, row0=rank * c.bs, cw_estimates=cw,
                                  num_bits_per_symbol=getattr(c, "num_bits_per_symbol", 2))
    else:
        model = channel.System_AWGN_model(c.n, c.k, enc, dec, cw_estimates=cw, device=device, generator=generator,
                                          num_bits_per_symbol=getattr(c, "num_bits_per_symbol", 2))
    return [model, name]


def main(argv=None):
    from .sim import PlotBER
    c = parse(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    pg = None
    if tc.cuda.is_available():
        # one GPU per rank whichever backend carries the counters: the decoders run on the
        # current device when the LLRs are produced on the CPU (gloo path)
        tc.cuda.set_device(local % tc.cuda.device_count())
    if world > 1:
        import torch.distributed as dist
        if c.llr_device == "cuda":
            dist.init_process_group("nccl", device_id=tc.device("cuda", local))
        else:
            dist.init_process_group("gloo")
        pg = dist.group.WORLD
    device = tc.device("cuda", local) if c.llr_device == "cuda" else tc.device("cpu")
    gen = tc.Generator(device=device).manual_seed(c.seed + rank) if device.type == "cuda" else None
    ebno_db = np.arange(0, c.snr_end, 0.5)
    codes = [gen_code(c, "SC", "sc", device, gen)]
    if "scl" in c.algos:
        codes.append(gen_code(c, f"SCL-{c.list_size}", "scl", device, gen))
    if "osd" in c.algos:
        codes.append(gen_code(c, f"OSD-{c.osd_t} (codeword BER)", "osd", device, gen))
    if "bp" in c.algos:
        codes.append(gen_code(c, f"BP-{c.bp_iter} ({c.bp_f})", "bp", device, gen))
    if "scan" in c.algos:
        codes.append(gen_code(c, f"SCAN-{c.scan_iter} ({c.scan_f})", "scan", device, gen))
    if "pac" in c.algos:
        codes.append(gen_code(c, f"PAC-{c.pac_list} (conv {c.pac_conv})", "pac", device, gen))
        if "osd" in c.algos:
            codes.append(gen_code(c, f"OSD-{c.osd_t} of the PAC code (codeword BER)", "osd_pac", device, gen))
    if "scf" in c.algos:
        codes.append(gen_code(c, f"SCF-{c.scf_flips} ({c.scf_f})", "scf", device, gen))
    if "ae" in c.algos:
        codes.append(gen_code(c, f"AE-{c.ae_perms} ({c.ae_kind}, {c.ae_f})", "ae", device, gen))
    if "scq" in c.algos:
        codes.append(gen_code(c, f"SCQ ({c.scq_qc},{c.scq_qi})", "scq", device, gen))
    plot = PlotBER(f"Performance of Short Len Codes (k={c.k}, n={c.n})")
    results = {}
    for model, name in codes:
        if rank == 0:
            print("\nRunning: " + name)
        set_seed(c.seed + rank)
        if gen is not None:
            gen.manual_seed(c.seed + rank)
        counter_dev = device if device.type == "cuda" else "cpu"
        ber, bler = plot.simulate(model, ebno_dbs=ebno_db, batch_size=c.bs, target_block_errs=c.target_block_errs,
                                  legend=name, soft_estimates=False, max_mc_iter=c.mc_iter, add_bler=True,
                                  device=counter_dev, process_group=pg)
        results[name] = (ber.numpy(), bler.numpy())
    if rank == 0 and c.plot:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        plt.figure(figsize=(16, 12))
        for i, leg in enumerate(plot.legend):
            if "BLER" in leg:
                plt.semilogy(ebno_db, plot.ber[i], c='C%d' % i, label=leg, linewidth=2,
                             linestyle='--' if "SC" in leg and "SCL" not in leg else '-')
        plt.grid(which="both")
        plt.xlabel(r"$E_b/N_0$ (dB)")
        plt.ylabel("BLER")
        plt.legend()
        plt.savefig(c.plot)
    if pg is not None:
        import torch.distributed as dist
        dist.destroy_process_group()
    return results


if __name__ == "__main__":
    main()
