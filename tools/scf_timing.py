"""Time the CRC-aided SC-Flip decoder (ops.scf_decode) next to SC, the hybrid SC / SC-list decoder and pure
CRC-aided SCL (L = 8) on the same 8192 rows, and record what each decodes:

  5g      the (500,1024) 5G NR uplink code, CRC11: the mother-code logits of the fused producer
          (channel.FusedAWGN5G), mother code (511 + CRC in n = 1024)
  plain   the reference (128,256) code whose last 24 information bits are a CRC24C, BPSK over AWGN

for both f modes, at the three Eb/N0 (of a 0.25 dB grid) where the share of rows whose SC result fails the CRC
is nearest 0.5, 0.1 and 0.01.

  python tools/scf_timing.py [--bs 8192 --reps 25 --out profiles/scf_timing.jsonl]

Per (code, f, Eb/N0) one JSON line: the SC CRC-fail share; for SC, SC-Flip at T = 4 / 16 / 64, hybrid and SCL
the median of `reps` launches timed one by one with HIP events after 5 warm-up rounds (the decoders alternate
inside the timed loop), and the BLER over the information bits without the CRC; the mean `attempts` of each
SC-Flip run; the kernels the plans run; the shader clock read by pl_clock_probe right after the timed loop.

Every (code, f) step is a child process under its own time limit; the first step that fails ends the run
(nothing more is started on a GPU after a fault or a hang).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = ("5g", "plain")
FS = ("minsum", "exact")
FLIPS = (4, 16, 64)
TARGETS = (0.5, 0.1, 0.01)
LIST = 8
STEP_TIMEOUT_S = 420


def make_rows(code, bs, ebno_db, point):
    """(n, frozen mask, crc name, truth bits [bs, k - deg] on the GPU, logits [bs, n] on the GPU)"""
    import numpy as np
    import torch

    import oracle
    import polar_amd
    from polar_amd import channel
    from polar_amd.mysn import crc_params
    if code == "5g":
        from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            enc = Polar5GEncoder(500, 1024)
            dec = Polar5GDecoder(enc, dec_type="SC")
        model = channel.FusedAWGN5G(enc, dec, device="cuda", seed=7)
        bits, _, llr = model.llrs(bs, ebno_db, stream=(point, 0))
        n = enc.n_polar
        return n, polar_amd.frozen_mask(np.asarray(enc._frozen_pos), n), enc.enc_crc.crc_degree, bits, llr
    k, n, crc = 128, 256, "CRC24C"
    fp = polar_amd.reference_frozen_pos(k, n).numpy()
    rng = np.random.default_rng(7)
    msg = rng.integers(0, 2, (bs, k - crc_params(crc)[0])).astype(np.float32)
    u = oracle.crc_encode(msg, crc)
    sigma = float(np.sqrt(1.0 / (2.0 * (k / n) * 10.0 ** (ebno_db / 10.0))))
    y = 2 * oracle.polar_encode(u, fp, n) - 1 + rng.standard_normal((bs, n)) * sigma
    llr = torch.from_numpy((y * 2 / sigma ** 2).astype(np.float32)).cuda()
    return n, polar_amd.frozen_mask(fp, n), crc, torch.from_numpy(msg).cuda(), llr


def step(code, f, bs, reps):
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd"), os.path.join(ROOT, "oracle")]
    import torch

    from polar_amd import _lib, ops
    from polar_amd.mysn import crc_params
    if not torch.cuda.is_available():
        raise SystemExit("scf_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    fm = _lib.PL_F_EXACT if f == "exact" else _lib.PL_F_MINSUM
    n, mask, crc, _, _ = make_rows(code, 64, 3.0, 0)
    sc = _lib.Plan(n, mask, 1, fm)
    sc.set_crc(*crc_params(crc))
    scl = _lib.Plan(n, mask, LIST, fm, flags=_lib.PL_PLAN_FAST_SCL)
    scl.set_crc(*crc_params(crc))
    k_msg = sc.k - crc_params(crc)[0]
    # the Eb/N0 of a 0.25 dB grid whose SC CRC-fail share is nearest each target
    grid = [0.25 * i for i in range(0, 29)]
    share = {}
    for i, e in enumerate(grid):
        _, _, _, _, llr = make_rows(code, bs, e, i)
        share[e] = 1.0 - float(ops.crc_status(sc, ops.sc_decode(sc, llr)).float().mean())
    picks = [min(grid, key=lambda e: abs(share[e] - t)) for t in TARGETS]
    for target, ebno in zip(TARGETS, picks):
        _, _, _, truth, llr = make_rows(code, bs, ebno, grid.index(ebno))
        outs = {name: torch.empty((bs, sc.k), device="cuda") for name in ("sc", "hybrid", "scl", *[f"scf{t}" for t in FLIPS])}
        ws = ops.scl_workspace(scl, bs, llr.device)
        fns = {"sc": lambda: ops.sc_decode(sc, llr, out=outs["sc"]),
               "hybrid": lambda: ops.hybrid_decode(sc, scl, llr, out=outs["hybrid"]),
               "scl": lambda: ops.scl_decode(scl, llr, out=outs["scl"], workspace=ws)}
        for t in FLIPS:
            fns[f"scf{t}"] = (lambda t=t: ops.scf_decode(sc, llr, t, out=outs[f"scf{t}"]))
        times = {name: [] for name in fns}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(-5, reps):
            for name, fn in fns.items():
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 0:
                    times[name].append(e0.elapsed_time(e1))
        clock = ops.shader_clock_ghz(llr.device)
        res = {"code": code, "f": f, "n": n, "k": sc.k, "crc": crc, "bs": bs, "reps": reps, "ebno_db": ebno,
               "target_fail": target, "sc_crc_fail": round(share[ebno], 4), "clock_ghz": round(clock, 3),
               "kernels": [sc.kernel()[0], scl.kernel()[0]]}
        for name in fns:
            res[name + "_ms"] = round(statistics.median(times[name]), 4)
            res[name + "_bler"] = round(float((outs[name][:, :k_msg] != truth).any(dim=1).float().mean()), 5)
        for t in FLIPS:
            _, _, _, att = ops.scf_decode(sc, llr, t, return_info=True)
            res[f"scf{t}_attempts"] = round(float(att.float().mean()), 3)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--step", nargs=2, metavar=("CODE", "F"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    if a.step:
        return step(a.step[0], a.step[1], a.bs, a.reps)
    lines = []
    for code in CODES:
        for f in FS:
            cmd = [sys.executable, os.path.abspath(__file__), "--bs", str(a.bs), "--reps", str(a.reps), "--step", code, f]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"step {code} {f}: no result after {STEP_TIMEOUT_S} s; stopping")
            if r.returncode != 0:
                raise SystemExit(f"step {code} {f} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}")
            for ln in r.stdout.splitlines():
                if ln.startswith("{"):
                    d = json.loads(ln)
                    lines.append(d)
                    print(f"{code:5s} {f:6s} {d['ebno_db']:5.2f} dB fail {d['sc_crc_fail']:.4f} | ms: SC {d['sc_ms']:.3f} "
                          f"SCF4 {d['scf4_ms']:.3f} SCF16 {d['scf16_ms']:.3f} SCF64 {d['scf64_ms']:.3f} hybrid "
                          f"{d['hybrid_ms']:.3f} SCL {d['scl_ms']:.3f} | BLER: SC {d['sc_bler']:.4f} SCF4 "
                          f"{d['scf4_bler']:.4f} SCF16 {d['scf16_bler']:.4f} SCF64 {d['scf64_bler']:.4f} hybrid "
                          f"{d['hybrid_bler']:.4f} SCL {d['scl_bler']:.4f} | attempts {d['scf4_attempts']} "
                          f"{d['scf16_attempts']} {d['scf64_attempts']} | {d['clock_ghz']} GHz", flush=True)
            if a.out:  # after every step: a later failure keeps what was measured
                with open(a.out, "w") as fo:
                    for d in lines:
                        fo.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
