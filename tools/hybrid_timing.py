"""Time the hybrid SC / SC-list decoder (ops.hybrid_decode) against pure CRC-aided SCL
(ops.scl_decode with the CRC plan) on the same tensor: (512,1024), CRC24C, L = 8, bs 8192, with
the min-sum plans and with the my_sn exact-f pair, at three noise levels.

  python tools/hybrid_timing.py [--bs 8192 --reps 25 --out FILE]

Per level it prints the SC pass fraction, n_list, and the medians of `reps` launches timed one by
one with HIP events (after a warm-up; the decoders alternate inside the timed loop): the hybrid
call, the pure list decode, and the pieces the hybrid time should add up to -- the SC launch, the
CRC flag launch, and the list decode of the n_list failing rows alone.  What is left,
hybrid - SC - CRC flag - SCL(n_list), is the compaction, the 8-byte read-back with its stream
synchronise, the gather, the scatter and the second CRC flag.

Every (pair, level) step is a child process under its own time limit; the first step that fails
ends the run (nothing more is started on a GPU after a fault or a hang).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, CRC, LIST = 512, 1024, "CRC24C", 8
PAIRS = ("minsum", "exact")
SIGMAS = (0.45, 0.50, 0.55)  # BPSK +-1 plus noise of this deviation, as LLRs 2 y / sigma^2
STEP_TIMEOUT_S = 240


def step(pair, sigma, bs, reps):
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd"), os.path.join(ROOT, "oracle")]
    import numpy as np
    import torch

    import oracle
    import polar_amd
    from polar_amd import _lib, ops
    from polar_amd.mysn import crc_params
    if not torch.cuda.is_available():
        raise SystemExit("hybrid_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    fp = polar_amd.reference_frozen_pos(K, N).numpy()
    mask = polar_amd.frozen_mask(fp, N)
    rng = np.random.default_rng(7)
    u = oracle.crc_encode(rng.integers(0, 2, (bs, K - crc_params(CRC)[0])).astype(np.float32), CRC)
    y = 2 * oracle.polar_encode(u, fp, N) - 1 + rng.standard_normal((bs, N)) * sigma
    llr = torch.from_numpy((y * 2 / sigma ** 2).astype(np.float32)).cuda()
    fm = _lib.PL_F_EXACT if pair == "exact" else _lib.PL_F_MINSUM
    sc = _lib.Plan(N, mask, 1, fm)
    scl = _lib.Plan(N, mask, LIST, fm, flags=_lib.PL_PLAN_FAST_SCL)
    scl.set_crc(*crc_params(CRC))
    out_h = torch.empty((bs, K), device="cuda")
    out_l = torch.empty((bs, K), device="cuda")
    out_s = torch.empty((bs, K), device="cuda")
    ws = ops.scl_workspace(scl, bs, llr.device)
    _, ok, rows, n_list = ops.hybrid_decode(sc, scl, llr, out=out_h, return_info=True)
    ok_sc = ops.crc_status(scl, ops.sc_decode(sc, llr, out=out_s))
    sub = llr[rows.long()].contiguous() if n_list else None
    out_r = torch.empty((max(n_list, 1), K), device="cuda")
    ws_r = ops.scl_workspace(scl, max(n_list, 1), llr.device)
    fns = {"hybrid_ms": lambda: ops.hybrid_decode(sc, scl, llr, out=out_h),
           "scl_ms": lambda: ops.scl_decode(scl, llr, out=out_l, workspace=ws),
           "sc_ms": lambda: ops.sc_decode(sc, llr, out=out_s),
           "crc_flag_ms": lambda: ops.crc_status(scl, out_s),
           "scl_rows_ms": (lambda: ops.scl_decode(scl, sub, out=out_r, workspace=ws_r)) if n_list else None}
    times = {name: [] for name, fn in fns.items() if fn}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(-5, reps):  # five warm-up rounds, then the timed ones; the decoders alternate
        for name, fn in fns.items():
            if fn is None:
                continue
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append(e0.elapsed_time(e1))
    res = {"pair": pair, "sigma": sigma, "bs": bs, "reps": reps, "sc_pass": round(float(ok_sc.float().mean()), 4),
           "out_crc_ok": round(float(ok.float().mean()), 4), "n_list": n_list,
           "kernels": [sc.kernel()[0], scl.kernel()[0]]}
    for name, t in times.items():
        res[name] = round(statistics.median(t), 4)
    res["rest_ms"] = round(res["hybrid_ms"] - res["sc_ms"] - res["crc_flag_ms"] - res.get("scl_rows_ms", 0.0), 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--step", nargs=2, metavar=("PAIR", "SIGMA"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    if a.step:
        return step(a.step[0], float(a.step[1]), a.bs, a.reps)
    lines = []
    print(f"{'pair':7s} {'sigma':>5s} {'SC pass':>8s} {'n_list':>6s} {'hybrid':>9s} {'pure SCL':>9s} {'SC':>8s} "
          f"{'CRC flag':>8s} {'SCL(n_list)':>11s} {'rest':>8s}   (ms, medians of {a.reps})", flush=True)
    for pair in PAIRS:
        for sigma in SIGMAS:
            cmd = [sys.executable, os.path.abspath(__file__), "--bs", str(a.bs), "--reps", str(a.reps),
                   "--step", pair, str(sigma)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"step {pair} sigma={sigma}: no result after {STEP_TIMEOUT_S} s; stopping")
            if r.returncode != 0:
                raise SystemExit(f"step {pair} sigma={sigma} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}")
            d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            lines.append(d)
            print(f"{d['pair']:7s} {d['sigma']:5.2f} {d['sc_pass']:8.4f} {d['n_list']:6d} {d['hybrid_ms']:9.4f} "
                  f"{d['scl_ms']:9.4f} {d['sc_ms']:8.4f} {d['crc_flag_ms']:8.4f} {d.get('scl_rows_ms', 0.0):11.4f} "
                  f"{d['rest_ms']:8.4f}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
