"""Time the fixed-point SC decoder (pl_scq_decode) and its quantiser (pl_llr_quantize) next to the float SC kernels,
and tabulate the BLER that the LLR widths cost:

  time    (128,256) and (512,1024) at 8192 and 65536 rows, in one process per shape: pl_scq_decode on int8 rows,
          pl_llr_quantize, the two back to back, pl_sc_decode on the generic kernel (PL_PLAN_GENERIC) and on the
          specialised kernel.  The five alternate inside the timed loop; every call of a kind takes the next of
          enough rotating input buffers that their footprint exceeds 512 MB (twice the Infinity Cache), so each
          launch streams its rows from HBM.  Per kind: the median of `reps` launches timed one by one with HIP
          events after 5 warm-up rounds, the algorithmic bytes per codeword (rows in, fp32 bits out) and their share
          of the HBM peak at that median.  The shader clock is read by pl_clock_probe before and after the loop.
  bler    (512,1024) on the pinned RM-weight set, the rows of the fused producer (channel.FusedAWGN), at the three
          Eb/N0 (the first, middle and last of a 0.25 dB grid) where float min-sum SC's BLER lies between 1e-1
          and 1e-3: float min-sum SC against (q_channel, q_internal) in {(4,4), (5,6), (6,6), (6,8)} at
          llr_max = 30 on the same rows.

  python tools/scq_timing.py [--reps 25 --out profiles/scq_timing.jsonl]

One JSON line per (shape, rows) and one per Eb/N0.  Every step is a child process under its own time limit; the
first step that fails ends the run (nothing more is started on a GPU after a fault or a hang).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((128, 256), (512, 1024))
ROWS = (8192, 65536)
WIDTHS = ((4, 4), (5, 6), (6, 6), (6, 8))
BLER_WINDOW = (1.5e-3, 8e-2)  # of the coarse pass (131072 rows a point): inside [1e-3, 1e-1] with a margin
BLER_ROWS = 1 << 20
LLR_MAX = 30.0
HBM_PEAK_GBS = 8000.0  # MI355X chip-level peak (bench.py's figure)
FOOTPRINT = 512 << 20
STEP_TIMEOUT_S = 420


def _setup():
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd"), os.path.join(ROOT, "oracle")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scq_timing needs a ROCm GPU (a time taken elsewhere says nothing)")


def step_time(k, n, bs, reps):
    _setup()
    import numpy as np
    import torch

    import polar_amd
    from polar_amd import _lib, ops
    mask = polar_amd.frozen_mask(polar_amd.reference_frozen_pos(k, n).numpy(), n)
    gen_plan = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
    spec_plan = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM)
    qc, qi = 6, 6
    inv_step = float(np.float32(((1 << (qc - 1)) - 1) / LLR_MAX))
    nf = -(-FOOTPRINT // (bs * n * 4))  # float buffers
    nq = -(-FOOTPRINT // (bs * n))      # int8 buffers
    g = torch.Generator(device="cuda").manual_seed(1)
    fl = [torch.randn((bs, n), device="cuda", generator=g) * 8.0 for _ in range(nf)]
    qs = [ops.llr_quantize(fl[i % nf].roll(i // nf, 0), inv_step, qc) for i in range(nq)]
    qout = torch.empty((bs, n), dtype=torch.int8, device="cuda")
    out = torch.empty((bs, k), device="cuda")
    turn = {"f": 0, "q": 0}

    def nxt(kind, pool):
        turn[kind] += 1
        return pool[turn[kind] % len(pool)]

    def both():
        ops.llr_quantize(nxt("f", fl), inv_step, qc, out=qout)
        ops.scq_decode(gen_plan, qout, qi, out=out)
    fns = {"scq": lambda: ops.scq_decode(gen_plan, nxt("q", qs), qi, out=out),
           "quantize": lambda: ops.llr_quantize(nxt("f", fl), inv_step, qc, out=qout),
           "quantize_scq": both,
           "sc_generic": lambda: ops.sc_decode(gen_plan, nxt("f", fl), out=out),
           "sc_specialized": lambda: ops.sc_decode(spec_plan, nxt("f", fl), out=out)}
    # bytes per codeword the algorithm needs: the rows in, what it writes out
    bytes_cw = {"scq": n + 4 * k, "quantize": 4 * n + n, "quantize_scq": 4 * n + n + n + 4 * k,
                "sc_generic": 4 * n + 4 * k, "sc_specialized": 4 * n + 4 * k}
    times = {name: [] for name in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    clock0 = None
    for rep in range(-5, reps):
        if rep == 0:
            clock0 = ops.shader_clock_ghz("cuda")
        for name, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append(e0.elapsed_time(e1))
    clock1 = ops.shader_clock_ghz("cuda")
    res = {"what": "time", "k": k, "n": n, "rows": bs, "reps": reps, "q_channel": qc, "q_internal": qi,
           "float_buffers": nf, "int8_buffers": nq, "clock_ghz": [round(clock0, 3), round(clock1, 3)],
           "kernels": {"sc_generic": gen_plan.kernel()[0], "sc_specialized": spec_plan.kernel()[0]}}
    for name in fns:
        ms = statistics.median(times[name])
        res[name] = {"ms": round(ms, 4), "min_ms": round(min(times[name]), 4), "mcw_s": round(bs / ms / 1e3, 1),
                     "bytes_per_cw": bytes_cw[name],
                     "hbm_share": round(bs * bytes_cw[name] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    print(json.dumps(res), flush=True)


def step_bler():
    _setup()
    import numpy as np
    import torch

    import polar_amd
    from polar_amd import _lib, channel, ops
    k, n, bs = 512, 1024, 65536
    fp = polar_amd.reference_frozen_pos(k, n)
    mask = polar_amd.frozen_mask(fp.numpy(), n)
    plan = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM)
    gen_plan = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
    model = channel.FusedAWGN(n, k, fp, polar_amd.SC_Dec(fp, n, device="cuda"), device="cuda", seed=11)

    def run(ebno, point, rows, widths):
        errs = {"float": 0, **{w: 0 for w in widths}}
        for it in range(rows // bs):
            bits, _, llr = model.llrs(bs, ebno, stream=(point, it))
            errs["float"] += int((ops.sc_decode(plan, llr) != bits).any(dim=1).sum())
            for qc, qi in widths:
                inv = float(np.float32(((1 << (qc - 1)) - 1) / LLR_MAX))
                got = ops.scq_decode(gen_plan, ops.llr_quantize(llr, inv, qc), qi)
                errs[(qc, qi)] += int((got != bits).any(dim=1).sum())
        return errs
    grid = [0.25 * i for i in range(12, 41)]  # 3 ... 10 dB: the RM-weight set needs about 5 dB at this length
    coarse = {e: run(e, i, 2 * bs, ())["float"] / (2 * bs) for i, e in enumerate(grid)}
    inside = [e for e in grid if BLER_WINDOW[0] <= coarse[e] <= BLER_WINDOW[1]]
    if len(inside) < 3:
        raise SystemExit(f"fewer than three grid points with float BLER in {BLER_WINDOW}: {coarse}")
    picks = [inside[0], inside[len(inside) // 2], inside[-1]]
    for e in picks:
        errs = run(e, 100 + grid.index(e), BLER_ROWS, WIDTHS)
        res = {"what": "bler", "k": k, "n": n, "rows": BLER_ROWS, "ebno_db": e, "llr_max": LLR_MAX,
               "in_window": bool(1e-3 <= errs["float"] / BLER_ROWS <= 1e-1),
               "float_minsum_bler": errs["float"] / BLER_ROWS, "float_block_errors": errs["float"]}
        for w in WIDTHS:
            res[f"q{w[0]}_{w[1]}_bler"] = errs[w] / BLER_ROWS
        print(json.dumps(res), flush=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    if a.step:
        if a.step[0] == "bler":
            return step_bler()
        return step_time(int(a.step[1]), int(a.step[2]), int(a.step[3]), a.reps)
    steps = [["time", str(k), str(n), str(bs)] for k, n in SHAPES for bs in ROWS] + [["bler"]]
    lines = []
    for st in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", *st]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {' '.join(st)}: no result after {STEP_TIMEOUT_S} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"step {' '.join(st)} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(json.loads(ln))
                print(ln, flush=True)
        if a.out:  # after every step: a later failure keeps what was measured
            with open(a.out, "w") as fo:
                for d in lines:
                    fo.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
