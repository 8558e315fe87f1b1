"""Time the belief-propagation decoder (ops.bp_decode, csrc/bp_kernel.hip) and count its block errors.

  python tools/bp_timing.py [--bs 8192 --reps 25 --out profiles/bp_timing.jsonl]

Timing: (128,256) and (512,1024), 8192 rows of the fused producer (ops.awgn_qpsk_llr) at EBNO_DB, 20
iterations, both f modes, early stop off and on (with it on, the mean of `iters` is in the record); SC
(the specialised kernel) and SCL L = 8 decode the same rows in the same process for scale.  Each record
is the median of `reps` launches timed one by one with HIP events after bench.py's warm-up pattern (100
ms of untimed launches so the clock leaves its idle state, then five more), with the shader clock right
before and after (pl_clock_probe) and the f evaluations a row costs, 2 n log2 n per iteration.
BLER: (32,64) and (512,1024), BP (20 iterations, exact f and min-sum scaled by 0.9375), SC and SCL L = 8 on
the same BLER_ROWS rows at BLER_EBNO_DB; 'what': 'bler' records.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((128, 256), (512, 1024))
BLER_SHAPES = ((32, 64), (512, 1024))
EBNO_DB, NUM_ITER = 2.0, 20
BLER_EBNO_DB, BLER_ROWS = 2.5, 65536


def timed(fn, reps, torch, ops):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:
        fn()
        torch.cuda.synchronize()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    clk0 = ops.shader_clock_ghz()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    clk1 = ops.shader_clock_ghz()
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "clock_ghz_before": round(clk0, 3), "clock_ghz_after": round(clk1, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd")]
    import torch

    import polar_amd
    from polar_amd import _lib, ops
    from polar_amd.channel import ebnodb2no
    if not torch.cuda.is_available():
        raise SystemExit("bp_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    lines = []

    def emit(d):
        d["library"] = _lib.lib().pl_version().decode()
        print(json.dumps(d), flush=True)
        lines.append(d)

    def plans(k, n):
        mask = polar_amd.frozen_mask(polar_amd.reference_frozen_pos(k, n).numpy(), n)
        bp = {f: _lib.Plan(n, mask, 1, fm, 19.3, flags=_lib.PL_PLAN_GENERIC)
              for f, fm in (("exact", _lib.PL_F_EXACT), ("minsum", _lib.PL_F_MINSUM))}
        return bp, _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM), _lib.Plan(n, mask, 8, _lib.PL_F_MINSUM)

    for k, n in SHAPES:
        bp, sc, scl = plans(k, n)
        no = float(ebnodb2no(EBNO_DB, 2, k / n))
        _, x = ops.awgn_qpsk_llr(sc, a.bs, no, 42, 0)
        base = {"what": "time", "k": k, "n": n, "bs": a.bs, "reps": a.reps, "ebno_db": EBNO_DB}
        for f in ("minsum", "exact"):
            for es in (False, True):
                r = ops.bp_decode(bp[f], x, NUM_ITER, early_stop=es, iters=True)
                mean_iters = float(r["iters"].float().mean())
                t = timed(lambda: ops.bp_decode(bp[f], x, NUM_ITER, early_stop=es, iters=True), a.reps, torch, ops)
                f_evals = 2 * n * (n.bit_length() - 1) * mean_iters
                emit({**base, "decoder": "bp", "f": f, "num_iter": NUM_ITER, "early_stop": es,
                      "mean_iters": round(mean_iters, 3), "f_evals_per_row": round(f_evals), **t,
                      "codewords_per_s": round(a.bs / t["ms_median"] * 1e3),
                      "f_evals_per_s": round(a.bs * f_evals / t["ms_median"] * 1e3)})
        out = torch.empty((a.bs, k), device="cuda")
        t = timed(lambda: ops.sc_decode(sc, x, out=out), a.reps, torch, ops)
        emit({**base, "decoder": "sc", "kernel": sc.kernel()[0], **t, "codewords_per_s": round(a.bs / t["ms_median"] * 1e3)})
        ws = ops.scl_workspace(scl, a.bs, x.device)
        t = timed(lambda: ops.scl_decode(scl, x, out=out, workspace=ws), a.reps, torch, ops)
        emit({**base, "decoder": "scl", "list_size": 8, "kernel": scl.kernel()[0], **t,
              "codewords_per_s": round(a.bs / t["ms_median"] * 1e3)})

    for k, n in BLER_SHAPES:
        bp, sc, scl = plans(k, n)
        no = float(ebnodb2no(BLER_EBNO_DB, 2, k / n))
        u, x = ops.awgn_qpsk_llr(sc, BLER_ROWS, no, 43, 0)

        def bler(bits):
            return int((bits != u).any(dim=1).sum())
        errs = {"bp_exact": bler(ops.bp_decode(bp["exact"], x, NUM_ITER)["bits"]),
                "bp_minsum_0.9375": bler(ops.bp_decode(bp["minsum"], x, NUM_ITER, scale=0.9375)["bits"]),
                "sc": bler(ops.sc_decode(sc, x)), "scl8": bler(ops.scl_decode(scl, x))}
        emit({"what": "bler", "k": k, "n": n, "rows": BLER_ROWS, "ebno_db": BLER_EBNO_DB, "num_iter": NUM_ITER,
              "block_errors": errs, "bler": {key: v / BLER_ROWS for key, v in errs.items()}})

    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
