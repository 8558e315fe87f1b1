"""Time the soft-cancellation decoder (ops.scan_decode, csrc/scan_kernel.hip) next to BP-20, SC and SCL L = 8, and
count its block errors.

  python tools/scan_timing.py [--bs 8192 --reps 25 --out profiles/scan_timing.jsonl]

Timing: (128,256), (512,1024) and (1024,2048; SCAN, SC and SCL only -- the BP kernel ends at n = 1024), 8192 rows of
the fused producer (ops.awgn_qpsk_llr) at EBNO_DB; SCAN with 1, 2 and 4 iterations, min-sum and exact f, early stop
off and on (with it on, the mean of `iters` is in the record); BP (20 iterations, both f, early stop off), SC (the
specialised kernel) and SCL L = 8 decode the same rows in the same process.  Each record is the median of `reps`
launches timed one by one with HIP events after bench.py's warm-up pattern (100 ms of untimed launches so the clock
leaves its idle state, then five more), with the shader clock right before and after (pl_clock_probe).
BLER: the three codes, SCAN-1 / 2 / 4 (exact f and min-sum), BP-20 (n <= 1024), SC and SCL L = 8 on the same
BLER_ROWS rows at BLER_EBNO_DB; 'what': 'bler' records.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((128, 256), (512, 1024), (1024, 2048))
SCAN_ITERS, BP_ITER, BP_MAX_N = (1, 2, 4), 20, 1024
EBNO_DB = 2.0
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
        raise SystemExit("scan_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    lines = []

    def emit(d):
        d["library"] = _lib.lib().pl_version().decode()
        print(json.dumps(d), flush=True)
        lines.append(d)

    def plans(k, n):
        mask = polar_amd.frozen_mask(polar_amd.reference_frozen_pos(k, n).numpy(), n)
        soft = {f: _lib.Plan(n, mask, 1, fm, 19.3, flags=_lib.PL_PLAN_GENERIC)
                for f, fm in (("exact", _lib.PL_F_EXACT), ("minsum", _lib.PL_F_MINSUM))}
        return soft, _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM), _lib.Plan(n, mask, 8, _lib.PL_F_MINSUM)

    for k, n in SHAPES:
        soft, sc, scl = plans(k, n)
        no = float(ebnodb2no(EBNO_DB, 2, k / n))
        _, x = ops.awgn_qpsk_llr(sc, a.bs, no, 42, 0)
        base = {"what": "time", "k": k, "n": n, "bs": a.bs, "reps": a.reps, "ebno_db": EBNO_DB}
        f_evals_iter = 2 * n * (n.bit_length() - 1)
        for f in ("minsum", "exact"):
            for num_iter in SCAN_ITERS:
                for es in (False, True):
                    r = ops.scan_decode(soft[f], x, num_iter, early_stop=es, iters=True)
                    mean_iters = float(r["iters"].float().mean())
                    t = timed(lambda: ops.scan_decode(soft[f], x, num_iter, early_stop=es, iters=True), a.reps, torch, ops)
                    emit({**base, "decoder": "scan", "f": f, "num_iter": num_iter, "early_stop": es,
                          "mean_iters": round(mean_iters, 3), "f_evals_per_row": round(f_evals_iter * mean_iters), **t,
                          "codewords_per_s": round(a.bs / t["ms_median"] * 1e3)})
            if n <= BP_MAX_N:
                t = timed(lambda: ops.bp_decode(soft[f], x, BP_ITER, iters=True), a.reps, torch, ops)
                emit({**base, "decoder": "bp", "f": f, "num_iter": BP_ITER, "early_stop": False,
                      "f_evals_per_row": f_evals_iter * BP_ITER, **t,
                      "codewords_per_s": round(a.bs / t["ms_median"] * 1e3)})
        out = torch.empty((a.bs, k), device="cuda")
        t = timed(lambda: ops.sc_decode(sc, x, out=out), a.reps, torch, ops)
        emit({**base, "decoder": "sc", "kernel": sc.kernel()[0], **t, "codewords_per_s": round(a.bs / t["ms_median"] * 1e3)})
        ws = ops.scl_workspace(scl, a.bs, x.device)
        t = timed(lambda: ops.scl_decode(scl, x, out=out, workspace=ws), a.reps, torch, ops)
        emit({**base, "decoder": "scl", "list_size": 8, "kernel": scl.kernel()[0], **t,
              "codewords_per_s": round(a.bs / t["ms_median"] * 1e3)})

    for k, n in SHAPES:
        soft, sc, scl = plans(k, n)
        no = float(ebnodb2no(BLER_EBNO_DB, 2, k / n))
        u, x = ops.awgn_qpsk_llr(sc, BLER_ROWS, no, 43, 0)

        def bler(bits):
            return int((bits != u).any(dim=1).sum())
        errs = {"sc": bler(ops.sc_decode(sc, x)), "scl8": bler(ops.scl_decode(scl, x))}
        for f in ("exact", "minsum"):
            for num_iter in SCAN_ITERS:
                errs[f"scan{num_iter}_{f}"] = bler(ops.scan_decode(soft[f], x, num_iter)["bits"])
            if n <= BP_MAX_N:
                errs[f"bp{BP_ITER}_{f}"] = bler(ops.bp_decode(soft[f], x, BP_ITER)["bits"])
        emit({"what": "bler", "k": k, "n": n, "rows": BLER_ROWS, "ebno_db": BLER_EBNO_DB,
              "block_errors": errs, "bler": {key: v / BLER_ROWS for key, v in errs.items()}})

    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
