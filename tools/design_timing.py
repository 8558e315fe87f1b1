"""Time the frozen-set design hot path (polar_amd.design: the fused producer over a plan without
frozen positions, then ops.genie_count, csrc/genie_kernel.hip) and measure what a designed code buys.

  python tools/design_timing.py [--bs 65536 --reps 25 --out profiles/design_timing.jsonl]

Per n in (256, 1024, 2048) one JSON line: the producer launch and the genie transform of one batch of
`bs` rows at rate 1/2, 2.5 dB, QPSK, timed one by one with HIP events after five warm-up launches -- the
median of `reps`, the shader clock right before and after (pl_clock_probe) -- and the bytes the transform
moves (4 n + n / 8 read per row; the counters are its only output).  Both kernels move 4 n bytes a row,
so `transform_over_producer` is the honest comparison.
Then one line for (512,1024) at 2.5 dB: SC block errors over 2^16 rows of the set designed there over
2^20 rows against the pinned RM-weight set (FusedAWGN + SC_Dec on the generic kernel, same Philox key).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd")]
EBNO_DB = 2.5


def timed(fn, reps):
    import torch

    from polar_amd import ops
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    clk0 = ops.shader_clock_ghz()
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


def batch_times(bs, reps):
    import numpy as np
    import torch

    from polar_amd import _lib, channel, ops
    lines = []
    for n in (256, 1024, 2048):
        plan = _lib.Plan(n, np.zeros(n, dtype=np.uint8), 1, flags=_lib.PL_PLAN_GENERIC)
        no = float(channel.ebnodb2no(EBNO_DB, 2, 0.5))
        _, ubits, _, llr = ops.awgn_qam_llr(plan, 2, bs, no, 0, 0, with_u=False, with_ubits=True)
        counts = torch.zeros(n, dtype=torch.int64, device="cuda")
        # the producer as design.bit_channel_errors calls it (it allocates its outputs; the allocator is warm)
        prod = timed(lambda: ops.awgn_qam_llr(plan, 2, bs, no, 0, 0, with_u=False, with_ubits=True), reps)
        gen = timed(lambda: ops.genie_count(n, llr, ubits, counts=counts), reps)
        read = bs * (4 * n + n // 8)
        d = {"what": "design_batch", "n": n, "bs": bs, "reps": reps, "ebno_db": EBNO_DB, "producer": prod,
             "transform": gen, "transform_over_producer": round(gen["ms_median"] / prod["ms_median"], 3),
             "transform_read_bytes": read, "transform_read_gb_per_s": round(read / gen["ms_median"] / 1e6, 1),
             "library": _lib.lib().pl_version().decode()}
        print(json.dumps(d), flush=True)
        lines.append(d)
    return lines


def designed_vs_rm(rows):
    from polar_amd import SC_Dec, _lib, channel, design, reference_frozen_pos
    k, n = 512, 1024

    class GenericSC(SC_Dec):
        def _make_plan(self, dev):
            return _lib.Plan(self.n, self._mask, 1, _lib.PL_F_MINSUM, self.llr_max, flags=_lib.PL_PLAN_GENERIC,
                             device=dev)
    counts, done = design.bit_channel_errors(n, k, EBNO_DB, 2 ** 20)
    sets = {"designed": design.select_frozen(counts, k), "rm_weight": reference_frozen_pos(k, n)}
    d = {"what": "designed_vs_rm_weight", "k": k, "n": n, "ebno_db": EBNO_DB, "design_rows": done, "rows": rows,
         "union_bound": design.union_bound(counts, done, sets["designed"]), "library": _lib.lib().pl_version().decode()}
    for name, fp in sets.items():
        model = channel.FusedAWGN(n, k, fp, GenericSC(fp, n, device="cuda"), seed=5)
        bits, hat = model(rows, EBNO_DB)
        d[name + "_block_errors"] = int((bits != hat).any(dim=1).sum())
        d[name + "_bler"] = d[name + "_block_errors"] / rows
    print(json.dumps(d), flush=True)
    return [d]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rows", type=int, default=2 ** 16, help="codewords of the designed-against-RM-weight run")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("design_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    lines = batch_times(a.bs, a.reps) + designed_vs_rm(a.rows)
    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
