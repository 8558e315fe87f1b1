"""Time the ordered-statistics decoder (ops.osd_decode, csrc/osd_kernel.hip) at bs = 8192:
(32,64) at t = 1, 2, 3, (64,128) at t = 1, 2 and (128,256) at t = 1, on BPSK-AWGN logits at 2 dB.

  python tools/osd_timing.py [--bs 8192 --reps 25 --out profiles/osd_timing.jsonl]
  python tools/osd_timing.py --reference DIR [--out FILE]     # the reference's CPU decoder, same shapes

Per case one JSON line: the median of `reps` launches timed one by one with HIP events after five
warm-up launches, the shader clock right before and right after them (pl_clock_probe), codewords/s,
candidates/s (codewords/s x patterns), and the VALU-issue yardstick of the search alone: a candidate
costs n/4 fp64 adds (one per nibble table), a wave-instruction serves 64 candidates, and the chip
issues 1024 (256 CUs x 4 SIMDs) of them per cycle at best -- `search_add_floor_ms` is that count over
the measured clock, an explicit lower bound, not a model of the kernel.
--reference imports my_sn/fec/osd/dec.py::OSDecoder from DIR and records its seconds per row on this
machine's CPU at a batch it can hold (its candidates are a [bs, C(k,t), n] fp32 tensor).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((32, 64, 1), (32, 64, 2), (32, 64, 3), (64, 128, 1), (64, 128, 2), (128, 256, 1))
EBNO_DB = 2.0
SIMDS = 256 * 4


sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from osd_ref import awgn_logits, polar_like  # noqa: E402


def logits(g, rows, seed=3):
    return awgn_logits(g, rows, EBNO_DB, seed)[0]


def gpu(bs, reps):
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd")]
    import torch

    from polar_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("osd_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    lines = []
    for k, n, t in CASES:
        g = polar_like(k, n)
        plan = _lib.OsdPlan(g, t)
        x = torch.from_numpy(logits(g, bs)).cuda()
        out = torch.empty((bs, n), device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            ops.osd_decode(plan, x, out=out)
        torch.cuda.synchronize()
        clk0 = ops.shader_clock_ghz()
        ms = []
        for _ in range(reps):
            e0.record()
            ops.osd_decode(plan, x, out=out)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        clk1 = ops.shader_clock_ghz()
        med = statistics.median(ms)
        adds = plan.n_patterns * (n // 4)  # fp64 adds of the search, per codeword
        clk = 0.5 * (clk0 + clk1)
        floor_ms = bs * adds / 64 / SIMDS / (clk * 1e9) * 1e3
        d = {"what": "gpu", "k": k, "n": n, "t": t, "bs": bs, "reps": reps, "patterns": plan.n_patterns,
             "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
             "clock_ghz_before": round(clk0, 3), "clock_ghz_after": round(clk1, 3),
             "codewords_per_s": round(bs / med * 1e3), "candidates_per_s": round(bs * plan.n_patterns / med * 1e3),
             "search_adds_per_codeword": adds, "search_add_floor_ms": round(floor_ms, 5),
             "floor_over_measured": round(floor_ms / med, 4), "library": _lib.lib().pl_version().decode()}
        print(json.dumps(d), flush=True)
        lines.append(d)
    return lines


def reference(ref_root):
    sys.path.insert(0, ref_root)
    import torch as tc
    from my_sn.fec.osd.dec import OSDecoder

    class Enc:
        def __init__(self, g):
            self.g, self.k = tc.tensor(g.astype("float32")), g.shape[0]

        def __call__(self, u):
            return (u @ self.g) % 2
    lines = []
    for k, n, t in CASES:
        g = polar_like(k, n)
        pats = sum(math.comb(k, i) for i in range(1, t + 1))
        rows = max(4, min(256, (1 << 25) // (pats * n)))  # candidates of <= 128 MB fp32
        dec = OSDecoder(t=t, encoder=Enc(g))
        x = tc.tensor(logits(g, rows))
        dec(x[:2])
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            dec(x)
            times.append(time.perf_counter() - t0)
        d = {"what": "reference_cpu", "k": k, "n": n, "t": t, "rows": rows, "patterns": pats,
             "s_per_row": statistics.median(times) / rows, "threads": tc.get_num_threads()}
        print(json.dumps(d), flush=True)
        lines.append(d)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--reference", default=None, help="time the reference's CPU decoder from this checkout instead")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    lines = reference(a.reference) if a.reference else gpu(a.bs, a.reps)
    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
