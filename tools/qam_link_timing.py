"""Time the fused link producers and one whole Monte-Carlo iteration at 2, 4, 6 and 8 bits per symbol
against the op-by-op chain at the same modulation, at the README's two shapes:

  plain  (512, 1024) x 65536 rows, SC_Dec (min-sum): channel.FusedAWGN vs channel.System_AWGN_model;
         m = 6 divides no power-of-two n and is left out
  nr     (500, 1024) uplink x 8192 rows, Polar5GDecoder SCL-8: channel.FusedAWGN5G vs
         channel.System5G_AWGN_model; m = 6 does not divide E = 1024 and runs at E = 1020

  python tools/qam_link_timing.py [--reps 25 --out profiles/qam_link_timing.jsonl]

Per (shape, m) it prints, and appends to --out as one JSON line, the median and the minimum over `reps`
HIP-event timings (after five warm-up rounds, the four paths alternating inside the timed loop) of
  fused_producer    the one-launch producer (llrs())
  unfused_producer  torch bits, encoder, Mapper, AWGN, Demapper (and rate recovery) on the GPU
  fused             error_counts(): producer, decoder, error count
  unfused           forward() + pl_count_errors
and the shader clock read with pl_clock_probe right after the timed loop.  Eb/N0 is chosen per m so
that the decoder works in its waterfall (the demapper's per-set pass depends on the noise level).
The op-by-op Demapper materialises [rows, symbols, 2^m / 2, m] gathers; where that would not fit a
sensible time or memory budget (plain, m = 8) it runs on `unfused_bs` rows and the line records both
row counts and the per-row ratio.

Every (shape, m) is a child process under its own time limit; the first one that fails ends the run
(nothing more is started on a GPU after a fault or a hang).
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBNO = {2: 2.5, 4: 5.5, 6: 9.0, 8: 13.0}
SETTINGS = [("plain", 2), ("plain", 4), ("plain", 8), ("nr", 2), ("nr", 4), ("nr", 6), ("nr", 8)]
UNFUSED_ROWS = {("plain", 8): 8192}
STEP_TIMEOUT_S = 240


def step(shape, m, reps):
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd")]
    import torch

    import polar_amd
    from polar_amd import channel, ops
    from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
    if not torch.cuda.is_available():
        raise SystemExit("qam_link_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    ebno = EBNO[m]
    gen = torch.Generator(device="cuda").manual_seed(42)
    if shape == "plain":
        k, n, bs = 512, 1024, 65536
        fp = polar_amd.reference_frozen_pos(k, n)
        dec = polar_amd.SC_Dec(fp, n, device="cuda")
        fused = channel.FusedAWGN(n, k, fp, dec, seed=42, num_bits_per_symbol=m)
        unfused = channel.System_AWGN_model(n, k, channel.GpuEncoder(fp, n), dec, device="cuda", generator=gen,
                                            num_bits_per_symbol=m)
        info = {"k": k, "n": n, "decoder": "SC"}
    else:
        k, n, bs = 500, 1024 if m != 6 else 1020, 8192
        with contextlib.redirect_stdout(io.StringIO()):
            enc = Polar5GEncoder(k, n)
            dec = Polar5GDecoder(enc, dec_type="SCL", list_size=8)
        fused = channel.FusedAWGN5G(enc, dec, seed=42, num_bits_per_symbol=m)
        unfused = channel.System5G_AWGN_model(enc, dec, device="cuda", generator=gen, num_bits_per_symbol=m)
        info = {"k_target": k, "n_target": n, "n_polar": enc.n_polar, "decoder": "SCL-8"}
    ubs = UNFUSED_ROWS.get((shape, m), bs)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    key = [0]

    def fused_iter():
        key[0] += 1
        assert fused.error_counts(bs, ebno, counts=counts, stream=(0, key[0])) is not None

    def unfused_iter():
        b, bh = unfused(ubs, ebno)
        ops.count_errors(b, bh.to(torch.float32), counts=counts)

    def fused_producer():
        key[0] += 1
        fused.llrs(bs, ebno, stream=(0, key[0]))

    def unfused_producer():
        llr = unfused.llrs(ubs, ebno)[2]
        if shape == "nr":
            dec.rate_recover(llr)

    fns = {"fused_ms": fused_iter, "unfused_ms": unfused_iter, "fused_producer_ms": fused_producer,
           "unfused_producer_ms": unfused_producer}
    times = {name: [] for name in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(-5, reps):  # five warm-up rounds, then the timed ones; the paths alternate
        for name, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append(e0.elapsed_time(e1))
    clock = ops.shader_clock_ghz()
    c = fused.error_counts(bs, ebno, stream=(1, 0))
    res = {"shape": shape, "bits_per_symbol": m, **info, "bs": bs, "unfused_bs": ubs, "ebno_db": ebno, "reps": reps,
           "bler_fused": round(int(c[1]) / bs, 4), "clock_ghz": round(clock, 3), "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        res[name.replace("_ms", "_median_ms")] = round(statistics.median(t), 4)
        res[name.replace("_ms", "_min_ms")] = round(min(t), 4)
    # per-row ratio of the producers (the op-by-op chain may have run on fewer rows)
    res["producer_speedup_per_row"] = round((res["unfused_producer_median_ms"] / ubs) /
                                            (res["fused_producer_median_ms"] / bs), 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qam_link_timing.jsonl"),
                    help="the result lines are appended to this file")
    ap.add_argument("--step", nargs=2, metavar=("SHAPE", "M"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer iterations are noise)")
    if a.step:
        return step(a.step[0], int(a.step[1]), a.reps)
    print(f"{'shape':6s} {'m':>2s} {'rows':>6s} {'fused prod.':>11s} {'unfused prod.':>13s} {'(rows)':>7s} {'fused':>9s} "
          f"{'unfused':>9s} {'x/row':>7s} {'GHz':>6s}   (ms, medians of {a.reps})", flush=True)
    for shape, m in SETTINGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", shape, str(m)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{shape} m={m}: no result after {STEP_TIMEOUT_S} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"{shape} m={m} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}")
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        print(f"{shape:6s} {m:2d} {d['bs']:6d} {d['fused_producer_median_ms']:11.4f} {d['unfused_producer_median_ms']:13.4f} "
              f"{d['unfused_bs']:7d} {d['fused_median_ms']:9.4f} {d['unfused_median_ms']:9.4f} "
              f"{d['producer_speedup_per_row']:7.1f} {d['clock_ghz']:6.3f}", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
