"""Time the PAC list decoder (ops.pac_decode) next to plain SCL (min-sum, same L, the plain polar code on the same
frozen set) and AE-8 on the same noise, and record what each decodes: the reference's row-weight frozen sets at
(64,128), (128,256) and (512,1024), generator 0o133, BPSK over AWGN, 8192 rows, at the Eb/N0 of a 0.25 dB grid
where plain SCL-32 has its BLER nearest 1e-2.

  python tools/pac_timing.py [--reps 25 --out profiles/pac_timing.jsonl]

Per code one JSON line per decoder: the median of `reps` launches timed one by one with HIP events after 5 warm-up
rounds (the decoders alternate inside the timed loop; a decoder with "timed": false is run once, for its BLER
only), and the BLER on those rows.  The PAC decoders see the PAC codewords of the same data bits under the same
noise samples as the plain decoders see the plain codewords.  (64,128) also gets OSD of order 3 on the PAC code's
generator matrix, the estimate of its maximum-likelihood BLER.  The shader clock is read by pl_clock_probe right
after the timed loop.

Every code is a child process under its own time limit; the first step that fails ends the run (nothing more is
started on a GPU after a fault or a hang).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = ((64, 128, (8, 32)), (128, 256, (8, 32)), (512, 1024, (8,)))  # (k, n, the list sizes timed)
BLER_LISTS = (8, 32)
ROWS = 8192
CONV = "133"
OSD_T = 3
STEP_TIMEOUT_S = 560


def step(k, n, reps):
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd")]
    import numpy as np
    import torch

    import polar_amd
    from polar_amd import _lib, automorphism, ops, pac
    if not torch.cuda.is_available():
        raise SystemExit("pac_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    bs = ROWS
    timed_lists = dict((c[:2], c[2]) for c in CODES)[(k, n)]
    fp = np.sort(polar_amd.reference_frozen_pos(k, n).numpy().astype(np.int64))
    mask = polar_amd.frozen_mask(fp, n)
    conv = pac.conv_from_octal(CONV)
    cmask = pac.conv_to_mask(conv)
    generic = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
    gen = torch.Generator(device="cuda").manual_seed(7)
    truth = (torch.rand((bs, k), device="cuda", generator=gen) < 0.5).float()
    noise = torch.randn((bs, n), device="cuda", generator=gen)
    xs = {"plain": 1.0 - 2.0 * ops.polar_encode(generic, truth), "pac": 1.0 - 2.0 * ops.pac_encode(generic, cmask, truth)}

    def rows_at(ebno_db, code):
        sigma = float(np.sqrt(1.0 / (2.0 * k / n * 10.0 ** (ebno_db / 10.0))))
        return ((xs[code] + sigma * noise) * (-2.0 / sigma ** 2)).contiguous()

    scl = {L: _lib.Plan(n, mask, L, _lib.PL_F_MINSUM) for L in BLER_LISTS}
    ws = {L: ops.scl_workspace(scl[L], bs, "cuda") for L in BLER_LISTS}

    def bler(out):
        return float((out != truth).any(dim=1).float().mean())
    grid = [0.25 * i for i in range(0, 29)]
    ref_l = max(BLER_LISTS)
    bler_ref = {e: bler(ops.scl_decode(scl[ref_l], rows_at(e, "plain"), workspace=ws[ref_l])) for e in grid}
    ebno = min(grid, key=lambda e: abs(bler_ref[e] - 1e-2))
    llr = {c: rows_at(ebno, c) for c in xs}

    fns, outs, timed = {}, {}, {}

    def add(name, fn, is_timed=True):
        outs[name] = torch.empty((bs, k), device="cuda")
        fns[name], timed[name] = fn, is_timed
    for L in BLER_LISTS:
        add(f"pac{L}", lambda L=L: ops.pac_decode(generic, cmask, L, llr["pac"], out=outs[f"pac{L}"]), L in timed_lists)
        add(f"scl{L}", lambda L=L: ops.scl_decode(scl[L], llr["plain"], out=outs[f"scl{L}"], workspace=ws[L]),
            L in timed_lists)
    try:
        table = ops.ae_perm_table(automorphism.stage_permutations(fp, n, 8, seed=0), "cuda")
        add("ae8", lambda: ops.ae_decode(generic, llr["plain"], table, out=outs["ae8"]))
    except ValueError as e:  # the frozen set has too few bit-index automorphisms
        print(json.dumps({"n": n, "k": k, "bs": bs, "skipped": "ae8", "why": str(e)}), flush=True)

    times = {name: [] for name in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn in fns.items():
        if not timed[name]:
            fn()
    for rep in range(-5, reps):
        for name, fn in fns.items():
            if not timed[name]:
                continue
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append(e0.elapsed_time(e1))
    clock = ops.shader_clock_ghz("cuda")
    base = {"n": n, "k": k, "bs": bs, "reps": reps, "conv": CONV, "ebno_db": ebno, "bler_scl32_grid": bler_ref[ebno]}
    for name in fns:
        res = dict(base, decoder=name, timed=timed[name], bler=round(bler(outs[name]), 6), clock_ghz=round(clock, 3))
        if timed[name]:
            res["ms"] = round(statistics.median(times[name]), 4)
        print(json.dumps(res), flush=True)
    if (k, n) == (64, 128):
        enc = polar_amd.PACEncoder(fp, n, conv, device="cuda")
        osd = polar_amd.OSDecoder(OSD_T, enc, device="cuda")
        cw_hat = osd(llr["pac"])
        cw = (1.0 - xs["pac"]) / 2.0
        print(json.dumps(dict(base, decoder=f"osd{OSD_T}_of_pac", timed=False,
                              bler=round(float((cw_hat != cw).any(dim=1).float().mean()), 6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--only", default=None, help="run only the code with this n (e.g. 128)")
    ap.add_argument("--step", nargs=2, metavar=("K", "N"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    if a.step:
        return step(int(a.step[0]), int(a.step[1]), a.reps)
    lines = []
    for k, n, _ in CODES:
        if a.only and int(a.only) != n:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(k), str(n)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step ({k},{n}): no result after {STEP_TIMEOUT_S} s; stopping")
        if p.returncode != 0:
            raise SystemExit(f"step ({k},{n}) failed ({p.returncode}); stopping\n{p.stderr[-2000:]}")
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                lines.append(d)
                if "decoder" in d:
                    ms = f"{d['ms']:9.3f} ms" if "ms" in d else "   (untimed)"
                    print(f"n {d['n']:5d} rows {d['bs']:6d} {d['ebno_db']:4.2f} dB {d['decoder']:14s} {ms}  "
                          f"BLER {d['bler']:.5f}", flush=True)
        if a.out:  # after every step: a later failure keeps what was measured
            with open(a.out, "w") as fo:
                for d in lines:
                    fo.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
