"""Time the automorphism-ensemble SC decoder (ops.ae_decode) next to SC and SCL (L = 8) on the same rows, and
record what each decodes: the Reed-Muller codes (64,128), (256,512) and (386,1024) -- the reference's row-weight
frozen sets at those (k, n) --, BPSK over AWGN, 8192 and 65536 rows, M = 4 ... 64 candidates, both f, bit-index
("stage") and GL(m, 2) ("linear") tables, at the Eb/N0 of a 0.25 dB grid where SC's BLER is nearest 0.1.

  python tools/ae_timing.py [--reps 25 --out profiles/ae_timing.jsonl]

Per (code, rows) one JSON line per decoder configuration: the median of `reps` launches timed one by one with HIP
events after 5 warm-up rounds (the configurations alternate inside the timed loop), the BLER on those rows and, for
AE, the share of rows the identity candidate wins.  One more AE-8 line per (code, rows) uses a gather-hostile
table, eight copies of the bit reversal, next to the seeded AE-8 stage line: the LDS gather's worst bank-conflict
case beside the typical one.  The shader clock is read by pl_clock_probe right after the timed loop.

Every (code, rows) step is a child process under its own time limit; the first step that fails ends the run
(nothing more is started on a GPU after a fault or a hang).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = ((3, 7), (4, 9), (4, 10))  # RM(r, m): (64,128), (256,512), (386,1024)
ROWS = (8192, 65536)
PERMS = (4, 8, 16, 32, 64)
FS = ("minsum", "exact")
KINDS = ("stage", "linear")
LIST = 8
STEP_TIMEOUT_S = 560


def encode(u):
    import numpy as np
    b = u.copy()
    n = b.shape[1]
    p = np.arange(n)
    h = 1
    while h < n:
        lo = p[(p & h) == 0]
        b[:, lo] ^= b[:, lo + h]
        h <<= 1
    return b


def step(r, m, bs, reps):
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd")]
    import numpy as np
    import torch

    import polar_amd
    from polar_amd import _lib, automorphism, ops
    if not torch.cuda.is_available():
        raise SystemExit("ae_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    n = 1 << m
    k, fp = automorphism.rm_code(r, m)
    mask = polar_amd.frozen_mask(fp, n)
    info = np.setdiff1d(np.arange(n), fp)
    rng = np.random.default_rng(7)
    bits = (rng.random((bs, k)) < 0.5).astype(np.uint8)
    u = np.zeros((bs, n), dtype=np.uint8)
    u[:, info] = bits
    xs = torch.from_numpy(1.0 - 2.0 * encode(u).astype(np.float32)).cuda()
    noise = torch.randn((bs, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    truth = torch.from_numpy(bits).cuda().float()

    def rows_at(ebno_db):
        sigma = float(np.sqrt(1.0 / (2.0 * k / n * 10.0 ** (ebno_db / 10.0))))
        return ((xs + sigma * noise) * (-2.0 / sigma ** 2)).contiguous()

    plans = {"minsum": _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM)}  # SC as the package runs it: the specialised kernel
    generic = {f: _lib.Plan(n, mask, 1, _lib.PL_F_EXACT if f == "exact" else _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_GENERIC)
               for f in FS}
    grid = [0.25 * i for i in range(0, 29)]
    bler_sc = {e: float((ops.sc_decode(plans["minsum"], rows_at(e)) != truth).any(dim=1).float().mean()) for e in grid}
    ebno = min(grid, key=lambda e: abs(bler_sc[e] - 0.1))
    llr = rows_at(ebno)

    fns, outs = {}, {}

    def add(name, fn):
        outs[name] = torch.empty((bs, k), device="cuda")
        fns[name] = fn
    add("sc", lambda: ops.sc_decode(plans["minsum"], llr, out=outs["sc"]))
    try:
        scl = _lib.Plan(n, mask, LIST, _lib.PL_F_MINSUM, flags=_lib.PL_PLAN_FAST_SCL)
        ws = ops.scl_workspace(scl, bs, llr.device)
        add(f"scl{LIST}", lambda: ops.scl_decode(scl, llr, out=outs[f"scl{LIST}"], workspace=ws))
    except _lib.PolarLibError as e:  # the list kernels do not take this shape
        print(json.dumps({"n": n, "k": k, "bs": bs, "skipped": f"scl{LIST}", "why": str(e)}), flush=True)
    tables = {kind: (automorphism.stage_permutations if kind == "stage" else automorphism.linear_permutations)(
        fp, n, max(PERMS), seed=0) for kind in KINDS}
    rev = np.array([int(format(i, f"0{m}b")[::-1], 2) for i in range(n)])
    tables["bitrev"] = np.stack([rev] * 8)
    for f in FS:
        for kind in KINDS:
            for mm in PERMS:
                t = ops.ae_perm_table(tables[kind][:mm], llr.device)
                name = f"ae{mm}_{kind}_{f}"
                add(name, lambda f=f, t=t, name=name: ops.ae_decode(generic[f], llr, t, out=outs[name]))
    t_rev = ops.ae_perm_table(tables["bitrev"], llr.device)
    add("ae8_bitrev_minsum", lambda: ops.ae_decode(generic["minsum"], llr, t_rev, out=outs["ae8_bitrev_minsum"]))

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
    for name in fns:
        res = {"code": f"RM({r},{m})", "n": n, "k": k, "bs": bs, "reps": reps, "ebno_db": ebno, "decoder": name,
               "ms": round(statistics.median(times[name]), 4),
               "bler": round(float((outs[name] != truth).any(dim=1).float().mean()), 6),
               "clock_ghz": round(clock, 3)}
        if name == "sc":
            res["kernel"] = plans["minsum"].kernel()[0]
        if name.startswith("ae"):
            mm, kind, f = name[2:].split("_")
            t = ops.ae_perm_table(tables[kind][:int(mm)], llr.device)
            _, idx, _ = ops.ae_decode(generic[f], llr, t, return_info=True)
            res["identity_wins"] = round(float((idx == 0).float().mean()), 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--only", default=None, help="run only the codes with this n (e.g. 128)")
    ap.add_argument("--step", nargs=3, metavar=("R", "M", "ROWS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    if a.step:
        return step(int(a.step[0]), int(a.step[1]), int(a.step[2]), a.reps)
    lines = []
    for r, m in CODES:
        if a.only and int(a.only) != 1 << m:
            continue
        for bs in ROWS:
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(r), str(m), str(bs)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"step RM({r},{m}) x {bs}: no result after {STEP_TIMEOUT_S} s; stopping")
            if p.returncode != 0:
                raise SystemExit(f"step RM({r},{m}) x {bs} failed ({p.returncode}); stopping\n{p.stderr[-2000:]}")
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    d = json.loads(ln)
                    lines.append(d)
                    if "decoder" in d:
                        print(f"n {d['n']:5d} rows {d['bs']:6d} {d['ebno_db']:4.2f} dB {d['decoder']:22s} {d['ms']:9.3f} ms  "
                              f"BLER {d['bler']:.5f}  {d['clock_ghz']} GHz", flush=True)
            if a.out:  # after every step: a later failure keeps what was measured
                with open(a.out, "w") as fo:
                    for d in lines:
                        fo.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
