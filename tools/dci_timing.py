"""Time the parity-constrained list decoder on the 5G downlink DCI code (polar_amd.dci, ops.pcl_decode) and record
what the distributed CRC buys: (A, E) = (40, 216), (64, 432), (140, 576), BPSK over AWGN, 8192 rows, L = 8 and 32.

  python tools/dci_timing.py [--reps 25 --out profiles/dci_timing.jsonl]

Per code and list size, JSON lines of three kinds:
  "time"   the median of `reps` launches timed one by one with HIP events after 5 warm-up rounds (the decoders
           alternate inside the timed loop) of the mother-code decode alone, rate recovery left out: pcl_decode
           (interleaver on, n_force = 0) on signal rows and on pure-noise rows -- with the share of rows that stopped
           early and the mean stop leaf -- and plain min-sum scl_decode and pac_decode (conv = 1) of the same n and L
           on the signal rows: the cost of visiting every leaf;
  "bler"   on the signal rows, for interleave on / off and n_force = 0 / the number of distributed bits: the block
           error rate (payload wrong or ok = 0) and the undetected-error rate (payload wrong and ok = 1);
  "noise"  on pure-noise rows, the same settings: the share of rows that end with ok = 1 (a false alarm), the
           share that stopped early and the mean stop leaf.
Signal rows are at the Eb/N0 (rate A / E) of a 0.25 dB grid where plain min-sum SCL-8 on the mother code, without any
CRC, has the BLER of its A + 24 bits nearest 1e-2.  Both encoders (interleaver on and off) carry the same payloads
under the same noise samples.  The shader clock is read by pl_clock_probe right after the timed loop.

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
CODES = ((40, 216), (64, 432), (140, 576))
LISTS = (8, 32)
ROWS = 8192
RNTI = 0xBEEF
NOISE_SIGMA = 4.0  # logits of a candidate that carries nothing
STEP_TIMEOUT_S = 560


def step(A, E, reps):
    sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd")]
    import contextlib
    import io

    import numpy as np
    import torch

    import polar_amd
    from polar_amd import _lib, dci, ops
    if not torch.cuda.is_available():
        raise SystemExit("dci_timing needs a ROCm GPU (a time taken elsewhere says nothing)")
    bs = ROWS
    with contextlib.redirect_stdout(io.StringIO()):
        encs = {il: polar_amd.DCIEncoder(A, E, rnti=RNTI, interleave=il, device="cuda") for il in (True, False)}
    enc = encs[True]
    n, K = enc.n_polar, enc.k_polar
    dist = dci.distributed_parity_bits(enc)
    gen = torch.Generator(device="cuda").manual_seed(7)
    truth = (torch.rand((bs, A), device="cuda", generator=gen) < 0.5).float()
    noise = torch.randn((bs, E), device="cuda", generator=gen)
    xs = {il: 1.0 - 2.0 * e(truth) for il, e in encs.items()}

    def decoder(il, L, nf):
        return polar_amd.DCIDecoder(encs[il], list_size=L, n_force=nf, return_crc_status=True)
    rec = decoder(True, 8, 0)  # its rate recovery serves every decoder: the tables do not depend on the interleaver

    def rows_at(ebno_db, il):
        sigma = float(np.sqrt(1.0 / (2.0 * A / E * 10.0 ** (ebno_db / 10.0))))
        return rec.rate_recover(((xs[il] + sigma * noise) * (-2.0 / sigma ** 2)).contiguous())

    mask = polar_amd.frozen_mask(enc.frozen_pos, n)
    scl = {L: _lib.Plan(n, mask, L, _lib.PL_F_MINSUM, 100.0) for L in LISTS}
    ws = {L: ops.scl_workspace(scl[L], bs, "cuda") for L in LISTS}
    generic = _lib.Plan(n, mask, 1, _lib.PL_F_MINSUM, 100.0, flags=_lib.PL_PLAN_GENERIC)
    sent = enc.mother_input(truth)  # the A + 24 bits at the information positions

    grid = [0.25 * i for i in range(0, 33)]
    bler_ref = {e: float((ops.scl_decode(scl[8], rows_at(e, True), workspace=ws[8]) != sent).any(dim=1).float().mean())
                for e in grid}
    ebno = min(grid, key=lambda e: abs(bler_ref[e] - 1e-2))
    llr = {il: rows_at(ebno, il) for il in encs}
    blind = rec.rate_recover((torch.randn((bs, E), device="cuda", generator=gen) * NOISE_SIGMA).contiguous())
    base = {"A": A, "E": E, "n_polar": n, "k_polar": K, "bs": bs, "reps": reps, "rnti": RNTI, "ebno_db": ebno,
            "bler_scl8_no_crc": bler_ref[ebno], "distributed_bits": dist}

    # ---- what is decoded -------------------------------------------------------------------------------
    settings = [(True, 0), (True, dist), (False, 0)]
    for L in LISTS:
        for il, nf in settings:
            d = decoder(il, L, nf)
            bits, _, ok, stop = d.decode_mother(llr[il])
            a_hat = bits[:, torch.as_tensor(d._deint, device="cuda")]
            wrong = (a_hat != truth).any(dim=1)
            okb = ok != 0
            print(json.dumps(dict(base, kind="bler", L=L, interleave=il, n_force=nf,
                                  bler=round(float((wrong | ~okb).float().mean()), 6),
                                  undetected=round(float((wrong & okb).float().mean()), 6),
                                  stopped_early=round(float((stop < n).float().mean()), 6))), flush=True)
            _, _, ok, stop = d.decode_mother(blind)
            print(json.dumps(dict(base, kind="noise", L=L, interleave=il, n_force=nf,
                                  false_alarm=round(float((ok != 0).float().mean()), 6),
                                  stopped_early=round(float((stop < n).float().mean()), 6),
                                  mean_stop=round(float(stop.float().mean()), 2))), flush=True)

    # ---- what it costs ---------------------------------------------------------------------------------
    fns, stops = {}, {}
    out = torch.empty((bs, K), device="cuda")
    okb = torch.empty(bs, dtype=torch.uint8, device="cuda")
    for L in LISTS:
        plan, table = decoder(True, L, 0).polar_dec.plan("cuda")
        for what, x in (("signal", llr[True]), ("noise", blind)):
            stops[(L, what)] = torch.empty(bs, dtype=torch.int32, device="cuda")
            fns[(f"pcl{L}", what)] = lambda L=L, x=x, p=plan, t=table, s=stops[(L, what)]: \
                ops.pcl_decode(p, t, L, x, out=out, ok=okb, stop=s)
        fns[(f"scl{L}", "signal")] = lambda L=L: ops.scl_decode(scl[L], llr[True], out=out, workspace=ws[L])
        fns[(f"pac{L}", "signal")] = lambda L=L: ops.pac_decode(generic, 1, L, llr[True], out=out)
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
    clock = ops.shader_clock_ghz("cuda")
    for (name, what), t in times.items():
        res = dict(base, kind="time", decoder=name, rows=what, L=int(name[3:]), ms=round(statistics.median(t), 4),
                   clock_ghz=round(clock, 3))
        if name.startswith("pcl"):
            s = stops[(res["L"], what)]
            res.update(stopped_early=round(float((s < n).float().mean()), 6), mean_stop=round(float(s.float().mean()), 2))
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--only", default=None, help="run only the code with this payload length A (e.g. 40)")
    ap.add_argument("--step", nargs=2, metavar=("A", "E"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (medians of fewer launches are noise)")
    if a.step:
        return step(int(a.step[0]), int(a.step[1]), a.reps)
    lines = []
    for A, E in CODES:
        if a.only and int(a.only) != A:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(A), str(E)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step ({A},{E}): no result after {STEP_TIMEOUT_S} s; stopping")
        if p.returncode != 0:
            raise SystemExit(f"step ({A},{E}) failed ({p.returncode}); stopping\n{p.stderr[-2000:]}")
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                lines.append(d)
                print(ln, flush=True)
        if a.out:  # after every step: a later failure keeps what was measured
            with open(a.out, "w") as fo:
                for d in lines:
                    fo.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
