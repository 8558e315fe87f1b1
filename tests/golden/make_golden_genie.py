"""Generate tests/golden/genie.npz: the reference SC decoder's own leaf LLRs.

TEST INFRASTRUCTURE ONLY; imports the reference (read-only at /root/reference) as make_golden.py
does, so it runs only in the build container.  After SC_Dec.forward
(x_run_sn_polar/polar/polar_sc.py:113-133) msg_llr[:, 0, :] holds the leaf LLR of every position
given the decoder's own earlier decisions; on rows it decodes correctly those decisions are the
true bits, i.e. the genie's.  Two row families per n in (8, 64, 256), 64 rows each:

  ok_n<n>    a random frozen set of rate 1/2, random information, BPSK-like logits with Gaussian
             noise; only rows the reference decodes correctly are kept.
  last_n<n>  frozen_pos = arange(n - 1): every fed-back bit is the frozen 0 whatever the input, so
             arbitrary logits are pinned -- exact zeros, -0, integer ties, a x40 saturated row
             (genie_ref.special_llrs).  u[n-1] is the reference's decision.  (The fully frozen code
             cannot be used: the reference's forward fails on k = 0.)

Each case stores logits [64, n] fp32, u [64, n] uint8 (the u-domain word, frozen positions 0) and
leaf [64, n] fp32 = msg_llr[:, 0, :].

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_genie.py
"""
import os
import sys

import numpy as np
import torch as tc

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path += [os.path.join(REF, "x_run_sn_polar"), REF, OUT]

from polar.polar_sc import SC_Dec as XSC  # noqa: E402

import genie_ref  # noqa: E402

ROWS = 64


def encode(u):
    x = u.copy()
    n = x.shape[1]
    h = 1
    while h < n:
        p = np.arange(n)
        lo = p[(p & h) == 0]
        x[:, lo] ^= x[:, lo + h]
        h *= 2
    return x


def run(fp, n, logits):
    dec = XSC(tc.from_numpy(fp), n)
    dec(tc.from_numpy(logits))
    return dec.msg_uhat[:, 0, :].numpy().astype(np.uint8), dec.msg_llr[:, 0, :].numpy().astype(np.float32)


def main():
    out = {}
    for n in (8, 64, 256):
        rng = np.random.default_rng(1000 + n)
        fp = np.sort(rng.permutation(n)[: n // 2]).astype(np.int64)
        info = np.setdiff1d(np.arange(n), fp)
        u = np.zeros((8 * ROWS, n), dtype=np.uint8)
        u[:, info] = rng.integers(0, 2, (8 * ROWS, len(info)))
        x = encode(u)
        # logits log P(1)/P(0): positive for a transmitted 1
        logits = ((2.0 * x - 1.0) * 4.0 + rng.standard_normal(x.shape) * 1.2).astype(np.float32)
        uhat, leaf = run(fp, n, logits)
        ok = np.flatnonzero((uhat == u).all(axis=1))[:ROWS]
        assert len(ok) == ROWS, f"n={n}: only {len(ok)} correctly decoded rows"
        out[f"ok_n{n}_logits"], out[f"ok_n{n}_u"], out[f"ok_n{n}_leaf"] = logits[ok], u[ok], leaf[ok]
        out[f"ok_n{n}_frozen"] = fp

        fp = np.arange(n - 1, dtype=np.int64)
        logits = genie_ref.special_llrs(rng, ROWS, n)
        uhat, leaf = run(fp, n, logits)
        assert not uhat[:, : n - 1].any()
        out[f"last_n{n}_logits"], out[f"last_n{n}_u"], out[f"last_n{n}_leaf"] = logits, uhat, leaf
    path = os.path.join(OUT, "genie.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for key in sorted(k for k in out if k.endswith("_leaf")):
        name = key[: -len("_leaf")]
        mine = genie_ref.leaf_llrs(out[name + "_logits"], out[name + "_u"])
        same = np.array_equal(mine.view(np.uint32), out[key].view(np.uint32))
        print(name, "genie_ref bit-identical:", same, "| value-equal:", np.array_equal(mine, out[key]))


if __name__ == "__main__":
    main()
