"""Generate tests/golden/osd.npz from the reference's ordered-statistics decoder.

TEST INFRASTRUCTURE ONLY.  Imports the reference (jaco267/polar-code-pytorch-sionna) from the
directory given on the command line and runs my_sn/fec/osd/dec.py::OSDecoder on the CPU, so it runs
only where the reference is; the tests read the committed osd.npz.

Per set NAME = k{k}n{n}t{t}: NAME_G uint8 [k, n], NAME_llr fp32 [rows, n] (BPSK-AWGN logits log P(1)/P(0)
at 1-3 dB Eb/N0), NAME_cw uint8 [rows, n] (OSDecoder.forward), NAME_d fp32 [rows] (the reference's
_get_dist of that word, dec.py:68-81).

The generator asserts, for every row of every set -- change the seed rather than drop a row:
  * no two equal |llr| and no |llr| >= 100 (the reference's argsort leaves ties open, and clipping makes ties);
  * the restatement (osd_ref.py) returns the reference's codeword;
  * the restatement's fp64 gap between the chosen Delta and the runner-up exceeds 1e-9, far above the
    ~1e-13 that the order of an fp64 sum of <= 256 fp32 terms can move it;
  * the fp64 metric of the returned word is within 256 * 2^-24 relative of the reference's fp32 one (n fp32
    additions).  The reference's fp32 log(1 + exp(x)) loses the small terms, so a set whose metrics are
    tiny (k = n = 8 at 3 dB) misses this through the reference's own rounding: that set is drawn at 1 dB.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_osd.py <reference checkout>
"""
import os
import sys

import numpy as np
import torch as tc

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, OUT)

import osd_ref  # noqa: E402


random_full_rank = osd_ref.random_full_rank


class DenseEncoder:
    """u -> u G mod 2, with .k, as the reference's constructor expects of an encoder."""

    def __init__(self, g):
        self.g = tc.tensor(g.astype(np.float32))
        self.k = g.shape[0]

    def __call__(self, u):
        return (u @ self.g) % 2


# (k, n, t, rows, Eb/N0 dB, generator matrix, seed)
def sets():
    rng = np.random.default_rng(2024)
    g65, g3, g8 = random_full_rank(65, 130, rng), random_full_rank(3, 7, rng), random_full_rank(8, 8, rng)
    g1 = np.array([[1, 1]], dtype=np.uint8)
    out = [(16, 32, t, 256, 1.0 + 0.5 * t, osd_ref.polar_like(16, 32), 10 + t) for t in range(4)]
    out += [(32, 64, 2, 256, 2.0, osd_ref.polar_like(32, 64), 20),
            (64, 128, 1, 128, 2.0, osd_ref.polar_like(64, 128), 30),
            (64, 128, 2, 128, 3.0, osd_ref.polar_like(64, 128), 31),
            (65, 130, 1, 64, 3.0, g65, 40),
            (3, 7, 3, 64, 2.0, g3, 50),
            (1, 2, 1, 32, 1.0, g1, 60),
            (8, 8, 1, 32, 1.0, g8, 70)]
    return out


def main(ref_root):
    sys.path.insert(0, ref_root)
    from my_sn.fec.osd.dec import OSDecoder
    data, names = {}, []
    for k, n, t, rows, ebno, g, seed in sets():
        name = f"k{k}n{n}t{t}"
        rng = np.random.default_rng(seed)
        llr, _ = osd_ref.awgn_logits(g, rows, ebno, rng)
        mag = np.abs(llr)
        assert all(len(np.unique(r)) == n for r in mag), (name, "equal |llr| in a row: change the seed")
        assert mag.max() < 100.0, (name, "clipped value: change the seed")
        dec = OSDecoder(t=t, encoder=DenseEncoder(g))
        cw, d = [], []
        for lo in range(0, rows, 32):
            x = tc.tensor(llr[lo:lo + 32])
            c = dec(x)
            cw.append(c.numpy())
            d.append(dec._get_dist(tc.clip(x, -100., 100.), c.unsqueeze(1)).squeeze(1).numpy())
        cw = np.concatenate(cw).astype(np.uint8)
        d = np.concatenate(d).astype(np.float32)
        mine, dist, pattern, gap = osd_ref.osd_decode(g, llr, t)
        assert np.array_equal(mine, cw), (name, "restatement differs from the reference",
                                          int((mine != cw).any(1).sum()))
        assert gap.min() > 1e-9, (name, "runner-up within 1e-9: change the seed", float(gap.min()))
        assert np.allclose(dist, d, rtol=256 * 2.0 ** -24, atol=0), name
        data[name + "_G"], data[name + "_llr"], data[name + "_cw"], data[name + "_d"] = g, llr, cw, d
        names.append(name)
        print(name, "rows", rows, "c0 kept", int((pattern < 0).sum()), "min gap", float(gap.min()))
    data["sets"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "osd.npz"), **data)
    print("wrote", os.path.join(OUT, "osd.npz"), os.path.getsize(os.path.join(OUT, "osd.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
