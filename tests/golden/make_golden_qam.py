"""Generate tests/golden/qam.npz: the reference's square-QAM blocks at 2, 4, 6 and 8 bits per symbol.

TEST INFRASTRUCTURE ONLY, as make_golden.py: it imports the reference (jaco267/polar-code-pytorch-sionna,
read-only; POLAR_REFERENCE_DIR, default /root/reference) on the CPU and writes inputs and expected
outputs only.  Nothing in the reference tree changes: the 16-QAM harness run replaces four attributes
of a constructed System_AWGN_model.

Reference call sites (file:line under the reference):
  * constellation  my_sn/trans/mapping.py:7-48, :49-95      qam(), QamConstell.points
  * mapper         my_sn/trans/mapping.py:111-149           Mapper.forward
  * demapper       my_sn/trans/mapping.py:151-241           Demapper.forward (logsumexp, logits log P1/P0)
  * harness        x_run_sn_polar/z_sys_model/awgn_model.py:16-44, x_run_sn_polar/polar/polar_sc.py:113-133

Contents, for m in (2, 4, 6, 8):
  points_m       complex64 [2^m]      QamConstell(m).points
  map_bits_m     float32 [1, m 2^m + m]  every symbol index once, in order, then one more all-ones symbol
  map_out_m      complex64            Mapper output for map_bits_m
  demap_y_m      complex64 [1, 320]   received symbols: the points themselves, midpoints of neighbouring
                                      points (exactly on decision boundaries), the origin and the axes,
                                      points far outside (|y| about 10), and seeded Gaussian draws
  demap_no       float32 [2]          the two noise variances (0.5 and 0.002)
  demap_llr_m    float32 [2, m 320]   Demapper output at demap_no[0], demap_no[1]
and the 16-QAM harness run of the (128, 256) code with the reference SC decoder:
  bler_k, bler_n, bler_m, bler_rows (4096), bler_seed, bler_ebno_db, bler_block_errors, bler_bler,
  bler_llr64     float32 [64, 256]    the LLRs of a separate 64-row run at the same seed and Eb/N0

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qam.py
"""
import os
import sys

import numpy as np
import torch as tc

REF = os.environ.get("POLAR_REFERENCE_DIR") or "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path += [os.path.join(REF, "x_run_sn_polar"), REF]

from my_sn.trans import mapping  # noqa: E402
from polar.froze import get_Kern_frozen_bits  # noqa: E402
from polar.polar_sc import SC_Dec as XSC  # noqa: E402
from z_sys_model.awgn_model import System_AWGN_model  # noqa: E402

F2 = tc.tensor([[1, 0], [1, 1]], dtype=tc.float32)
DEMAP_NO = np.array([0.5, 0.002], dtype=np.float32)
BLER_K, BLER_N, BLER_M, BLER_ROWS, BLER_SEED, BLER_EBNO_DB = 128, 256, 4, 4096, 2024, 6.5


class DenseEncoder(tc.nn.Module):
    """Arithmetic twin of x_run_sn_polar/polar/enc.py:30-43 (c[:,info]=u; (c@G)%2, fp32), as make_golden.py."""

    def __init__(self, frozen_pos, n, G):
        super().__init__()
        self.n = n
        self.info_pos = np.setdiff1d(np.arange(n), np.asarray(frozen_pos))
        self.G = G

    def forward(self, u):
        c = tc.zeros([u.shape[0], self.n], dtype=tc.float32)
        c[..., tc.from_numpy(self.info_pos)] = u
        return (c @ self.G % 2).to(tc.float32)


class Capture(tc.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.seen = []

    def forward(self, llr):
        self.seen.append(llr.clone())
        return self.inner(llr)


def demap_inputs(points, m):
    """320 fixed received symbols for one constellation (see the module docstring)."""
    p = points.astype(np.complex128)
    lv = np.unique(np.round(p.real, 9))
    mid = (lv[:-1] + lv[1:]) / 2
    ys = list(p[:64])                                                    # points themselves
    ys += [complex(a, b) for a in mid[:4] for b in lv[:4]]                # on a real-axis boundary
    ys += [complex(a, b) for a in lv[:4] for b in mid[:4]]                # on an imaginary-axis boundary
    ys += [complex(a, a) for a in mid]                                    # on both
    ys += [0j, 1 + 0j, -1 + 0j, 1j, -1j]
    ys += [10 + 0j, -10 + 0j, 10j, -10j, 7 + 7j, -7 - 7j, 7 - 7j, -7 + 7j, 10 + 0.05j, -0.05 + 10j]
    rng = np.random.default_rng(100 + m)
    rest = 320 - len(ys)
    g = rng.standard_normal((rest, 2)) * np.where(np.arange(rest)[:, None] % 2 == 0, 0.8, 0.15)
    base = p[rng.integers(0, len(p), rest)] * (np.arange(rest) % 2 == 1)
    ys += list(base + g[:, 0] + 1j * g[:, 1])
    return np.asarray(ys, dtype=np.complex64)[None, :]


def blocks(out):
    for m in (2, 4, 6, 8):
        const = mapping.QamConstell(m)
        mapper, demapper = mapping.Mapper(constell=const), mapping.Demapper(constell=const)
        pts = const.points.numpy()
        out[f"points_{m}"] = pts
        bits = np.array([list(np.binary_repr(i, m)) for i in range(2 ** m)] + [["1"] * m], dtype=np.float32)
        bits = bits.reshape(1, -1)
        out[f"map_bits_{m}"] = bits
        out[f"map_out_{m}"] = mapper(tc.from_numpy(bits)).numpy()
        y = demap_inputs(pts, m)
        assert y.shape == (1, 320)
        out[f"demap_y_{m}"] = y
        out[f"demap_llr_{m}"] = np.stack(
            [demapper([tc.from_numpy(y), tc.tensor(no, dtype=tc.float32)]).numpy()[0] for no in DEMAP_NO])
        print(f"  m={m}: {len(pts)} points, llr range {out[f'demap_llr_{m}'].min():.4g} .. "
              f"{out[f'demap_llr_{m}'].max():.4g}")
    out["demap_no"] = DEMAP_NO


def qam_model(k, n, m, decoder):
    """The reference's System_AWGN_model with its modulation attributes replaced (its constructor fixes 2)."""
    G, _, fp = get_Kern_frozen_bits(n, n - k, F2)
    model = System_AWGN_model(n, k, DenseEncoder(fp, n, G), decoder(fp, n))
    model.n_bits_per_sym = m
    model.constell = mapping.QamConstell(m)
    model.mapper = mapping.Mapper(constell=model.constell)
    model.demapper = mapping.Demapper(constell=model.constell)
    return model


def harness(out):
    k, n, m = BLER_K, BLER_N, BLER_M
    ebno = tc.tensor(BLER_EBNO_DB, dtype=tc.float32)
    model = qam_model(k, n, m, XSC)
    tc.manual_seed(BLER_SEED)
    with tc.no_grad():
        b, b_hat = model(BLER_ROWS, ebno)
    errs = int((b != b_hat).any(dim=1).sum())
    model = qam_model(k, n, m, lambda fp, n_: Capture(XSC(fp, n_)))
    tc.manual_seed(BLER_SEED)
    with tc.no_grad():
        model(64, ebno)
    cap = model.decoder.seen[0].numpy().astype(np.float32)
    out.update(bler_k=k, bler_n=n, bler_m=m, bler_rows=BLER_ROWS, bler_seed=BLER_SEED,
               bler_ebno_db=np.float32(BLER_EBNO_DB), bler_block_errors=errs, bler_bler=errs / BLER_ROWS,
               bler_llr64=cap)
    print(f"  ({k},{n}) 16-QAM SC at {BLER_EBNO_DB} dB: {errs}/{BLER_ROWS} block errors = {errs / BLER_ROWS:.4f}")
    assert 0.05 <= errs / BLER_ROWS <= 0.5, "pick another BLER_EBNO_DB"


def main():
    tc.set_num_threads(8)
    out = {}
    blocks(out)
    harness(out)
    np.savez_compressed(os.path.join(OUT, "qam.npz"), **out)
    print("wrote", os.path.join(OUT, "qam.npz"), os.path.getsize(os.path.join(OUT, "qam.npz")), "bytes")


if __name__ == "__main__":
    main()
