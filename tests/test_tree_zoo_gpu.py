"""The rate-0 zoo (tests/golden/tree_zoo_ref.py, audited by tests/test_tree_zoo_ref.py) on the GPU: the register
trees of pl_scq_decode, pl_scf_decode's flip kernel and pl_ae_decode against their numpy restatements, bit for
bit (SCQ is integer; SC-Flip runs min-sum, one fp32 rounding per operation in a fixed order; AE runs on the exact
grid).  Generic plans throughout: nothing is compiled here.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import ae_ref  # noqa: E402
import scf_ref  # noqa: E402
import scq_ref  # noqa: E402
import tree_zoo_ref as zoo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(codes):
    return [c[0] for c in codes]


def _plan(mask, crc=None):
    from polar_amd import _lib
    p = _lib.Plan(len(mask), np.ascontiguousarray(mask, dtype=np.uint8), 1, _lib.PL_F_MINSUM, 30.0,
                  flags=_lib.PL_PLAN_GENERIC, device=DEV)
    if crc is not None:
        p.set_crc(*crc)
    return p


def _rows_differing(got, want):
    return np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))


@pytest.mark.parametrize("code", zoo.codes_for("scq"), ids=_ids(zoo.codes_for("scq")))
def test_scq(code):
    from polar_amd import ops
    name, mask, _ = code
    n, fp = len(mask), zoo.frozen_pos(mask)
    q = zoo.scq_rows(name, n)
    plan = _plan(mask)
    for qi in zoo.SCQ_WIDTHS:
        want, st = scq_ref.sc_decode(q, fp, qi, return_stats=True)
        assert qi != 3 or st["g_clamped"] > 0
        got = ops.scq_decode(plan, torch.as_tensor(q, device=DEV), qi, out_dtype=torch.uint8).cpu().numpy()
        bad = _rows_differing(got, want)
        print(f"SCQ {name} q_internal={qi}: rows differing {len(bad)} of {len(q)}")
        assert got.shape == want.shape and np.array_equal(got, want), (name, qi, list(bad[:8]))


@pytest.mark.parametrize("code", zoo.codes_for("scf"), ids=_ids(zoo.codes_for("scf")))
def test_scf(code):
    from polar_amd import ops
    name, mask, _ = code
    n = len(mask)
    fp, crc, x = zoo.scf_rows(name, mask)
    T = zoo.scf_max_flips(n - len(fp))
    ref = scf_ref.scf_decode(x, fp, n, crc, T)
    assert 2 * (ref["attempts"] > 1).sum() > len(x) and (ref["flip_pos"] >= 0).any() and (~ref["crc_ok"]).any()
    bits, ok, pos, att = ops.scf_decode(_plan(mask, crc), torch.as_tensor(x, device=DEV), T, out_dtype=torch.uint8,
                                        return_info=True)
    got = {"bits": bits.cpu().numpy(), "crc_ok": ok.cpu().numpy(), "flip_pos": pos.cpu().numpy(),
           "attempts": att.cpu().numpy()}
    for key in ("bits", "crc_ok", "flip_pos", "attempts"):
        bad = _rows_differing(got[key], ref[key])
        print(f"SCF {name} {key}: rows differing {len(bad)} of {len(x)}")
        assert np.array_equal(got[key], ref[key]), (name, key, list(bad[:8]))


@pytest.mark.parametrize("code", zoo.codes_for("ae"), ids=_ids(zoo.codes_for("ae")))
def test_ae(code):
    from polar_amd import ops
    name, mask, _ = code
    n, fp = len(mask), zoo.frozen_pos(mask)
    x = zoo.ae_rows(name, mask)
    plan = _plan(mask)
    for table in zoo.ae_tables_compared(zoo.ae_table(n)):
        ref = ae_ref.ae_decode(x, fp, n, table)
        want_bits, metric = ae_ref.winner(ref)
        bits, idx, met = ops.ae_decode(plan, torch.as_tensor(x, device=DEV), ops.ae_perm_table(table, DEV),
                                       out_dtype=torch.uint8, return_info=True)
        for key, g, r in (("best_idx", idx.cpu().numpy(), ref["best_idx"]),
                          ("best_metric", met.cpu().numpy().view(np.uint32), metric.astype(np.float32).view(np.uint32)),
                          ("bits", bits.cpu().numpy(), want_bits)):
            bad = _rows_differing(g, r)
            print(f"AE {name} M={len(table)} {key}: rows differing {len(bad)} of {len(x)}")
            assert np.array_equal(g, r), (name, key, list(bad[:8]))
