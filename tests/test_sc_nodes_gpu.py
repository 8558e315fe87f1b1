"""Both SC kernels on the node zoo: every shortcut node type at every stage of n = 64 ... 2048,
on its fast path and on each of its escapes to the recursion, bit-exact against the oracle.

The codes are polar_amd.build.node_zoo() (pre-built by build(): nothing compiles here); the rows
are tests/golden/sc_nodes_ref.make_batch, whose classes tests/test_sc_nodes_ref.py audits on the
CPU.  An escape is decided by any_lane over the wave, and a wave decodes the 64 / G consecutive
rows cw0 ... cw0 + 64 / G - 1, cw0 = (blockIdx.x * kWaves + wave) * (64 / G) (csrc/sc_static.h
decode(): "const int64_t cw0 = ..."; csrc/sc_kernel.hip has the same line), so the aligned 64-row
runs of one class keep whole waves on the fast path at every G, and a mixed run has one escaping
row at the first, a middle or the last slot of its wave.  The batch ends in a ragged tail.
Min-sum only (see tests/test_sc_nodes_ref.py).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import sc_nodes_ref as ref  # noqa: E402
from polar_amd import build  # noqa: E402

ZOO = build.node_zoo()
IDS = [name for name, _, _ in ZOO]
KINDS = ("specialized", "generic")


@functools.lru_cache(maxsize=1)
def case(i):
    """(batch, oracle bits) of zoo code i, shared by the two kernels (the cases of one code are
    adjacent)."""
    name, mask, planted = ZOO[i]
    b = ref.make_batch(len(mask), mask, planted)
    return b, oracle.sc_decode(b["llr"], np.flatnonzero(mask))


def _where(i, b, row):
    """The planted node and class of a constructed row (for a failure message)."""
    name, mask, planted = ZOO[i]
    k = int(b["row_node"][row])
    if k < 0:
        return "unconstructed row"
    s, q, t = planted[k]
    _, alphas = ref.sc_ref(b["llr"][row:row + 1], mask, [(s, q)])
    run = b["runs"][row // ref.RUN]
    return f"node s={s} q={q} {t}, class {ref.classify(alphas[(s, q)], t)[0]}, {run['kind']} run of {run['cls']}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(ZOO)), ids=IDS)
def test_sc_node_zoo(i, kind):
    import polar_amd
    from polar_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    name, mask, planted = ZOO[i]
    b, want = case(i)
    # specialised: only pre-built code objects (build.py), never a compile on the GPU box
    flags = _lib.PL_PLAN_GENERIC if kind == "generic" else _lib.PL_PLAN_CACHE_ONLY
    plan = _lib.Plan(len(mask), mask, 1, _lib.PL_F_MINSUM, flags=flags)
    assert plan.kernel()[0] == kind, plan.kernel()
    x = torch.from_numpy(b["llr"]).cuda()
    for dtype in (torch.float32, torch.uint8):
        got = polar_amd.ops.sc_decode(plan, x, out_dtype=dtype).cpu().numpy()
        assert got.shape == want.shape
        bad = np.flatnonzero((got != want.astype(got.dtype)).any(axis=1))
        if len(bad):
            pytest.fail(f"{dtype}: {len(bad)} of {len(got)} rows differ, first row {int(bad[0])}: "
                        + _where(i, b, int(bad[0])))
