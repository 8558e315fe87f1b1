"""The node zoo (polar_amd.build.node_zoo) and the rows tests/test_sc_nodes_gpu.py decodes, checked
on the CPU: what keeps the GPU test honest.

  * classifier: every planted node has its type in the NT table of the specialised kernel's
    source, below general ancestors (so its shortcut is the code that runs)
  * the instrumented restatement (tests/golden/sc_nodes_ref.py, no shortcuts) equals the oracle
  * the row constructor sets a node's input vector exactly
  * coverage audit: every class of every planted node -- fast path and each escape -- is hit by an
    aligned 64-row run (whole waves on the fast path at every lane-group width) and by a mixed run
Min-sum only: exact-f codes compile the rate-1 and SPC shortcuts out and their f is not
transparent to the constructor (f(v, BIG) != v); the ulp tests (test_exactf_ulp*.py) cover them.

Declared unreachable, and nothing else: an SPC left child cannot see a minimum above llr_max (its
input is an f output; it gets the minimum equal to llr_max instead), and two size-2 shortcut
nodes cannot be siblings under a general parent (together they are a size-4 shortcut node), so
size-2 nodes sit next to a filler and are not planted on both sides for every type.  Rate-0 nodes
and REP nodes below size 8 have a single class, so no run of theirs can mix.
"""
import os
import re
import sys

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import sc_nodes_ref as ref  # noqa: E402
from polar_amd import build  # noqa: E402

ZOO = build.node_zoo()
IDS = [name for name, _, _ in ZOO]
TYPE_ID = {"R0": 0, "R1": 1, "REP": 2, "SPC": 3, "GEN": 4}  # csrc/sc_static.h


@pytest.fixture(scope="module", params=range(len(ZOO)), ids=IDS)
def zoo(request):
    """(code, batch, bits, alphas) of one zoo code: the restatement runs once per code."""
    name, mask, planted = ZOO[request.param]
    b = ref.make_batch(len(mask), mask, planted)
    bits, alphas = ref.sc_ref(b["llr"], mask, [(s, q) for s, q, _ in planted])
    return ZOO[request.param], b, bits, alphas


def test_zoo_scope():
    """Every type at every stage 1 ... log_n - 2, on both sides from stage 2 up; every root half
    once as REP, SPC and rate-1 next to a general half; at most 64 codes."""
    assert len(ZOO) <= 64 and len(set(IDS)) == len(ZOO)
    for n in build.ZOO_NS:
        log_n = n.bit_length() - 1
        seen = set()
        for name, mask, planted in ZOO:
            if len(mask) == n:
                seen |= {(s, q & 1, t) for s, q, t in planted}
        for t in ("R0", "R1", "REP", "SPC"):
            for s in range(2, log_n - 1):
                assert (s, 0, t) in seen and (s, 1, t) in seen, (n, s, t)
        for t in ("R0", "R1", "REP"):  # a size-2 SPC is a size-2 REP (same mask)
            assert {(1, 0, t), (1, 1, t)} & seen, (n, t)
        for t in ("R1", "REP", "SPC"):
            assert (log_n - 1, 0, t) in seen and (log_n - 1, 1, t) in seen, (n, t)


@pytest.mark.parametrize("i", range(len(ZOO)), ids=IDS)
def test_classifier(i):
    """The NT table the specialised kernel is compiled with: each planted node has its type at
    heap index (n >> s) + q and every ancestor is GEN.  The tuned_wide codes (n = 256 ... 1024)
    decode their lane-level SPC nodes (s <= log_n - 6) by the recursion: those read GEN; n = 2048
    keeps them SPC (the DPP shortcut of lnode)."""
    from polar_amd import _lib
    name, mask, planted = ZOO[i]
    n = len(mask)
    log_n = n.bit_length() - 1
    src, _ = _lib.sc_source(n, mask, 0)
    if isinstance(src, bytes):
        src = src.decode()
    m = re.search(r"NT\[(\d+)\] = \{([0-9,]+)\}", src)
    nt = [int(v) for v in m.group(2).split(",")]
    assert int(m.group(1)) == len(nt) == 2 * n
    lane_spc = 0
    for s, q, t in planted:
        want = t
        if t == "SPC" and 8 <= log_n <= 10 and s <= log_n - 6:
            want = "GEN"
        lane_spc += t == "SPC" and log_n == 11 and s <= 4
        assert nt[(n >> s) + q] == TYPE_ID[want], (s, q, t)
        for up in range(s + 1, log_n + 1):
            assert nt[(n >> up) + (q >> (up - s))] == TYPE_ID["GEN"], (s, q, t, up)
    if log_n == 11 and any(t == "SPC" and s <= 4 for s, _, t in planted):
        assert lane_spc > 0


def test_reference_equals_oracle(zoo):
    (name, mask, planted), b, bits, _ = zoo
    want = oracle.sc_decode(b["llr"], np.flatnonzero(mask))
    bad = np.flatnonzero((bits != want).any(axis=1))
    assert len(bad) == 0, (len(bad), int(bad[0]), int(b["row_node"][bad[0]]))


def test_constructor_is_exact(zoo):
    """The restatement reports, at the planted node, exactly the alpha each run was built from."""
    (name, mask, planted), b, _, alphas = zoo
    for run, want in zip(b["runs"], b["alpha"]):
        s, q, t = planted[run["node"]]
        got = alphas[(s, q)][run["start"]: run["start"] + ref.RUN]
        assert got.dtype == np.float32 and np.array_equal(got, want), (s, q, t, run["cls"], run["kind"])


def test_coverage_audit(zoo):
    """Classes as the restatement sees them (not as the constructor meant them): every class of
    every planted node fills one aligned run, and every escape class is the single such row of a
    mixed run whose other 63 rows take the fast path, at the run's recorded slot."""
    (name, mask, planted), b, _, alphas = zoo
    hit = set()
    for run in b["runs"]:
        s, q, t = planted[run["node"]]
        a = alphas[(s, q)][run["start"]: run["start"] + ref.RUN]
        cls = ref.classify(a, t)
        esc = ref.escapes_of(t, 1 << s)
        if run["kind"] == "aligned":
            assert (cls == run["cls"]).all(), (s, q, t, run["cls"], sorted(set(cls)))
            if run["cls"] == "odd_clip":  # at llr_max on a left child, strictly above on a right one
                mn = np.abs(a).min(axis=1)
                assert (mn == ref.LLR_MAX).all() if q & 1 == 0 else (mn > ref.LLR_MAX).all(), (s, q)
        else:
            others = np.delete(cls, run["slot"])
            assert cls[run["slot"]] == run["cls"] and not set(others) & set(esc), (s, q, t, run["cls"])
            hit |= {(run["node"], c, "mixed") for c in others}
        hit.add((run["node"], run["cls"], run["kind"]))
    for k, (s, q, t) in enumerate(planted):
        for c in ref.classes_of(t, 1 << s):
            assert (k, c, "aligned") in hit, (s, q, t, c)
            if ref.escapes_of(t, 1 << s):
                assert (k, c, "mixed") in hit, (s, q, t, c)
    assert len(b["llr"]) % ref.RUN != 0  # ragged tail


def test_every_escape_at_every_slot():
    """Over the codes of one n, every escape class of every type sits at the first, a middle and
    the last slot of a mixed run."""
    for n in build.ZOO_NS:
        seen = set()
        for name, mask, planted in ZOO:
            if len(mask) != n:
                continue
            for s, q, typ in planted:
                seen |= {(typ, c, slot) for c, kind, slot in ref.run_plan(s, q, typ) if kind == "mixed"}
        for t, c in (("SPC", "zero"), ("SPC", "odd_tie"), ("SPC", "odd_clip"), ("R1", "zero"), ("REP", "order")):
            assert {(t, c, s) for s in ref.SLOTS} <= seen, (n, t, c)


def test_rep_order_rows():
    """The order-sensitive REP rows: both sequential sums disagree in sign with SC's pairwise sum,
    64 rows per size, all within a left child's range."""
    for s in range(3, 11):
        a = ref.rep_order_rows(1 << s)
        assert a.shape == (ref.RUN, 1 << s) and (np.abs(a) < ref.LLR_MAX).all()
        pair, seq, rev = ref.rep_sums(a)
        assert (((seq > 0) == (rev > 0)) & ((seq > 0) != (pair > 0))).all()
        assert (pair != 0).all() and (seq != 0).all() and (rev != 0).all()


def _wrong_rule(typ):
    """Shortcut rules that are subtly wrong: REP summed left to right instead of in SC's pairwise
    order; rate-1 and SPC (Wagner flip at the first minimum) without their escapes."""
    def rep(a):
        return np.repeat(ref.rep_sums(a)[1][:, None] <= 0, a.shape[1], axis=1)

    def r1(a):
        return a <= 0

    def spc(a):
        b = a <= 0
        odd = (b.sum(axis=1) & 1) == 1
        b[np.flatnonzero(odd), np.abs(a).argmin(axis=1)[odd]] ^= True
        return b
    return {"REP": rep, "R1": r1, "SPC": spc}[typ]


def test_rows_catch_wrong_rules(zoo):
    """The rows are sharp enough: with the wrong rules above at every planted node at once (a
    constructed row's alpha at its node depends on no decision elsewhere), the information bits of
    the node differ from the recursion's in every row of REP's order run, in some rows of the zero run
    of rate-1 and of the tie and clip runs of SPC, and in no row of a fast-path run."""
    (name, mask, planted), b, bits, _ = zoo
    rules = {(s, q): _wrong_rule(t) for s, q, t in planted if t != "R0" and not (t == "REP" and s < 3)}
    wrong, _ = ref.sc_ref(b["llr"], mask, rules=rules)
    info = np.cumsum(1 - np.asarray(mask, np.int64)) - 1  # position -> information index
    for run in b["runs"]:
        s, q, t = planted[run["node"]]
        if (s, q) not in rules or run["kind"] != "aligned":
            continue
        pos = np.arange(q << s, (q + 1) << s)
        cols = info[pos[mask[pos] == 0]]
        rows = slice(run["start"], run["start"] + ref.RUN)
        diff = (wrong[rows][:, cols] != bits[rows][:, cols]).any(axis=1)
        if run["cls"] == "order":
            assert diff.all(), (s, q, t, run["cls"], int(diff.sum()))
        elif (t, run["cls"]) == ("SPC", "zero"):
            pass  # a single zero is a unique minimum: the Wagner flip agrees with the recursion there
        elif run["cls"] in ref.escapes_of(t, 1 << s):
            assert diff.any(), (s, q, t, run["cls"])
        else:
            assert not diff.any(), (s, q, t, run["cls"], int(diff.sum()))
