"""The rate-0 zoo of the SC-Flip, AE and fixed-point SC register trees (tests/golden/tree_zoo_ref.py), audited
on the CPU: what keeps tests/test_tree_zoo_gpu.py from passing by construction.

  * scope: the placements the three trees have a code path for are all planted
  * the switches that model a wrong decoder (a falsely taken rate-0 skip, a g computed with bl = 0) do nothing
    when they name a node that really is rate-0 / whose left child really is, and the switched restatements
    agree with each other
  * sensitivity audit: for every placement of every code, each wrong decoder of tree_zoo_ref.wrong_decoders
    changes what the GPU test compares, in at least one row of the very batch the GPU test decodes.  The count
    of sensitive rows per placement is printed; none may be zero.
    SCQ is asserted at q_internal = 8 (at 3 some g see x = 0); AE over what its GPU test compares: the whole
    table and candidate 0 alone.
  * the SC-Flip rows fail attempt 0 in their majority (the flip kernel's tree runs), some are rescued, some never
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import ae_ref  # noqa: E402
import scf_ref  # noqa: E402
import scq_ref  # noqa: E402
import tree_zoo_ref as zoo  # noqa: E402

from polar_amd import build  # noqa: E402

ALL = zoo.all_codes()


def _ids(codes):
    return [c[0] for c in codes]


def test_scope():
    names = _ids(ALL)
    assert len(set(names)) == len(names)
    for name, mask, placed in ALL:
        n = len(mask)
        assert placed, name
        for s, q, sib in placed:
            m = 1 << s
            assert mask[q * m: (q + 1) * m].all(), (name, s, q)
            other = mask[(q ^ 1) * m: ((q ^ 1) + 1) * m]
            assert not other.all() and build.node_type(other) == sib, (name, s, q, sib)
    # small codes: every stage, first / middle / last parent, both sides, a repetition sibling
    for n in zoo.SMALL_NS:
        log_n = n.bit_length() - 1
        seen = {(s, q) for name, mask, placed in zoo.small_codes() if len(mask) == n for s, q, sib in placed
                if sib == "REP"}
        for s in range(1, log_n):
            parents = n >> (s + 1)
            for par in (0, parents // 2, parents - 1):
                assert (s, 2 * par) in seen and (s, 2 * par + 1) in seen, (n, s, par)
    # n >= 64: both sides at every stage 1 ... log2 n - 2; a rate-0 root half on each side; beside a repetition
    # node on both sides at the stage log2 G of `bottom` and at every stage below it (`inl`); the first and the
    # last used flag word
    for n in zoo.BIG_NS:
        log_n, log_g = n.bit_length() - 1, max(n.bit_length() - 8, 0)
        seen = {(s, q & 1, sib) for name, mask, placed in ALL if len(mask) == n for s, q, sib in placed}
        bits = {n - (n >> (s - 1)) + q for name, mask, placed in ALL if len(mask) == n for s, q, sib in placed}
        for s in range(1, log_n - 1):
            assert {side for t, side, _ in seen if t == s} == {0, 1}, (n, s)
        assert (log_n - 1, 0, "GEN") in seen and (log_n - 1, 1, "GEN") in seen, n
        for s in range(1, max(log_g, 1) + 1):
            assert (s, 0, "REP") in seen and (s, 1, "REP") in seen, (n, s)
        assert min(bits) // 32 == 0 and max(bits) // 32 == (n - 2) // 32, (n, min(bits), max(bits))
    assert all(len(c[1]) <= zoo.SCF_NMAX for c in zoo.codes_for("scf") + zoo.codes_for("ae"))
    assert {len(c[1]) for c in zoo.codes_for("scq")} == set(zoo.SMALL_NS + zoo.BIG_NS)


def test_switches_are_inert_on_real_rate0_nodes_and_agree_across_restatements():
    """Naming the planted rate-0 node itself, or a parent whose left child is rate-0, changes nothing; on integer
    inputs that never saturate the float and the integer restatement are the same decoder, switched or not."""
    for name, mask, placed in (zoo.small_codes()[5], zoo.small_codes()[-3], zoo.extra_codes()[0]):
        n, fp = len(mask), zoo.frozen_pos(mask)
        info = np.flatnonzero(mask == 0)
        q8 = np.random.default_rng(n).integers(-1, 2, size=(40, n)).astype(np.int8)  # |sums| <= n <= 127
        none = np.full(40, -1)
        plain = scq_ref.sc_decode(q8, fp, 8)
        assert np.array_equal(plain, scf_ref.sc_flip(q8.astype(np.float32), fp, n, none)[0][:, info])
        for s, q, _ in placed:
            assert np.array_equal(plain, scq_ref.sc_decode(q8, fp, 8, wrong={"false_r0": (s, q)}))
            if q & 1 == 0:
                assert np.array_equal(plain, scq_ref.sc_decode(q8, fp, 8, wrong={"bl0": (s + 1, q >> 1)}))
            for what, sw in zoo.wrong_decoders(mask, (s, q, _)):
                a = scq_ref.sc_decode(q8, fp, 8, wrong=sw)
                b = scf_ref.sc_flip(q8.astype(np.float32), fp, n, none, **sw)[0][:, info]
                assert np.array_equal(a, b), (name, what, sw)


def _report(tag, name, counts):
    print(f"{tag} {name}: sensitive rows " + ", ".join(f"s{s}q{q} {what} {c}" for (s, q, what), c in counts.items()))
    for key, c in counts.items():
        assert c > 0, (tag, name, key)


@pytest.mark.parametrize("code", zoo.codes_for("scq"), ids=_ids(zoo.codes_for("scq")))
def test_scq_rows_are_sensitive(code):
    name, mask, placed = code
    n, fp = len(mask), zoo.frozen_pos(mask)
    q8 = zoo.scq_rows(name, n)
    assert q8.shape[0] <= 67 and (q8 == -128).any()
    for qi in zoo.SCQ_WIDTHS:
        want, st = scq_ref.sc_decode(q8, fp, qi, return_stats=True)
        assert qi != 3 or st["g_clamped"] > 0
        counts = {}
        for pl in placed:
            for what, sw in zoo.wrong_decoders(mask, pl):
                got = scq_ref.sc_decode(q8, fp, qi, wrong=sw)
                counts[(pl[0], pl[1], what)] = int((got != want).any(axis=1).sum())
        # at q_internal = 3 a long chain of f ends at 0 on uniform inputs and a g with x = 0 does not see bl: the
        # counts of that width are printed, q_internal = 8 carries every placement
        if qi == 8:
            _report("SCQ q_internal=8", name, counts)
        else:
            print(f"SCQ q_internal={qi} {name}: " + ", ".join(f"s{s}q{q} {what} {c}" for (s, q, what), c in counts.items()))


def _scf_differs(a, b):
    return ((a["bits"] != b["bits"]).any(axis=1) | (a["crc_ok"] != b["crc_ok"]) | (a["flip_pos"] != b["flip_pos"])
            | (a["attempts"] != b["attempts"]))


@pytest.mark.parametrize("code", zoo.codes_for("scf"), ids=_ids(zoo.codes_for("scf")))
def test_scf_rows_are_sensitive_and_of_every_class(code):
    """The switch is applied to the flip attempts alone: attempt 0 and the candidate list come from other kernels."""
    name, mask, placed = code
    n = len(mask)
    fp, crc, x = zoo.scf_rows(name, mask)
    k = n - len(fp)
    T = zoo.scf_max_flips(k)
    assert x.shape[0] <= 67 and crc == zoo.scf_crc(k)
    ref = scf_ref.scf_decode(x, fp, n, crc, T)
    fail0, rescued, never = int((ref["attempts"] > 1).sum()), int((ref["flip_pos"] >= 0).sum()), int((~ref["crc_ok"]).sum())
    print(f"SCF {name}: k {k}, CRC degree {crc[0]}, T {T}: fail attempt 0 {fail0} of {len(x)}, rescued {rescued}, never {never}")
    assert 2 * fail0 > len(x) and rescued > 0 and never > 0
    counts = {}
    for pl in placed:
        for what, sw in zoo.wrong_decoders(mask, pl):
            counts[(pl[0], pl[1], what)] = int(_scf_differs(scf_ref.scf_decode(x, fp, n, crc, T, flip_tree=sw), ref).sum())
    _report("SCF", name, counts)


@pytest.mark.parametrize("code", zoo.codes_for("ae"), ids=_ids(zoo.codes_for("ae")))
def test_ae_rows_are_sensitive(code):
    """Over what the GPU test compares: the winner of the whole table, and candidate 0 (the identity) alone, where
    the tree's own decode of every row shows."""
    name, mask, placed = code
    n, fp = len(mask), zoo.frozen_pos(mask)
    x, table = zoo.ae_rows(name, mask), zoo.ae_table(n)
    assert x.shape[0] <= 67 and np.array_equal(x * 8, np.rint(x * 8)) and np.abs(x).max() <= 16

    def outputs(tree=None):
        out = []
        for t in zoo.ae_tables_compared(table):
            r = ae_ref.ae_decode(x, fp, n, t, tree=tree)
            assert r["metric"].max() < 2 ** 15  # the grid's fp32 sums are exact
            out.append(ae_ref.winner(r) + (r["best_idx"],))
        return out

    ref = outputs()
    counts = {}
    for pl in placed:
        for what, sw in zoo.wrong_decoders(mask, pl):
            rows = np.zeros(len(x), bool)
            for (gb, gm, gi), (rb, rm, ri) in zip(outputs(sw), ref):
                rows |= (gb != rb).any(axis=1) | (gm != rm) | (gi != ri)
            counts[(pl[0], pl[1], what)] = int(rows.sum())
    _report("AE", name, counts)


def test_ae_tables():
    from polar_amd import automorphism
    for n in zoo.SMALL_NS + tuple(v for v in zoo.BIG_NS if v <= zoo.AE_NMAX):
        t = zoo.ae_table(n)
        g = max(1, n // 128)
        assert t.shape == (zoo.ae_num_perms(n), n) and t.shape[0] == min(2 * (64 // g) + 1, 64)
        assert np.array_equal(t[0], np.arange(n)) and all(automorphism.is_permutation(pi, n) for pi in t)
        assert len({row.tobytes() for row in t}) == len(t) or n == 4
        log_n = n.bit_length() - 1
        # the last one is no bit-index permutation (n >= 8: a random permutation is one with probability ~ 0)
        lin = all(t[-1][1 << b] & (t[-1][1 << b] - 1) == 0 for b in range(log_n))
        assert n <= 4 or not lin
