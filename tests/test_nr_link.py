"""CPU-side checks of the fused 5G NR link (tests/test_nr_link_gpu.py runs it): the CLI switch, the two
new C-ABI symbols, the FusedAWGN5G argument checks that need no GPU, and the packed-count rule."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_parse_5g_switch_and_old_defaults():
    from polar_amd import cli
    c = cli.parse(["--code", "5g", "--hybrid_sc", "--k", "500", "--n", "1024"])
    assert c.code == "5g" and c.hybrid_sc is True and (c.k, c.n) == (500, 1024)
    d = cli.parse([])
    assert d.code == "plain" and d.hybrid_sc is False
    assert (d.k, d.n, d.algos, d.bs, d.snr_end, d.mc_iter, d.list_size, d.llr_device, d.llr_producer, d.seed) == \
        (32, 64, ["scl"], 3, 5, 10, 8, "cuda", "fused", 42)
    with pytest.raises(SystemExit):
        cli.parse(["--code", "lte"])


def test_new_symbols_declared_and_bound():
    from polar_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polar_mi355x.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in (("pl_nr_awgn_qpsk_llr", 19), ("pl_count_errors_packed", 8)):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(L, name).argtypes) == nargs


def test_count_errors_packed_rejects_bad_arguments_without_gpu():
    # argument validation happens before any HIP call
    import ctypes
    from polar_amd import _lib
    L = _lib.lib()
    counts = (ctypes.c_int64 * 2)()
    assert L.pl_count_errors_packed(None, _lib.PL_OUT_F32, 4, 8, 9, None, counts, None) == _lib.PL_EINVAL  # k_cmp > row_len
    assert b"k_cmp" in L.pl_last_error_string()
    assert L.pl_count_errors_packed(None, 7, 4, 8, 8, None, counts, None) == _lib.PL_EINVAL  # unknown kind
    assert L.pl_count_errors_packed(None, _lib.PL_OUT_U8, 4, 8, 8, None, None, None) == _lib.PL_EINVAL  # no counters
    assert L.pl_count_errors_packed(None, _lib.PL_OUT_U8, 0, 8, 8, None, counts, None) == _lib.PL_OK  # no rows


def test_fused_awgn5g_argument_checks():
    from polar_amd import channel
    from polar_amd.polar5g import Polar5GDecoder, Polar5GEncoder
    with contextlib.redirect_stdout(io.StringIO()):
        enc, other = Polar5GEncoder(64, 128), Polar5GEncoder(64, 128)
        down = Polar5GEncoder(64, 128, channel_type="downlink")
        dec, dec_other, dec_down = Polar5GDecoder(enc), Polar5GDecoder(other), Polar5GDecoder(down)
    with pytest.raises(ValueError, match="downlink"):
        channel.FusedAWGN5G(down, dec_down, device="cuda:0")
    with pytest.raises(ValueError, match="built on enc"):
        channel.FusedAWGN5G(enc, dec_other, device="cuda:0")
    with pytest.raises(ValueError):
        channel.FusedAWGN5G(enc, None, device="cuda:0")
    for row0 in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="row0"):
            channel.FusedAWGN5G(enc, dec, device="cuda:0", row0=row0)
    model = channel.FusedAWGN5G(enc, dec, device="cuda:0", seed=9, row0=2 ** 32 - 8)
    assert model.k == 64 and model.coderate == 0.5 and model.keyed_streams
    # the draw bounds of FusedAWGN, checked before anything is launched
    for stream in ((0, 2 ** 32), (0, -1), (2 ** 31, 0), (-1, 0)):
        with pytest.raises(ValueError):
            model.forward(8, 1.0, stream=stream)
    with pytest.raises(ValueError, match="2\\^32"):
        model.forward(9, 1.0, stream=(0, 0))  # row0 + batch_size past 2^32
    assert model.key() == 9
    model.next_epoch()
    assert model.key() == channel.splitmix64(9 + 0x9E3779B97F4A7C15)


def _count_packed(bits, ref_words, k_cmp):
    """numpy restatement of pl_count_errors_packed's rule."""
    i = np.arange(k_cmp)
    want = (ref_words[:, i >> 5].astype(np.uint32) >> (i & 31).astype(np.uint32)) & 1
    diff = (np.asarray(bits)[:, :k_cmp] != 0) != (want != 0)
    return [int(diff.sum()), int(diff.any(axis=1).sum())]


def test_packed_count_rule_hand_cases():
    # bit m of a row is bit m % 32 of word m // 32
    ref = np.array([[0b1011, 0], [0xFFFFFFFF, 0b1], [0, 0]], dtype=np.uint32)
    bits = np.zeros((3, 40), dtype=np.float32)
    bits[0, [0, 1, 3]] = 1      # row 0 equals its reference
    bits[1, :33] = 1            # row 1 equals its reference ...
    bits[1, 5] = 0              # ... but for bit 5
    bits[2, 34] = 1             # row 2: one wrong bit, at column 34
    assert _count_packed(bits, ref, 40) == [2, 2]
    assert _count_packed(bits, ref, 34) == [1, 1]   # column 34 is past k_cmp: not counted
    assert _count_packed(bits, ref, 5) == [0, 0]
    assert _count_packed(bits.astype(np.uint8) * 7, ref, 40) == [2, 2]  # bytes: nonzero = 1
    from polar_amd import ops
    import torch
    packed = ops.pack_bits(torch.from_numpy(bits)).numpy().view(np.uint32)
    assert _count_packed(bits, packed, 40) == [0, 0]  # pack_bits is this layout
