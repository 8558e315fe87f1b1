"""Hybrid SC / SC-list decoding and CRC status: what can be checked without a GPU -- the module
options construct (no plan is built before the first forward) and the C header, the library and
the ctypes binding agree on the new entry points."""
import contextlib
import io
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polar_mi355x.h")
NEW_SYMBOLS = ("pl_hybrid_workspace_size", "pl_hybrid_decode", "pl_crc_status")


def test_mysn_scl_dec_hybrid_constructs():
    import polar_amd
    from polar_amd import mysn
    fp = polar_amd.reference_frozen_pos(32, 64)
    dec = mysn.SCL_Dec(fp, 64, crc_degree="CRC11", use_hybrid_sc=True)
    assert dec._use_hybrid_sc is True and dec.msg_pm is None and dec.last_list_rows == 0
    assert mysn.SCL_Dec(fp, 64, crc_degree="CRC11")._use_hybrid_sc is False
    mysn.SCL_Dec(fp, 64, crc_degree="CRC11", use_hybrid_sc=True, return_crc_status=True)
    with pytest.raises(ValueError, match="Hybrid SC requires an outer CRC."):
        mysn.SCL_Dec(fp, 64, use_hybrid_sc=True)
    with pytest.raises(ValueError):  # as before: a CRC status needs a CRC
        mysn.SCL_Dec(fp, 64, return_crc_status=True)


def test_polar5g_decoder_hybrid_option():
    from polar_amd import mysn, polar5g
    with contextlib.redirect_stdout(io.StringIO()):
        enc = polar5g.Polar5GEncoder(32, 64)
        dec = polar5g.Polar5GDecoder(enc, dec_type="SCL", hybrid_sc=True)
        assert isinstance(dec.polar_dec, mysn.SCL_Dec) and dec.polar_dec._use_hybrid_sc is True
        assert polar5g.Polar5GDecoder(enc, dec_type="SCL").polar_dec._use_hybrid_sc is False
        with pytest.raises(ValueError):
            polar5g.Polar5GDecoder(enc, dec_type="SC", hybrid_sc=True)
        with pytest.raises(NotImplementedError):  # the reference cannot construct it either
            polar5g.Polar5GDecoder(enc, dec_type="hybSCL", hybrid_sc=True)


def test_header_library_and_binding_agree_on_the_new_symbols():
    from polar_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pl_[a-z_0-9]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (run __graft_entry__.build())")
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/polar_mi355x.h"
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), f"{name} not exported by the library"
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    # the prototype the binding mirrors: two plans, ..., a HOST int64 count, workspace, stream
    proto = re.search(r"int pl_hybrid_decode\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(L.pl_hybrid_decode.argtypes) == 12
    assert len(L.pl_hybrid_workspace_size.argtypes) == 3 and len(L.pl_crc_status.argtypes) == 6


def test_hybrid_argument_checks_before_any_device_call():
    """NULL plans are refused before the library touches HIP (there is no GPU here)."""
    import ctypes
    from polar_amd import _lib
    L = _lib.lib()
    n = ctypes.c_int64(0)
    assert L.pl_hybrid_workspace_size(None, None, 16) == 0
    assert L.pl_hybrid_decode(None, None, None, 0, None, 0, None, None, ctypes.byref(n), None, 0, None) == _lib.PL_EINVAL
    assert L.pl_crc_status(None, None, 0, 0, None, None) == _lib.PL_EINVAL
    with pytest.raises(_lib.PolarLibError) as e:
        _lib.check(_lib.PL_EINVAL, "pl_hybrid_decode")
    assert e.value.code == _lib.PL_EINVAL and isinstance(e.value, ValueError)
