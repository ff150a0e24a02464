"""Host side of BEST mode on the device (cmb_match_best_device, cmb_best_host_reads, cmb_best_sam_device): the symbols, their
declarations, and the argument checks that need no GPU.  The results are tested in tests/test_gpu_best_device.py."""
import ctypes
import os
import re

import numpy as np

import columba_amd as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMB_ERR_INVALID = -1


def _decl(name):
    hdr = open(os.path.join(ROOT, "include", "columba_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_symbols_and_declarations():
    L = ctypes.CDLL(ca.build_library())
    for name in ("cmb_match_best_device", "cmb_best_host_reads", "cmb_best_sam_device"):
        assert hasattr(L, name) and name in ca.EXPORTS
    assert _decl("cmb_match_best_device") == _decl("cmb_match_best")  # (its arguments are those of cmb_match_best)
    assert _decl("cmb_best_host_reads") == ["const cmb_best* r", "uint8_t* status", "uint32_t* n"]
    assert _decl("cmb_best_sam_device") == ["cmb_best* r", "const cmb_sam_inputs* in", "int unmapped_records", "int xa_tag", "const char** text",
                                            "uint64_t* length", "uint64_t* host_reads"]
    assert hasattr(ca, "match_best_device") and hasattr(ca, "best_sam_device") and hasattr(ca.BestDevice, "sam_device")


def test_invalid_arguments():
    L = ca.lib()
    offs = np.zeros(2, np.uint64)
    seqs = np.zeros(1, np.uint8)
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))  # (never looked into: the checks come first)
    args = (ca._p(seqs), ca._p(offs), 1)
    assert L.cmb_match_best_device(None, None, 0, 95, *args, ctypes.byref(out)) == CMB_ERR_INVALID
    assert L.cmb_match_best_device(fake, None, 0, 95, *args, ctypes.byref(out)) == CMB_ERR_INVALID
    assert L.cmb_match_best_device(fake, fake, 0, 95, *args, None) == CMB_ERR_INVALID  # NULL out
    assert L.cmb_match_best_device(fake, fake, 0, 95, ca._p(seqs), None, 1, ctypes.byref(out)) == CMB_ERR_INVALID
    assert L.cmb_match_best_device(fake, fake, 0, 49, *args, ctypes.byref(out)) == CMB_ERR_INVALID  # identity 49
    assert L.cmb_match_best_device(fake, fake, 0, 101, *args, ctypes.byref(out)) == CMB_ERR_INVALID
    assert b"identity" in L.cmb_last_error()
    assert out.value is None
    n = ctypes.c_uint32(7)
    assert L.cmb_best_host_reads(None, None, ctypes.byref(n)) == CMB_ERR_INVALID
    text, length, host = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    inp = ca.SamInputs()
    assert L.cmb_best_sam_device(None, ctypes.byref(inp), 1, 0, ctypes.byref(text), ctypes.byref(length), ctypes.byref(host)) == CMB_ERR_INVALID
    assert L.cmb_best_sam_device(fake, None, 1, 0, ctypes.byref(text), ctypes.byref(length), ctypes.byref(host)) == CMB_ERR_INVALID
    assert L.cmb_best_sam_device(fake, ctypes.byref(inp), 1, 0, None, ctypes.byref(length), None) == CMB_ERR_INVALID
