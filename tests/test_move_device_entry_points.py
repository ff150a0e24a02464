"""The device SAM / BEST entry points of the b-move backend refuse null handles before they touch a device, and the C++ adapter
that calls them still compiles on its own.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import columba_amd as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handles_are_refused():
    L = ca.lib()
    assert L.cmb_move_batch_keep_device_lists(None, 1) == ca.CMB_ERR_INVALID
    assert b"null" in L.cmb_last_error()
    ids, names = ca.pack_fields(["@r0"]), ca.pack_fields(["chr1"])
    seqs = np.frombuffer(b"ACGT", np.uint8)
    inp = ca.SamInputs(ca._p(seqs), ca._p(ids[0]), ca._p(ids[1]), None, None, ca._p(names[0]), ca._p(names[1]), 1)
    text, n, host = C.c_void_p(), C.c_uint64(), C.c_uint64()
    assert L.cmb_move_batch_sam_device(None, C.byref(inp), 1, 0, C.byref(text), C.byref(n), C.byref(host)) == ca.CMB_ERR_INVALID
    offs = np.array([0, 4], np.uint64)
    h = C.c_void_p()
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    assert L.cmb_move_match_best_device(None, st.h, 0, 95, 8, ca._p(seqs), ca._p(offs), 1, C.byref(h)) == ca.CMB_ERR_INVALID
    assert not h.value


def test_bmove_adapter_is_plain_cpp():
    """as test_cabi_exports.test_header_is_plain_c compiles the other adapters"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = '#include "columba_amd_bmove.hpp"\nint main() { return 0; }\n'
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "include"), "-"],
                   input=src, text=True, check=True)
