"""cmb_pair_sam_device_classes and cmb_move_pair_sam_device (include/columba_amd.h): the symbols exist and their argument checks come
before any work, so they answer on a box without a GPU.  What they compute is tests/test_gpu_pair_classes_device.py's."""
import ctypes as C

import numpy as np
import pytest

import columba_amd as ca

ENTRIES = ("cmb_pair_sam_device_classes", "cmb_move_pair_sam_device")
CMB_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L():
    ca.build_library()
    return ca.lib()


def _inputs():
    """packed inputs of one read that pass every check, and what keeps them alive"""
    seqs = np.frombuffer(b"ACGT", np.uint8).copy()
    ids = np.frombuffer(b"@r", np.uint8).copy()
    offs = np.array([0, 2], np.uint64)
    names = np.frombuffer(b"s", np.uint8).copy()
    noffs = np.array([0, 1], np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return ca.SamInputs(p(seqs), p(ids), p(offs), None, None, p(names), p(noffs), 1), (seqs, ids, offs, names, noffs)


def _call(L, name, m1, m2, prm, in1, in2, classes, text, n):
    return getattr(L, name)(m1, m2, prm, in1, in2, classes, text, n, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_exported(L, name):
    assert name in ca.EXPORTS
    assert hasattr(C.CDLL(ca.build_library()), name)


def test_class_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "columba_amd.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define CMB_PAIR_CLASS_(\w+) (\d+)u", hdr)}
    assert got == {"ONE_UNMAPPED": 1, "DISCORDANT": 2, "UNPAIRED": 4, "OVER_LIMIT": 8, "ALL": 15}
    assert (ca.PAIR_CLASS_ONE_UNMAPPED, ca.PAIR_CLASS_DISCORDANT, ca.PAIR_CLASS_UNPAIRED, ca.PAIR_CLASS_OVER_LIMIT, ca.PAIR_CLASS_ALL) == (1, 2, 4, 8, 15)
    assert [f for f, _ in ca.PairClassStats._fields_] == list(ca.PAIR_CLASS_STATS) and C.sizeof(ca.PairClassStats) == 72


@pytest.mark.parametrize("name", ENTRIES)
def test_null_arguments_are_invalid(L, name):
    inp, keep = _inputs()
    prm = ca.PairParams(ca.ORIENTATION_FR, 500, 0, 1, 1)
    text, n = C.c_void_p(), C.c_uint64()
    m1, m2 = C.c_void_p(8), C.c_void_p(16)  # (never looked at: every call below fails a check that comes first)
    good = dict(m1=m1, m2=m2, prm=C.byref(prm), in1=C.byref(inp), in2=C.byref(inp), classes=0, text=C.byref(text), n=C.byref(n))
    for missing in ("m1", "m2", "prm", "in1", "in2", "text", "n"):
        args = dict(good)
        args[missing] = None
        assert _call(L, name, **args) == CMB_ERR_INVALID, missing
        assert L.cmb_last_error()
    assert _call(L, name, **dict(good, m2=m1)) == CMB_ERR_INVALID  # one batch for both mates
    bad = ca.PairParams(3, 500, 0, 1, 1)
    assert _call(L, name, **dict(good, prm=C.byref(bad))) == CMB_ERR_INVALID  # no such orientation


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("classes", [16, 17, 1 << 31])
def test_unknown_class_bits_are_invalid(L, name, classes):
    inp, keep = _inputs()
    prm = ca.PairParams(ca.ORIENTATION_FR, 500, 0, 1, 1)
    text, n = C.c_void_p(), C.c_uint64()
    rc = _call(L, name, C.c_void_p(8), C.c_void_p(16), C.byref(prm), C.byref(inp), C.byref(inp), classes, C.byref(text), C.byref(n))
    assert rc == CMB_ERR_INVALID
    assert b"CMB_PAIR_CLASS" in L.cmb_last_error()
