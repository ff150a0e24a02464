"""Host side of the device SAM path (cmb_batch_sam_device): the packing of identifiers, qualities and sequence names, the
ctypes view of cmb_sam_inputs, the symbol.  No GPU here; the text itself is tested in tests/test_gpu_sam_device.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import columba_amd as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_fields_round_trip():
    fields = [b"@read0/1 some description", b"", b">x", b"@", b"IIII#!~", b"", b"chr1"]
    buf, offs = ca.pack_fields(fields)
    assert buf.dtype == np.uint8 and offs.dtype == np.uint64 and offs.shape[0] == len(fields) + 1
    assert offs[0] == 0 and int(offs[-1]) == sum(len(f) for f in fields) and np.all(np.diff(offs.astype(np.int64)) >= 0)
    assert ca.unpack_fields(buf, offs) == fields
    # str entries are encoded as ASCII; the bytes are the same
    sbuf, soffs = ca.pack_fields([f.decode() for f in fields])
    assert np.array_equal(soffs, offs) and ca.unpack_fields(sbuf, soffs) == fields
    # a packed pair passes through
    pbuf, poffs = ca.pack_fields((buf, offs))
    assert np.array_equal(pbuf, buf) and np.array_equal(poffs, offs)


def test_pack_fields_empty_inputs():
    buf, offs = ca.pack_fields([])
    assert offs.tolist() == [0] and buf.shape[0] >= 1  # (a valid pointer for the C side)
    buf, offs = ca.pack_fields([b"", "", b""])
    assert offs.tolist() == [0, 0, 0, 0] and ca.unpack_fields(buf, offs) == [b"", b"", b""]


def test_pack_fields_refuses_what_is_not_ascii():
    with pytest.raises(ValueError):
        ca.pack_fields(["réad"])
    with pytest.raises(ValueError):
        ca.pack_fields([b"ok", b"\xc3\xa9"])


def test_pack_fields_many_entries_without_per_entry_objects():
    rng = np.random.default_rng(3)
    fields = [bytes(rng.integers(33, 127, int(n), dtype=np.uint8)) for n in rng.integers(0, 40, 5000)]
    buf, offs = ca.pack_fields(fields)
    assert ca.unpack_fields(buf, offs) == fields


def test_inputs_struct_matches_the_header():
    """cmb_sam_inputs as ctypes sees it has the header's members in the header's order"""
    hdr = open(os.path.join(ROOT, "include", "columba_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} cmb_sam_inputs;", hdr)
    assert m, "cmb_sam_inputs is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    members = re.findall(r"(\w+)\s*;", body)
    assert members == [f[0] for f in ca.SamInputs._fields_]
    assert ctypes.sizeof(ca.SamInputs) == 8 * 8  # seven pointers and a 32-bit count, padded


def test_symbol_is_exported():
    L = ctypes.CDLL(ca.build_library())
    assert hasattr(L, "cmb_batch_sam_device") and "cmb_batch_sam_device" in ca.EXPORTS
    assert hasattr(ca.Batch, "sam_device")
