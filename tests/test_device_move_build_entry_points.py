"""The entry points of the device builder of the b-move index (cmb_build_move_*, cmb_build_pack_lfbp; include/columba_amd.h) where no
GPU is needed: the symbols load, the argument checks that come before any device work answer CMB_ERR_INVALID / CMB_ERR_UNSUPPORTED, a
machine without a GPU gets CMB_ERR_DEVICE, and the host-only columba_build refuses --rlc --device as it refuses --device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import columba_amd as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVE_BUILD_SYMBOLS = ("cmb_build_move_sizes_of", "cmb_build_move_arrays", "cmb_build_move_index", "cmb_build_pack_lfbp")


@pytest.fixture(scope="module")
def L():
    ca.build_library()
    return ca.lib()


def test_symbols_load(L):
    for name in MOVE_BUILD_SYMBOLS:
        assert name in ca.EXPORTS and hasattr(L, name), name
    assert hasattr(ca.DeviceBuild, "move_arrays") and hasattr(ca.DeviceBuild, "move_index")


def test_argument_checks_need_no_device(L):
    h = C.c_void_p()
    z = ca.BuildMoveSizes()
    out = np.zeros(64, np.uint64)
    fake = C.c_void_p(ca._p(out).value)   # (a non-null handle: the checks below return before they look at it)
    assert L.cmb_build_move_sizes_of(None, 64, C.byref(z)) == ca.CMB_ERR_INVALID
    assert L.cmb_build_move_sizes_of(fake, 64, None) == ca.CMB_ERR_INVALID
    for bits in (0, 16, 48, 128):
        assert L.cmb_build_move_sizes_of(fake, bits, C.byref(z)) == ca.CMB_ERR_INVALID
        assert b"length_bits" in L.cmb_last_error()
    a = ca._BuildMoveArrays()
    assert L.cmb_build_move_arrays(None, C.byref(a), None) == ca.CMB_ERR_INVALID
    assert L.cmb_build_move_arrays(fake, None, None) == ca.CMB_ERR_INVALID
    assert L.cmb_build_move_arrays(fake, C.byref(a), None) == ca.CMB_ERR_INVALID   # (no buffers)
    for k, _ in ca._BuildMoveArrays._fields_:
        if not k.endswith("_cap") and k != "length_bits":
            setattr(a, k, ca._p(out))
    a.length_bits = 16
    assert L.cmb_build_move_arrays(fake, C.byref(a), None) == ca.CMB_ERR_INVALID
    assert b"length_bits" in L.cmb_last_error()
    assert L.cmb_build_move_index(None, 1, 0, None, 0, C.byref(h)) == ca.CMB_ERR_INVALID
    assert L.cmb_build_move_index(fake, 1, 0, None, 0, None) == ca.CMB_ERR_INVALID
    assert not h.value
    # the packing hook: rows {head, start, LF, run}
    rows = np.array([[1, 0, 1, 1], [0, 4, 0, 0]], np.uint64)
    buf, size = np.zeros(256, np.uint8), C.c_uint64()
    pack = lambda n, r, zero, rows_p, bits, out_p, cap, size_p: L.cmb_build_pack_lfbp(n, r, zero, rows_p, bits, out_p, cap, size_p)
    assert pack(5, 2, 4, None, 64, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_INVALID
    assert pack(5, 2, 4, ca._p(rows), 64, None, 256, C.byref(size)) == ca.CMB_ERR_INVALID
    assert pack(5, 2, 4, ca._p(rows), 64, ca._p(buf), 256, None) == ca.CMB_ERR_INVALID
    assert pack(5, 2, 4, ca._p(rows), 48, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_INVALID
    assert pack(5, 1, 4, ca._p(rows), 64, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_INVALID      # one run
    assert pack(5, 6, 4, ca._p(rows), 64, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_INVALID      # more runs than rows of the BWT
    assert pack(5, 2, 5, ca._p(rows), 64, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_INVALID      # the '$' outside the text
    assert pack((1 << 32) + 1, 2, 4, ca._p(rows), 32, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_INVALID
    assert pack(8, 2, 4, ca._p(rows), 64, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_UNSUPPORTED
    assert b"power of two" in L.cmb_last_error()
    assert pack((1 << 40) + 1, 2, 4, ca._p(rows), 64, ca._p(buf), 256, C.byref(size)) == ca.CMB_ERR_UNSUPPORTED
    # 24 bytes of header, 2 + 1 rows of ceil((3 + 2 * 3 + 1) / 8) bytes; the size is known without a device
    assert pack(5, 2, 4, ca._p(rows), 64, ca._p(buf), 29, C.byref(size)) == ca.CMB_ERR_OVERFLOW
    assert size.value == 24 + 3 * 2 and not buf.any()
    assert pack(5, 2, 4, ca._p(rows), 32, ca._p(buf), 0, C.byref(size)) == ca.CMB_ERR_OVERFLOW and size.value == 12 + 3 * 2


def test_no_gpu_means_loud_failure(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(ca.CmbError) as e:
        ca.DeviceBuild(b"ACGTACGTTTGACA" * 20 + b"$").move_arrays()
    assert e.value.code == ca.CMB_ERR_DEVICE   # no CPU fallback
    with pytest.raises(ca.CmbError) as e:
        ca.device_pack_lfbp(5, np.array([[1, 0, 1, 1], [0, 4, 0, 0]], np.uint64), 4)
    assert e.value.code == ca.CMB_ERR_DEVICE


def test_host_tool_refuses_the_device_option_with_rlc(tmp_path):
    exe = str(tmp_path / "columba_build")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_build.cpp"),
                           "-o", exe, "-lz"])
    (tmp_path / "t.fa").write_text(">s\nACGTACGTTGCA\n")
    r = subprocess.run([exe, "--rlc", "--device", "-r", str(tmp_path / "x"), "-f", str(tmp_path / "t.fa")], capture_output=True, text=True)
    assert r.returncode != 0 and "built without the device path" in r.stderr
    assert not os.path.exists(str(tmp_path / "x.meta"))
    subprocess.check_call([exe, "--rlc", "-r", str(tmp_path / "x"), "-f", str(tmp_path / "t.fa")])
    assert os.path.exists(str(tmp_path / "x.LFBP"))
