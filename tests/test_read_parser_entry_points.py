"""The entry points of the device FASTQ parser (cmb_reads_*; include/columba_amd.h) where no GPU is needed: the symbols load, the
argument checks that come before any device work answer CMB_ERR_INVALID / CMB_ERR_UNSUPPORTED, a machine without a GPU gets
CMB_ERR_DEVICE, and the host layers on top (DeviceReader, ParsedChunk, the adapter's overloads, columba_align) compile warning-free."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import columba_amd as ca
import test_cabi_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READS_SYMBOLS = ("cmb_reads_create", "cmb_reads_destroy", "cmb_reads_parse_fastq", "cmb_reads_arrays", "cmb_reads_device_arrays")


@pytest.fixture(scope="module")
def L():
    ca.build_library()
    return ca.lib()


def test_symbols_load(L):
    for name in READS_SYMBOLS:
        assert name in ca.EXPORTS and hasattr(L, name), name
    test_cabi_exports.test_header_symbols_are_exported(ca.build_library())  # (the header and EXPORTS are in step, the new symbols included)
    assert "reads.hip" in ca.build_units()
    for cls in (ca.Batch, ca.MoveBatch, ca.BestDevice):
        assert hasattr(cls, "sam_device_bytes_packed")
    assert hasattr(ca.ReadParser, "parse") and hasattr(ca.ParsedReads, "records") and hasattr(ca.ParsedReads, "packed")
    hdr = open(os.path.join(ROOT, "include", "columba_amd.h")).read()
    assert "#define CMB_READS_MAX_WINDOW (1ull << 30)" in hdr and ca.READS_MAX_WINDOW == 1 << 30   # at least 1 GiB, stated in the header


def test_argument_checks_need_no_device(L):
    h = C.c_void_p()
    assert L.cmb_reads_create(0, None) == ca.CMB_ERR_INVALID
    info, view = ca.ReadsInfo(), ca.ReadsView()
    scratch = np.zeros(64, np.uint64)
    fake = C.c_void_p(ca._p(scratch).value)   # (a non-null handle: the checks below return before they look at it)
    data = np.frombuffer(b"@a\nAC\n+\nII\n", np.uint8)
    parse = L.cmb_reads_parse_fastq
    assert parse(None, ca._p(data), data.size, 10, 1, C.byref(info)) == ca.CMB_ERR_INVALID
    assert parse(fake, ca._p(data), data.size, 10, 1, None) == ca.CMB_ERR_INVALID
    assert parse(fake, None, data.size, 10, 1, C.byref(info)) == ca.CMB_ERR_INVALID
    assert parse(fake, ca._p(data), data.size, 0, 1, C.byref(info)) == ca.CMB_ERR_INVALID
    assert b"max_records" in L.cmb_last_error()
    # larger than the largest window: refused by its size alone (the bytes are not looked at)
    assert parse(fake, ca._p(data), ca.READS_MAX_WINDOW + 1, 10, 1, C.byref(info)) == ca.CMB_ERR_UNSUPPORTED
    assert str(ca.READS_MAX_WINDOW).encode() in L.cmb_last_error()
    for fasta in (b">s\nACGT\n", b"\n\r\n\rx\n>s\nACGT\n"):
        d = np.frombuffer(fasta, np.uint8)
        assert parse(fake, ca._p(d), d.size, 10, 1, C.byref(info)) == ca.CMB_ERR_UNSUPPORTED
        assert b"FASTA" in L.cmb_last_error()
    assert L.cmb_reads_arrays(None, C.byref(view)) == ca.CMB_ERR_INVALID
    assert L.cmb_reads_arrays(fake, None) == ca.CMB_ERR_INVALID
    ptrs, sizes = (C.c_void_p * ca.READS_DEV_ARRAYS)(), (C.c_uint64 * ca.READS_DEV_ARRAYS)()
    assert L.cmb_reads_device_arrays(None, C.byref(ptrs), C.byref(sizes)) == ca.CMB_ERR_INVALID
    assert L.cmb_reads_device_arrays(fake, None, C.byref(sizes)) == ca.CMB_ERR_INVALID
    assert L.cmb_reads_device_arrays(fake, C.byref(ptrs), None) == ca.CMB_ERR_INVALID
    L.cmb_reads_destroy(None)
    assert not h.value


def test_no_gpu_means_loud_failure(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(ca.CmbError) as e:
        ca.ReadParser()
    assert e.value.code == ca.CMB_ERR_DEVICE   # no CPU fallback


def test_host_layers_compile_without_warnings(tmp_path):
    """DeviceReader and ParsedChunk under the flags of test_header_is_plain_c plus -Werror, used (so that the member functions are
    instantiated), and columba_align with the adapter's overloads for packed chunks"""
    inc = os.path.join(ROOT, "include")
    test_cabi_exports.test_header_is_plain_c()
    src = ('#include "columba_amd_io.hpp"\n'
           "int main(int argc, char** argv) {\n"
           "    columba_amd::DeviceReader r(argv[argc - 1]);\n"
           "    columba_amd::ParsedChunk c;\n"
           "    size_t n = 0;\n"
           "    while (r.getNextChunk(c, 1000)) n += c.records().size();\n"
           "    return n == 0 && !r.onDevice();\n"
           "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, "-"], input=src, text=True, check=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, os.path.join(ROOT, "tests", "reader_driver.cpp")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DREADER_DEVICE", "-I", inc,
                           os.path.join(ROOT, "tests", "reader_driver.cpp")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc, os.path.join(ROOT, "examples", "columba_align.cpp")])
