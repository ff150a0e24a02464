"""cmb_batch_trim_on_device / cmb_batch_trim_stats without a GPU: exported, declared, bound, and loud where there is no device.
What they compute is tests/test_gpu_trim_device.py's."""
import ctypes
import os
import re

import pytest

import columba_amd as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmb_batch_trim_on_device", "cmb_batch_trim_stats")


def test_exported_declared_and_bound():
    L = ctypes.CDLL(ca.build_library())
    hdr = open(os.path.join(ROOT, "include", "columba_amd.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in ca.EXPORTS
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert getattr(ca.lib(), name).argtypes is not None, name
    for macro, value in (("CMB_SPANS_OVER_END", 1), ("CMB_SPANS_TRIMMED", 2), ("CMB_SPANS_DROPPED", 4)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    assert callable(ca.Batch.trim_on_device) and callable(ca.Batch.trim_stats)


def test_null_handles_are_refused():
    L = ca.lib()
    assert L.cmb_batch_trim_on_device(None, 1) == -1  # CMB_ERR_INVALID
    assert L.cmb_batch_trim_stats(None, None, None, None) == -1
    assert b"null argument" in L.cmb_last_error()


def test_no_gpu_means_loud_failure():
    """the project's convention for product entry points (tests/test_cabi_exports.py): a Batch needs an Index on the device, so without
    one the chain ends at ca.Index with CMB_ERR_DEVICE — there is no CPU path that trim_on_device could reach.  (The call itself is
    never reached here, and the test passes without the feature: what the entry points do is tests/test_gpu_trim_device.py's.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from columba_amd import indexbuild as ib
    ix = ib.build_index(b"ACGTACGTTTGACA" * 20)
    with pytest.raises(ca.CmbError) as e:
        b = ca.Batch(ca.Index(ix), ca.SearchStrategy("columba"), 2, [b"ACGTACGTTTGACA"])
        b.want_alignments()
        b.trim_on_device()
    assert e.value.code == -2  # CMB_ERR_DEVICE: no CPU fallback


def test_adapter_switch_compiles():
    """samOfChunkAll reads CMB_TRIM_DEVICE (both overloads call cmb_batch_trim_on_device); the header still compiles as C++17"""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    hpp = open(os.path.join(ROOT, "include", "columba_amd.hpp")).read()
    assert hpp.count("cmb_batch_trim_on_device(b, trimOnDevice())") == 2 and 'getenv("CMB_TRIM_DEVICE")' in hpp
    src = '#include "columba_amd.hpp"\n#include "columba_amd_io.hpp"\nint main() { return 0; }\n'
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "include"), "-"], input=src,
                   text=True, check=True)
