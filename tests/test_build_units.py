"""The directory is the list of translation units, and the compiler's own record says which unit includes what: the frontier kernels
(kernels.hpp) are compiled in one unit only, and so are the SAM, pair and BEST-mode kernels.  No GPU."""
import os

import pytest

import columba_amd as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "columba_amd", "csrc")


@pytest.fixture(scope="module")
def deps():
    ca.build_library()
    return {u: ca.unit_dependencies(u) for u in ca.build_units()}


def units_with(deps, header):
    return sorted(u for u, d in deps.items() if os.path.join(CSRC, header) in d)


def test_units_are_the_hip_files_of_csrc(deps):
    assert sorted(deps) == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert all(deps.values()), [u for u, d in deps.items() if not d]


def test_every_unit_depends_on_itself_and_the_public_header(deps):
    for unit, d in deps.items():
        assert os.path.join(CSRC, unit) in d, unit
        assert os.path.join(ROOT, "include", "columba_amd.h") in d, unit


def test_kernel_headers_live_in_one_unit_each(deps):
    assert units_with(deps, "kernels.hpp") == ["columba_amd.hip"]
    assert units_with(deps, "dev_sam.hpp") == units_with(deps, "dev_pair.hpp")
    assert len(units_with(deps, "dev_sam.hpp")) == 1
    assert len(units_with(deps, "dev_best.hpp")) == 1
