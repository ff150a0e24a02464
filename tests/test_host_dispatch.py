"""The selectors of columba_amd/csrc/host_dispatch.hpp: runtime flags and small integers to template arguments, and the rule for the
record geometry of the frontier.

No GPU: tests/host_dispatch_driver.cpp (own main, g++ with the address and undefined-behaviour sanitizers) includes only that header and
prints what each selector hands its functor.  The rules: withBools passes one constant per flag, in the order given, for four, two and
no flags; withInt<3> hands out 0, 1, 2 and the last instance beyond the range; the frontier runs on GeoX exactly where the tables are wide
and the distance is beyond MX_MAX_ED, on GeoN32 exactly where they are narrow, the distance is at most MXS_MAX_ED, no phase has
overflowed the small matrix and the 64-bit words are not forced.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO_X, GEO_W, GEO_N32, GEO_N = 0, 1, 2, 3   # enum FrontierGeo


def _limit(name):
    """a constexpr limit of dev_matrix.hpp, so that the table below follows the kernels' own"""
    src = open(os.path.join(ROOT, "columba_amd", "csrc", "dev_matrix.hpp")).read()
    return int(re.search(r"\b%s = (\d+)" % name, src).group(1))


MX_MAX_ED, MXS_MAX_ED = _limit("MX_MAX_ED"), _limit("MXS_MAX_ED")


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_dispatch") / "host_dispatch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "columba_amd", "csrc"), os.path.join(ROOT, "tests", "host_dispatch_driver.cpp"), "-o", exe])
    r = subprocess.run([exe, str(MX_MAX_ED), str(MXS_MAX_ED)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in r.stdout.splitlines()}


def test_limits_are_the_kernels():
    assert (MX_MAX_ED, MXS_MAX_ED) == (10, 6)


@pytest.mark.parametrize("m", range(16))
def test_four_flags_in_order(out, m):
    assert out["four_%d" % m] == [m >> 3 & 1, m >> 2 & 1, m >> 1 & 1, m & 1]


def test_two_flags_and_none(out):
    for m in range(4):
        assert out["two_%d" % m] == [m >> 1 & 1, m & 1]
    assert out["zero"] == [7]


def test_small_integer_range(out):
    assert [out["int3_%d" % v] for v in (0, 1, 2)] == [[0], [1], [2]]
    assert [out["int3_%d" % v] for v in (3, 4, 5)] == [[2], [2], [2]]   # beyond the range: the last instance
    assert out["int3_-1"] == [0] and out["int1_4"] == [0]


def test_frontier_geometry_table(out):
    seen = set()
    for k in range(14):
        for wide in (0, 1):
            for no_small in (0, 1):
                for forced64 in (0, 1):
                    got = out["geo_%d_%d" % (k, wide << 2 | no_small << 1 | forced64)][0]
                    geo_x = bool(wide) and k > MX_MAX_ED
                    small32 = not wide and k <= MXS_MAX_ED and not no_small and not forced64
                    assert (got == GEO_X) == geo_x, (k, wide, no_small, forced64)
                    assert (got == GEO_N32) == small32, (k, wide, no_small, forced64)
                    if not geo_x and not small32:
                        assert got == (GEO_W if wide else GEO_N), (k, wide, no_small, forced64)
                    seen.add(got)
    assert seen == {GEO_X, GEO_W, GEO_N32, GEO_N}
