"""The launch-geometry knobs of columba_amd/csrc/host_grid.hpp: CMB_TEST_GRID_CAP and the clamps of the knobs beside it.

No GPU: tests/grid_cap_driver.cpp (own main, g++ with the address and undefined-behaviour sanitizers) includes only that header and
prints what a launch would be given under the environment of its process.  The rules: with nothing set every launch keeps its own
geometry; the cap is in blocks and is min'ed with the launch's own; zero, negative and non-numeric values count as 1 block, never 0;
a slot count is a positive multiple of the block; where a knob and the cap are both set the smaller wins.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = (0, 1, 4, 128, 1024, 8192, 16384)   # a launch's own blocks, as the driver asks them
UNCAPPED = 0xFFFFFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid_cap") / "grid_cap_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "columba_amd", "csrc"), os.path.join(ROOT, "tests", "grid_cap_driver.cpp"), "-o", exe])
    return exe


def _run(driver, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("CMB_TEST_GRID_CAP", "GRID_KNOB", "SLOT_KNOB")}
    e.update(env)
    r = subprocess.run([driver], env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}, r.stderr


# (value of CMB_TEST_GRID_CAP, the cap in blocks): unset, 0, -3, abc, 1, 3 and a value above every default
CAPS = [(None, UNCAPPED), ("0", 1), ("-3", 1), ("abc", 1), ("", 1), ("1", 1), ("3", 3), ("100000", 100000)]


@pytest.mark.parametrize("value,cap", CAPS)
def test_cap_in_blocks_and_lanes(driver, value, cap):
    out, err = _run(driver, **({} if value is None else {"CMB_TEST_GRID_CAP": value}))
    assert out["cap"] == cap
    for own in OWN:
        assert out["blocks_%d" % own] == min(own, cap)   # (0 blocks: nothing to launch, with or without the cap)
    assert out["slots_8M"] == 256 * min(32768, cap)
    assert out["slots_256k"] == 256 * min(1024, cap)
    assert out["slots_256"] == 256 and out["slots_0"] == 0
    assert out["lanes64_16384"] == 64 * min(16384, cap)
    # no knob set: the defaults, under the cap
    assert out["knob_blocks"] == 8192 and out["knob_slots"] == 256 * 1536 and out["knob_slots_most"] == 256 * 1024
    assert out["both_blocks"] == min(8192, cap) and out["both_slots"] == 256 * min(1536, cap)
    if value is None or value == "100000":   # nothing set, or a cap above every default: the geometry is the default's
        assert [out["blocks_%d" % own] for own in OWN] == list(OWN)
        assert (out["slots_8M"], out["slots_256k"]) == (256 * 32768, 256 * 1024)
    assert err == "[grid] k_test 769 items, 256 lanes\n"   # (the line is built only when verbose is set)


# (value of a knob, what it gives in blocks, in slots, in slots of at most 2048 blocks)
KNOBS = [("0", 1, 256, 256), ("-3", 1, 256, 256), ("abc", 1, 256, 256), ("", 1, 256, 256), ("1", 1, 256, 256), ("3", 3, 256, 256),
         ("100", 100, 256, 256), ("255", 255, 256, 256), ("256", 256, 256, 256), ("257", 257, 256, 256), ("1000", 1000, 768, 768),
         ("1048576", 1048576, 1048576, 256 * 2048), ("99999999999999999999", 0x7FFFFFFF, 0x7FFFFF00, 256 * 2048)]


@pytest.mark.parametrize("value,blocks,slots,slots_most", KNOBS)
def test_knobs_never_give_an_empty_launch(driver, value, blocks, slots, slots_most):
    out, _ = _run(driver, GRID_KNOB=value, SLOT_KNOB=value)
    assert (out["knob_blocks"], out["knob_slots"], out["knob_slots_most"]) == (blocks, slots, slots_most)
    assert out["knob_slots"] % 256 == 0 and out["knob_slots"] >= 256
    assert (out["both_blocks"], out["both_slots"]) == (blocks, slots)   # (no cap)


@pytest.mark.parametrize("knob,cap,blocks,slots", [("5", "3", 3, 256), ("2", "3", 2, 256), ("2000", "3", 3, 768), ("2000", "100", 100, 1792),
                                                   ("0", "0", 1, 256), ("abc", "-1", 1, 256)])
def test_the_smaller_of_knob_and_cap_wins(driver, knob, cap, blocks, slots):
    out, _ = _run(driver, GRID_KNOB=knob, SLOT_KNOB=knob, CMB_TEST_GRID_CAP=cap)
    assert (out["both_blocks"], out["both_slots"]) == (blocks, slots)
