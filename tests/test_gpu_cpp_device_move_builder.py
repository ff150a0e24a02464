"""`columba_build --rlc --device` (include/columba_amd_build_device.hpp: the parts of cmb_build_move_arrays, the host builder's
preprocessing and file writer) against the host tool: every file of the run-length compressed index is byte-identical, on two FASTA
files with several sequences, lower case and runs of N.  And a BMove made from text on the device (BMove::FromText, bmoveFromFasta)
reports the cmb_move_info and the exact matches of a BMove loaded from those files (tests/bmove_from_text_driver.cpp).

Run with `pytest -m gpu` on an MI355X."""
import os
import subprocess

import pytest

from columba_amd import synth
import columba_amd as ca

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["meta", "cct", "txt.bin", "pos", "sna", "fsid", "headerSN.bin", "LFBP", "rev.LFBP"] + [e + ".u64" for e in (
    "smpf", "smpl", "rev.smpf", "rev.smpl", "prdf", "ftr", "prdl", "ltr", "plcp.pos", "plcp.sum")]
LINK = ["-L", os.path.join(ROOT, "columba_amd"), "-lcolumba_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "columba_amd"), "-Wl,-rpath,/opt/rocm/lib"]


def _write_fasta(path, records, width=70):
    with open(path, "w") as f:
        for k, (name, seq) in enumerate(records):
            f.write(f">{name} description {k}\n")
            s = seq.decode()
            if k % 2 == 0:
                s = s.lower()
            for o in range(0, len(s), width):
                f.write(s[o:o + width] + "\n")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("cpp_device_move_builder"))
    ca.build_library()
    host, dev = os.path.join(tmp, "columba_build"), os.path.join(tmp, "columba_build_device")
    inc, src = os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_build.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", inc, src, "-o", host, "-lz"])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-DCOLUMBA_AMD_DEVICE_BUILD", "-I", inc, src, "-o", dev] + LINK)
    g, _ = synth.genome_rep(seed=41, n=200_000, scale=4.0)
    g = g[:30_000]
    seqs = [g[0:9_000].tobytes(), g[9_000:9_700].tobytes() + b"N" * 37 + g[9_700:16_000].tobytes(), b"NNNNN" + g[16_000:24_000].tobytes() + b"RYK",
            g[0:6_000].tobytes()]   # (the last sequence repeats the first: runs and a long PLCP)
    f1, f2 = os.path.join(tmp, "a.fa"), os.path.join(tmp, "b.fasta")
    _write_fasta(f1, [("chrA", seqs[0]), ("chrB", seqs[1])])
    _write_fasta(f2, [("chrC", seqs[2]), ("chrD", seqs[3])])
    bh, bd = os.path.join(tmp, "h"), os.path.join(tmp, "d")
    subprocess.check_call([host, "--rlc", "--keep-text", "-r", bh, "-f", f1, f2])
    subprocess.check_call([dev, "--rlc", "--keep-text", "--device", "-r", bd, "-f", f1, f2])
    return {"tmp": tmp, "host": bh, "dev": bd, "fasta": [f1, f2], "genome": g}


def test_device_tool_writes_the_host_tools_move_files(world):
    for ext in FILES:
        a, b = open(f"{world['host']}.{ext}", "rb").read(), open(f"{world['dev']}.{ext}", "rb").read()
        assert len(a) > 0 and a == b, (ext, len(a), len(b))
    tmp = world["tmp"]
    assert sorted(f[1:] for f in os.listdir(tmp) if f.startswith("d.")) == sorted(f[1:] for f in os.listdir(tmp) if f.startswith("h.")) == \
        sorted("." + e for e in FILES)


def test_bmove_from_text_equals_bmove_from_files(world):
    tmp = world["tmp"]
    exe = os.path.join(tmp, "bmove_from_text_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "bmove_from_text_driver.cpp"),
                           "-o", exe] + LINK)
    g = world["genome"]
    reads = [g[o:o + 40].tobytes().decode() for o in range(100, 100 + 45 * 600, 600)] + ["ACGTTGCATTAGCCATAGGCATTACCGATTAGGACCATTG"] * 5
    assert len(reads) == 50
    rf = os.path.join(tmp, "reads.txt")
    with open(rf, "w") as f:
        f.write("\n".join(reads) + "\n")
    r = subprocess.run([exe, world["host"], rf] + world["fasta"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.returncode, r.stdout, r.stderr)
    n, runs, matches = (int(x) for x in r.stdout.split()[1:4])
    # the 15 reads from 100 .. 8500 lie inside chrA, the first 10 of them inside chrD as well
    assert n == os.path.getsize(world["host"] + ".txt.bin") - 8 and runs > 1000 and matches >= 25
