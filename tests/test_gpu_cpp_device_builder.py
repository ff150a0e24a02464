"""`columba_build --device` (include/columba_amd_build_device.hpp: the arrays of cmb_build_*, the host builder's preprocessing and file
writer) against the host tool, compiled as tests/test_cpp_builder.py compiles it: every file of the index is byte-identical — on two
FASTA files with several sequences, lower case and runs of N, with -s 8, with -a and with -l 4.  And `columba_align -G <fasta>` (the
index built on the device, no files) writes the SAM text of `columba_align -r` on the host-built files.

Run with `pytest -m gpu` on an MI355X."""
import os
import subprocess

import numpy as np
import pytest

from columba_amd import synth
import columba_amd as ca

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["meta", "cct", "txt.bin", "bwt", "brt", "rev.brt", "pos", "sna", "fsid", "headerSN.bin"]
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
    tmp = str(tmp_path_factory.mktemp("cpp_device_builder"))
    ca.build_library()
    host, dev = os.path.join(tmp, "columba_build"), os.path.join(tmp, "columba_build_device")
    inc, src = os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_build.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", inc, src, "-o", host, "-lz"])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-DCOLUMBA_AMD_DEVICE_BUILD", "-I", inc, src, "-o", dev] + LINK)
    g, _ = synth.genome_rep(seed=41, n=200_000, scale=4.0)
    g = g[:30_000]
    seqs = [g[0:9_000].tobytes(), g[9_000:9_700].tobytes() + b"N" * 37 + g[9_700:16_000].tobytes(), b"NNNNN" + g[16_000:24_000].tobytes() + b"RYK",
            g[24_000:30_000].tobytes()]
    f1, f2 = os.path.join(tmp, "a.fa"), os.path.join(tmp, "b.fasta")
    _write_fasta(f1, [("chrA", seqs[0]), ("chrB", seqs[1])])
    _write_fasta(f2, [("chrC", seqs[2]), ("chrD", seqs[3])])
    return {"tmp": tmp, "host": host, "dev": dev, "fasta": [f1, f2], "genome": g}


@pytest.mark.parametrize("name,args,factors", [("s8", ["-s", "8"], (8,)), ("all", ["-a"], (1, 2, 4, 8, 16, 32, 64, 128)), ("l4", ["-l", "4"], (4,))])
def test_device_tool_writes_the_host_tools_files(world, name, args, factors):
    bh, bd = os.path.join(world["tmp"], "h_" + name), os.path.join(world["tmp"], "d_" + name)
    subprocess.check_call([world["host"]] + args + ["-r", bh, "-f"] + world["fasta"])
    subprocess.check_call([world["dev"], "--device"] + args + ["-r", bd, "-f"] + world["fasta"])
    for ext in FILES + [f"sa.{s}" for s in factors] + [f"sa.bv.{s}" for s in factors]:
        a, b = open(f"{bh}.{ext}", "rb").read(), open(f"{bd}.{ext}", "rb").read()
        assert len(a) > 0 and a == b, (ext, len(a), len(b))
    assert sorted(f for f in os.listdir(world["tmp"]) if f.startswith("d_" + name + ".")) == sorted(
        "d" + f[1:] for f in os.listdir(world["tmp"]) if f.startswith("h_" + name + "."))


def test_align_from_fasta_writes_the_sam_of_the_host_built_index(world):
    tmp = world["tmp"]
    exe = os.path.join(tmp, "columba_align")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_align.cpp"), "-o", exe]
                          + LINK)
    base = os.path.join(tmp, "h_align")
    subprocess.check_call([world["host"], "-s", "4", "-r", base, "-f"] + world["fasta"])
    reads = synth.sample_reads(world["genome"], 300, 100, seed=12)
    fq = os.path.join(tmp, "reads.fq")
    with open(fq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i} x\n{r.decode()}\n+\n{'I' * len(r)}\n")
    common = ["-f", fq, "-a", "all", "-e", "3", "-s", "4", "-b", "128"]
    subprocess.check_call([exe, "-r", base, "-o", os.path.join(tmp, "r.sam")] + common)
    subprocess.check_call([exe, "-G"] + world["fasta"] + ["-o", os.path.join(tmp, "g.sam")] + common)
    # (the @PG line quotes the command line, which names the index or the FASTA files)
    want = [ln for ln in open(os.path.join(tmp, "r.sam"), "rb").read().split(b"\n") if not ln.startswith(b"@PG")]
    got = [ln for ln in open(os.path.join(tmp, "g.sam"), "rb").read().split(b"\n") if not ln.startswith(b"@PG")]
    assert got == want
    assert sum(ln.startswith(b"@SQ") for ln in got) == 4 and sum(1 for ln in got if ln and not ln.startswith(b"@")) >= 300
    r = subprocess.run([exe, "-r", base, "-G", world["fasta"][0], "-o", os.path.join(tmp, "x.sam"), "-f", fq], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
