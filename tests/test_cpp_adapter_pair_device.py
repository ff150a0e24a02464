"""The C++ host adapter's device path for read pairs in ALL mode: samOfChunkPairedAll with CMB_PAIR_DEVICE=1 (two batches whose lists
stay in HBM, cmb_pair_sam_device) returns, byte for byte, what the same call returns without the variable (cmb_pair_sam per pair)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import columba_amd as ca
from test_cpp_adapter import ROOT, _build_align


def test_pair_device_entry_point_checks_its_arguments():
    """no GPU needed: NULL arguments are refused before anything touches the device"""
    L = ca.lib()
    assert "cmb_pair_sam_device" in ca.EXPORTS and hasattr(L, "cmb_pair_sam_device")
    text, n = C.c_void_p(), C.c_uint64()
    assert L.cmb_pair_sam_device(None, None, None, None, None, C.byref(text), C.byref(n), None) == -1  # CMB_ERR_INVALID
    assert L.cmb_last_error()


@pytest.mark.gpu
def test_align_driver_pairs_on_the_device(tmp_path):
    from columba_amd import indexbuild as ib, synth
    exe = _build_align(str(tmp_path))
    g, starts = synth.genome_rep(seed=2, n=300_000, scale=2.0)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    ix.seq_names = [f"chr{i}" for i in range(len(starts) - 1)]
    ib.save_index(ix, str(tmp_path / "idx"))
    rng = np.random.default_rng(4)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    n, L = 250, 80
    r1, r2 = [], []
    for i in range(n):
        frag = int(rng.integers(200, 380))
        p0 = int(rng.integers(500, len(g) - 900))
        f = g[p0:p0 + frag].tobytes()
        a, b = bytearray(f[:L]), bytearray(f[-L:].translate(comp)[::-1])
        if i % 7 == 0:
            b = bytearray(bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)))  # a mate from nowhere
        if i % 5 == 0:
            a[10] = ord("N")
        if i % 2:
            a, b = b, a
        r1.append(bytes(a))
        r2.append(bytes(b))
    q = "".join(chr(33 + i % 40) for i in range(L))
    (tmp_path / "r1.fq").write_text("".join(f"@p{i}/1 x\n{r1[i].decode()}\n+\n{q}\n" for i in range(n)))
    (tmp_path / "r2.fq").write_text("".join(f"@p{i}/2 x\n{r2[i].decode()}\n+\n{q}\n" for i in range(n)))
    bodies, logs = {}, {}
    for device in ("0", "1"):
        out = tmp_path / f"o{device}.sam"
        env = dict(os.environ, CMB_PAIR_DEVICE=device, CMB_VERBOSE="1")
        run = subprocess.run([exe, "-r", str(tmp_path / "idx"), "-f", str(tmp_path / "r1.fq"), "-F", str(tmp_path / "r2.fq"), "-o", str(out),
                              "-a", "all", "-e", "2", "-S", "multiple_opt", "-b", "100", "-X", "500", "-N", "100"], capture_output=True, text=True, env=env)
        assert run.returncode == 0, run.stderr
        bodies[device] = b"".join(ln for ln in out.read_bytes().splitlines(keepends=True) if not ln.startswith(b"@"))
        logs[device] = run.stderr
    assert "[host] pair sam:" in logs["1"] and "[host] pair sam:" not in logs["0"], "the variable selects the path"
    assert bodies["1"] == bodies["0"] and bodies["0"].count(b"\n") > 2 * 0.6 * n
    # the number of mapped pairs the call hands back beside the text (the CLI does not print it): samOfChunkPairedAll on the whole chunk
    # from the driver of tools/pair_sam_cost.py, once per path
    cost = os.path.join(str(tmp_path), "pair_sam_cost")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "pair_sam_cost.cpp"), "-o", cost,
                           "-L", os.path.join(ROOT, "columba_amd"), "-lcolumba_amd", "-Wl,-rpath," + os.path.join(ROOT, "columba_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    (tmp_path / "r1.txt").write_bytes(b"\n".join(r1) + b"\n")
    (tmp_path / "r2.txt").write_bytes(b"\n".join(r2) + b"\n")
    lines = {}
    for device in ("0", "1"):
        run = subprocess.run([cost, str(tmp_path / "idx"), str(tmp_path / "r1.txt"), str(tmp_path / "r2.txt"), str(len(ix.seq_names)), "2", "500", "100", "1"],
                             capture_output=True, text=True, env=dict(os.environ, CMB_PAIR_DEVICE=device))
        assert run.returncode == 0, run.stderr
        lines[device] = json.loads(run.stdout.strip().splitlines()[-1])
    assert lines["0"]["path"] == "host" and lines["1"]["path"] == "device"
    for key in ("mapped_pairs", "text_bytes", "text_hash"):
        assert lines["1"][key] == lines["0"][key], key
    assert 0.6 * n < lines["0"]["mapped_pairs"] < n and lines["0"]["text_bytes"] == len(bodies["0"])
