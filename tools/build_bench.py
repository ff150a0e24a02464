#!/usr/bin/env python3
"""How long the device index builder takes, beside the ways to build an index that existed before it.

On synth's human-like text at 2^24, 2^28 and 3.0 * 10^9 characters (or the sizes given):
  * `DeviceBuild` (cmb_build_create): the whole create, the download into IndexArrays, the resident index (cmb_build_index), and the
    phases of the create from cmb_build_timings, every doubling round by itself;
  * `indexbuild.build_index(device="cuda:0")` on the same text: the torch builder of the harness (DESIGN.md section 7 quotes 17 s for it at
    3.0 Gbp, and 6.5 s for bench.py's own doubling: both printed beside the measurement);
  * the two builders' arrays are compared field by field at every size — beyond 2^31 characters this is the only check there is;
  * the host builder `columba_build` (SA-IS, one thread) at the sizes where it stays within minutes (up to 2^28), as the ratio a C++ user sees.
A warm-up build at 2^20 characters comes first (library load, rocPRIM's first launches); every device measurement is repeated
`--reps` times at sizes up to 2^28 (best and median are reported) and taken once at larger sizes, where a build is seconds long.
Prints one JSON object (profiles/device_build_times.json).

    python tools/build_bench.py [--sizes 16777216,268435456,3000000000] [--reps 3] [--no-host] [--host-max N] [--out F]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import columba_amd as ca  # noqa: E402
from columba_amd import indexbuild as ib, synth  # noqa: E402

FIELDS = ("text", "counts", "bv_fwd", "cnt_fwd", "bv_rev", "cnt_rev", "bwt_words", "sa_bv", "sa_bv_counts", "sa_samples")


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def one_size(n, reps, host_exe, host_max):
    import torch
    g, _ = synth.genome_human_like(n - 1, seed=2025, device="cuda:0")
    text = np.concatenate([g.cpu().numpy(), np.frombuffer(b"$", np.uint8)])
    del g
    torch.cuda.empty_cache()
    res = {"characters": n}
    creates, rounds = [], None
    for _ in range(reps):
        b, t = timed(lambda: ca.DeviceBuild(text))
        creates.append(t)
        rounds = b.timings()
        if _ + 1 < reps:
            b.close()
    res["device_create_s"] = {"best": min(creates), "median": statistics.median(creates), "all": creates}
    res["device_create_phases_ms"] = rounds
    got, res["device_arrays_download_s"] = timed(lambda: b.arrays(4))
    ix, res["device_resident_index_s"] = timed(lambda: b.index(sparseness=4))
    ix.close()
    b.close()
    want, res["torch_build_index_s"] = timed(lambda: ib.build_index(torch.from_numpy(text), sparseness=4, device="cuda:0"))
    torch.cuda.empty_cache()
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), (n, f)
    assert got.dollar_pos_fwd == want.dollar_pos_fwd and got.dollar_pos_rev == want.dollar_pos_rev
    res["arrays_equal_torch_builder"] = True
    res["device_over_torch"] = res["device_create_s"]["best"] / res["torch_build_index_s"]
    if host_exe and n <= host_max:
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "t.fa")
            with open(fa, "wb") as f:
                f.write(b">s\n")
                f.write(text[:-1].tobytes())
                f.write(b"\n")
            t = time.perf_counter()
            subprocess.check_call([host_exe, "-s", "4", "-r", os.path.join(tmp, "h"), "-f", fa], stdout=subprocess.DEVNULL)
            res["host_columba_build_s"] = time.perf_counter() - t   # (with reading the FASTA file and writing the index files)
            res["host_over_device"] = res["host_columba_build_s"] / res["device_create_s"]["best"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16777216,268435456,3000000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-max", type=int, default=1 << 28, help="the host builder runs at sizes up to this one")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    ca.build_library()
    host_exe = None
    tmp = tempfile.mkdtemp()
    if not a.no_host:
        host_exe = os.path.join(tmp, "columba_build")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_build.cpp"),
                               "-o", host_exe, "-lz"])
    ca.DeviceBuild(synth.genome_human_like((1 << 20) - 1, device="cuda:0")[0].cpu().numpy().tobytes() + b"$").close()   # warm-up
    out = {"tool": "tools/build_bench.py", "gpu": torch.cuda.get_device_name(0), "text": "synth.genome_human_like(seed=2025)", "sparseness": 4,
           "quoted_in_DESIGN_7": {"torch_builder_3.0e9_s": 17, "bench_py_doubling_3.0e9_s": 6.5}, "sizes": []}
    for n in (int(s) for s in a.sizes.split(",")):
        out["sizes"].append(one_size(n, a.reps if n <= (1 << 28) else 1, host_exe, a.host_max))
        print(json.dumps(out["sizes"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
