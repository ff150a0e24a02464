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

--rlc: the run-length compressed (b-move) index instead, on `movebuild.pangenome` (64 haplotypes, 0.5 % SNPs: the stand-in of bench.py's
rlc leg) at 2^24, 2^28 and that leg's own 256 * 10^6 characters.  Timed each by itself: cmb_build_create; the move derivation (the first
cmb_build_move_sizes_of) with its phases from cmb_build_timings; the download (cmb_build_move_arrays); the resident index
(cmb_build_move_index).  Beside them the ways that existed before: `build_move(device="cuda:0", with_locate=False)` + `plcp_gpu` (what
bench.py does), `build_move_resident(device="cuda")`, and the host's `columba_build --rlc` up to --host-max.  Every array of the device
build is compared with build_move_resident's at every size (profiles/device_move_build_times.json).  Every route is warmed up on a text of
2^20 characters first; the torch routes are timed once per size.

    python tools/build_bench.py --rlc [--sizes 16777216,268435456,256000000] [--reps 3] [--no-host] [--host-max N] [--no-torch-plcp] [--out F]
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


MOVE_FIELDS = ("lfbp_fwd", "lfbp_rev", "smpf", "smpl", "rev_smpf", "rev_smpl", "pred_first", "first_to_run", "pred_last", "last_to_run",
               "plcp_pos", "plcp_sum")
HAPLOTYPES, SNP = 64, 0.005


def one_size_rlc(n, reps, host_exe, host_max, torch_plcp):
    import torch
    from columba_amd import movebuild
    text = np.concatenate([movebuild.pangenome(n // HAPLOTYPES, HAPLOTYPES, SNP, seed=1), np.frombuffer(b"$", np.uint8)])
    res = {"characters": int(text.shape[0]), "haplotypes": HAPLOTYPES, "snp": SNP}
    creates, derives, downloads, residents, phases = [], [], [], [], None
    for _ in range(reps):
        b, t = timed(lambda: ca.DeviceBuild(text))
        creates.append(t)
        z, t = timed(lambda: b.move_sizes())
        derives.append(t)
        got, t = timed(lambda: b.move_arrays())
        downloads.append(t)
        ix, t = timed(lambda: b.move_index())
        residents.append(t)
        ix.close()
        phases = {k: v for k, v in b.timings().items() if k.startswith("move ")}
        b.close()
    stat = lambda v: {"best": min(v), "median": statistics.median(v), "all": v}
    res["device_create_s"], res["device_move_derive_s"] = stat(creates), stat(derives)
    res["device_move_download_s"], res["device_move_resident_index_s"] = stat(downloads), stat(residents)
    res["device_move_phases_ms"] = phases
    res["runs"], res["rev_runs"], res["plcp_runs"] = int(z.runs), int(z.rev_runs), int(z.n_plcp)
    res["device_text_to_resident_index_s"] = min(creates) + min(derives) + min(residents)
    torch.cuda.empty_cache()
    want, res["torch_build_move_resident_s"] = timed(lambda: movebuild.build_move_resident(text, device="cuda"))
    torch.cuda.empty_cache()
    for f in MOVE_FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (n, f)
    res["arrays_equal_build_move_resident"] = True
    if torch_plcp:
        def bench_py_route():
            mv = movebuild.build_move(text[:-1], device="cuda:0", with_locate=False)
            mv.plcp = movebuild.plcp_gpu(mv)
            return mv
        mv, res["torch_build_move_plus_plcp_gpu_s"] = timed(bench_py_route)
        assert np.array_equal(mv.lfbp_fwd, got.lfbp_fwd) and np.array_equal(mv.lfbp_rev, got.lfbp_rev), n
        del mv
        torch.cuda.empty_cache()
        res["device_over_bench_py_route"] = (min(creates) + min(derives) + min(downloads)) / res["torch_build_move_plus_plcp_gpu_s"]
    res["device_over_build_move_resident"] = (min(creates) + min(derives) + min(downloads)) / res["torch_build_move_resident_s"]
    if host_exe and n <= host_max:
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "t.fa")
            with open(fa, "wb") as f:
                f.write(b">s\n")
                f.write(text[:-1].tobytes())
                f.write(b"\n")
            t = time.perf_counter()
            subprocess.check_call([host_exe, "--rlc", "-r", os.path.join(tmp, "h"), "-f", fa], stdout=subprocess.DEVNULL)
            res["host_columba_build_rlc_s"] = time.perf_counter() - t   # (with reading the FASTA file and writing the index files)
            assert np.array_equal(np.fromfile(os.path.join(tmp, "h.LFBP"), np.uint8), got.lfbp_fwd), n
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rlc", action="store_true", help="the b-move index on a pan-genome instead (see above)")
    ap.add_argument("--no-torch-plcp", action="store_true", help="--rlc: leave out build_move + plcp_gpu, the slowest baseline")
    ap.add_argument("--sizes")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-max", type=int, help="the host builder runs at sizes up to this one (2^28; --rlc: 2^24)")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.sizes = a.sizes or ("16777216,268435456,256000000" if a.rlc else "16777216,268435456,3000000000")
    a.host_max = a.host_max or (1 << 24 if a.rlc else 1 << 28)
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
    if a.rlc:
        from columba_amd import movebuild
        warm = np.concatenate([movebuild.pangenome(1 << 14, HAPLOTYPES, SNP, seed=1), np.frombuffer(b"$", np.uint8)])   # warm-up of both routes
        b = ca.DeviceBuild(warm)
        b.move_arrays(), b.move_index().close(), b.close()
        movebuild.build_move_resident(warm, device="cuda")
        if not a.no_torch_plcp:
            movebuild.plcp_gpu(movebuild.build_move(warm[:-1], device="cuda:0", with_locate=False))
        out = {"tool": "tools/build_bench.py --rlc", "gpu": torch.cuda.get_device_name(0),
               "text": f"movebuild.pangenome(n / {HAPLOTYPES}, {HAPLOTYPES}, {SNP}, seed=1)", "sizes": []}
        for n in (int(s) for s in a.sizes.split(",")):
            out["sizes"].append(one_size_rlc(n, a.reps if n <= (1 << 24) else 1, host_exe, a.host_max, not a.no_torch_plcp))
            print(json.dumps(out["sizes"][-1]), file=sys.stderr, flush=True)
            if a.out:   # (after every size: a later size that runs out of time keeps the earlier ones)
                with open(a.out, "w") as f:
                    f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
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
