#!/usr/bin/env python3
"""How long a chunk takes in BEST mode (the default of columba_align): the host bookkeeping against the device's.

    a  cmb_match_best        + cmb_best_results     every stratum downloaded, host containers per read (the baseline)
    b  cmb_match_best_device + cmb_best_results     strata kept in HBM, the final lists downloaded
    c  cmb_match_best_device + cmb_best_sam_device  ... and the SAM text written on the device instead

One process, seeded, the arms alternating; the host clock around calls that end in a synchronise.  (a) and (b) must return
identical arrays.  Beside the arms: what the device path spends where (cmb_best_timings: gather of the reads, batch creation,
the strata's kernels as cmb_batch_timings names them, the bookkeeping kernels, the final selection).

Workload: 10^6 x 150 bp reads on a synth.genome_human_like text of 256 Mbp, columba scheme, edit distance, dynamic
partitioning, x = 0, identity 95.

    python tools/best_rate.py --out profiles/best_device_rate.json
    python tools/best_rate.py --align 200000 --out ...      also columba_align end to end on a FASTQ of that many reads,
                                                            CMB_BEST_HOST=1 against CMB_BEST_DEVICE=1, alternating
    rocprofv3 --kernel-trace --stats -d DIR -o best -- python tools/best_rate.py --reps 1 --device-only   (a run of its own)
    python tools/best_rate.py --rlc --out profiles/move_best_device_rate.json
                                                            the same arms on the b-move backend (cmb_move_match_best against
                                                            cmb_move_match_best_device) on a `bench.py --config rlc` style text
"""
import argparse
import ctypes as C
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


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "all_ms": [round(x, 3) for x in ms]}


def _faster(base, arm):
    """§4.7's rule: faster than the baseline by more than both spreads"""
    return bool(base["median_ms"] - arm["median_ms"] > max(base["max_ms"] - base["min_ms"], arm["max_ms"] - arm["min_ms"]))


def _align(index_ix, buf, offs, n_reads, read_len, reps, tmp):
    exe = os.path.join(tmp, "columba_align")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_align.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "columba_amd"), "-lcolumba_amd", "-lz",
                           "-Wl,-rpath," + os.path.join(ROOT, "columba_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    ib.save_index(index_ix, os.path.join(tmp, "idx"))
    rng = np.random.default_rng(23)
    raw = buf.tobytes()
    with open(os.path.join(tmp, "reads.fq"), "wb") as f:
        for i in range(n_reads):
            q = (rng.integers(0, 41, read_len, dtype=np.uint8) + 33).tobytes()
            f.write(b"@SRR0000001.%d %d length=%d\n%s\n+\n%s\n" % (i + 1, i + 1, read_len, raw[int(offs[i]):int(offs[i + 1])], q))
    wall = {"host": [], "device": []}
    texts = {}
    for _ in range(reps + 1):  # (the first round warms the file cache and is dropped)
        for arm, env in (("host", {"CMB_BEST_HOST": "1"}), ("device", {"CMB_BEST_DEVICE": "1"})):
            e = {k: v for k, v in os.environ.items() if k not in ("CMB_BEST_HOST", "CMB_BEST_DEVICE")}
            e.update(env)
            os.makedirs(os.path.join(tmp, arm), exist_ok=True)  # (the header names the command line: the same relative file name)
            t = time.perf_counter()
            subprocess.run([exe, "-r", os.path.join(tmp, "idx"), "-f", os.path.join(tmp, "reads.fq"), "-o", "out.sam"], check=True, env=e,
                           capture_output=True, cwd=os.path.join(tmp, arm))
            wall[arm].append((time.perf_counter() - t) * 1e3)
            with open(os.path.join(tmp, arm, "out.sam"), "rb") as f:
                texts[arm] = f.read()
    same = texts["host"] == texts["device"]
    assert same, "columba_align wrote different SAM files on the two paths"
    res = {"reads": n_reads, "sam_bytes": len(texts["host"]), "files_identical": same,
           "host_wall": _stats(wall["host"][1:]), "device_wall": _stats(wall["device"][1:])}
    res["device_below_host_by_more_than_either_spread"] = _faster(res["host_wall"], res["device_wall"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=256)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--x", type=int, default=0)
    ap.add_argument("--identity", type=int, default=95)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device-only", action="store_true", help="leave the host path out (profiling runs)")
    ap.add_argument("--align", type=int, default=0, help="also run columba_align end to end on a FASTQ of this many reads")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rlc", action="store_true", help="the b-move backend on a pan-genome-like text (below 2^32 characters)")
    ap.add_argument("--haplotypes", type=int, default=64)
    ap.add_argument("--base-mbp", type=float, default=4)
    ap.add_argument("--snp", type=float, default=0.005)
    ap.add_argument("--kmer-size", type=int, default=10)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    n = int(args.genome_mbp * 1e6)
    t0 = time.time()
    R, L = args.reads, args.read_len
    if args.rlc:
        from columba_amd import movebuild
        base = int(args.base_mbp * 1e6)
        text = movebuild.pangenome(base, args.haplotypes, args.snp, seed=1)
        mv = movebuild.build_move(text, device=dev, with_locate=False)
        mv.plcp = movebuild.plcp_gpu(mv)
        torch.cuda.empty_cache()
        index = ca.MoveIndex(mv, device=0)
        n = int(text.shape[0])
        starts = np.array([min(j * base, n) for j in range(args.haplotypes)] + [n], dtype=np.uint32)
        index.attach_text(text, starts)
        print(f"[best_rate] b-move index of {n / 1e6:.1f} Mbp ({args.haplotypes} haplotypes), n/r = {mv.n / mv.runs_fwd:.1f}, built in "
              f"{time.time() - t0:.1f} s", flush=True)
        g = torch.from_numpy(text).to(dev)
        ix = None
    else:
        g, starts = synth.genome_human_like(n, seed=2025, device=dev)
        ix = ib.build_index(g, seq_starts=starts, device=dev, with_bwt=False)
        index = ca.Index(ix, device=0)
        print(f"[best_rate] index for {n / 1e6:.0f} Mbp, {len(starts) - 1} sequences, built in {time.time() - t0:.1f} s", flush=True)
    buf, offs = synth.sample_reads_fast(g, R, L, seed=3, device=dev)
    del g
    torch.cuda.empty_cache()
    rng = np.random.default_rng(17)
    ids = [b"@SRR0000001.%d %d length=%d" % (i + 1, i + 1, L) for i in range(R)]
    quals = (rng.integers(0, 41, R * L, dtype=np.uint8) + 33)
    qoffs = (np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    names = [b"chr%d" % (j + 1) for j in range(len(starts) - 1)]
    pi, pn = ca.pack_fields(ids), ca.pack_fields(names)  # (packed once: the arms measure the library)
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    lib = ca.lib()

    host_fn, dev_fn = (lib.cmb_move_match_best, lib.cmb_move_match_best_device) if args.rlc else (lib.cmb_match_best, lib.cmb_match_best_device)

    def match(fn):
        h = C.c_void_p()
        extra = (args.kmer_size,) if args.rlc else ()
        rc = fn(index.h, st.h, args.x, args.identity, *extra, ca._p(buf), ca._p(offs), R, C.byref(h))
        assert rc == 0, lib.cmb_last_error()
        return h

    def arm_results(fn):
        t = time.perf_counter()
        h = match(fn)
        t1 = time.perf_counter()
        res = ca._best_results(h, R)
        t2 = time.perf_counter()
        return h, res, (t2 - t) * 1e3, (t1 - t) * 1e3

    def arm_sam():
        t = time.perf_counter()
        h = match(dev_fn)
        t1 = time.perf_counter()
        inp = ca.SamInputs(ca._p(buf), ca._p(pi[0]), ca._p(pi[1]), ca._p(quals), ca._p(qoffs), ca._p(pn[0]), ca._p(pn[1]), len(names))
        text, length, host_reads = C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = lib.cmb_best_sam_device(h, C.byref(inp), 1, 0, C.byref(text), C.byref(length), C.byref(host_reads))
        t2 = time.perf_counter()  # (the call returns after the download: the text is in host memory)
        assert rc == 0, lib.cmb_last_error()
        return h, (t2 - t) * 1e3, (t2 - t1) * 1e3, int(length.value), int(host_reads.value)

    def timings(h):
        names_ = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        k = lib.cmb_best_timings(h, names_, ms, 64)
        return {names_[i].decode(): round(float(ms[i]), 3) for i in range(k)}

    a, b, b_match, c, c_sam = [], [], [], [], []
    equal, parts, text_bytes, host_reads, n_occ = None, {}, 0, 0, 0
    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        ra = None
        if not args.device_only:
            h, ra, dt, _ = arm_results(host_fn)
            lib.cmb_best_destroy(h)
            if keep:
                a.append(dt)
        h, rb, dt, dm = arm_results(dev_fn)
        if keep:
            b.append(dt), b_match.append(dm)
            parts = timings(h)
        lib.cmb_best_destroy(h)
        n_occ = int(len(rb[0]))
        if ra is not None:
            equal = all(np.array_equal(x, y) for x, y in zip(ra[:6], rb[:6])) and ra[6] == rb[6]
            assert equal, "cmb_match_best_device differs from cmb_match_best"
        del ra, rb
        h, dt, ds, text_bytes, host_reads = arm_sam()
        lib.cmb_best_destroy(h)
        if keep:
            c.append(dt), c_sam.append(ds)
        print(f"[best_rate] repetition {rep}: a {a[-1] if a and keep else float('nan'):.1f} ms, b {b[-1] if keep else float('nan'):.1f} ms, "
              f"c {c[-1] if keep else float('nan'):.1f} ms", flush=True)
    res = {"tool": "best_rate --rlc" if args.rlc else "best_rate", "genome_mbp": n / 1e6, "reads": R, "read_len": L, "x": args.x, "identity": args.identity, "reps": args.reps,
           "occurrences": n_occ, "sam_text_bytes": text_bytes, "host_reads": host_reads, "a_equals_b": equal,
           "result_bytes": int(n_occ * (16 + 24) + 16 * (R + 1)),
           "b_match_best_device_plus_results": _stats(b), "b_match_call_alone": _stats(b_match),
           "c_match_best_device_plus_sam_device": _stats(c), "c_sam_call_alone": _stats(c_sam),
           "device_path_parts_ms_last_repetition": parts}
    if a:
        res["a_match_best_plus_results"] = _stats(a)
        res["b_below_a_by_more_than_either_spread"] = _faster(res["a_match_best_plus_results"], res["b_match_best_device_plus_results"])
        res["c_below_a_by_more_than_either_spread"] = _faster(res["a_match_best_plus_results"], res["c_match_best_device_plus_sam_device"])
    if args.align and not args.rlc:
        with tempfile.TemporaryDirectory() as tmp:
            res["columba_align"] = _align(ix, buf, offs, min(args.align, R), L, 3, tmp)
    else:
        res["columba_align"] = "not measured"
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
