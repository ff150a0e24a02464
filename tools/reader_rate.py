#!/usr/bin/env python3
"""What a FASTQ chunk costs from the file to the packed arrays the batches take: (a) Reader::getNextChunk plus the packing loop
columba_align runs on its records, against (b) DeviceReader::getNextChunk (window read, upload, the kernels of csrc/dev_reads.hpp,
download into page-locked arrays).  One process (tools/reader_rate.cpp, built here with g++), the two alternating chunk by chunk on
one file that holds warm-up + repetitions chunks and lies in the page cache; then the parts of (b) — upload, kernels, download — as
the library prints them under CMB_VERBOSE, from a second pass over the file.

Workload: columba_align's default chunk — 10^6 x 150 bp reads with FASTQ-like identifiers and qualities.

    python tools/reader_rate.py --out profiles/read_parser_rate.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o reads -- <dir>/reader_rate <dir>/reads.fq 1000000 2     (a run of its own; --keep)

"resolved" is the rule of DESIGN.md §4.7: (b)'s median lies below (a)'s by more than the sum of the two spreads (max - min).
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import columba_amd as ca  # noqa: E402


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "all_ms": [round(x, 3) for x in ms]}


def fastq_block(reads: int, read_len: int, seed: int = 17) -> bytes:
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, reads * read_len)].tobytes()
    qual = (rng.integers(0, 41, reads * read_len, dtype=np.uint8) + 33).tobytes()
    L = read_len
    return b"".join(b"@SRR0000001.%d %d length=%d\n%s\n+\n%s\n" % (i + 1, i + 1, L, seq[i * L:(i + 1) * L], qual[i * L:(i + 1) * L])
                    for i in range(reads))


def build_driver(directory: str) -> str:
    ca.build_library()
    exe = os.path.join(directory, "reader_rate")
    lib_dir = os.path.join(ROOT, "columba_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "reader_rate.cpp"),
                           "-o", exe, "-L", lib_dir, "-lcolumba_amd", "-lz", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the FASTQ file and the driver go (default: a temporary directory)")
    ap.add_argument("--keep", action="store_true", help="keep the directory (for a profiling run of the driver)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    directory = args.dir or tempfile.mkdtemp(prefix="reader_rate_")
    os.makedirs(directory, exist_ok=True)
    chunks = args.warmup + args.reps
    try:
        exe = build_driver(directory)
        block = fastq_block(args.reads, args.read_len)
        fq = os.path.join(directory, "reads.fq")
        with open(fq, "wb") as f:
            for _ in range(chunks):
                f.write(block)
        with open(fq, "rb") as f:  # (read once: the file is in the page cache)
            while f.read(1 << 26):
                pass
        print(f"[reader_rate] {chunks} chunks of {args.reads} records, {len(block) * chunks / 1e6:.0f} MB in {fq}", flush=True)
        env = dict(os.environ)
        env.pop("CMB_VERBOSE", None)
        run = subprocess.run([exe, fq, str(args.reads), str(chunks)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
        sys.stderr.write("".join(ln + "\n" for ln in run.stderr.splitlines() if not ln.startswith("[grid]")))
        assert run.returncode == 0, run.returncode
        a = [float(x) for x in re.findall(r"^A ([0-9.]+)$", run.stdout, re.M)]
        b = [float(x) for x in re.findall(r"^B ([0-9.]+)$", run.stdout, re.M)]
        equal = re.findall(r"^EQUAL (\d) (\d+)$", run.stdout, re.M)
        assert len(a) == len(b) == len(equal) == chunks, run.stdout
        assert all(e == "1" and int(n) == args.reads for e, n in equal), equal
        parts = re.findall(r"\[reads\] (\d+) bytes, (\d+) records: upload ([0-9.]+) ms, kernels ([0-9.]+) ms, download ([0-9.]+) ms", run.stderr)
        parts = [p for p in parts if int(p[1]) == args.reads][args.warmup:]
        sa, sb = _stats(a[args.warmup:]), _stats(b[args.warmup:])
        res = {"tool": "reader_rate", "reads": args.reads, "read_len": args.read_len, "reps": args.reps, "warmup": args.warmup,
               "chunk_bytes": len(block), "arrays_equal": True,
               "a_reader_and_packing": sa, "b_device_reader": sb,
               "a_gb_per_s": round(len(block) / sa["median_ms"] / 1e6, 3), "b_gb_per_s": round(len(block) / sb["median_ms"] / 1e6, 3),
               "b_below_a_by_more_than_the_sum_of_the_spreads": bool(
                   sa["median_ms"] - sb["median_ms"] > (sa["max_ms"] - sa["min_ms"]) + (sb["max_ms"] - sb["min_ms"]))}
        if parts:
            res["b_window_bytes"] = statistics.median(float(p[0]) for p in parts)
            for k, name in ((2, "b_upload"), (3, "b_kernels"), (4, "b_download")):
                res[name] = _stats([float(p[k]) for p in parts])
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    finally:
        if not args.keep and not args.dir:
            shutil.rmtree(directory, ignore_errors=True)


if __name__ == "__main__":
    main()
