#!/usr/bin/env python3
"""What a chunk on a reference of many short sequences costs with the occurrences over a sequence end trimmed by the host class of
cmb_batch_sam_device (samOfRead -> trimOccurrence: two blocking round trips per occurrence) against the same chunk with the run
trimming them itself (cmb_batch_trim_on_device).  One process, seeded, the two paths alternating; either path is cmb_batch_run with
alignments + cmb_batch_sam_device (packing of the inputs included), the switch-off path being the code as it was before the switch
existed.

Workload: 150 bp reads, k = 4, edit distance, columba scheme, dynamic partitioning, on a synth.genome_human_like text cut into
sequences whose mean length (default 1500) makes roughly a tenth of the reads run over a sequence end.

    python tools/trim_rate.py --out profiles/trim_device_rate.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import columba_amd as ca  # noqa: E402
from columba_amd import indexbuild as ib, synth  # noqa: E402


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "all_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=256)
    ap.add_argument("--mean-seq-len", type=int, default=1500)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    n = int(args.genome_mbp * 1e6)
    t0 = time.time()
    g, _ = synth.genome_human_like(n, seed=2025, device=dev)
    rng = np.random.default_rng(11)
    cuts = np.unique(rng.integers(1, n, max(1, n // args.mean_seq_len - 1)))
    starts = np.concatenate([[0], cuts, [n]]).astype(np.uint32)
    ix = ib.build_index(g, seq_starts=starts, device=dev, with_bwt=False)
    index = ca.Index(ix, device=0)
    n_seqs = len(starts) - 1
    print(f"[trim_rate] index for {n / 1e6:.0f} Mbp in {n_seqs} sequences (mean {n / n_seqs:.0f}), built in {time.time() - t0:.1f} s", flush=True)
    R, L = args.reads, args.read_len
    buf, offs = synth.sample_reads_fast(g, R, L, seed=3, device=dev)
    del g
    torch.cuda.empty_cache()
    ids = [b"@SRR0000001.%d %d length=%d" % (i + 1, i + 1, L) for i in range(R)]
    qual_bytes = (rng.integers(0, 41, R * L, dtype=np.uint8) + 33)
    quals = [qual_bytes[i * L:(i + 1) * L].tobytes() for i in range(R)]
    names = [b"ctg%d" % (j + 1) for j in range(n_seqs)]
    L_ = ca.lib()
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    batches = {}
    for label, on in (("off", False), ("on", True)):
        b = ca.Batch(index, st, args.k, packed=(buf, offs))
        b.want_alignments()
        if on:
            b.trim_on_device()
        batches[label] = b

    def chunk(b):
        """cmb_batch_run + cmb_batch_sam_device -> (total, run, sam) in ms, the text, the reads the host formatted"""
        t = time.perf_counter()
        b.run()
        t1 = time.perf_counter()
        pi, pq, pn = ca.pack_fields(ids), ca.pack_fields(quals), ca.pack_fields(names)
        inp = ca.SamInputs(ca._p(buf), ca._p(pi[0]), ca._p(pi[1]), ca._p(pq[0]), ca._p(pq[1]), ca._p(pn[0]), ca._p(pn[1]), len(names))
        text, length, host_reads = C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = L_.cmb_batch_sam_device(b.h, C.byref(inp), 1, 0, C.byref(text), C.byref(length), C.byref(host_reads))
        t2 = time.perf_counter()
        assert rc == 0, L_.cmb_last_error()
        return ((t2 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3), C.string_at(text.value, length.value), int(host_reads.value)

    times = {"off": ([], [], []), "on": ([], [], [])}
    stage = {}
    host_reads = {}
    equal = None
    for rep in range(args.warmup + args.reps):
        texts = {}
        for label in ("off", "on"):
            ms, texts[label], host_reads[label] = chunk(batches[label])
            if rep >= args.warmup:
                for acc, v in zip(times[label], ms):
                    acc.append(v)
                if label == "on":
                    for name, v in batches["on"].timings().items():
                        if name.startswith("k_trim"):
                            stage.setdefault(name, []).append(v)
            print(f"[trim_rate] repetition {rep} switch {label}: run {ms[1]:.1f} ms, sam {ms[2]:.1f} ms, host_reads {host_reads[label]}", flush=True)
        equal = texts["off"] == texts["on"]
        assert equal, "the text with the switch differs from the text without"
    occs, _, _ = batches["on"].results()
    res = {"tool": "trim_rate", "genome_mbp": n / 1e6, "sequences": n_seqs, "mean_seq_len": round(n / n_seqs, 1), "reads": R, "read_len": L,
           "k": args.k, "reps": args.reps, "occurrences": int(len(occs)), "trim_stats": batches["on"].trim_stats(),
           "host_reads_switch_off": host_reads["off"], "host_reads_switch_on": host_reads["on"], "texts_equal": equal,
           "text_bytes": len(texts["on"])}
    for label in ("off", "on"):
        res[f"switch_{label}_total"], res[f"switch_{label}_run"], res[f"switch_{label}_sam_device"] = (_stats(x) for x in times[label])
    res["switch_on_stage"] = {name: _stats(v) for name, v in stage.items()}
    a, b = res["switch_off_total"], res["switch_on_total"]
    res["on_below_off_by_more_than_the_sum_of_the_spreads"] = bool(
        a["median_ms"] - b["median_ms"] > (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"]))
    for b_ in batches.values():
        b_.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
