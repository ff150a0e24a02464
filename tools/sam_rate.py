#!/usr/bin/env python3
"""How long the SAM text of a single-end chunk takes: the host formatter (ONE cmb_batch_sam call into a sufficient buffer)
against the device path (cmb_batch_sam_device, including the packing of its inputs, their upload and the download of the
text), beside the matching itself (cmb_batch_run with alignments).  One process, seeded, the three alternating.

Workload: columba_align's default chunk — 10^6 x 150 bp reads with FASTQ-like identifiers and qualities, k = 4, edit
distance, columba scheme, dynamic partitioning — on a synth.genome_human_like text (default 256 Mbp).

    python tools/sam_rate.py --out profiles/sam_device_rate.json
    rocprofv3 --kernel-trace --stats -d DIR -o sam -- python tools/sam_rate.py --reps 2 --device-only   (a run of its own)

--rlc: the same question on the b-move backend, on a `bench.py --config rlc` style text (haplotypes of one random sequence; below
2^32 characters, so that the text fits beside the index): the host path (MoveBatch.sam's steps: download of the records, conversion
to 32-bit records, cmb_sam_chunk) against cmb_move_batch_sam_device on the lists the batch kept in HBM, beside cmb_move_batch_run
with and without those lists.

    python tools/sam_rate.py --rlc --out profiles/move_sam_device_rate.json
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


def main_rlc(args):
    import torch
    from columba_amd import movebuild
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    t0 = time.time()
    base = int(args.base_mbp * 1e6)
    text = movebuild.pangenome(base, args.haplotypes, args.snp, seed=1)
    mv = movebuild.build_move(text, device=dev, with_locate=False)
    mv.plcp = movebuild.plcp_gpu(mv)
    torch.cuda.empty_cache()
    index = ca.MoveIndex(mv, device=0)
    n = int(text.shape[0])
    starts = np.array([min(j * base, n) for j in range(args.haplotypes)] + [n], dtype=np.uint32)
    index.attach_text(text, starts)
    print(f"[sam_rate] b-move index of {n / 1e6:.1f} Mbp ({args.haplotypes} haplotypes), n/r = {mv.n / mv.runs_fwd:.1f}, built in "
          f"{time.time() - t0:.1f} s", flush=True)
    R, L = args.reads, args.read_len
    buf, offs = synth.sample_reads_fast(torch.from_numpy(text).to(dev), R, L, seed=3, device=dev)
    torch.cuda.empty_cache()
    rng = np.random.default_rng(17)
    ids = [b"@SRR0000001.%d %d length=%d" % (i + 1, i + 1, L) for i in range(R)]
    qual_bytes = (rng.integers(0, 41, R * L, dtype=np.uint8) + 33)
    quals = [qual_bytes[i * L:(i + 1) * L].tobytes() for i in range(R)]
    names = [b"hap%d" % (j + 1) for j in range(args.haplotypes)]
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    plain = ca.MoveBatch(index, st, args.k, packed=(buf, offs), kmer_size=args.kmer_size)
    plain.want_alignments()
    kept = ca.MoveBatch(index, st, args.k, packed=(buf, offs), kmer_size=args.kmer_size)
    kept.want_alignments()
    kept.keep_device_lists()
    L_ = ca.lib()
    ai, aq, an = (C.c_char_p * R)(*ids), (C.c_char_p * R)(*quals), (C.c_char_p * len(names))(*names)
    tix = L_.cmb_move_text_index(index.h)

    def run(b):
        t = time.perf_counter()
        b.run()
        return (time.perf_counter() - t) * 1e3

    host_buf = {}

    def host_sam():  # MoveBatch.sam's steps on the plain batch
        t = time.perf_counter()
        occ, occ_offs, _ = plain.results()
        aln, ops = plain.alignments()
        t1 = time.perf_counter()
        occ32 = np.zeros(max(len(occ), 1), ca.OCC_DTYPE)
        for f in ("begin", "end", "distance", "strand"):
            occ32[f][:len(occ)] = occ[f]
        t2 = time.perf_counter()
        a = (tix, args.k, ca.METRIC["edit"], ca._p(buf), ca._p(offs), R, ai, aq, an, ca._p(occ32), ca._p(occ_offs), ca._p(aln), ca._p(ops), 1,
             int(args.xa))
        if "out" not in host_buf:  # (sizes the buffer; not timed)
            need = L_.cmb_sam_chunk(*a, None, 0)
            assert need >= 0, L_.cmb_last_error()
            host_buf["out"] = C.create_string_buffer(int(need) + 1)
            t2 = time.perf_counter()
        out = host_buf["out"]
        got = L_.cmb_sam_chunk(*a, out, len(out))
        t3 = time.perf_counter()
        assert 0 <= got < len(out)
        return ((t3 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), got, len(occ)

    def device_sam():
        t = time.perf_counter()
        pi, pq, pn = ca.pack_fields(ids), ca.pack_fields(quals), ca.pack_fields(names)
        t1 = time.perf_counter()
        inp = ca.SamInputs(ca._p(buf), ca._p(pi[0]), ca._p(pi[1]), ca._p(pq[0]), ca._p(pq[1]), ca._p(pn[0]), ca._p(pn[1]), len(names))
        text_, length, host_reads = C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = L_.cmb_move_batch_sam_device(kept.h, C.byref(inp), 1, int(args.xa), C.byref(text_), C.byref(length), C.byref(host_reads))
        t2 = time.perf_counter()
        assert rc == 0, L_.cmb_last_error()
        return (t2 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3, text_.value, int(length.value), int(host_reads.value)

    a, a_keep, b, b_fetch, b_conv, b_fmt, c, c_pack, c_call = [], [], [], [], [], [], [], [], []
    equal, n_occ, length, host_reads = None, 0, 0, 0
    for rep_ in range(args.warmup + args.reps):
        keep = rep_ >= args.warmup
        da, dk = run(plain), run(kept)
        if not args.device_only:
            hb, n_host, n_occ = host_sam()
        dt, dp, dc, text_, length, host_reads = device_sam()
        if not args.device_only:
            equal = (length == n_host) and C.string_at(text_, length) == host_buf["out"].raw[:n_host]
            assert equal, "the device text differs from the host text"
        if keep:
            a.append(da), a_keep.append(dk), c.append(dt), c_pack.append(dp), c_call.append(dc)
            if not args.device_only:
                b.append(hb[0]), b_fetch.append(hb[1]), b_conv.append(hb[2]), b_fmt.append(hb[3])
        print(f"[sam_rate] repetition {rep_}: run {da:.1f} ms, run with kept lists {dk:.1f} ms, device sam {dt:.1f} ms", flush=True)
    res = {"tool": "sam_rate --rlc", "text_mbp": n / 1e6, "haplotypes": args.haplotypes, "n_over_r": round(mv.n / mv.runs_fwd, 1), "reads": R,
           "read_len": L, "k": args.k, "xa": bool(args.xa), "reps": args.reps, "occurrences": int(n_occ), "text_bytes": length,
           "host_reads": host_reads, "texts_equal": equal, "a_run_with_alignments": _stats(a), "a_run_with_kept_lists": _stats(a_keep),
           "c_sam_device_total": _stats(c), "c_packing": _stats(c_pack), "c_call": _stats(c_call),
           "link_ms_at_63GBps": round(length / 63e9 * 1e3, 3)}
    if b:
        res["b_sam_host_total"] = _stats(b)
        res["b_fetch_records"], res["b_convert_records"], res["b_cmb_sam_chunk"] = _stats(b_fetch), _stats(b_conv), _stats(b_fmt)
        sb, sc = res["b_sam_host_total"], res["c_sam_device_total"]
        res["c_below_b_by_more_than_either_spread"] = bool(
            sb["median_ms"] - sc["median_ms"] > max(sb["max_ms"] - sb["min_ms"], sc["max_ms"] - sc["min_ms"]))
    plain.close()
    kept.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=256)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--xa", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="leave the host formatter out (profiling runs)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rlc", action="store_true", help="the b-move backend on a pan-genome-like text (see above)")
    ap.add_argument("--haplotypes", type=int, default=64)
    ap.add_argument("--base-mbp", type=float, default=4)
    ap.add_argument("--snp", type=float, default=0.005)
    ap.add_argument("--kmer-size", type=int, default=10)
    args = ap.parse_args()
    if args.rlc:
        return main_rlc(args)

    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    n = int(args.genome_mbp * 1e6)
    t0 = time.time()
    g, starts = synth.genome_human_like(n, seed=2025, device=dev)
    ix = ib.build_index(g, seq_starts=starts, device=dev, with_bwt=False)
    index = ca.Index(ix, device=0)
    print(f"[sam_rate] index for {n / 1e6:.0f} Mbp, {len(starts) - 1} sequences, built in {time.time() - t0:.1f} s", flush=True)
    R, L = args.reads, args.read_len
    buf, offs = synth.sample_reads_fast(g, R, L, seed=3, device=dev)
    del g
    torch.cuda.empty_cache()
    rng = np.random.default_rng(17)
    ids = [b"@SRR0000001.%d %d length=%d" % (i + 1, i + 1, L) for i in range(R)]
    qual_bytes = (rng.integers(0, 41, R * L, dtype=np.uint8) + 33)
    quals = [qual_bytes[i * L:(i + 1) * L].tobytes() for i in range(R)]
    names = [b"chr%d" % (j + 1) for j in range(len(starts) - 1)]

    batch = ca.Batch(index, ca.SearchStrategy("columba", "edit", "dynamic"), args.k, packed=(buf, offs))
    batch.want_alignments()
    L_ = ca.lib()
    # the host formatter's inputs: char* arrays, made once outside the timed calls
    ai, aq, an = (C.c_char_p * R)(*ids), (C.c_char_p * R)(*quals), (C.c_char_p * len(names))(*names)

    def run():
        t = time.perf_counter()
        batch.run()  # (ends in a synchronise: the results are on the host)
        return (time.perf_counter() - t) * 1e3

    host_buf = {}

    def host_sam():
        if "out" not in host_buf:  # (sizes the buffer; not timed)
            need = L_.cmb_batch_sam(batch.h, ca._p(buf), ai, aq, an, 1, int(args.xa), None, 0)
            assert need >= 0, need
            host_buf["out"] = C.create_string_buffer(int(need) + 1)
        out = host_buf["out"]
        t = time.perf_counter()
        got = L_.cmb_batch_sam(batch.h, ca._p(buf), ai, aq, an, 1, int(args.xa), out, len(out))
        dt = (time.perf_counter() - t) * 1e3
        assert 0 <= got < len(out)
        return dt, got

    def device_sam():
        t = time.perf_counter()
        pi, pq, pn = ca.pack_fields(ids), ca.pack_fields(quals), ca.pack_fields(names)
        t1 = time.perf_counter()
        inp = ca.SamInputs(ca._p(buf), ca._p(pi[0]), ca._p(pi[1]), ca._p(pq[0]), ca._p(pq[1]), ca._p(pn[0]), ca._p(pn[1]), len(names))
        text, length, host_reads = C.c_void_p(), C.c_uint64(), C.c_uint64()
        rc = L_.cmb_batch_sam_device(batch.h, C.byref(inp), 1, int(args.xa), C.byref(text), C.byref(length), C.byref(host_reads))
        t2 = time.perf_counter()  # (the call returns after the download: the text is in host memory)
        assert rc == 0, L_.cmb_last_error()
        return (t2 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3, text.value, int(length.value), int(host_reads.value)

    for _ in range(args.warmup):
        run()
        if not args.device_only:
            host_sam()
        device_sam()
    a, b, c, c_pack, c_call = [], [], [], [], []
    equal = None
    for _ in range(args.reps):
        a.append(run())
        if not args.device_only:
            dt, n_host = host_sam()
            b.append(dt)
        dt, dp, dc, text, length, host_reads = device_sam()
        c.append(dt), c_pack.append(dp), c_call.append(dc)
        if not args.device_only:
            equal = (length == n_host) and C.string_at(text, length) == host_buf["out"].raw[:n_host]
            assert equal, "the device text differs from the host text"
    occs, _, _ = batch.results()
    res = {"tool": "sam_rate", "genome_mbp": n / 1e6, "reads": R, "read_len": L, "k": args.k, "xa": bool(args.xa), "reps": args.reps,
           "occurrences": int(len(occs)), "text_bytes": length, "host_reads": host_reads, "texts_equal": equal,
           "input_bytes": int(sum(len(x) for x in ids) + R * L + 16 * (R + 1)),
           "a_run_with_alignments": _stats(a), "c_sam_device_total": _stats(c), "c_packing": _stats(c_pack), "c_call": _stats(c_call),
           "link_ms_at_63GBps": round(length / 63e9 * 1e3, 3)}
    if b:
        res["b_sam_host"] = _stats(b)
        sb, sc = res["b_sam_host"], res["c_sam_device_total"]
        res["c_below_b_by_more_than_either_spread"] = bool(
            sb["median_ms"] - sc["median_ms"] > max(sb["max_ms"] - sb["min_ms"], sc["max_ms"] - sc["min_ms"]))
    batch.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
