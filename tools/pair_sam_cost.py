#!/usr/bin/env python3
"""Milliseconds per 10^6 read pairs that the SAM text of an ALL-mode chunk costs behind the matching: the host path of the C++ adapter
(samOfChunkPairedAll: lists copied, cmb_pair_sam per pair) against its device path (CMB_PAIR_DEVICE=1: cmb_pair_sam_device_classes with every
class on the device; CMB_PAIR_DEVICE_CLASSES=0 in the environment gives cmb_pair_sam_device's split).

150 bp reads, k = 4, FR, true fragments of 250 - 500 bp with an edit in about half of the mates and a mate from nowhere in --junk of the
pairs.  The reference is a synthetic text of --mbp: the repeat-rich one of the tests, or with --text human the human-like one of tools/sam_rate.py.  Every GPU step is a process of its own under a time
limit: the index build, the host path, the device path; the first one that fails ends the run.  Prints the two JSON lines of
tools/pair_sam_cost.cpp and a summary line; the two texts must be the same.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args):
    import numpy as np
    import columba_amd as ca  # noqa: F401
    from columba_amd import indexbuild as ib, synth
    if args.text == "human":  # the human-like text of tools/sam_rate.py: chromosomes, repeat families at their natural share
        gd, starts = synth.genome_human_like(int(args.mbp * 1e6), seed=2025, device="cuda:0")
        g = gd.cpu().numpy()
        del gd
    else:
        g, starts = synth.genome_rep(seed=2, n=int(args.mbp * 1e6), scale=2.0)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    ix.seq_names = [f"chr{i}" for i in range(len(starts) - 1)]
    ib.save_index(ix, os.path.join(args.dir, "idx"))
    rng = np.random.default_rng(4)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    L = 150
    p0 = rng.integers(1000, len(g) - 2000, args.pairs)
    frag = rng.integers(250, 501, args.pairs)
    with open(os.path.join(args.dir, "r1.txt"), "wb") as f1, open(os.path.join(args.dir, "r2.txt"), "wb") as f2:
        for i in range(args.pairs):
            f = g[int(p0[i]):int(p0[i]) + int(frag[i])].tobytes()
            a, b = bytearray(f[:L]), bytearray(f[-L:].translate(comp)[::-1])
            if rng.random() < args.junk:
                b = bytearray(rng.integers(0, 4, L).astype(np.uint8).tobytes().translate(bytes.maketrans(bytes(range(4)), b"ACGT")))
            for m in (a, b):
                if rng.random() < 0.5:
                    q = int(rng.integers(10, L - 10))
                    m[q] = b"ACGT"[(b"ACGT".index(m[q]) + 1) % 4]
            if i % 2:
                a, b = b, a
            f1.write(bytes(a) + b"\n")
            f2.write(bytes(b) + b"\n")
    print(json.dumps({"sequences": len(starts) - 1, "text": len(g)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=16.0, help="size of the reference")
    ap.add_argument("--text", choices=["rep", "human"], default="rep", help="synth.genome_rep (repeat-rich) or synth.genome_human_like")
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--junk", type=float, default=0.02, help="share of pairs with a mate from nowhere (formatted on the host)")
    ap.add_argument("--repetitions", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="time limit of every GPU step in seconds")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "build":
        return build(args)
    import columba_amd as ca
    ca.build_library()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pair_sam_cost")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "pair_sam_cost.cpp"), "-o", exe,
                               "-L", os.path.join(ROOT, "columba_amd"), "-lcolumba_amd", "-Wl,-rpath," + os.path.join(ROOT, "columba_amd"),
                               "-Wl,-rpath,/opt/rocm/lib"])
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "build", "--dir", tmp, "--mbp", str(args.mbp), "--pairs", str(args.pairs),
                              "--junk", str(args.junk), "--text", args.text], capture_output=True, text=True, timeout=args.limit)
        if out.returncode:
            sys.exit(f"the index build failed ({out.returncode}): {out.stderr[-2000:]}")
        world = json.loads(out.stdout.strip().splitlines()[-1])
        lines = {}
        for device in ("0", "1"):
            run = subprocess.run([exe, os.path.join(tmp, "idx"), os.path.join(tmp, "r1.txt"), os.path.join(tmp, "r2.txt"), str(world["sequences"]), "4", "500",
                                  "200", str(args.repetitions)], capture_output=True, text=True, timeout=args.limit, env=dict(os.environ, CMB_PAIR_DEVICE=device))
            if run.returncode:
                sys.exit(f"the {'device' if device == '1' else 'host'} path failed ({run.returncode}): {run.stderr[-2000:]}")
            lines[device] = json.loads(run.stdout.strip().splitlines()[-1])
            print(json.dumps(lines[device]))
        host, dev = lines["0"], lines["1"]
        same = host["text_hash"] == dev["text_hash"] and host["text_bytes"] == dev["text_bytes"]
        print(json.dumps({"text": args.text, "reference_bp": world["text"], "pairs": args.pairs, "host_ms_per_1e6_pairs": host["after_ms_per_1e6_pairs"],
                          "device_ms_per_1e6_pairs": dev["after_ms_per_1e6_pairs"], "speedup": round(host["after_ms_per_1e6_pairs"] / max(dev["after_ms_per_1e6_pairs"], 1e-9), 2),
                          "host_pair_share": dev["host_pair_share"], "same_text": same}))
        if not same:
            sys.exit("the two paths wrote different texts")


if __name__ == "__main__":
    main()
