"""The C++ host adapter's device path for read pairs in ALL mode with every class of pairs on the device: samOfChunkPairedAll with
CMB_PAIR_DEVICE=1 calls cmb_pair_sam_device_classes with CMB_PAIR_CLASS_ALL, so columba_align writes the same SAM body as on the host
path — with and without discordant pairs — and only the pairs with an occurrence over a sequence end reach the host formatter."""
import os
import re
import subprocess

import numpy as np
import pytest

import columba_amd as ca
from test_cpp_adapter import _build_align

pytestmark = pytest.mark.gpu

K, N, L = 2, 252, 80


def _spanning_pairs(dev, r1, r2):
    """the pairs with an occurrence the host has to trim: cmb_aln.spans != 0 in either mate's per-strand lists"""
    spans = []
    for reads in (r1, r2):
        b = ca.Batch(dev, ca.SearchStrategy("multiple_opt", "edit", "dynamic"), K, reads=reads)
        b.want_alignments()
        ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
        b.run()
        _, offs, _ = b.results()
        aln, _ = b.alignments()
        b.close()
        spans.append([bool(np.any(aln["spans"][int(offs[i]):int(offs[i + 1])])) for i in range(len(reads))])
    return sum(a or b for a, b in zip(*spans))


def test_align_driver_pairs_every_class_on_the_device(tmp_path):
    from columba_amd import indexbuild as ib, synth
    exe = _build_align(str(tmp_path))
    g, starts = synth.genome_rep(seed=2, n=300_000, scale=2.0)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    ix.seq_names = [f"chr{i}" for i in range(len(starts) - 1)]
    ib.save_index(ix, str(tmp_path / "idx"))
    assert len(starts) > 2, "mates in another sequence need a second sequence"
    rng = np.random.default_rng(9)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    r1, r2 = [], []
    for i in range(N):
        frag = int(rng.integers(200, 380))
        p0 = int(rng.integers(500, len(g) - 900))
        f = g[p0:p0 + frag].tobytes()
        a, b = bytearray(f[:L]), bytearray(f[-L:].translate(comp)[::-1])
        if i % 7 == 0:
            b = bytearray(bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)))  # a mate from nowhere
        if i % 7 == 3:  # a mate in another sequence
            s = int(np.searchsorted(starts, p0, side="right")) % (len(starts) - 1)
            q0 = int(rng.integers(int(starts[s]) + 200, int(starts[s + 1]) - 200 - L))
            b = bytearray(g[q0:q0 + L].tobytes().translate(comp)[::-1])
        if i % 2:
            a, b = b, a
        r1.append(bytes(a))
        r2.append(bytes(b))
    q = "".join(chr(33 + i % 40) for i in range(L))
    (tmp_path / "r1.fq").write_text("".join(f"@p{i}/1 x\n{r1[i].decode()}\n+\n{q}\n" for i in range(N)))
    (tmp_path / "r2.fq").write_text("".join(f"@p{i}/2 x\n{r2[i].decode()}\n+\n{q}\n" for i in range(N)))
    spanning = _spanning_pairs(ca.Index(ix), r1, r2)
    for extra in ([], ["-nD"]):
        bodies, logs = {}, {}
        for device in ("0", "1"):
            out = tmp_path / f"o{device}.sam"
            env = dict(os.environ, CMB_PAIR_DEVICE=device, CMB_VERBOSE="1")
            env.pop("CMB_PAIR_DEVICE_CLASSES", None)
            run = subprocess.run([exe, "-r", str(tmp_path / "idx"), "-f", str(tmp_path / "r1.fq"), "-F", str(tmp_path / "r2.fq"), "-o", str(out),
                                  "-a", "all", "-e", str(K), "-S", "multiple_opt", "-b", "100", "-X", "500", "-N", "100"] + extra,
                                 capture_output=True, text=True, env=env)
            assert run.returncode == 0, run.stderr
            bodies[device] = b"".join(ln for ln in out.read_bytes().splitlines(keepends=True) if not ln.startswith(b"@"))
            logs[device] = run.stderr
        assert bodies["1"] == bodies["0"] and bodies["0"].count(b"\n") > 2 * 0.6 * N
        lines = [ln for ln in logs["1"].splitlines() if ln.startswith("[host] pair sam:")]
        assert lines and not any(ln.startswith("[host] pair sam:") for ln in logs["0"].splitlines())
        counts = {name: sum(int(re.search(rf"(\d+) {name}", ln).group(1)) for ln in lines)
                  for name in ("pairs", "of them formatted on the host", "one unmapped", "discordant", "unpaired", "concordant")}
        print(extra, counts, "spanning:", spanning)
        assert counts["pairs"] == N and counts["of them formatted on the host"] == spanning
        # (the text is rich in repeats, so a mate from another sequence may still find a concordant partner: at least half of them do not)
        assert counts["one unmapped"] >= N // 7 - spanning
        assert counts["unpaired" if extra else "discordant"] >= N // 14 and counts["discordant" if extra else "unpaired"] == 0
        assert all("(classes 15)" in ln for ln in lines)
