"""The SAM text of a chunk — single-end in ALL and BEST mode, read pairs in ALL and BEST mode — validated against the reference
SEQUENCE alone (tests/samcheck.py): no occurrence array, no oracle result takes part.  Every other SAM test compares one formatter with
another written from the same reading of the reference aligner; a misreading they share is invisible there.  Here every alignment a record or an XA
entry claims is walked over read and text window, its edits must be the window's edit distance by plain dynamic programming
(oracle/groundtruth.c) and at most NM = AS <= k (the read's cut-off in BEST mode); flags, SEQ / QUAL, MAPQ, X0 / X1, RNEXT / PNEXT /
TLEN follow from the records themselves.  For read pairs cut from a uniform random text the fragment must come back as a proper pair
where it was cut (ALL mode is lossless; BEST at x = 0 whenever the edits are within the cut-off).

The CPU tests run the checker on the oracle's text and on pairs built by hand, and show that it rejects corrupted text.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

from columba_amd import synth  # noqa: E402
from test_ground_truth import gt  # noqa: E402,F401
from test_best_ground_truth import LENGTHS, _world, chunk as best_chunk, cutoff  # noqa: E402
import samcheck  # noqa: E402

NAMES = ["chrA", "chrB", "chrC", "chrD"]


def _se_chunk(k, metric="edit", seed=0):
    """about 210 reads of 40 ... 250 characters with up to k + 1 edits, and three reads across every inner sequence end"""
    w = _world()
    g, starts = w["genome"], w["starts"]
    model = dict(p_sub=1.0, p_ins=0.0) if metric == "hamming" else {}
    reads = []
    for li, length in enumerate(LENGTHS):
        reads += synth.sample_reads(g, 40, length, seed=4000 + 10 * k + li + seed, n_frac=0.03,
                                    edit_choices=(0, 0, 1, 2, max(k - 1, 0), k, k + 1), **model)
    for s in starts[1:-1]:
        reads += [g[s - 50:s + 50].tobytes(), g[s - 2:s + 98].tobytes(), g[s - 147:s + 3].tobytes()]
    reads[3] = reads[3].lower()
    rng = np.random.default_rng(17 + k)
    ids = [("@" if i % 2 else ">") + f"read{i}/1 length={len(r)}" for i, r in enumerate(reads)]
    ids[1] = "@nospace"
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    return reads, ids, quals


def _reference(gt):
    w = _world()
    return samcheck.Reference(w["text"], NAMES, w["starts"], gt)


def _report(label, st):
    print(f"{label}: " + ", ".join(f"{k} {v}" for k, v in st.items()))


def _check_all_mode(gt, label, text, reads, ids, quals, k, xa, metric="edit", unmapped=True):
    ref = _reference(gt)
    st = samcheck.check_single_end(text, ref, reads, ids, quals, limit=k, unmapped=unmapped, xa=xa, metric=metric)
    _report(label, st)
    assert len(text) > 10_000
    assert st["mapped"] >= 60 and st["alignments"] >= 150 and st["reverse"] >= 20
    assert st["secondary"] >= 20
    assert st["loose"] * 50 <= st["alignments"], st
    if unmapped:
        assert st["unmapped"] >= 5 and st["absent"] == 0
    return st


# ------------------------------------------------------------------------------------------------ CPU: oracle text, hand-made pairs
@pytest.fixture(scope="module")
def cpu_world(oracle_built):
    import oracle_py as op
    from columba_amd import indexbuild as ib
    w = _world()
    ix = ib.build_index(w["text"], seq_starts=np.asarray(w["starts"], np.uint32), device="cpu")
    return {"op": op, "orc": op.OracleIndex(ix), "texts": {}}


ALL_CONFIGS = [("columba", "edit", 4, False), ("multiple_opt", "edit", 2, True), ("columba", "edit", 9, False)]


def _oracle_text(cw, spec, metric, k, xa):
    import schemes_py as sp
    key = (spec, metric, k, xa)
    if key not in cw["texts"]:
        reads, ids, quals = _se_chunk(k, metric)
        cw["texts"][key] = cw["op"].match_batch_sam(cw["orc"], cw["op"].OracleStrategy(sp.BY_NAME[spec], metric, "dynamic"), k, reads, ids,
                                                    quals, NAMES, unmapped=True, xa=xa)
    return cw["texts"][key]


@pytest.mark.parametrize("spec,metric,k,xa", ALL_CONFIGS)
def test_oracle_sam_text_against_the_reference_sequence(cpu_world, gt, spec, metric, k, xa):
    reads, ids, quals = _se_chunk(k, metric)
    _check_all_mode(gt, f"oracle {spec} k={k} xa={xa}", _oracle_text(cpu_world, spec, metric, k, xa), reads, ids, quals, k, xa, metric)


def _edit_line(text, pick, change):
    """the text with `change(fields)` applied to the first line `pick(fields)` accepts"""
    lines = text.splitlines()
    for i, ln in enumerate(lines):
        f = ln.split("\t")
        if pick(f):
            lines[i] = "\t".join(change(f))
            return "\n".join(lines) + "\n"
    raise AssertionError("no line to corrupt")


def test_checker_rejects_corrupted_text(cpu_world, gt):
    """the checker itself: one field of one record changed, a record dropped, two records swapped — each is caught"""
    reads, ids, quals = _se_chunk(4)
    good = _oracle_text(cpu_world, "columba", "edit", 4, False)
    xa_good = _oracle_text(cpu_world, "multiple_opt", "edit", 2, True)
    reads2, ids2, quals2 = _se_chunk(2)

    def rejected(text, xa=False):
        args = (reads2, ids2, quals2, 2) if xa else (reads, ids, quals, 4)
        with pytest.raises(AssertionError):
            samcheck.check_single_end(text, _reference(gt), *args[:3], limit=args[3], unmapped=True, xa=xa)

    def put(i, v):
        def change(f):
            f[i] = v(f[i])
            return f
        return change

    mapped = lambda f: not int(f[1]) & 4  # noqa: E731
    with_edit = lambda f: mapped(f) and "NM:i:0" not in f and int(f[3]) > 1  # noqa: E731
    rejected(_edit_line(good, with_edit, put(3, lambda v: str(int(v) + 1))))           # POS shifted by one
    rejected(_edit_line(good, with_edit, put(3, lambda v: str(int(v) - 1))))
    rejected(_edit_line(good, lambda f: f[4] == "60", put(4, lambda v: "59")))           # MAPQ
    rejected(_edit_line(good, lambda f: f[4] == "0" and mapped(f), put(4, lambda v: "3")))
    rejected(_edit_line(good, mapped, put(2, lambda v: "chrE")))                         # RNAME
    rejected(_edit_line(good, lambda f: f[1] == "0", put(1, lambda v: "16")))            # strand
    rejected(_edit_line(good, lambda f: f[1] == "16", put(10, lambda v: v[::-1] if v != v[::-1] else v[1:] + "!")))  # QUAL not reversed
    rejected(_edit_line(good, with_edit, put(12, lambda v: "NM:i:0")))                   # NM below the window's distance
    rejected(_edit_line(good, lambda f: "I" in f[5] or "D" in f[5], put(5, lambda v: f"{samcheck.cigar_width(v)}M")))  # CIGAR
    rejected(_edit_line(good, lambda f: f[1] == "4", put(9, lambda v: v[:-1])))          # SEQ of an unmapped read
    lines = good.splitlines()
    first_of_two = next(i for i in range(len(lines) - 1) if int(lines[i].split("\t")[1]) in (0, 16)
                        and int(lines[i + 1].split("\t")[1]) & 256 and lines[i].split("\t")[4] != "0")
    rejected("\n".join(lines[:first_of_two] + [lines[first_of_two + 1], lines[first_of_two]] + lines[first_of_two + 2:]) + "\n")  # swapped
    tie = next(i for i in range(len(lines) - 1) if int(lines[i + 1].split("\t")[1]) & 256 and lines[i + 1].split("\t")[4] != "0")
    rejected("\n".join(lines[:tie + 1] + lines[tie + 2:]) + "\n")                        # a co-optimal record dropped: MAPQ no longer fits
    only = next(i for i in range(1, len(lines) - 1) if lines[i].split("\t")[4] == "60")
    rejected("\n".join(lines[:only] + lines[only + 1:]) + "\n")                          # the only record of a read dropped
    rejected("\n".join(lines[1:] + lines[:1]) + "\n")                                    # input order
    rejected(_edit_line(xa_good, lambda f: any(t.startswith("X0:i:") for t in f), lambda f: [("X0:i:7" if t.startswith("X0:i:") else t) for t in f]), xa=True)
    rejected(_edit_line(xa_good, lambda f: any(t.startswith("XA:Z:c") for t in f),
                        lambda f: [(t.replace(",+", ",-", 1) if "+" in t else t.replace(",-", ",+", 1)) if t.startswith("XA:Z:") else t for t in f]), xa=True)


def _pairs(g, starts, regions, k, seed, n=150, n_far=20, n_junk=10, length=100):
    """FR fragments with inserts of 200 ... 450 and 0 ... k edits per mate; n_far pairs with the mates 5 kb apart; n_junk pairs with a random
    mate, those with at most one edit.  Returns reads1, reads2 and per pair the truth (sequence, 1-based POS of the forward mate, of the reverse one) or None."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def edited(s, ne):
        r = bytearray(s)
        for _ in range(ne):
            p = int(rng.integers(2, len(r) - 2))
            u = rng.random()
            if u < 0.7:
                r[p] = b"ACGT"[(b"ACGT".index(bytes([r[p]])) + int(rng.integers(1, 4))) % 4]
            elif u < 0.85:
                r.insert(p, b"ACGT"[int(rng.integers(0, 4))])
            else:
                del r[p]
        return bytes(r)

    r1, r2, truth = [], [], []
    for i in range(n + n_far + n_junk):
        lo, hi = regions[i % len(regions)]
        frag = int(rng.integers(200, 451))
        gap = 5000 if n <= i < n + n_far else 0
        p0 = int(rng.integers(lo, hi - frag - gap))
        q0 = p0 + gap + frag - length
        # (outside the fragments at most one edit: where no pair is formed BEST mode asks the strata 0, 1, 3, 5, ... of a mate already
        # searched only whether THEY hold something, hasUpdate in searchstrategy.cpp:668-674, so a mate whose best alignment has 2 or 4
        # edits is reported unmapped there; tests/test_pairing_best.py has that case)
        most = k if i < n else 1
        a = edited(g[p0:p0 + length].tobytes(), int(rng.integers(0, most + 1)))
        b = edited(synth.revcomp(g[q0:q0 + length].tobytes()), int(rng.integers(0, most + 1)))
        if i >= n + n_far:
            b = acgt[rng.integers(0, 4, length)].tobytes()
        sid = int(np.searchsorted(np.asarray(starts), p0, side="right") - 1)
        t = (sid, p0 - starts[sid] + 1, q0 - starts[sid] + 1) if i < n else None
        if i % 2:  # the fragment from the other strand: mate 1 is the reverse-complement end
            a, b = b, a
        r1.append(a)
        r2.append(b)
        truth.append(t)
    return r1, r2, truth


def _pair_inputs(r1, r2):
    n = len(r1)
    rng = np.random.default_rng(5)
    ids1, ids2 = [f"@pair{i}/1 first" for i in range(n)], [f"@pair{i}/2 second" for i in range(n)]
    q1 = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in r1]
    q2 = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in r2]
    return ids1, ids2, q1, q2


def _assert_fragments_found(groups, truth, names, k):
    """every simulated fragment is a proper pair at the place it was cut from: both POS within 4k (2k for the filter's window on the
    begin, 2k for the width of an alignment with k indels)"""
    found = 0
    for g, t in zip(groups, truth):
        if t is None:
            continue
        sid, pf, pr = t
        fw = [r for r in g if r["flag"] & 2 and not r["flag"] & 16 and r["rname"] == names[sid] and abs(r["pos"] - pf) <= 4 * k]
        ok = any(r["rnext"] in ("=", names[sid]) and abs(r["pnext"] - pr) <= 4 * k for r in fw)
        assert ok, (t, [r["line"] for r in g])
        found += 1
    return found


def test_paired_checker_on_pairs_built_by_hand(gt):
    """cmb_pair_sam (host code of the library: no GPU) on occurrence lists written down from where the mates were cut, substitutions only:
    the paired rules hold, the fragments come back, and corrupted text is rejected"""
    import columba_amd as ca
    g, starts = synth.genome_small(seed=4, n=60_000)
    starts = [int(s) for s in starts]
    names = ["one", "two"]
    rng = np.random.default_rng(12)
    L = 100
    r1, r2, truth, occs = [], [], [], []
    for i in range(40):
        frag = int(rng.integers(200, 451))
        far = i % 8 == 7
        p0 = int(rng.integers(40_000, 52_000 - frag))
        q0 = p0 + frag - L + (3000 if far else 0)
        a, b = bytearray(g[p0:p0 + L].tobytes()), bytearray(synth.revcomp(g[q0:q0 + L].tobytes()))
        da, db = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        for m, d in ((a, da), (b, db)):
            for p in rng.choice(np.arange(5, 95), d, replace=False):
                m[p] = b"ACGT"[(b"ACGT".index(bytes([m[p]])) + 1) % 4]
        lone = i % 8 == 5
        sid = 1
        oa = [(sid, p0 - starts[sid], p0 - starts[sid] + L, p0, da, 0, np.array([L << 2], np.uint16))]
        ob = [] if lone else [(sid, q0 - starts[sid], q0 - starts[sid] + L, q0, db, 1, np.array([L << 2], np.uint16))]
        if lone:
            b = bytearray(b"ACGT"[int(c)] for c in rng.integers(0, 4, L))
        t = None if (far or lone) else (sid, p0 - starts[sid] + 1, q0 - starts[sid] + 1)
        if i % 2:
            a, b, oa, ob = b, a, ob, oa
        r1.append(bytes(a))
        r2.append(bytes(b))
        truth.append(t)
        occs.append((oa, ob))
    ids1, ids2, q1, q2 = _pair_inputs(r1, r2)
    for disc in (True, False):
        text = []
        for i in range(len(r1)):
            rd = []
            for reads, ids, quals, oc in ((r1, ids1, q1, occs[i][0]), (r2, ids2, q2, occs[i][1])):
                sid, seq, rc, rq = ca.read_prepare(ids[i], reads[i].decode(), quals[i])
                rd.append((sid, seq, rc, quals[i], rq, oc))
            text.append(ca.pair_sam(rd[0], rd[1], names, ca.ORIENTATION_FR, 600, 100, disc, True)[0])
        text = "".join(text)
        ref = samcheck.Reference(g.tobytes(), names, starts, gt)
        st, groups = samcheck.check_paired(text, ref, r1, r2, ids1, ids2, q1, q2, limit=2, orientation=samcheck.ORIENTATION_FR, min_frag=100,
                                           max_frag=600)
        _report(f"hand-made pairs, discordant pairs {'allowed' if disc else 'not allowed'}", st)
        assert _assert_fragments_found(groups, truth, names, 2) == 30
        assert st["proper"] == 60 and st["unmapped"] == 5 and st["mate_unmapped"] == 5
        assert (st["discordant"], st["unpaired"]) == ((10, 0) if disc else (0, 10))

        def rejected(bad):
            with pytest.raises(AssertionError):
                samcheck.check_paired(bad, samcheck.Reference(g.tobytes(), names, starts, gt), r1, r2, ids1, ids2, q1, q2, limit=2,
                                      orientation=samcheck.ORIENTATION_FR, min_frag=100, max_frag=600)

        def put(i, v):
            def change(f):
                f[i] = v(f[i])
                return f
            return change

        proper = lambda f: int(f[1]) & 2  # noqa: E731
        rejected(_edit_line(text, proper, put(3, lambda v: str(int(v) + 1))))            # POS: the alignment and the mate's PNEXT
        rejected(_edit_line(text, proper, put(7, lambda v: str(int(v) + 1))))            # PNEXT
        rejected(_edit_line(text, proper, put(8, lambda v: str(int(v) + 1))))            # TLEN
        rejected(_edit_line(text, proper, put(8, lambda v: str(-int(v)))))               # its sign
        rejected(_edit_line(text, proper, put(1, lambda v: str(int(v) ^ 32))))           # flag 32
        rejected(_edit_line(text, proper, put(1, lambda v: str(int(v) ^ 192))))          # first / second in pair
        rejected(_edit_line(text, lambda f: int(f[1]) & 4, put(1, lambda v: str(int(v) ^ 8))))  # flag 8
        if disc:  # a discordant pair called proper
            rejected(_edit_line(text, lambda f: not int(f[1]) & (2 | 4 | 8) and f[6] != "*", put(1, lambda v: str(int(v) | 2))))


# ------------------------------------------------------------------------------------------------ GPU: the HIP paths
@pytest.fixture(scope="module")
def gpu_world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import columba_amd as ca
    from columba_amd import indexbuild as ib, movebuild
    w = _world()
    starts = np.asarray(w["starts"], np.uint32)
    ix = ib.build_index(w["text"], seq_starts=starts, device="cuda")
    mdev = ca.MoveIndex(movebuild.build_move(w["text"], device="cuda"))
    mdev.attach_text(w["text"], starts)
    pg, pstarts = synth.genome_small(seed=4, n=200_000)
    pix = ib.build_index(pg.tobytes(), seq_starts=pstarts, device="cuda")
    return {"ca": ca, "dev": ca.Index(ix), "mdev": mdev, "pg": pg, "pstarts": [int(s) for s in pstarts], "pdev": ca.Index(pix)}


@pytest.mark.gpu
@pytest.mark.parametrize("spec,metric,k,xa", ALL_CONFIGS + [("columba", "hamming", 3, False)])
def test_all_mode_sam_text(gpu_world, gt, spec, metric, k, xa):
    """Batch.sam (host formatter) and Batch.sam_device (k_sam_plan, k_sam_write)"""
    ca = gpu_world["ca"]
    reads, ids, quals = _se_chunk(k, metric)
    b = ca.Batch(gpu_world["dev"], ca.SearchStrategy(spec, metric, "dynamic"), k, reads)
    b.want_alignments()
    b.run()
    host = b.sam(ids, quals, NAMES, unmapped=True, xa=xa)
    dev, _ = b.sam_device(ids, quals, NAMES, unmapped=True, xa=xa)
    bare, _ = b.sam_device(ids, None, NAMES, unmapped=False, xa=xa)
    b.close()
    _check_all_mode(gt, f"Batch.sam {spec} {metric} k={k} xa={xa}", host, reads, ids, quals, k, xa, metric)
    _check_all_mode(gt, f"Batch.sam_device {spec} {metric} k={k} xa={xa}", dev, reads, ids, quals, k, xa, metric)
    _check_all_mode(gt, "Batch.sam_device without qualities and unmapped records", bare, reads, ids, None, k, xa, metric, unmapped=False)


@pytest.mark.gpu
@pytest.mark.parametrize("x,xa", [(0, False), (0, True), (1, False), (1, True)])
def test_best_mode_sam_text(gpu_world, gt, x, xa):
    """BestDevice.sam_device (k_sam_plan_best) on the mixed-length chunk of tests/test_best_ground_truth.py: NM within the read's own
    cut-off, nHits counted before duplicates are removed"""
    ca = gpu_world["ca"]
    cfg = ("columba", "edit", x, 95 - x)
    reads = best_chunk(cfg)
    rng = np.random.default_rng(3)
    ids = [f"@best{i} x={x}" for i in range(len(reads))]
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    cuts = [cutoff(cfg[0], cfg[3], len(r)) for r in reads]
    b = ca.BestDevice(gpu_world["dev"], ca.SearchStrategy(cfg[0], cfg[1], "dynamic"), reads, x=x, min_identity=cfg[3])
    text, _ = b.sam_device(ids, quals, NAMES, unmapped=True, xa=xa)
    b.close()
    st = samcheck.check_single_end(text, _reference(gt), reads, ids, quals, limit=cuts, unmapped=True, xa=xa, best_mode=True)
    _report(f"BestDevice.sam_device x={x} xa={xa}", st)
    assert len(text) > 10_000
    assert st["mapped"] >= 60 and st["unmapped"] >= 20 and st["alignments"] >= 150 and st["reverse"] >= 20 and st["secondary"] >= 20
    assert st["loose"] * 50 <= st["alignments"]


@pytest.mark.gpu
def test_bmove_sam_text(gpu_world, gt):
    """MoveBatch.sam: the records of the b-move backend's occurrences"""
    ca = gpu_world["ca"]
    reads, ids, quals = _se_chunk(4, seed=1)
    mb = ca.MoveBatch(gpu_world["mdev"], ca.SearchStrategy("columba", "edit", "dynamic"), 4, reads=reads, kmer_size=8)
    mb.want_alignments()
    mb.run()
    text = mb.sam(ids, quals, NAMES)
    mb.close()
    _check_all_mode(gt, "MoveBatch.sam columba k=4", text, reads, ids, quals, 4, False)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all", "best"])
def test_paired_sam_text(gpu_world, gt, mode):
    """pair_chunk_sam / pair_chunk_sam_best on fragments cut from a uniform random text, away from its duplicated segment"""
    ca = gpu_world["ca"]
    pg, pstarts = gpu_world["pg"], gpu_world["pstarts"]
    names = ["left", "right"]
    k = 3
    regions = [(46_000, 99_000), (154_000, 199_000)]  # (genome_small copies [20 000, 45 000) to [128 571, 153 571))
    r1, r2, truth = _pairs(pg, pstarts, regions, k, seed=31 if mode == "all" else 32)
    ids1, ids2, q1, q2 = _pair_inputs(r1, r2)
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    for disc in (True, False):
        if mode == "all":
            text, mapped = ca.pair_chunk_sam(gpu_world["pdev"], st, k, r1, r2, ids1, ids2, q1, q2, names, ca.ORIENTATION_FR, 600, 100, disc, True)
            limit = k
        else:
            text, mapped, _ = ca.pair_chunk_sam_best(gpu_world["pdev"], st, r1, r2, ids1, ids2, q1, q2, names, x=0, min_identity=95,
                                                     orientation=ca.ORIENTATION_FR, max_frag=600, min_frag=100, discordant_allowed=disc)
            limit = [(cutoff("columba", 95, len(a)), cutoff("columba", 95, len(b))) for a, b in zip(r1, r2)]
        ref = samcheck.Reference(pg.tobytes(), names, pstarts, gt)
        c, groups = samcheck.check_paired(text, ref, r1, r2, ids1, ids2, q1, q2, limit=limit, orientation=samcheck.ORIENTATION_FR,
                                          min_frag=100, max_frag=600)
        _report(f"pairs, {mode} mode, discordant pairs {'allowed' if disc else 'not allowed'}", c)
        assert len(text) > 10_000
        assert _assert_fragments_found(groups, truth, names, k) == 150
        assert c["proper"] >= 300 and c["unmapped"] >= 8 and c["mate_unmapped"] >= 8
        assert (c["discordant"] >= 30 and c["unpaired"] == 0) if disc else (c["discordant"] == 0 and c["unpaired"] >= 30)
