"""The HIP paths on references of many short sequences (tests/contigs.py): 383 sequences of 1 ... 599 characters, and 20 000 sequences of
6.  On such a reference a quarter of all occurrences runs over a sequence end, so what is the exception everywhere else in the suite is
the rule here: findSeqName's assignment with a lookup deeper than 2^14, the `spans` flag, trimming with re-verification
(trimOccurrence -> cmb_verify_window -> cmb_cigar_windows, beyond 7 errors through k_verify_wide) onto next sequences shorter than the
read, occurrences over three and more sequences, the host class of the three device SAM writers for MOST mapped reads, bestCheckHost moving
trimmed occurrences between strata, the `over` flag of k_pair_plan, sequence names from 2 to 70 bytes in k_sam_write and k_pair_write.

Bars: the oracle's text and lists, byte for byte and bit for bit; tests/samcheck.py; and ground truth that knows the sequences
(contigs.per_sequence_truth, contigs.check_per_sequence): ZERO truth ends without a record within 4k, no record whose NM is above the true
distance of its window, and in BEST mode at x = 0 `best == d*` for every read.  tests/test_contigs.py holds the oracle alone to the same
conditions on the same inputs, without a GPU.

Run with `pytest -m gpu` on an MI355X.  Observed there (printed by the tests):
  lookup      contig_world k = 2 (FM and b-move): 324 occurrences, 73 over a sequence end, 24 over three sequences or more; b-move
              k = 0: 218 / 56 / 13; dense_world: 60 / 60 / 60, sequences from below 2^10 to above 2^14; the miniature layouts: 129, 67
              and 126 occurrences, 129, 39 and 24 of them begin in the last sequence, 0, 3 and 6 run over an end; CIGARs of 463 (k = 4)
              and 733 (k = 10) occurrences
  ALL mode    path                   k  occurrences  over an end  host_reads  mapped  unmapped  ends judged  exceptions
              Batch columba          2          324           73          72     159        69          609           0
              Batch multiple_opt XA  4          436          117          97     141        87         1918           0
              Batch columba          7          646          162          91     160        68         3666           0
              Batch columba         10          589          196          99     156        72         3639           0
              MoveBatch columba      4          436          117          97     141        87         1918           0
              MoveBatch kuch1        0          218           56          56     108       120          162           0
              Batch kuch1 Hamming    2          209           51          50     119       109   (158 windows inside a sequence, all
                                                                                               reported; 47 reads with spanning windows only)
              host_reads is the number of reads with a spanning occurrence everywhere: 42 ... 69 % of the mapped reads; every text is
              the oracle's and the host formatter's, byte for byte; loose 0 everywhere
  dense       60 occurrences, all over an end; 60 unmapped records, host_reads 60
  BEST        columba x = 0 95 %: best == d* on 400 of 400 (167 mapped), 238 records, 129 host reads; multiple_opt x = 0 97 %: 400 of
              400 (63 mapped), 108 records, 39 host reads; columba x = 1 95 %: 103 mapped, 129 records, 130 host reads, best differs
              from d* on 67 reads — 63 with d* = 0 (stratum 0 is never looked at with x > 0) and 4 others
  pairs       170 pairs, 124 mapped; k_pair_plan left 55 to the host class and wrote 1040 records itself; 1546 proper records (a
              tandem repeat gives one fragment hundreds of pairs), 8 discordant, 61 unmapped, 31 with an unmapped mate; BEST mode: 1546
              proper, 6 discordant, 75 unmapped
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import columba_amd as ca  # noqa: E402
from columba_amd import indexbuild as ib, movebuild, synth  # noqa: E402
from test_ground_truth import gt  # noqa: E402,F401
from test_best_ground_truth import NONE, assert_oracle_parity, cutoff, max_supported, norm_lib, norm_oracle  # noqa: E402
from test_sam_ground_truth import _assert_fragments_found, _pair_inputs, _report  # noqa: E402
from test_contigs import best_truth, check_all_mode, check_best_equals_dstar, check_hamming  # noqa: E402
import contigs  # noqa: E402
import samcheck  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(oracle_built):
    """the three indexes of the module: FM index and b-move index (with its text) of contig_world, FM index of dense_world"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    out = {"op": op}
    for w in (contigs.contig_world(), contigs.dense_world()):
        ix = ib.build_index(w["text"], seq_starts=np.asarray(w["starts"], np.uint32), device="cuda")
        out[w["label"]] = dict(w, ix=ix, dev=ca.Index(ix), orc=op.OracleIndex(ix))
    w = out["contig"]
    w["mdev"] = ca.MoveIndex(movebuild.build_move(w["text"], device="cuda"))
    w["mdev"].attach_text(w["text"], np.asarray(w["starts"], np.uint32))
    return out


def _same(a, b, what):
    if a != b:
        n = min(len(a), len(b))
        i = next((j for j in range(n) if a[j] != b[j]), n)
        raise AssertionError(f"{what}: lengths {len(a)} / {len(b)}, first difference at {i}: {a[max(0, i - 120):i + 60]!r} / {b[max(0, i - 120):i + 60]!r}")


def _dense_reads():
    d = contigs.dense_world()
    rng = np.random.default_rng(3)
    return [d["text"][p:p + 30] for p in rng.integers(0, 120_000 - 30, 60).tolist()]


def _spanning_reads(aln, offs, n):
    return sum(1 for i in range(n) if (aln["spans"][int(offs[i]):int(offs[i + 1])] != 0).any())


# ------------------------------------------------------------------------------------------------ a. the sequence lookup
def _lookup_of_batch(b, starts, label):
    b.want_alignments()
    b.run()
    occ, offs, _ = b.results()
    aln, _ = b.alignments()
    assert len(aln) == len(occ)
    n_spans, n_last, n_three = contigs.assert_lookup(aln, occ, starts)
    print(f"{label}: {len(occ)} occurrences, {n_spans} over a sequence end, {n_three} over three sequences or more, {n_last} begin in the last sequence")
    b.close()
    return occ, n_spans, n_last, n_three


def test_lookup_contig_world(world):
    """k_cigar's binary search over 384 starts: seq_id, seq_begin and spans of every occurrence at k = 2"""
    w = world["contig"]
    reads, _, _ = contigs.chunk(2)
    occ, n_spans, _, n_three = _lookup_of_batch(ca.Batch(w["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), 2, reads), w["starts"], "contig_world k=2")
    assert len(occ) >= 250 and n_spans * 10 >= len(occ) and n_three >= 5


def test_lookup_dense_world(world):
    """... over 20 001 starts: deeper than 2^14.  Every occurrence of a 30-character read runs over five sequences at least"""
    w = world["dense"]
    reads = _dense_reads()
    occ, n_spans, _, n_three = _lookup_of_batch(ca.Batch(w["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), 2, reads), w["starts"], "dense_world k=2")
    assert len(occ) >= 60 and n_spans == n_three == len(occ)
    st = np.asarray(w["starts"], np.int64)
    first = np.searchsorted(st, occ["begin"].astype(np.int64), side="right") - 1
    last = np.searchsorted(st, occ["end"].astype(np.int64) - 1, side="right") - 1
    assert (last - first >= 4).all() and first.max() > 1 << 14 and first.min() < 1 << 10


@pytest.mark.parametrize("layout", [0, 1, 2], ids=["one-sequence-no-starts", "two-sequences", "three-sequences"])
def test_lookup_miniature_layouts(layout):
    """1, 2 and 3 sequences (the first without seq_starts at all): the other end of the search's depth.  Reads over every inner sequence
    end, the first and the last 100 characters of the text"""
    label, g, starts = contigs.mini_layouts()[layout]
    ix = ib.build_index(g.tobytes(), device="cuda") if starts is None else ib.build_index(g.tobytes(), seq_starts=np.asarray(starts, np.uint32), device="cuda")
    real = [0, len(g)] if starts is None else starts
    assert [int(s) for s in ix.seq_starts] == real
    reads = synth.sample_reads(g, 60, 100, seed=40 + layout, edit_choices=(0, 0, 1, 2))
    for s in real[1:-1]:
        reads += [g[s - 50:s + 50].tobytes(), g[s - 1:s + 99].tobytes(), g[s - 99:s + 1].tobytes(), g[s:s + 100].tobytes(), g[s - 100:s].tobytes()]
    reads += [g[:100].tobytes(), g[-100:].tobytes()]
    dev = ca.Index(ix)
    occ, n_spans, n_last, _ = _lookup_of_batch(ca.Batch(dev, ca.SearchStrategy("columba", "edit", "dynamic"), 2, reads), real, label)
    dev.close()
    assert len(occ) >= 60 and n_last >= 1 and n_spans >= 3 * (len(real) - 2)
    assert (occ["end"] == len(g)).any() and (occ["begin"] == 0).any()


@pytest.mark.parametrize("k", [4, 10])
def test_cigars_on_contig_world(world, oracle_built, k):
    """k_cigar (k = 4) and k_cigar_wide (k = 10): the CIGAR of every occurrence is findCIGAR's, the sequence assignment findSeqName's
    (the assertions of test_gpu_parity._check_alignments, here with spans set on a quarter of the occurrences)"""
    from test_gpu_parity import _check_alignments
    w = world["contig"]
    reads = contigs.chunk(k, 50, (40, 60, 100, 150))[0] + synth.sample_reads(w["genome"], 120, 100, seed=60 + k, edit_choices=(2, 3, 4), p_sub=0.3, p_ins=0.35)
    n = _check_alignments(w, oracle_built, "columba", "edit", k, reads, 300)
    print(f"contig_world k={k}: CIGARs of {n} occurrences")


@pytest.mark.parametrize("spec,k", [("columba", 2), ("kuch1", 0)])
def test_lookup_bmove(world, spec, k):
    """MoveBatch.alignments(): the device lookup at k = 2, the host's upper_bound at k = 0"""
    w = world["contig"]
    reads, _, _ = contigs.chunk(k)
    mb = ca.MoveBatch(w["mdev"], ca.SearchStrategy(spec, "edit", "dynamic"), k, reads=reads, kmer_size=8)
    occ, n_spans, _, n_three = _lookup_of_batch(mb, w["starts"], f"b-move contig_world k={k}")
    assert len(occ) >= 150 and n_spans * 10 >= len(occ) and n_three >= 3


# ------------------------------------------------------------------------------------------------ b. ALL mode, single end, FM index
# (strategy, metric, k, XA tag, lengths of the sampled reads: at 10 errors 40 instead of 30 characters — with a third of a read in errors
# the oracle alone leaves the per-sequence rule, tests/test_contigs.py)
ALL_CONFIGS = [("columba", "edit", 2, False, (30, 60, 100, 150)), ("multiple_opt", "edit", 4, True, (30, 60, 100, 150)),
               ("columba", "edit", 7, False, (30, 60, 100, 150)), ("columba", "edit", 10, False, (40, 60, 100, 150))]


def _texts_of_batch(world, b, label, spec, metric, k, xa, reads, ids, quals):
    """host text == device text == oracle text, with and without unmapped records; host_reads == the reads with a spanning occurrence.
    Returns (text with unmapped records, host_reads)"""
    import schemes_py as sp
    w, op = world["contig"], world["op"]
    _, offs, _ = b.results()
    aln, _ = b.alignments()
    spanning = _spanning_reads(aln, offs, len(reads))
    n_spans = int((aln["spans"] != 0).sum())
    ost = op.OracleStrategy(sp.BY_NAME[spec], metric, "dynamic")
    keep = None
    for unmapped in (True, False):
        host = b.sam(ids, quals, w["names"], unmapped=unmapped, xa=xa)
        got, host_reads = b.sam_device(ids, quals, w["names"], unmapped=unmapped, xa=xa)
        print(f"{label} unmapped={unmapped}: {len(aln)} occurrences, {n_spans} over a sequence end, {len(got)} bytes, host_reads={host_reads}, spanning reads={spanning}")
        _same(got, host, "device text / host text")
        assert host_reads == spanning
        if k > 0:  # (at k = 0 the reference's order of equal matches is the suffix array's: tests/test_gpu_sam_device._norm_k0)
            _same(got, op.match_batch_sam(w["orc"], ost, k, reads, ids, quals, w["names"], unmapped=unmapped, xa=xa), "device text / oracle text")
        keep = keep or (got, host_reads)
    assert n_spans * 10 >= len(aln)
    return keep


@pytest.mark.parametrize("spec,metric,k,xa,lengths", ALL_CONFIGS)
def test_all_mode_fm(world, gt, spec, metric, k, xa, lengths):
    """Batch.sam, Batch.sam_device (k_sam_plan, k_sam_write: the host class for a quarter of the mapped reads at least) and the oracle"""
    w = world["contig"]
    reads, ids, quals = contigs.chunk(k, 50, lengths)
    label = f"Batch {spec} {metric} k={k} xa={xa}"
    b = ca.Batch(w["dev"], ca.SearchStrategy(spec, metric, "dynamic"), k, reads)
    b.want_alignments()
    b.run()
    text, host_reads = _texts_of_batch(world, b, label, spec, metric, k, xa, reads, ids, quals)
    b.close()
    st = check_all_mode(gt, label, text, reads, ids, quals, k, xa)
    assert host_reads * 4 >= st["mapped"], (host_reads, st)


# ------------------------------------------------------------------------------------------------ c. Hamming distance
def test_hamming_drops_spanning_occurrences(world, gt):
    """under Hamming distance an occurrence over a sequence end is dropped, never trimmed: the records are exactly the windows of the
    read's length with <= k mismatches that lie inside one sequence, and a read all of whose windows span an end is unmapped"""
    w = world["contig"]
    k = 2
    reads, ids, quals = contigs.chunk(k)
    b = ca.Batch(w["dev"], ca.SearchStrategy("kuch1", "hamming", "dynamic"), k, reads)
    b.want_alignments()
    b.run()
    text, host_reads = _texts_of_batch(world, b, "Batch kuch1 hamming k=2", "kuch1", "hamming", k, False, reads, ids, quals)
    b.close()
    st = check_hamming(gt, "Batch.sam_device kuch1 hamming k=2", text, reads, ids, quals, k)
    print(f"host_reads={host_reads}")
    assert host_reads >= 30


# ------------------------------------------------------------------------------------------------ d. dense_world
def test_dense_world_all_unmapped(world):
    """60 exact reads of 30 characters on sequences of 6: every read has occurrences, all of them over an end, and no trim window of 6
    characters holds 30 characters within 2 errors — 60 unmapped records, all written by the host class"""
    import schemes_py as sp
    w, op = world["dense"], world["op"]
    reads = _dense_reads()
    ids, quals = [f"@dense{i} x" for i in range(60)], ["".join(chr(40 + (i + j) % 30) for j in range(30)) for i in range(60)]
    b = ca.Batch(w["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), 2, reads)
    b.want_alignments()
    b.run()
    _, offs, _ = b.results()
    aln, _ = b.alignments()
    assert (np.diff(offs.astype(np.int64)) > 0).all() and (aln["spans"] != 0).all()
    ost = op.OracleStrategy(sp.BY_NAME["columba"], "edit", "dynamic")
    for unmapped in (True, False):
        host = b.sam(ids, quals, w["names"], unmapped=unmapped)
        got, host_reads = b.sam_device(ids, quals, w["names"], unmapped=unmapped)
        _same(got, host, "device text / host text")
        _same(got, op.match_batch_sam(w["orc"], ost, 2, reads, ids, quals, w["names"], unmapped=unmapped), "device text / oracle text")
        assert host_reads == 60
        lines = got.splitlines()
        assert len(lines) == (60 if unmapped else 0) and all(x.split("\t")[1:4] == ["4", "*", "0"] for x in lines)
    b.close()


# ------------------------------------------------------------------------------------------------ e. BEST mode
@pytest.mark.parametrize("spec,x,min_identity", [("columba", 0, 95), ("multiple_opt", 0, 97), ("columba", 1, 95)])
def test_best_mode(world, gt, spec, x, min_identity):
    """match_best (bestCheckHost), match_best_device and best_sam_device where the best alignment of most reads lies next to a sequence
    end: the oracle's lists bit for bit; at x = 0 best == d* for every read; at x = 1 (the reference does not look at every stratum
    there) sound records, and the number of reads whose best is not d* printed"""
    import schemes_py as sp
    from test_gpu_best_device import _assert_same, _sam_of_best
    w, op = world["contig"], world["op"]
    reads = contigs.best_chunk()
    st = ca.SearchStrategy(spec, "edit", "dynamic")
    O = norm_oracle(op.match_best(w["orc"], op.OracleStrategy(sp.BY_NAME[spec], "edit", "dynamic"), reads, x=x, min_identity=min_identity,
                                  max_supported=max_supported(spec), threads=8))
    host = ca.match_best(w["dev"], st, reads, x=x, min_identity=min_identity)
    dev = ca.match_best_device(w["dev"], st, reads, x=x, min_identity=min_identity)
    assert_oracle_parity(O, norm_lib(host))
    assert_oracle_parity(O, norm_lib(dev))
    _assert_same(host, dev)
    cuts, dstar = best_truth(gt, spec, min_identity, reads)
    label = f"BEST {spec} x={x} {min_identity} %"
    for name, res in (("match_best", host), ("match_best_device", dev)):
        check_best_equals_dstar(f"{label} {name}", res[4], cuts, dstar, assert_it=x == 0)
    mapped, flagged = int((host[4] != NONE).sum()), int(dev[7].sum())
    rng = np.random.default_rng(3)
    ids = [f"@best{i} x={x}" for i in range(len(reads))]
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    ref = samcheck.Reference(w["text"], w["names"], w["starts"], gt)
    for xa in (False, True):
        text, host_reads = ca.best_sam_device(w["dev"], st, reads, ids, quals, w["names"], x=x, min_identity=min_identity, unmapped=True, xa=xa)
        _same(text, _sam_of_best(host, reads, ids, quals, w["names"], True, xa), "best_sam_device / the host path's text")
        c = samcheck.check_single_end(text, ref, reads, ids, quals, limit=cuts, unmapped=True, xa=xa, best_mode=True)
        assert host_reads == flagged and c["mapped"] == mapped
    _report(label, dict(c, records_of_match_best=len(host[0]), host_reads=flagged))
    assert mapped >= 40 and len(reads) - mapped >= 40 and c["loose"] == 0
    if spec == "columba":  # (multiple_opt stops at exact matches: nothing to trim, nothing for the host)
        assert flagged * 4 >= mapped, (flagged, mapped)


# ------------------------------------------------------------------------------------------------ f. b-move
@pytest.mark.parametrize("spec,k", [("columba", 4), ("kuch1", 0)])
def test_all_mode_bmove(world, gt, spec, k):
    """MoveBatch.sam and MoveBatch.sam_device (the kept lists, the host class for a quarter of the mapped reads at least)"""
    w = world["contig"]
    reads, ids, quals = contigs.chunk(k)
    label = f"MoveBatch {spec} edit k={k}"
    mb = ca.MoveBatch(w["mdev"], ca.SearchStrategy(spec, "edit", "dynamic"), k, reads=reads, kmer_size=8)
    mb.want_alignments()
    mb.keep_device_lists()
    mb.run()
    # (the b-move flavour labels an occurrence found on both strands by its own rule, tests/test_best_ground_truth.py: no oracle text here)
    _, offs, _ = mb.results()
    aln, _ = mb.alignments()
    spanning = _spanning_reads(aln, offs, len(reads))
    for unmapped in (True, False):
        host = mb.sam(ids, quals, w["names"], unmapped=unmapped)
        got, host_reads = mb.sam_device(ids, quals, w["names"], unmapped=unmapped)
        print(f"{label} unmapped={unmapped}: {len(aln)} occurrences, {int((aln['spans'] != 0).sum())} over a sequence end, {len(got)} bytes, "
              f"host_reads={host_reads}, spanning reads={spanning}")
        _same(got, host, "device text / host text")
        assert host_reads == spanning
        if unmapped:
            text = got
    mb.close()
    if k > 0:
        st = check_all_mode(gt, label, text, reads, ids, quals, k, False)
    else:
        ref = samcheck.Reference(w["text"], w["names"], w["starts"], gt)
        st = samcheck.check_single_end(text, ref, reads, ids, quals, limit=0, unmapped=True)
        recs = contigs.sam_records(text, ids, w["names"])
        # exact matches: every copy of the read inside one sequence has its record, on either strand
        truth = contigs.per_sequence_truth(gt, w["text"], w["starts"], reads, 0)
        st["ends"], st["miss4"], st["miss8"], st["other_strand"] = contigs.check_per_sequence(recs, truth, 0)
        _report(label, st)
        assert st["miss4"] == 0 and st["ends"] >= 100 and st["mapped"] >= 80 and st["unmapped"] >= 40
    assert host_reads * 4 >= st["mapped"], (host_reads, st)


# ------------------------------------------------------------------------------------------------ g. read pairs
PAIR_K, MAX_FRAG, MIN_FRAG = 2, 500, 100


def _pair_chunk():
    """120 FR fragments of 250 ... 400 characters inside one sequence, 40 that straddle a sequence end (the mates in different contigs,
    or one mate over the end), 10 pairs with a random mate; mates of 100 characters with up to 2 edits.  Returns reads 1, reads 2 and per
    pair the truth (sequence, 1-based POS of the forward mate, of the reverse one) or None"""
    w = contigs.contig_world()
    g, starts = w["genome"], np.asarray(w["starts"], np.int64)
    lens = np.diff(starts)
    rng = np.random.default_rng(21)

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
    for i in range(170):
        frag = int(rng.integers(250, 401))
        if i < 120:
            s = int(rng.choice(np.flatnonzero(lens >= frag)))
            p0 = int(starts[s] + rng.integers(0, lens[s] - frag + 1))
            t = (s, p0 - int(starts[s]) + 1, p0 + frag - 100 - int(starts[s]) + 1)
        else:
            s = int(rng.choice(np.flatnonzero((starts[:-1] >= 400) & (starts[:-1] <= len(g) - 400))))
            p0 = int(starts[s] - rng.integers(1, frag))  # (the end before sequence s lies inside the fragment)
            t = None
        a = edited(g[p0:p0 + 100].tobytes(), int(rng.integers(0, PAIR_K + 1)))
        b = edited(synth.revcomp(g[p0 + frag - 100:p0 + frag].tobytes()), int(rng.integers(0, PAIR_K + 1)))
        if i >= 160:
            b = synth.ACGT[rng.integers(0, 4, 100)].tobytes()
        if i % 2:
            a, b = b, a
        r1.append(a)
        r2.append(b)
        truth.append(t)
    return r1, r2, truth


def test_read_pairs(world, gt):
    """pair_chunk_sam (cmb_pair_sam on trimmed lists) and pair_chunk_sam_device (k_pair_plan: the `over` flag sends a pair with an
    occurrence over a sequence end to the host class; k_pair_write: names of 2 ... 70 bytes) byte for byte; the paired rules of samcheck on
    it and on pair_chunk_sam_best; every fragment cut inside one sequence comes back as a proper pair in that sequence"""
    w = world["contig"]
    names = w["names"]
    r1, r2, truth = _pair_chunk()
    ids1, ids2, q1, q2 = _pair_inputs(r1, r2)
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    want, want_mapped = ca.pair_chunk_sam(w["dev"], st, PAIR_K, r1, r2, ids1, ids2, q1, q2, names, ca.ORIENTATION_FR, MAX_FRAG, MIN_FRAG, True, True)
    got, mapped, stats = ca.pair_chunk_sam_device(w["dev"], st, PAIR_K, r1, r2, ids1, ids2, q1, q2, names, ca.ORIENTATION_FR, MAX_FRAG, MIN_FRAG, True, True)
    print(f"pairs: {len(r1)} pairs, {mapped} mapped, {stats}")
    _same(got, want, "pair_chunk_sam_device / pair_chunk_sam")
    assert mapped == want_mapped == stats["mapped_pairs"]
    ref = samcheck.Reference(w["text"], names, w["starts"], gt)
    c, groups = samcheck.check_paired(got, ref, r1, r2, ids1, ids2, q1, q2, limit=PAIR_K, orientation=samcheck.ORIENTATION_FR, min_frag=MIN_FRAG,
                                      max_frag=MAX_FRAG)
    _report("pairs, ALL mode", dict(c, **stats))
    assert _assert_fragments_found(groups, truth, names, PAIR_K) == 120
    assert c["proper"] >= 240 and c["loose"] == 0
    assert stats["host_pairs"] >= 30 and len(r1) - stats["host_pairs"] >= 60 and stats["device_records"] >= 120
    best, best_mapped, _ = ca.pair_chunk_sam_best(w["dev"], st, r1, r2, ids1, ids2, q1, q2, names, x=0, min_identity=95, orientation=ca.ORIENTATION_FR,
                                                  max_frag=MAX_FRAG, min_frag=MIN_FRAG, discordant_allowed=True)
    cut = cutoff("columba", 95, 100)
    limit = [(cutoff("columba", 95, len(a)), cutoff("columba", 95, len(b))) for a, b in zip(r1, r2)]
    cb, _ = samcheck.check_paired(best, ref, r1, r2, ids1, ids2, q1, q2, limit=limit, orientation=samcheck.ORIENTATION_FR, min_frag=MIN_FRAG,
                                  max_frag=MAX_FRAG)
    _report(f"pairs, BEST mode (cut-off {cut})", dict(cb, mapped_pairs=best_mapped))
    assert cb["proper"] >= 200
