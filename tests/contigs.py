"""References of many short sequences, and ground truth that knows the sequences (helper of tests/test_contigs.py and
tests/test_gpu_contigs.py, no test in itself).

Every other world of the suite has one to eight long sequences, so an occurrence that touches a sequence end is the exception there
and the ground-truth layer leaves such reads out.  Here it is the rule:

  contig_world   60 000 characters of synth.genome_rep in 383 sequences of 1 ... 599 characters, a tenth of them shorter than 8; names
                 of 2 ... 70 bytes.  A quarter of all occurrences runs over a sequence end; many run over three or more sequences, begin in
                 the last one, or are trimmed onto a next sequence that is shorter than the read.
  dense_world    120 000 uniform random characters in 20 000 sequences of exactly 6: the sequence lookup is deeper than 2^14, every
                 occurrence of a 30-character read runs over five sequences at least and none of them can be trimmed.
  mini_layouts   one 20 000-character text as 1 sequence (starts not given at all), as 2 and as 3 sequences.

The judge is oracle/groundtruth.c asked about ONE SEQUENCE AT A TIME (per_sequence_truth): for every read, strand and sequence the end
positions j with min_b ED(read, sequence[b, j)) = d <= k.  check_per_sequence then wants, for every such (sequence, j, d), a record in that
sequence with NM <= d that ends within 4k of j (2k for the redundancy window on the begin, 2k for the width of an
alignment with k indels: the rule of tests/test_ground_truth.py, which works on the concatenated text and knows no sequences).
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from columba_amd import synth
import samcheck

_W = {}


# ------------------------------------------------------------------------------------------------ the worlds
def contig_name(i: int) -> str:
    """mostly c<i>; every seventh contig_<i>_ and i % 60 filler characters (the longest has 70 bytes: wider than a wavefront)"""
    return f"contig_{i}_" + "".join("abcdefghij"[j % 10] for j in range(i % 60)) if i % 7 == 0 else f"c{i}"


def contig_world():
    if "contig" not in _W:
        g = synth.genome_rep(seed=9, n=60_000, scale=1.0)[0]
        rng = np.random.default_rng(1)
        starts, at = [0], 0
        while at < len(g):
            u = rng.random()
            if u < 0.1:
                ln = int(rng.integers(1, 8))
            elif u < 0.4:
                ln = int(rng.integers(20, 90))
            elif u < 0.7:
                ln = int(rng.integers(90, 130))
            else:
                ln = int(rng.integers(130, 600))
            at = min(at + ln, len(g))
            starts.append(at)
        assert len(starts) - 1 == 383 and all(b > a for a, b in zip(starts, starts[1:]))
        names = [contig_name(i) for i in range(len(starts) - 1)]
        assert len(set(names)) == len(names) and max(map(len, names)) > 64
        _W["contig"] = {"label": "contig", "genome": g, "text": g.tobytes(), "starts": starts, "names": names}
    return _W["contig"]


def dense_world():
    if "dense" not in _W:
        rng = np.random.default_rng(2)
        g = synth.ACGT[rng.integers(0, 4, 120_000)]
        starts = list(range(0, 120_001, 6))
        assert len(starts) - 1 == 20_000 > 1 << 14
        _W["dense"] = {"label": "dense", "genome": g, "text": g.tobytes(), "starts": starts, "names": [f"d{i}" for i in range(20_000)]}
    return _W["dense"]


def mini_layouts():
    """(label, genome, starts or None): None is an index built without seq_starts, whose one sequence is the whole text"""
    if "mini" not in _W:
        g = synth.genome_rep(seed=9, n=20_000, scale=2.0)[0]
        _W["mini"] = [("mini1", g, None), ("mini2", g, [0, 7_321, 20_000]), ("mini3", g, [0, 5_003, 12_001, 20_000])]
    return _W["mini"]


def chunk(k: int, per_length: int = 50, lengths=(30, 60, 100, 150)):
    """50 reads each of 30, 60, 100 and 150 characters with 0 ... k edits, and the first 200 characters of every 13th sequence of at least
    25 characters (a read that IS a whole contig); identifiers and qualities as tests/test_sam_ground_truth._se_chunk.
    Returns (reads, ids, quals)."""
    key = ("chunk", k, per_length, lengths)
    if key not in _W:
        w = contig_world()
        g, starts = w["genome"], w["starts"]
        reads = []
        for length in lengths:
            reads += synth.sample_reads(g, per_length, length, seed=length + k, edit_choices=(0, 0, 1, 2, k, k))
        whole = [s for s in range(0, len(starts) - 1, 13) if starts[s + 1] - starts[s] >= 25]
        assert len(whole) == 28
        for s in whole:
            reads.append(g[starts[s]:min(starts[s] + 200, starts[s + 1])].tobytes())
        rng = np.random.default_rng(17 + k)
        ids = [("@" if i % 2 else ">") + f"read{i}/1 length={len(r)}" for i, r in enumerate(reads)]
        ids[1] = "@nospace"
        quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
        _W[key] = (reads, ids, quals)
    return _W[key]


def best_chunk(per_length: int = 100):
    """reads of 40, 64, 100 and 151 characters for BEST mode: 0 ... 9 edits, so that every length has reads beyond its cut-off"""
    key = ("best_chunk", per_length)
    if key not in _W:
        g = contig_world()["genome"]
        reads = []
        for length in (40, 64, 100, 151):
            reads += synth.sample_reads(g, per_length, length, seed=7 * length, edit_choices=(0, 0, 0, 1, 1, 2, 3, 4, 5, 7, 9))
        _W[key] = reads
    return _W[key]


# ------------------------------------------------------------------------------------------------ the sequence lookup
def lookup(starts, begin, end):
    """IndexInterface::findSeqName (indexinterface.cpp:799-832) by numpy: (sequence, begin inside it, runs over its end)"""
    st = np.asarray(starts, np.int64)
    b, e = np.asarray(begin).astype(np.int64), np.asarray(end).astype(np.int64)
    idx = np.searchsorted(st, b, side="right") - 1
    return idx, b - st[idx], e > st[idx + 1]


def assert_lookup(aln, occ, starts):
    """the assertions at the end of test_gpu_parity._check_alignments; returns (occurrences that span, that begin in the last sequence,
    that run over three sequences or more)"""
    st = np.asarray(starts, np.int64)
    idx, inside, spans = lookup(st, occ["begin"], occ["end"])
    assert np.array_equal(aln["seq_id"], idx.astype(np.uint32)), np.flatnonzero(aln["seq_id"] != idx)[:10]
    assert np.array_equal(aln["seq_begin"], inside.astype(np.uint32)), np.flatnonzero(aln["seq_begin"] != inside)[:10]
    assert np.array_equal(aln["spans"] != 0, spans), np.flatnonzero((aln["spans"] != 0) != spans)[:10]
    last = np.searchsorted(st, occ["end"].astype(np.int64) - 1, side="right") - 1  # (the sequence of the last character)
    return int(spans.sum()), int((idx == len(st) - 2).sum()), int((last - idx >= 2).sum())


# ------------------------------------------------------------------------------------------------ ground truth per sequence
def per_sequence_truth(gt, text: bytes, starts, reads, k):
    """k: one distance, or one per read (the cut-offs of BEST mode).  Per read a dict
         "ends":  per strand an int64 array of rows (sequence, end position j inside it, d) for every sequence s with
                  len(s) >= len(read) - k and every j with min_b ED(read on that strand, s[b, j)) = d <= k
         "dstar": the minimum of d over both strands and all sequences, k + 1 if there is none
    computed once per (text, reads, k) and shared (about a second for 228 reads on the 383 sequences of contig_world)."""
    ks = tuple(int(x) for x in k) if hasattr(k, "__len__") else (int(k),) * len(reads)
    key = ("truth", hash(text), tuple(starts), tuple(reads), ks)
    if key in _W:
        return _W[key]
    st = np.asarray(starts, np.int64)
    lens = np.diff(st)
    seqs = [text[starts[s]:starts[s + 1]] for s in range(len(lens))]
    n_text = int(st[-1])

    def one(i):
        fw = samcheck.clean(reads[i])
        kk = ks[i]
        assert len(fw) > kk
        out, dstar = [], kk + 1
        whole = np.zeros(n_text + 1, np.uint8)
        best = np.zeros(int(lens.max()) + 1, np.uint8)
        whole_p, best_p = whole.ctypes.data_as(C.c_void_p), best.ctypes.data_as(C.c_void_p)
        for p in (fw, samcheck.revcomp(fw)):
            # an alignment inside a sequence is one in the concatenated text as well, so the sequences to ask are those in which an
            # end position of the whole text lies: one pass over the text picks them, every one of them is then asked by itself
            gt.gt_semiglobal_ends(text, n_text, p, len(p), kk, whole_p, None)
            hits = np.flatnonzero(whole <= kk)
            cand = np.unique(np.searchsorted(st, hits[hits > 0] - 1, side="right") - 1)
            rows = []
            for s in cand[lens[cand] >= len(p) - kk]:
                n = int(lens[s])
                gt.gt_semiglobal_ends(seqs[s], n, p, len(p), kk, best_p, None)
                j = np.flatnonzero(best[:n + 1] <= kk)
                if len(j):
                    rows.append(np.stack([np.full(len(j), s, np.int64), j.astype(np.int64), best[j].astype(np.int64)], axis=1))
            rows = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
            if len(rows):
                dstar = min(dstar, int(rows[:, 2].min()))
            out.append(rows)
        return {"ends": tuple(out), "dstar": dstar}

    with ThreadPoolExecutor(8) as ex:  # (ctypes and numpy release the interpreter lock)
        _W[key] = list(ex.map(one, range(len(reads))))
    return _W[key]


def hamming_windows(text: bytes, starts, read: bytes, k: int):
    """(the windows of the read's length with <= k mismatches that lie inside one sequence, as record rows (sequence, begin, end,
    mismatches, strand); the number of such windows that run over a sequence end), by sliding the read over the whole text"""
    ta, n = np.frombuffer(text, np.uint8), len(text)
    fw = samcheck.clean(read)
    inside, over = set(), 0
    for strand, p in enumerate((fw, samcheck.revcomp(fw))):
        pa = np.frombuffer(p, np.uint8)
        m = len(pa)
        mism = np.zeros(n - m + 1, np.uint8)  # (reads are shorter than 256 characters)
        for c in range(m):
            if pa[c] == ord("N"):
                mism += 1
            else:
                mism += ta[c:n - m + 1 + c] != pa[c]
        b = np.flatnonzero(mism <= k)
        sid, at, spans = lookup(starts, b, b + m)
        over += int(spans.sum())
        inside |= {(int(s), int(a), int(a) + m, int(d), strand) for s, a, d in zip(sid[~spans], at[~spans], mism[b][~spans])}
    return inside, over


def sam_records(text: str, ids, names):
    """per read the alignments its records and XA entries claim, as int64 rows (sequence, begin, end, NM, strand) with begin and end
    inside the sequence, 0-based and half open.  Nothing is validated here: that is samcheck's work."""
    qn = {samcheck.qname(s): i for i, s in enumerate(ids)}
    sid = {n: i for i, n in enumerate(names)}
    out = [[] for _ in ids]
    for line in text.splitlines():
        f = line.split("\t")
        flag = int(f[1])
        if flag & 4:
            continue
        tags = {t[:2]: t[5:] for t in f[11:]}
        i = qn[f[0]]
        out[i].append((sid[f[2]], int(f[3]) - 1, int(f[3]) - 1 + samcheck.cigar_width(f[5]), int(tags["NM"]), (flag >> 4) & 1))
        for e in tags.get("XA", "").split(";")[:-1]:
            name, pos, cig, nm = e.rsplit(",", 3)
            b = int(pos[1:]) - 1
            out[i].append((sid[name], b, b + samcheck.cigar_width(cig), int(nm), int(pos[0] == "-")))
    return [np.asarray(r, np.int64).reshape(-1, 5) for r in out]


def check_per_sequence(records, truth, k: int, per_strand: bool = False):
    """records: per read rows (sequence, begin, end, NM, strand); truth: per_sequence_truth.  Every truth end (s, j, d) wants a record in
    sequence s with NM <= d ending within 4k of j.  Returns (ends judged, those without such a record within 4k, those without one within
    8k, those whose only such records within 4k lie on the other strand); the caller asserts on the first three.

    The strand: ALL mode filters the occurrences of both strands of a read TOGETHER, and the filter compares begin, distance and width,
    never the strand (getUniqueTextOccurrences, indexinterface.cpp:1451-1485), so where a read aligns on both strands within 2k positions
    (a tandem repeat whose unit is close to its own reverse complement) the better alignment stands for both, whatever its strand.  The
    record of the other strand is then legitimately missing, and the fourth count says how often that was needed.  per_strand=True asks
    for the record on the strand of the truth end: for lists whose strands were filtered each by itself (mapRead)."""
    judged = miss4 = miss8 = other = 0
    for rec, tr in zip(records, truth):
        for strand in (0, 1):
            ends = tr["ends"][strand]
            judged += len(ends)
            for o in range(0, len(ends), 2048):
                e = ends[o:o + 2048]
                ok = (rec[None, :, 0] == e[:, None, 0]) & (rec[None, :, 3] <= e[:, None, 2])
                same = rec[None, :, 4] == strand
                gap = np.abs(rec[None, :, 2] - e[:, None, 1])
                near = (ok & (gap <= 4 * k) & same).any(axis=1)
                near_any = (ok & (gap <= 4 * k)).any(axis=1)
                other += int((near_any & ~near).sum())
                if per_strand:
                    ok = ok & same
                    near_any = near
                miss4 += int((~near_any).sum())
                miss8 += int((~(ok & (gap <= 8 * k)).any(axis=1)).sum())
    return judged, miss4, miss8, other


def records_inside_sequences(records, starts):
    """no record runs over the end of its sequence"""
    lens = np.diff(np.asarray(starts, np.int64))
    return all(((r[:, 1] >= 0) & (r[:, 1] < r[:, 2]) & (r[:, 2] <= lens[r[:, 0]])).all() for r in records if len(r))
