"""The CPU oracle on a reference of many short sequences (tests/contigs.py), held to ground truth that knows the sequences.

These tests keep the INPUTS of tests/test_gpu_contigs.py honest: the oracle alone, on contig_world, satisfies every condition the HIP
paths are then held to — the per-sequence completeness rule without a single exception within 4k, no reported distance above the true
distance of its window, and in BEST mode at x = 0 `best == d*` for every read, none left out for lying near a sequence end.  They also
show that each checker can fail.

Observed on the oracle (printed by the tests):
  ALL mode    strategy      k  reads  occurrences  over an end  mapped  unmapped  ends judged  exceptions  other strand
              columba       2    228          324    73 (23 %)     159        69          609           0             0
              multiple_opt  4    228          436   117 (27 %)     141        87         1918           0             6
              columba       7    228          646   162 (25 %)     160        68         3666           0           144
              columba       9    108          248    48 (19 %)      80        28         1322           0             0
              columba      10    228          589   196 (33 %)     156        72         3639           0             0
              ("other strand": truth ends whose record lies on the other strand, on two reads cut from tandem repeats; see
              contigs.check_per_sequence.  At k = 10 the sampled reads have 40 instead of 30 characters, see ALL_CONFIGS)
  Hamming     kuch1 k = 2: 119 mapped, 109 unmapped, 158 windows inside a sequence = 158 alignments, 51 windows over an end, 47 reads
              with such windows only
  BEST x = 0  columba 95 %       400 reads: best == d* for all 400; 167 mapped, 233 unmapped, cut-offs 2, 3, 5, 7
              multiple_opt 97 %  400 reads: best == d* for all 400;  63 mapped, 337 unmapped, cut-off 0 (no scheme for one error)
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

from test_ground_truth import gt  # noqa: E402,F401
from test_best_ground_truth import NONE, cutoff, max_supported, norm_oracle  # noqa: E402
from test_sam_ground_truth import _edit_line, _report  # noqa: E402
import contigs  # noqa: E402
import samcheck  # noqa: E402

# (strategy, k, XA tag, reads per length, lengths).  Fewer reads at 9 errors.  At 10, where the GPU tests run k_cigar_wide and k_verify_wide,
# reads of 40 instead of 30 characters: with a third of a read in errors the oracle itself leaves the rule (30-character reads at
# k = 10: 4 of 8121 ends without a record and one record above its window's distance, all on occurrences trimmed at a sequence end)
LENGTHS = (30, 60, 100, 150)
ALL_CONFIGS = [("columba", 2, False, 50, LENGTHS), ("multiple_opt", 4, True, 50, LENGTHS), ("columba", 7, False, 50, LENGTHS),
               ("columba", 9, False, 20, LENGTHS), ("columba", 10, False, 50, (40, 60, 100, 150))]
BEST_CONFIGS = [("columba", 95), ("multiple_opt", 97)]


def check_all_mode(gt, label, text, reads, ids, quals, k, xa, metric="edit", unmapped=True, per_strand=False):
    """samcheck and the per-sequence completeness rule on the SAM text of a chunk of contig_world; the conditions of the module docstring
    and the thresholds that keep them from being vacuous (set well under what the oracle gives: 141 ... 160 mapped and 68 ... 87 unmapped
    of 228 reads, 600 ends or more)"""
    w = contigs.contig_world()
    ref = samcheck.Reference(w["text"], w["names"], w["starts"], gt)
    st = samcheck.check_single_end(text, ref, reads, ids, quals, limit=k, unmapped=unmapped, xa=xa, metric=metric)
    recs = contigs.sam_records(text, ids, w["names"])
    assert contigs.records_inside_sequences(recs, w["starts"])
    st["ends"], st["miss4"], st["miss8"], st["other_strand"] = contigs.check_per_sequence(
        recs, contigs.per_sequence_truth(gt, w["text"], w["starts"], reads, k), k, per_strand)
    _report(label, st)
    assert st["miss4"] == 0 and st["loose"] == 0, st
    assert st["ends"] >= 600 and st["mapped"] * 228 >= 100 * len(reads), st
    if unmapped:
        assert st["unmapped"] * 228 >= 40 * len(reads) and st["absent"] == 0, st
    return st


@pytest.fixture(scope="module")
def cpu_world(oracle_built):
    import oracle_py as op
    from columba_amd import indexbuild as ib
    w = contigs.contig_world()
    ix = ib.build_index(w["text"], seq_starts=np.asarray(w["starts"], np.uint32), device="cpu")
    return {"op": op, "orc": op.OracleIndex(ix), "texts": {}}


def _oracle_text(cw, spec, k, xa, per_length=50, lengths=LENGTHS):
    import schemes_py as sp
    key = (spec, k, xa, per_length, lengths)
    if key not in cw["texts"]:
        reads, ids, quals = contigs.chunk(k, per_length, lengths)
        cw["texts"][key] = cw["op"].match_batch_sam(cw["orc"], cw["op"].OracleStrategy(sp.BY_NAME[spec], "edit", "dynamic"), k, reads, ids,
                                                    quals, contigs.contig_world()["names"], unmapped=True, xa=xa)
    return cw["texts"][key]


def test_the_worlds():
    w = contigs.contig_world()
    lens = np.diff(w["starts"])
    assert len(lens) == 383 and lens.min() >= 1 and (lens < 8).sum() >= 30 and (lens < 150).sum() >= 200 and w["starts"][-1] == 60_000
    assert max(len(n) for n in w["names"]) > 64 and min(len(n) for n in w["names"]) == 2
    d = contigs.dense_world()
    assert len(d["starts"]) == 20_001 and set(np.diff(d["starts"]).tolist()) == {6} and d["starts"][-1] == len(d["text"]) == 120_000
    reads, ids, quals = contigs.chunk(4)
    assert len(reads) == len(ids) == len(quals) == 228 and sorted({len(r) for r in reads[:200]}) == [30, 60, 100, 150]
    starts = set(w["starts"])
    assert all(w["text"].find(r) in starts for r in reads[200:]), "the last reads are the beginnings of whole sequences"
    assert [n for _, _, s in contigs.mini_layouts() for n in [None if s is None else len(s) - 1]] == [None, 2, 3]


@pytest.mark.parametrize("spec,k,xa,per_length,lengths", ALL_CONFIGS)
def test_oracle_all_mode_per_sequence(cpu_world, gt, spec, k, xa, per_length, lengths):
    import schemes_py as sp
    op = cpu_world["op"]
    w = contigs.contig_world()
    reads, ids, quals = contigs.chunk(k, per_length, lengths)
    occ, _, _ = op.match_batch(cpu_world["orc"], op.OracleStrategy(sp.BY_NAME[spec], "edit", "dynamic"), k, reads, threads=4)
    _, _, spans = contigs.lookup(w["starts"], occ["begin"], occ["end"])
    print(f"oracle {spec} k={k}: {len(reads)} reads, {len(occ)} occurrences, {int(spans.sum())} over a sequence end")
    assert spans.sum() * 10 >= len(occ) >= len(reads)
    check_all_mode(gt, f"oracle {spec} k={k} xa={xa}", _oracle_text(cpu_world, spec, k, xa, per_length, lengths), reads, ids, quals, k, xa)


def test_oracle_hamming_drops_spanning_occurrences(cpu_world, gt):
    """under Hamming distance an occurrence over a sequence end is dropped, never trimmed: the records are exactly the windows of the
    read's length with <= k mismatches inside one sequence, and a read all of whose windows run over an end is unmapped"""
    import schemes_py as sp
    op = cpu_world["op"]
    w = contigs.contig_world()
    k = 2
    reads, ids, quals = contigs.chunk(k)
    text = op.match_batch_sam(cpu_world["orc"], op.OracleStrategy(sp.BY_NAME["kuch1"], "hamming", "dynamic"), k, reads, ids, quals, w["names"])
    check_hamming(gt, "oracle kuch1 hamming k=2", text, reads, ids, quals, k)


def check_hamming(gt, label, text, reads, ids, quals, k):
    w = contigs.contig_world()
    ref = samcheck.Reference(w["text"], w["names"], w["starts"], gt)
    st = samcheck.check_single_end(text, ref, reads, ids, quals, limit=k, unmapped=True, metric="hamming")
    recs = contigs.sam_records(text, ids, w["names"])
    assert contigs.records_inside_sequences(recs, w["starts"])
    st["inside_windows"] = st["spanning_windows"] = st["reads_with_spanning_windows_only"] = 0
    for i, rd in enumerate(reads):
        want, over = contigs.hamming_windows(w["text"], w["starts"], rd, k)
        assert {tuple(r) for r in recs[i].tolist()} == want, (i, recs[i].tolist(), want)
        st["inside_windows"] += len(want)
        st["spanning_windows"] += over
        st["reads_with_spanning_windows_only"] += bool(over and not want)
    _report(label, st)
    # (the oracle: 119 mapped, 109 unmapped, 158 windows inside a sequence)
    assert st["mapped"] >= 80 and st["unmapped"] >= 60 and st["inside_windows"] >= 120 and st["spanning_windows"] >= 30, st
    assert st["reads_with_spanning_windows_only"] >= 20, st
    return st


def best_truth(gt, spec, min_identity, reads):
    """per read (cut-off, d* or NONE): the minimal distance over all sequences taken one by one, within the read's own cut-off"""
    w = contigs.contig_world()
    cuts = [cutoff(spec, min_identity, len(r)) for r in reads]
    tr = contigs.per_sequence_truth(gt, w["text"], w["starts"], reads, cuts)
    return cuts, np.asarray([t["dstar"] if t["dstar"] <= c else NONE for t, c in zip(tr, cuts)], np.uint32)


def check_best_equals_dstar(label, best, cuts, dstar, assert_it=True):
    differ = np.flatnonzero(np.asarray(best) != dstar)
    mapped = int((dstar != NONE).sum())
    print(f"{label}: {len(dstar)} reads, best differs from d* on {len(differ)} ({int((dstar[differ] == 0).sum())} of them with d* = 0); "
          f"d*: {mapped} mapped, {len(dstar) - mapped} unmapped, cut-offs {sorted(set(cuts))}")
    if assert_it:
        assert len(differ) == 0, [(int(i), int(best[i]), int(dstar[i]), cuts[i]) for i in differ[:10]]
    return len(differ)


@pytest.mark.parametrize("spec,min_identity", BEST_CONFIGS)
def test_oracle_best_mode_finds_the_per_sequence_minimum(cpu_world, gt, spec, min_identity):
    """x = 0: best == d* for EVERY read, most of whose best alignments touch a sequence end (trimmed occurrences move between strata)"""
    import schemes_py as sp
    op = cpu_world["op"]
    reads = contigs.best_chunk()
    R = norm_oracle(op.match_best(cpu_world["orc"], op.OracleStrategy(sp.BY_NAME[spec], "edit", "dynamic"), reads, x=0,
                                  min_identity=min_identity, max_supported=max_supported(spec), threads=8))
    cuts, dstar = best_truth(gt, spec, min_identity, reads)
    check_best_equals_dstar(f"oracle {spec} {min_identity} %", R["best"], cuts, dstar)
    assert (dstar != NONE).sum() >= 40 and (dstar == NONE).sum() >= 40
    assert (R["best"] != NONE).tolist() == (np.diff(R["offs"]) > 0).tolist()


def test_checkers_reject_corrupted_text(cpu_world, gt):
    """a record moved to the neighbouring contig, a record deleted, a POS shifted so that the alignment runs over its sequence end, an NM
    raised, an NM lowered: each is caught, by samcheck or by the per-sequence rule"""
    w = contigs.contig_world()
    names, starts = w["names"], w["starts"]
    lens = np.diff(starts)
    k = 2
    reads, ids, quals = contigs.chunk(k)
    good = _oracle_text(cpu_world, "columba", k, False)
    check_all_mode(gt, "the text before it is corrupted", good, reads, ids, quals, k, False)

    def rejected(text):
        with pytest.raises(AssertionError):
            check_all_mode(gt, "corrupted", text, reads, ids, quals, k, False)

    def put(i, v):
        def change(f):
            f[i] = v(f)
            return f
        return change

    mapped = lambda f: not int(f[1]) & 4  # noqa: E731
    width = lambda f: samcheck.cigar_width(f[5])  # noqa: E731
    neighbour = lambda f: names[names.index(f[2]) + 1]  # noqa: E731
    # ... to the neighbouring contig, where the window is another text: the CIGAR's edits are no longer its distance
    rejected(_edit_line(good, lambda f: mapped(f) and width(f) >= 60 and names.index(f[2]) + 1 < len(names)
                        and lens[names.index(f[2]) + 1] >= int(f[3]) - 1 + width(f), put(2, neighbour)))
    # ... and where the neighbour is too short to hold it
    rejected(_edit_line(good, lambda f: mapped(f) and names.index(f[2]) + 1 < len(names) and lens[names.index(f[2]) + 1] < width(f), put(2, neighbour)))
    lines = good.splitlines()
    only = next(i for i in range(1, len(lines) - 1) if lines[i].split("\t")[4] == "60")
    rejected("\n".join(lines[:only] + lines[only + 1:]) + "\n")                              # the only record of a read deleted
    second = next(i for i in range(len(lines)) if int(lines[i].split("\t")[1]) & 256 and lines[i].split("\t")[4] == "0")
    rejected("\n".join(lines[:second] + lines[second + 1:]) + "\n")                          # a record above the minimum deleted: the rule alone sees it
    at_end = lambda f: mapped(f) and int(f[3]) - 1 + width(f) == lens[names.index(f[2])]  # noqa: E731
    rejected(_edit_line(good, at_end, put(3, lambda f: str(int(f[3]) + 1))))                 # POS shifted over the sequence end
    rejected(_edit_line(good, lambda f: mapped(f) and "NM:i:1" in f, put(12, lambda f: "NM:i:2")))  # NM raised (AS stays)
    rejected(_edit_line(good, lambda f: mapped(f) and f[4] == "60" and "NM:i:0" in f,
                        lambda f: [t.replace(":i:0", ":i:1") if t[:2] in ("NM", "AS") else t for t in f]))  # NM and AS raised: above d
    rejected(_edit_line(good, lambda f: mapped(f) and "NM:i:2" in f, lambda f: [t.replace(":i:2", ":i:1") if t[:2] in ("NM", "AS") else t for t in f]))


def test_lookup_assertion_rejects_shifted_starts():
    """contigs.assert_lookup (what the GPU tests hold seq_id, seq_begin and spans to) fails when the starts are off by one, when one is
    missing, and on a single wrong field"""
    w = contigs.contig_world()
    starts = np.asarray(w["starts"], np.int64)
    rng = np.random.default_rng(4)
    occ = np.zeros(4000, [("begin", np.uint32), ("end", np.uint32)])
    occ["begin"] = rng.integers(0, 60_000 - 160, len(occ))
    occ["begin"][:len(starts) - 1] = starts[:-1]                # every first character
    occ["begin"][400:400 + len(starts) - 2] = starts[1:-1] - 1  # every last one
    occ["end"] = np.minimum(occ["begin"] + rng.integers(20, 160, len(occ)), 60_000)
    idx, inside, spans = contigs.lookup(starts, occ["begin"], occ["end"])
    aln = np.zeros(len(occ), [("seq_id", np.uint32), ("seq_begin", np.uint32), ("spans", np.uint8)])
    aln["seq_id"], aln["seq_begin"], aln["spans"] = idx, inside, spans
    n_spans, n_last, n_three = contigs.assert_lookup(aln, occ, starts)
    assert n_spans >= 400 and n_last >= 1 and n_three >= 100
    # by the definition, not by searchsorted
    for j in range(0, len(occ), 37):
        s = max(i for i in range(len(starts) - 1) if starts[i] <= occ["begin"][j])
        assert (idx[j], inside[j], spans[j]) == (s, occ["begin"][j] - starts[s], occ["end"][j] > starts[s + 1])
    shifted = starts.copy()
    shifted[1:-1] += 1
    for wrong in (shifted, np.delete(starts, 200)):
        with pytest.raises(AssertionError):
            contigs.assert_lookup(aln, occ, wrong)
    for field in ("seq_id", "seq_begin", "spans"):
        bad = aln.copy()
        bad[field][1234] ^= 1
        with pytest.raises(AssertionError):
            contigs.assert_lookup(bad, occ, starts)
