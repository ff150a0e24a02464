"""Crossings of the kernel selectors that no other test makes in one run, on a world small enough for a few seconds per case: the byte
text and the packed text with alignments at k = 2 (32-bit matrix words, narrow trace rows) and k = 6 (64-bit words, wide rows); the
three partitioning modes on reads of 300 characters (the long-read instances of k_parts / k_exact, several verification stages);
Hamming distance; and the same reads through the b-move backend with alignments.

Bar: the oracle — occurrence lists, the counters tests/test_gpu_parity.py compares, and, with alignments wanted, the CIGAR the oracle's
findCIGAR gives for every occurrence and findSeqName's sequence assignment.  The text has 20 000 characters in 3 sequences, with a
repeat; the 64 reads are 150 and 300 characters long, some carry an N, two lie across a sequence boundary.
"""
import os
import subprocess

import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

STARTS = np.array([0, 6_000, 13_000, 20_000], dtype=np.int64)


@pytest.fixture(scope="module")
def world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    from columba_amd import movebuild
    rng = np.random.default_rng(77)
    g = synth.ACGT[rng.integers(0, 4, int(STARTS[-1]))]
    g[15_000:17_000] = synth._mutate(rng, g[2_000:4_000], 0.02)   # a repeat: reads with several occurrences
    reads = {}
    for ln in (150, 300):
        rd = synth.sample_reads(g, 31, ln, seed=ln, n_frac=0.2, edit_choices=(0, 1, 2, 2, 3, 5, 6))
        assert any(b"N" in r for r in rd)
        reads[ln] = rd + [g[int(STARTS[1]) - ln // 2:int(STARTS[1]) + ln - ln // 2].tobytes()]   # across a sequence boundary
    text = g.tobytes()
    ix = ib.build_index(text, seq_starts=STARTS, device="cuda")
    os.environ["CMB_TEXT_BYTES"] = "1"
    try:
        dev_bytes = ca.Index(ix)
    finally:
        del os.environ["CMB_TEXT_BYTES"]
    mv = movebuild.build_move(text, device="cuda")
    mdev = ca.MoveIndex(mv)
    mdev.attach_text(text, STARTS.astype(np.uint64))
    return {"text": text, "reads": reads, "all": reads[150] + reads[300], "op": op, "oracle_dir": oracle_built,
            "packed": ca.Index(ix), "bytes": dev_bytes, "orc": op.OracleIndex(ix), "mdev": mdev, "morc": op.OracleMoveIndex(mv)}


def _check_alignments(w, reads, occ, offs, aln, ops, gapless):
    """every CIGAR is findCIGAR's for (read on its strand, text[begin, end), distance); the sequence is findSeqName's"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    cmds, who = [], []
    for i, r in enumerate(reads):
        fw = bytes(c if c in b"ACGT" else ord("N") for c in r.upper())
        rc = fw.translate(comp)[::-1]
        for j in range(int(offs[i]), int(offs[i + 1])):
            o = occ[j]
            if gapless:
                assert ca.cigar_string(ops[int(aln[j]["cigar_off"]):int(aln[j]["cigar_off"]) + int(aln[j]["cigar_len"])]) == f"{len(r)}M"
            else:
                seq = rc if o["strand"] else fw
                cmds.append(f"findcigar {seq.decode()} {w['text'][int(o['begin']):int(o['end'])].decode()} {int(o['distance'])}")
                who.append(j)
    if cmds:
        res = subprocess.run([os.path.join(w["oracle_dir"], "oracle_driver")], input="\n".join(cmds) + "\n", capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(res) == len(cmds)
        for j, want in zip(who, res):
            got = ca.cigar_string(ops[int(aln[j]["cigar_off"]):int(aln[j]["cigar_off"]) + int(aln[j]["cigar_len"])])
            assert got == want, (j, occ[j], got, want)
    begin, end = occ["begin"].astype(np.int64), occ["end"].astype(np.int64)
    idx = np.searchsorted(STARTS, begin, side="right") - 1
    assert np.array_equal(aln["seq_id"], idx.astype(np.uint32))
    assert np.array_equal(aln["seq_begin"], (begin - STARTS[idx]).astype(np.uint32))
    assert np.array_equal(aln["spans"] != 0, end > STARTS[idx + 1])
    assert (aln["spans"] != 0).sum() > 0   # (the reads across the boundary)


@pytest.mark.parametrize("text", ["packed", "bytes"])
@pytest.mark.parametrize("k", [2, 6])
def test_text_layouts_with_alignments(world, text, k):
    w = {"dev": world[text], "orc": world["orc"], "op": world["op"]}
    reads = world["all"]
    _compare(w, "multiple_opt", "edit", "dynamic", k, reads, dups_rare=False)
    b = ca.Batch(world[text], ca.SearchStrategy("multiple_opt", "edit", "dynamic"), k, reads)
    b.want_alignments()
    b.run()
    occ, offs, _ = b.results()
    aln, ops = b.alignments()
    assert len(aln) == len(occ) >= len(reads) // 2
    _check_alignments(world, reads, occ, offs, aln, ops, gapless=False)
    o2, f2, _ = ca.match_batch(world[text], ca.SearchStrategy("multiple_opt", "edit", "dynamic"), k, reads)
    assert np.array_equal(o2, occ) and np.array_equal(f2, offs)   # (what a run without alignments gives)
    b.close()


@pytest.mark.parametrize("partition", ["uniform", "static", "dynamic"])
def test_partitioning_modes_on_long_reads(world, partition):
    w = {"dev": world["packed"], "orc": world["orc"], "op": world["op"]}
    cnt = _compare(w, "kuch1", "edit", partition, 2, world["reads"][300], dups_rare=False)
    assert cnt["IN_TEXT_STARTED"] > 0


def test_hamming_distance(world):
    w = {"dev": world["packed"], "orc": world["orc"], "op": world["op"]}
    _compare(w, "kuch1", "hamming", "dynamic", 2, world["all"], dups_rare=False)


@pytest.mark.parametrize("k", [2, 6])
def test_bmove_with_alignments(world, k):
    import schemes_py as sp
    op, reads = world["op"], world["all"]
    o_occ, o_off, o_cnt = world["morc"].match_batch(op.OracleStrategy(sp.BY_NAME["multiple_opt"], "edit", "dynamic"), k, reads, threads=8, word_size=8)
    mb = ca.MoveBatch(world["mdev"], ca.SearchStrategy("multiple_opt", "edit", "dynamic"), k, reads=reads, kmer_size=8)
    mb.want_alignments()
    mb.run()
    occ, offs, cnt = mb.results()
    aln, ops = mb.alignments()
    assert len(o_occ) >= len(reads) // 2 and np.array_equal(o_off, offs) and len(aln) == len(occ)
    for f in ("begin", "end", "distance"):
        assert np.array_equal(o_occ[f].astype(np.uint64), occ[f].astype(np.uint64)), f
    # (the strand label of an occurrence found on both strands is the reference's unstable sort's to choose)
    assert (o_occ["strand"] != occ["strand"]).sum() <= 1
    surplus = {"TOTAL_REPORTED_POSITIONS": o_cnt["SURVIVING_DUP_ROWS"], "LOCATED_ROWS": o_cnt["SURVIVING_DUP_ROWS"]}
    for n in ("NODE_COUNTER", "EXPANSIONS", "TOTAL_REPORTED_POSITIONS", "LOCATED_ROWS", "SEARCH_STARTED", "MATRIX_ROWS"):
        assert o_cnt[n] - surplus.get(n, 0) == cnt[n], (n, o_cnt[n], surplus.get(n, 0), cnt[n])
    _check_alignments(world, reads, occ, offs, aln, ops, gapless=False)
    mb.close()
