"""SAM text of a single-end chunk in ALL mode on the b-move backend, written on the device from the lists the batch keeps in HBM
for its whole chunk (cmb_move_batch_keep_device_lists + cmb_move_batch_sam_device): byte for byte the text of the
host formatter on the batch's downloaded records (MoveBatch.sam: cmb_sam_chunk), whatever the slices and halves the chunk ran in."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import columba_amd as ca  # noqa: E402
from columba_amd import movebuild, synth  # noqa: E402
from test_gpu_move import _pangenome  # noqa: E402
from test_gpu_sam_device import _env, _heavy_text, _same, _text_of  # noqa: E402

pytestmark = pytest.mark.gpu

BOUNDS = (250_000, 640_000)


def pan_text():
    """the pan-genome-like text of tests/test_gpu_move_search.py: 16 haplotypes, a repeat-rich stretch, a random tail"""
    rng = np.random.default_rng(15)
    return np.concatenate([_pangenome(rng, 40_000, 16, 0.005), synth.genome_rep(seed=3, n=150_000, scale=4.0)[0],
                           np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20_000)]])


@pytest.fixture(scope="module")
def mworld():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g = pan_text()
    dev = ca.MoveIndex(movebuild.build_move(g.tobytes(), device="cuda"))
    dev.attach_text(g.tobytes(), np.array([0, BOUNDS[0], BOUNDS[1], len(g)], dtype=np.uint64))
    return {"g": g, "dev": dev, "names": ["chrA", "chrB", "chrC"]}


def boundary_reads(g, length=150):
    """two reads per sequence boundary whose occurrences run over the end of a sequence (spans = 1)"""
    out = []
    for s0 in BOUNDS:
        out += [g[s0 - length // 2:s0 + length - length // 2].tobytes(), g[s0 - 2:s0 + length - 2].tobytes()]
    return out


def _fields(reads, seed=5):
    rng = np.random.default_rng(seed)
    ids = [("@" if i % 2 else ">") + f"read{i}/1 some description" for i in range(len(reads))]
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    return ids, quals


def _batch(w, spec, metric, k, reads, keep=True, per_strand=False):
    b = ca.MoveBatch(w["dev"], ca.SearchStrategy(spec, metric, "dynamic"), k, reads=reads, kmer_size=8)
    b.want_alignments()
    if per_strand:
        b.filter_per_strand()
    if keep:
        b.keep_device_lists()
    b.run()
    return b


CONFIGS = [("columba", "edit", 4, False), ("multiple_opt", "edit", 2, True), ("kuch1", "hamming", 2, False),
           ("kuch1", "edit", 0, False), ("columba", "edit", 9, False), ("columba", "edit", 12, True)]


@pytest.mark.parametrize("spec,metric,k,xa", CONFIGS)
def test_device_text_equals_host_text(mworld, spec, metric, k, xa):
    """1: byte for byte the host formatter's text, with and without unmapped records (also at k = 0, whose records are built on
    the host and uploaded, and beyond 9 errors); the reads the host formatted are exactly those with an occurrence over the end
    of its sequence: the four boundary reads and what the sampling puts before a boundary in one of the haplotypes"""
    w = mworld
    g = w["g"]
    reads = synth.sample_reads(g, 600, 150, seed=950 + k, n_frac=0.01, edit_choices=(0, 1, 2, 4, 9)) + boundary_reads(g)
    assert len(reads) == 604
    ids, quals = _fields(reads, 5 + k)
    b = _batch(w, spec, metric, k, reads)
    occ, offs, _ = b.results()
    aln, _ = b.alignments()
    assert len(occ) > 400
    spanning = sum(1 for i in range(len(reads)) if (aln["spans"][int(offs[i]):int(offs[i + 1])] == 1).any())
    for unmapped in (True, False):
        host = b.sam(ids, quals, w["names"], unmapped=unmapped, xa=xa, metric=metric)
        got, host_reads = b.sam_device(ids, quals, w["names"], unmapped=unmapped, xa=xa)
        print(f"{spec} {metric} k={k} xa={xa} unmapped={unmapped}: {len(got)} bytes, host_reads={host_reads}, spanning={spanning}")
        _same(got, host)
        assert len(got) > 50_000
        assert host_reads == spanning
        assert 4 <= host_reads <= 0.05 * len(reads)
    b.close()


def test_slices_and_halves(mworld):
    """2: a chunk matched in five slices (the kept lists grow past their first size), as two halves, as both, and with every strand
    filtered by itself: always the text of the plain run of that filter mode and of the host formatter; a second run gives the
    same text again (the lists start empty)"""
    w = mworld
    g = w["g"]
    reads = synth.sample_reads(g, 296, 150, seed=21, n_frac=0.01, edit_choices=(0, 1, 2, 4, 9))
    for at, r in zip((10, 100, 200, 299), boundary_reads(g)):  # (a host-formatted read in several slices and in both halves)
        reads.insert(at, r)
    assert len(reads) == 300
    ids, quals = _fields(reads, 22)
    for per_strand in (False, True):
        plain = _batch(w, "columba", "edit", 4, reads, per_strand=per_strand)
        want, want_host = plain.sam_device(ids, quals, w["names"], xa=per_strand)
        _same(want, plain.sam(ids, quals, w["names"], xa=per_strand))
        assert want_host >= 4 and len(want) > 50_000
        plain.close()
        ways = [{"CMB_MOVE_SLICE": "64"}, {"CMB_MOVE_SUBBATCHES": "2"}, {"CMB_MOVE_SLICE": "64", "CMB_MOVE_SUBBATCHES": "2"}]
        for env in (ways[0], ways[2]) if per_strand else ways:  # (slices alone: the per-strand offsets of a slice are what is rebased)
            with _env(**env):
                b = _batch(w, "columba", "edit", 4, reads, per_strand=per_strand)
                got, host_reads = b.sam_device(ids, quals, w["names"], xa=per_strand)
                _same(got, want)
                _same(got, b.sam(ids, quals, w["names"], xa=per_strand))
                assert host_reads == want_host
                b.run()
                again, host_again = b.sam_device(ids, quals, w["names"], xa=per_strand)
                _same(again, want)
                assert host_again == want_host
                b.close()


def test_quirks(mworld):
    """3: no qualities; empty qualities (plain and XA path); lower-case reads; identifiers without a space, of one character and
    empty; reads of 30 and 480 characters, and one of 3 characters (not longer than the number of parts: naive backtracking);
    a chunk without any occurrence"""
    w = mworld
    g = w["g"]
    reads = synth.sample_reads(g, 100, 150, seed=31, n_frac=0.01, edit_choices=(0, 1, 2, 4, 9))
    reads[3] = reads[3].lower()
    reads[4] = bytes(c + 32 if i % 3 else c for i, c in enumerate(reads[4]))
    reads.append(g[70_000:70_030].tobytes())
    reads.append(g[690_000:690_480].tobytes())
    reads.append(synth.revcomp(g[700_000:700_480].tobytes()))
    n = len(reads)
    ids = [f"@r{i} d{i} e" for i in range(n)]
    ids[0], ids[1], ids[2], ids[5], ids[6] = "@nospace", "@", ">x", "@ lead", ""
    rng = np.random.default_rng(8)
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    some_empty = [("" if i % 3 == 0 else q) for i, q in enumerate(quals)]
    names = w["names"]
    b = _batch(w, "columba", "edit", 4, reads)
    for xa in (False, True):
        for unmapped in (True, False):
            for q in (quals, some_empty):
                got, _ = b.sam_device(ids, q, names, unmapped=unmapped, xa=xa)
                _same(got, b.sam(ids, q, names, unmapped=unmapped, xa=xa))
            got, _ = b.sam_device(ids, None, names, unmapped=unmapped, xa=xa)
            _same(got, b.sam(ids, ["*"] * n, names, unmapped=unmapped, xa=xa))
    text, _ = b.sam_device(ids, quals, names)
    lines = text.splitlines()
    assert lines[0].startswith("nospace\t") and any("\t4\t*\t0\t0\t*" in x for x in lines)
    assert all(x.split("\t")[9] == x.split("\t")[9].upper() for x in lines)
    b.close()
    # a read of 3 characters among ordinary ones: as many parts as characters at 2 errors, so it is matched naively
    short = [reads[0], b"ACG", reads[1]]
    b = _batch(w, "kuch1", "edit", 2, short)
    _, offs, _ = b.results()
    print(f"the 3-character read: {int(offs[2]) - int(offs[1])} occurrences")
    assert int(offs[2]) - int(offs[1]) > 0
    for xa in (False, True):
        got, _ = b.sam_device(ids[:3], quals[:1] + ["III"] + quals[1:2], names, xa=xa)
        _same(got, b.sam(ids[:3], quals[:1] + ["III"] + quals[1:2], names, xa=xa))
    b.close()
    # a chunk whose reads all lack occurrences
    rng = np.random.default_rng(99)
    junk = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150)) for _ in range(70)]
    b = _batch(w, "columba", "edit", 2, junk)
    occs, _, _ = b.results()
    assert len(occs) == 0
    jid = [f"@j{i}" for i in range(70)]
    for unmapped in (True, False):
        got, host_reads = b.sam_device(jid, None, names, unmapped=unmapped)
        _same(got, b.sam(jid, ["*"] * 70, names, unmapped=unmapped))
        assert host_reads == 0 and (got == "") == (not unmapped)
    b.close()


def test_a_heavy_read():
    """4: a read with more than a thousand occurrences — with the XA tag its line is far longer than what a wavefront stages at once"""
    unit, g = _heavy_text()
    dev = ca.MoveIndex(movebuild.build_move(g.tobytes(), device="cuda"))
    dev.attach_text(g.tobytes(), np.array([0, 84_000, 168_000, len(g)], dtype=np.uint64))
    w = {"dev": dev}
    reads = [unit, unit[:100], synth.revcomp(unit)]
    ids = ["@heavy first", "@part", "@back"]
    quals = ["I" * len(r) for r in reads]
    names = ["s0", "s1", "s2"]
    b = _batch(w, "columba", "edit", 2, reads)
    occs, offs, _ = b.results()
    d = occs["distance"][int(offs[0]):int(offs[1])]
    print(f"{len(d)} occurrences, {(d == d.min()).sum()} at the minimal distance {d.min()}")
    assert len(d) > 1000
    for xa in (False, True):
        got, host_reads = b.sam_device(ids, quals, names, xa=xa)
        _same(got, b.sam(ids, quals, names, xa=xa))
        assert host_reads == 0
        if xa:
            assert max(len(x) for x in got.splitlines()) > 16_000
    b.close()
    dev.close()


def test_packed_inputs_that_do_not_start_at_zero(mworld):
    """5: identifiers and qualities whose offsets begin at 7 and 5 give the text of the zero-based packing, with host-formatted reads
    among the 65 (one more than a wavefront has lanes)"""
    w = mworld
    g = w["g"]
    reads = synth.sample_reads(g, 63, 150, seed=71, n_frac=0.01, edit_choices=(0, 1, 2)) + boundary_reads(g)[:2]
    assert len(reads) == 65 and all(len(r) == 150 for r in reads)
    rng = np.random.default_rng(72)
    ids = ca.pack_fields([("@" if i % 2 else ">") + f"read{i}/1 some description" for i in range(65)])
    quals = ca.pack_fields(["".join(chr(33 + int(q)) for q in rng.integers(0, 41, 150)) for _ in reads])
    names = ca.pack_fields(w["names"])
    shifted_ids = (np.concatenate([np.frombuffer(b"\tjunk \n", np.uint8), ids[0]]), ids[1] + np.uint64(7))
    shifted_quals = (np.concatenate([np.frombuffer(b"~~~~\n", np.uint8), quals[0]]), quals[1] + np.uint64(5))
    b = _batch(w, "columba", "edit", 2, reads)
    entry = ca.lib().cmb_move_batch_sam_device
    for xa in (False, True):
        want, host_reads = _text_of(entry, b, ids, quals, names, xa)
        got, host_shifted = _text_of(entry, b, shifted_ids, shifted_quals, names, xa)
        _same(got, want)
        assert host_shifted == host_reads >= 1 and want.count("\n") >= 65
    _same(_text_of(entry, b, ids, quals, names, False)[0], b.sam_device(ids, quals, names)[0])
    b.close()


def test_refusals(mworld):
    """6: before run; without kept lists; kept lists without alignments, or without the text beside the index: CMB_ERR_INVALID"""
    w = mworld
    g = w["g"]
    reads = synth.sample_reads(g, 20, 150, seed=61)
    ids, quals, names = [f"@r{i}" for i in range(20)], ["I" * 150] * 20, w["names"]
    st = ca.SearchStrategy("columba", "edit", "dynamic")

    def refused(call):
        with pytest.raises(ca.CmbError) as e:
            call()
        assert e.value.code == ca.CMB_ERR_INVALID

    b = ca.MoveBatch(w["dev"], st, 2, reads=reads, kmer_size=8)
    refused(b.keep_device_lists)  # alignments were not asked for
    b.want_alignments()
    b.keep_device_lists()
    refused(lambda: b.sam_device(ids, quals, names))  # not run
    b.run()
    assert b.sam_device(ids, quals, names)[0] == b.sam(ids, quals, names)
    b.close()
    b = ca.MoveBatch(w["dev"], st, 2, reads=reads, kmer_size=8)
    b.want_alignments()
    b.run()
    refused(lambda: b.sam_device(ids, quals, names))  # the lists were not kept
    b.close()
    unit, t = _heavy_text()
    bare = ca.MoveIndex(movebuild.build_move(t[:30_000].tobytes(), device="cuda"))  # no text beside it
    b = ca.MoveBatch(bare, st, 2, reads=[unit], kmer_size=8)
    refused(b.want_alignments)
    refused(b.keep_device_lists)
    b.close()
    bare.close()
