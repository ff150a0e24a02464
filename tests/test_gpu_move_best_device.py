"""BEST (+x strata) mode on the b-move backend with the strata bookkeeping on the device (cmb_move_match_best_device: b-move batches
with kept lists as strata): every array and counter of the host path (cmb_move_match_best), bit for bit, and the SAM
text cmb_best_sam_device writes from the result."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import columba_amd as ca  # noqa: E402
from columba_amd import movebuild, synth  # noqa: E402
from test_gpu_best_device import NONE, _assert_same, _cutoff, _env, _first_difference, _sam_of_best  # noqa: E402
from test_gpu_move_sam_device import BOUNDS, pan_text  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = [("columba", "edit", 0, 96), ("columba", "edit", 1, 96), ("kuch1", "hamming", 0, 98), ("minU", "edit", 2, 97),
           ("columba", "edit", 0, 92)]


@pytest.fixture(scope="module")
def bworld():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g = pan_text()
    dev = ca.MoveIndex(movebuild.build_move(g.tobytes(), device="cuda"))
    dev.attach_text(g.tobytes(), np.array([0, BOUNDS[0], BOUNDS[1], len(g)], dtype=np.uint32))
    return {"g": g, "dev": dev, "names": ["chrA", "chrB", "chrC"], "runs": {}}


def _reads(w, cfg):
    """500 sampled reads, the boundary reads and the oddities of test_gpu_move_search.test_bmove_best_mode"""
    spec, metric, x, min_identity = cfg
    g = w["g"]
    deep = min_identity in (92, 93)  # identities that let the strata run beyond 7 errors
    reads = synth.sample_reads(g, 500, 150, seed=300 + x, n_frac=0.01,
                               edit_choices=(0, 1, 3, 6, 8, 9, 10, 11, 12, 13) if deep else (0, 0, 1, 2, 3, 5, 6, 9))
    for s0 in BOUNDS:  # reads across sequence ends: trimmed or dropped (findSeqName)
        reads += [g[s0 - 75:s0 + 75].tobytes(), g[s0 - 3:s0 + 147].tobytes(), g[s0 - 147:s0 + 3].tobytes(), g[s0 - 5:s0 + 145].tobytes()]
    reads += [b"ACGT" * 37 + b"AC", b"N" * 150, g[:150].tobytes(), g[-150:].tobytes()]
    return reads


def _run(w, cfg):
    """host path and device path of one configuration, computed once for all tests"""
    if cfg not in w["runs"]:
        spec, metric, x, min_identity = cfg
        reads = _reads(w, cfg)
        st = ca.SearchStrategy(spec, metric, "dynamic")
        host = ca.match_best(w["dev"], st, reads, x=x, min_identity=min_identity, kmer_size=8)
        dev = ca.match_best_device(w["dev"], st, reads, x=x, min_identity=min_identity, kmer_size=8)
        w["runs"][cfg] = {"reads": reads, "host": host, "dev": dev}
    return w["runs"][cfg]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_results_equal_the_host_path(bworld, cfg):
    """7: every array and every counter of cmb_move_match_best; host-read flags only on reads that keep an occurrence over a sequence
    end under edit distance (few: the boundary reads and what the sampling puts before a boundary in a haplotype), none under
    Hamming distance"""
    w = bworld
    spec, metric, x, min_identity = cfg
    r = _run(w, cfg)
    reads = r["reads"]
    _assert_same(r["host"], r["dev"])
    d_occ, d_aln, d_ops, d_off, d_best, d_hits, d_cnt, flagged = r["dev"]
    n_flagged = int(flagged.sum())
    print(f"{cfg}: {len(reads)} reads, {len(d_occ)} records, mapped {(d_best != NONE).sum()}, host reads {n_flagged}")
    assert (d_best != NONE).sum() > 100 and (d_best == NONE).sum() > 0
    for n in ("IN_TEXT_STARTED", "IMMEDIATE_SWITCH", "ABORTED_IN_TEXT_VERIF"):
        assert d_cnt[n] == 0, n
    if metric == "hamming":
        assert n_flagged == 0
        return
    assert 1 <= n_flagged <= 0.05 * len(reads)
    b = ca.MoveBatch(w["dev"], ca.SearchStrategy(spec, metric, "dynamic"), _cutoff(spec, min_identity), reads=reads, kmer_size=8)
    b.filter_per_strand()
    b.want_alignments()
    b.run()
    _, offs, _ = b.results()
    aln, _ = b.alignments()
    for i in np.flatnonzero(flagged):
        assert (aln["spans"][int(offs[i]):int(offs[i + 1])] != 0).any(), i
    b.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_grid_edges(bworld, n):
    """8a: chunks around the sizes of a wavefront and of a block, the boundary reads first"""
    w = bworld
    reads = _reads(w, CONFIGS[0])
    reads = (reads[500:] + reads[:500])[:n]
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    for x in (0, 1):
        host = ca.match_best(w["dev"], st, reads, x=x, min_identity=96, kmer_size=8)
        got = ca.match_best_device(w["dev"], st, reads, x=x, min_identity=96, kmer_size=8)
        _assert_same(host, got)
        assert len(got[3]) == n + 1 and len(got[7]) == n
        if n >= 63:
            assert got[7].sum() >= 1


@pytest.mark.parametrize("cfg,env", [(CONFIGS[1], {"CMB_MOVE_SLICE": "64"}), (CONFIGS[3], {"CMB_MOVE_SUBBATCHES": "2"})],
                         ids=["slices", "halves"])
def test_composite_strata(bworld, cfg, env):
    """8b: strata matched in slices of 64 reads (the kept lists grow slice by slice), and as two halves: identical results"""
    w = bworld
    spec, metric, x, min_identity = cfg
    r = _run(w, cfg)
    with _env(**env):
        got = ca.match_best_device(w["dev"], ca.SearchStrategy(spec, metric, "dynamic"), r["reads"], x=x, min_identity=min_identity, kmer_size=8)
    _assert_same(r["host"], got)
    assert np.array_equal(got[7], r["dev"][7])


@pytest.mark.parametrize("cfg,xa,unmapped", [(CONFIGS[0], False, True), (CONFIGS[1], True, True), (CONFIGS[3], True, False),
                                             (CONFIGS[2], False, False)], ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_sam_text(bworld, cfg, xa, unmapped):
    """9: the text cmb_best_sam_device writes from the b-move result is, byte for byte, the one samOfBest assembles from
    cmb_move_match_best's; the reads the host formatted are the flagged ones"""
    w = bworld
    spec, metric, x, min_identity = cfg
    r = _run(w, cfg)
    reads = list(r["reads"])
    reads[3] = reads[3].lower()
    rng = np.random.default_rng(17)
    ids = [("@" if i % 2 else ">") + f"read{i}/1 some description" for i in range(len(reads))]
    ids[0], ids[1], ids[2] = "@", "@nospace", ">x"
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(rd))) for rd in reads]
    names = w["names"]
    st = ca.SearchStrategy(spec, metric, "dynamic")
    host = ca.match_best(w["dev"], st, reads, x=x, min_identity=min_identity, kmer_size=8)
    b = ca.BestDevice(w["dev"], st, reads, x=x, min_identity=min_identity, kmer_size=8)
    flagged = int(b.host_reads().sum())
    for q in (quals, None):
        want = _sam_of_best(host, reads, ids, q, names, unmapped, xa)
        got, host_reads = b.sam_device(ids, q, names, unmapped=unmapped, xa=xa)
        print(f"{cfg} xa={xa} unmapped={unmapped}: {len(got)} bytes, host_reads={host_reads}")
        assert got == want, _first_difference(got, want)
        assert host_reads == flagged
        assert len(got) > 10_000
    _assert_same(host, b.results())  # (the lists are still what they were)
    b.close()
