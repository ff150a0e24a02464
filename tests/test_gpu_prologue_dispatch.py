"""The prologue of the FM-index search: k_parts starts the searches of a read x strand itself — the items of the
part-level pre-verification, a search task for every search whose approximate matching begins after its first part
(or on the complete range), and a list entry for every search with further exact phases, which k_exact then runs.

Bar: occurrences and counters (NODE_COUNTER, EXPANSIONS, SEARCH_STARTED, IMMEDIATE_SWITCH among them) equal to the
oracle's, on a repeat-rich text where wide first parts and narrow parts occur in the same read.  What the prologue
queued is read from the library's CMB_VERBOSE lines:
    [prologue] <items> items, <tasks> search tasks, <n> searches with further exact phases
    [retry] queues too small: items tasks exact       (the queues that overflowed)
"""
import re

import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth
from test_gpu_parity import _compare, _tuples

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    g, starts = synth.genome_rep(seed=23, n=1_000_000, scale=2.0)  # repeat-rich: Alu-like copies at twice the usual density
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    return {"genome": g, "ix": ix, "op": op, "dev": ca.Index(ix), "orc": op.OracleIndex(ix),
            "dev4": ca.Index(ix, kmer_size=4), "orc4": op.OracleIndex(ix, kmer_size=4)}


def _reads(g, n, length, seed, odd=True, metric="edit"):
    """sampled reads (a few with an N) plus, with `odd`, reads with several N, reads not longer than any scheme's number of
    parts (naive backtracking) and, for edit distance, an empty read"""
    reads = synth.sample_reads(g, n, length, seed=seed, n_frac=0.03)
    if odd:
        reads += [b"N" * length, b"ACGTN" * (length // 5), g[1000:1000 + length // 2].tobytes() + b"NN" + g[2000:2000 + length // 2].tobytes(),
                  g[500:503].tobytes(), b"AC", b"G", g[-length - 1:-1].tobytes(), g[0:length].tobytes()]
        if metric == "edit":
            reads.append(b"")
    return reads


def _prologue_lines(err):
    """([(items, tasks, exact)] per attempt, [set of overflowed queues] per retry) from the CMB_VERBOSE output"""
    runs = [tuple(int(x) for x in m.groups())
            for m in re.finditer(r"\[prologue\] (\d+) items, (\d+) search tasks, (\d+) searches with further exact phases", err)]
    retries = [set(m.group(1).split()) for m in re.finditer(r"\[retry\] queues too small:([ a-z]*)", err)]
    return runs, retries


# kuch1 at k = 4 has the search {0,1,2,3,4} U = {0,0,4,4,4}, kuch2 at k = 3 {3,4,2,1,0} U = {0,0,3,3,3}, kianfar at k = 4
# {4,3,2,1,0} U = {0,0,4,4,4}: two exact phases (tests/golden/search_schemes)
@pytest.mark.parametrize("spec,metric,partition,k", [
    ("kuch1", "edit", "dynamic", 4), ("kuch1", "hamming", "uniform", 4), ("kuch1", "edit", "static", 4),
    ("kuch2", "edit", "static", 3), ("kuch2", "hamming", "dynamic", 3), ("kianfar", "edit", "uniform", 4),
])
def test_searches_with_a_second_exact_phase(world, monkeypatch, capfd, spec, metric, partition, k):
    g = world["genome"]
    # (kianfar's first search allows errors in its first part: ~20 000 nodes per read for the oracle)
    reads = _reads(g, 200 if spec == "kianfar" else 700, 120, seed=40 + k, metric=metric)
    monkeypatch.setenv("CMB_VERBOSE", "1")
    capfd.readouterr()
    _compare(world, spec, metric, partition, k, reads, dups_rare=False)
    runs, _ = _prologue_lines(capfd.readouterr().err)
    assert runs, "no [prologue] line in the verbose output"
    items, tasks, exact = runs[-1]
    assert exact > 0, "no search went on to k_exact: the read set does not exercise the list"
    assert tasks > 0 and items > 0


def test_multiple_opt_needs_no_exact_kernel(world, monkeypatch, capfd):
    """every search of the multiple_opt schemes has one exact phase: the list stays empty"""
    reads = _reads(world["genome"], 600, 150, seed=7)
    monkeypatch.setenv("CMB_VERBOSE", "1")
    capfd.readouterr()
    _compare(world, "multiple_opt", "edit", "dynamic", 4, reads, dups_rare=False)
    runs, _ = _prologue_lines(capfd.readouterr().err)
    assert runs and runs[-1][2] == 0 and runs[-1][0] > 0 and runs[-1][1] > 0


# A scheme for 2 errors on 3 parts whose searches start in all three ways.  Error patterns (e0, e1, e2), e0 + e1 + e2 <= 2:
#   {0,1,2} L 0,0,0 U 0,0,2   e0 = e1 = 0                          two exact phases        -> list entry for k_exact
#   {2,1,0} L 0,0,1 U 0,2,2   e2 = 0, at least one error           approximate from part 1 -> search task with idx 1
#   {1,2,0} L 0,1,1 U 1,2,2   e1 <= 1, 1 <= e1 + e2 <= 2           U[0] > 0                -> search task on the complete range
# Every pattern is covered: e2 = 0 by the second (or the first, without errors); e2 >= 1 with e0 = e1 = 0 by the first; the other
# patterns with e2 >= 1 are (1,0,1) and (0,1,1), both in the third.
THREE_STARTS = {"kmer_cutoff": 20, "schemes": {2: [[([0, 1, 2], [0, 0, 0], [0, 0, 2]), ([2, 1, 0], [0, 0, 1], [0, 2, 2]),
                                                    ([1, 2, 0], [0, 1, 1], [1, 2, 2])]]}}


def _compare_tables(world, spec, metric, partition, k, reads):
    op = world["op"]
    o_occ, o_off, o_cnt = op.match_batch(world["orc"], op.OracleStrategy(spec, metric, partition), k, reads, threads=8)
    d_occ, d_off, d_cnt = ca.match_batch(world["dev"], ca.SearchStrategy.from_tables(spec, metric, partition), k, reads)
    assert len(o_occ) > 0
    assert np.array_equal(o_off, d_off)
    strand_only = 0
    for i in range(len(reads)):
        a, b = _tuples(o_occ, o_off, i), _tuples(d_occ, d_off, i)
        if a != b:  # (equal (begin, end, distance) on both strands: the reference's choice is unspecified, see test_gpu_parity)
            assert [t[:3] for t in a] == [t[:3] for t in b], (i, reads[i], a, b)
            strand_only += 1
    assert strand_only <= max(1, len(o_occ) // 1000)
    for n in ("NODE_COUNTER", "EXPANSIONS", "SEARCH_STARTED", "IMMEDIATE_SWITCH", "IN_TEXT_STARTED", "MATRIX_ROWS"):
        assert o_cnt[n] == d_cnt[n], (n, o_cnt[n], d_cnt[n])


@pytest.mark.parametrize("metric,partition", [("edit", "dynamic"), ("edit", "uniform"), ("hamming", "dynamic"), ("hamming", "uniform")])
def test_custom_scheme_that_starts_on_the_complete_range(world, monkeypatch, capfd, metric, partition):
    reads = _reads(world["genome"], 250, 60, seed=91, metric=metric)
    monkeypatch.setenv("CMB_VERBOSE", "1")
    capfd.readouterr()
    _compare_tables(world, THREE_STARTS, metric, partition, 2, reads)
    runs, _ = _prologue_lines(capfd.readouterr().err)
    assert runs
    items, tasks, exact = runs[-1]
    n_rs = 2 * sum(1 for r in reads if len(r) > 3)   # (reads of up to three characters take the naive path)
    assert tasks >= n_rs        # the third search of every searched read x strand starts on the complete range
    assert exact > 0


@pytest.mark.parametrize("spec,metric,partition,k", [("kuch1", "edit", "dynamic", 4), ("kuch1", "hamming", "static", 4)])
def test_every_prologue_queue_overflows_and_is_grown(world, monkeypatch, capfd, spec, metric, partition, k):
    """CMB_TEST_SMALL_POOLS: the item queue, the task queue and the list for k_exact start from almost nothing; each has to
    overflow at least once, and the re-run gives the oracle's result"""
    reads = _reads(world["genome"], 700, 120, seed=40 + k, metric=metric)
    monkeypatch.setenv("CMB_VERBOSE", "1")
    monkeypatch.setenv("CMB_TEST_SMALL_POOLS", "1")
    capfd.readouterr()
    _compare(world, spec, metric, partition, k, reads, dups_rare=False)
    runs, retries = _prologue_lines(capfd.readouterr().err)
    grown = set().union(*retries) if retries else set()
    assert {"items", "tasks", "exact"} <= grown, (grown, runs)
    assert runs[-1][2] > 16     # (the list's first capacity under CMB_TEST_SMALL_POOLS)


@pytest.mark.parametrize("spec,metric,partition", [("kuch1", "edit", "dynamic"), ("pigeon", "edit", "uniform"), ("kuch1", "edit", "static")])
def test_exact_matching_is_untouched(world, spec, metric, partition):
    """k = 0: one lane of k_exact per read x strand runs the whole exact search"""
    reads = synth.sample_reads(world["genome"], 600, 100, seed=12, n_frac=0.03, edit_choices=(0, 0, 0, 1))
    reads += [b"N" * 100, b"A", world["genome"][0:100].tobytes(), world["genome"][-101:-1].tobytes()]
    _compare(world, spec, metric, partition, 0, reads, dups_rare=False)


@pytest.mark.parametrize("metric,partition", [("hamming", "dynamic"), ("hamming", "uniform"), ("edit", "static"), ("edit", "dynamic")])
def test_eight_errors_on_the_wide_instances(world, monkeypatch, capfd, metric, partition):
    """k = 8: nine parts, the MAXP_WIDE instances of k_parts and k_exact"""
    g = world["genome"]
    reads = synth.sample_reads(g, 300, 150, seed=88, n_frac=0.02, edit_choices=(0, 2, 5, 8, 8))
    reads += [g[5000:5009].tobytes(), g[77:80].tobytes(), b"N" * 150, g[-151:-1].tobytes()]
    monkeypatch.setenv("CMB_VERBOSE", "1")
    capfd.readouterr()
    _compare(world, "columba", metric, partition, 8, reads, dups_rare=False)
    runs, _ = _prologue_lines(capfd.readouterr().err)
    assert runs and runs[-1][1] > 0


def test_wide_first_parts_and_narrow_parts_in_one_read(world, monkeypatch, capfd):
    """a third of the text is copies of one 300 bp element: 150 bp reads that straddle the edge of a copy have parts inside it
    (wide ranges: search tasks) and parts in unique sequence (narrow ranges: items) — k_parts fills both queues from one read x
    strand, under all three partitionings"""
    reads = synth.sample_reads(world["genome"], 1500, 150, seed=77, edit_choices=(0, 1, 2, 4))
    monkeypatch.setenv("CMB_VERBOSE", "1")
    for partition in ("dynamic", "uniform", "static"):
        capfd.readouterr()
        _compare(world, "multiple_opt", "edit", partition, 4, reads, dups_rare=False)
        runs, _ = _prologue_lines(capfd.readouterr().err)
        assert runs and runs[-1][0] > 0 and runs[-1][1] > 0, (partition, runs)
