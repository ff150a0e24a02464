"""Every capped launch of the batch pipeline with more work than it has lanes.

Most launches of cmb_batch_run / cmb_move_batch_run are capped at a fixed number of lanes (sized for 10^6 ... 10^7 reads) and let each
lane loop over the items beyond the cap.  At the few hundred reads of the other tests every lane gets one item and every loop runs
once.  CMB_TEST_GRID_CAP=<blocks> (columba_amd/csrc/host_grid.hpp) lowers every cap, so that the second and later trips — where a lane
reuses its trace planes, its slab slot or its matrix registers, where a wavefront carries a partly filled chunk of a queue from one
trip into the next, where the last trip is ragged — run at test size.  Cap 1 is a stride of 256, cap 3 one of 768 (no power of two).

Bar: every case is held to the CPU oracle (occurrences and counters, bit for bit), never to an uncapped device run.

Vacuity guard: under CMB_VERBOSE each capped launch prints `[grid] <kernel> <items> items, <lanes> lanes`; every case names the kernels
it is there for and asserts, for each, a line with items >= 3 * lanes: a first, a middle and a last trip.  For the frontier kernels
(k_bfs_pass, k_hbfs_pass, k_naive_pass, k_mvs_pass, ...) `items` is the largest frontier of a pass.  The read sets are sized for that
from the oracle's counters (LOCATED_ROWS for k_verify, IN_TEXT_STARTED for the stage and wide kernels, CIGARS_IN_TEXT_VERIFICATION
for k_traceback, the occurrences for the CIGAR kernels, 2 x reads for k_parts and k_exact at k = 0).
Not reached, and why:
  k_naive_start (FM)    takes one lane per read x strand and does not loop: it is not capped.
  k_bfs_pass_events,    the event half of a pass handles only the nodes whose descendants were interrupted in the final column: a few
  k_mvs_pass_events     per cent of the frontier.  The trips they reach are printed, not asserted.

The second half runs the knobs INTEGRATION.md calls neutral ("none of them changes a result") against the same oracle answers.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import columba_amd as ca  # noqa: E402
from columba_amd import indexbuild as ib  # noqa: E402
from columba_amd import synth  # noqa: E402
import test_best_ground_truth as tbg  # noqa: E402
import test_gpu_move_search as tms  # noqa: E402
from test_best_ground_truth import gpu_world  # noqa: E402,F401
from test_gpu_move import _pangenome  # noqa: E402
from test_gpu_parity import _check_alignments, _compare, _edge_reads  # noqa: E402
from test_gpu_prologue_dispatch import _reads  # noqa: E402
from test_ground_truth import clean, gt  # noqa: E402,F401

pytestmark = pytest.mark.gpu

CAPS = (1, 3)


class _OracleOnce:
    """oracle_py as _compare sees it, every answer computed once: the cases at cap 1, at cap 3 and under the knobs share it"""

    def __init__(self, op):
        self._op, self._memo = op, {}

    def OracleStrategy(self, spec, metric="edit", partition="dynamic"):
        st = self._op.OracleStrategy(spec, metric, partition)
        st.key = (id(spec), metric, partition)
        return st

    def once(self, key, reads, compute):
        key += (len(reads), hash(tuple(reads)))
        if key not in self._memo:
            self._memo[key] = compute()
        return self._memo[key]

    def match_batch(self, index, strat, k, reads, threads=1):
        return self.once((id(index), strat.key, k), reads, lambda: self._op.match_batch(index, strat, k, reads, threads=threads))


class _MoveOracleOnce:
    def __init__(self, orc, once):
        self._orc, self._once = orc, once

    def match_batch(self, strat, k, reads, threads=1, word_size=10):
        return self._once.once((id(self._orc), strat.key, k, word_size), reads,
                               lambda: self._orc.match_batch(strat, k, reads, threads=threads, word_size=word_size))


def fm_text():
    # repeat-rich, as the world of test_gpu_prologue_dispatch.py; a quarter of its size: the reads of up to three characters of the first
    # case match all over the text, and the oracle's time for them grows with it
    return synth.genome_rep(seed=29, n=250_000, scale=4.0)


def move_text():
    rng = np.random.default_rng(31)
    # a small pan-genome: 8 haplotypes of a 25 kb sequence with 0.5 % SNPs, a repeat-rich stretch, a random tail
    return np.concatenate([_pangenome(rng, 25_000, 8, 0.005), synth.genome_rep(seed=5, n=80_000, scale=4.0)[0],
                           np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 10_000)]])


MOVE_STARTS = (0, 100_000, 200_000)   # (+ the end of the text: three sequences for the alignments on the b-move index)


@pytest.fixture(scope="module")
def world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    from columba_amd import movebuild
    g, starts = fm_text()
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    once = _OracleOnce(op)
    mg = move_text()
    mv = movebuild.build_move(mg.tobytes(), device="cuda")
    mdev = ca.MoveIndex(mv)
    mdev.attach_text(mg.tobytes(), np.array(MOVE_STARTS + (len(mg),), dtype=np.uint64))
    move = {"g": mg, "text": mg.tobytes(), "mv": mv, "dev": mdev, "orc": _MoveOracleOnce(op.OracleMoveIndex(mv), once), "ca": ca, "op": once}
    # (in_index: the same text under indexes that never switch to in-text verification, the reference's -i 0 — every first part that
    # occurs at all starts its searches in the index, so that a few thousand reads leave a few thousand searches with further exact phases)
    in_index = {"genome": g, "ix": ix, "op": once, "dev": ca.Index(ix, in_text_switch=0), "orc": op.OracleIndex(ix, switch_point=0),
                "dev4": ca.Index(ix, kmer_size=4, in_text_switch=0), "orc4": op.OracleIndex(ix, switch_point=0, kmer_size=4)}
    return {"genome": g, "ix": ix, "op": once, "dev": ca.Index(ix), "orc": op.OracleIndex(ix), "dev4": ca.Index(ix, kmer_size=4),
            "orc4": op.OracleIndex(ix, kmer_size=4), "in_index": in_index, "move": move, "reads": {}}


# ------------------------------------------------------------------------------------------------ read sets
def _boundary_and_edge(g, starts, k, n_edge):
    """reads across sequence boundaries (spans = 1) and reads whose edits are indels packed at one end (test_gpu_parity._edge_reads)"""
    out = [g[int(s) - 70:int(s) + 80].tobytes() for s in np.asarray(starts, dtype=np.int64)[1:-1][:8]]
    return out + _edge_reads(g, n_edge, max(k, 1), seed=71)


def fm_reads(name, g, starts):
    """the read set of a case (a function of the text alone, so that the sizes can be checked against the oracle's counters on a CPU)"""
    if name == "k4":      # 100 and 151 bp, the odd reads (several N, not longer than the number of parts, empty)
        return _reads(g, 2000, 100, seed=401) + _reads(g, 2000, 151, seed=402, odd=False)
    if name == "k4_aligned":   # (without the reads of up to three characters: a CIGAR per occurrence is asked of the oracle's driver)
        return _reads(g, 640, 100, seed=401, odd=False) + _reads(g, 600, 151, seed=402, odd=False) + _boundary_and_edge(g, starts, 4, 40)
    if name == "k7":
        return (synth.sample_reads(g, 2400, 150, seed=407, n_frac=0.02, edit_choices=(0, 1, 2, 3, 6, 7, 7, 8))
                + _boundary_and_edge(g, starts, 7, 40))
    if name == "k9":
        return (synth.sample_reads(g, 1200, 100, seed=409, n_frac=0.01, edit_choices=(0, 3, 6, 8, 9, 9, 10))
                + [b"N" * 100, g[-101:-1].tobytes(), g[0:100].tobytes()] + _boundary_and_edge(g, starts, 9, 40))
    if name == "k10":     # (k_cigar_wide takes over beyond 9 errors)
        return (synth.sample_reads(g, 1200, 100, seed=410, n_frac=0.01, edit_choices=(0, 3, 6, 8, 10, 10, 11)) + _boundary_and_edge(g, starts, 10, 40))
    if name == "k12":     # (fewer reads: every read seeds a hundred candidates at 12 errors)
        return synth.sample_reads(g, 300, 150, seed=412, n_frac=0.01, edit_choices=(0, 3, 6, 8, 12, 12, 13)) + [b"N" * 150, g[0:150].tobytes()]
    if name == "exact_phases":   # kuch1 / kuch2: searches with a second exact phase
        return _reads(g, 5000, 120, seed=444, odd=False)
    if name == "k0":
        return (synth.sample_reads(g, 1200, 100, seed=400, n_frac=0.03, edit_choices=(0, 0, 0, 1))
                + [b"N" * 100, b"A", g[0:100].tobytes(), g[-101:-1].tobytes()])
    raise KeyError(name)


def move_reads(name, g):
    if name == "k4":
        return tms._reads(g, 4, 1200, 150, seed=74)
    if name == "k9":
        return tms._reads(g, 9, 450, 150, seed=79)
    if name == "hamming":
        return tms._reads(g, 3, 1200, 100, seed=73) + synth.sample_reads(g, 400, 100, seed=8, p_sub=1.0, p_ins=0.0, edit_choices=(0, 1, 3, 3))
    raise KeyError(name)


def _fm(world, name):
    if name not in world["reads"]:
        world["reads"][name] = fm_reads(name, world["genome"], world["ix"].seq_starts)
    return world["reads"][name]


def _mv(world, name):
    if ("move", name) not in world["reads"]:
        world["reads"][("move", name)] = move_reads(name, world["move"]["g"])
    return world["reads"][("move", name)]


# ------------------------------------------------------------------------------------------------ the guard
def grid_lines(err):
    """kernel -> [(items, lanes)] from the CMB_VERBOSE output"""
    out = {}
    for m in re.finditer(r"\[grid\] (\w+) (\d+) items, (\d+) lanes", err):
        out.setdefault(m.group(1), []).append((int(m.group(2)), int(m.group(3))))
    return out


def guard(capfd, cap, need, block=256, also=()):
    """every kernel of `need` ran a launch of at most `cap` blocks with at least three trips; prints the most trips of every kernel"""
    lines = grid_lines(capfd.readouterr().err)
    most = {k: max(i / max(l, 1) for i, l in v) for k, v in lines.items()}
    print("cap %d: items / lanes " % cap + ", ".join("%s %.1f" % (k, most[k]) for k in sorted(most)))
    for k, v in lines.items():
        bl = 64 if k in ("k_mvs_parts", "k_mvs_exact") else block
        assert all(0 < l <= cap * bl and l % bl == 0 for _, l in v), (k, v)
    for k in need:
        assert k in lines, (k, "no [grid] line", sorted(lines))
        assert any(i >= 3 * l for i, l in lines[k]), (k, lines[k], "fewer than three trips: the read set is too small for this kernel")
    for k in also:
        assert k in lines, (k, "no [grid] line", sorted(lines))
    return most


@pytest.fixture
def capped(monkeypatch, capfd):
    def set_cap(cap, **env):
        monkeypatch.setenv("CMB_VERBOSE", "1")
        monkeypatch.setenv("CMB_TEST_GRID_CAP", str(cap))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
    return set_cap


# ------------------------------------------------------------------------------------------------ FM index, ALL mode
EDIT_PIPELINE = ("k_parts", "k_bfs_start", "k_bfs_pass", "k_verify", "k_verify_stage", "k_traceback")
FM_CASES = [
    # 32-bit matrix words in the frontier and in k_verify_stage, narrow trace rows, naive backtracking for the short reads
    ("multiple_opt", "edit", "dynamic", 4, "k4", EDIT_PIPELINE + ("k_naive_pass",)),
    # 64-bit matrix words, wide trace rows
    ("columba", "edit", "dynamic", 7, "k7", EDIT_PIPELINE),
    # beyond 7 errors: k_wide_filter + k_verify_wide on slab slots
    ("columba", "edit", "uniform", 9, "k9", ("k_wide_filter", "k_verify_wide", "k_verify")),
    ("columba", "edit", "static", 12, "k12", ("k_wide_filter", "k_verify_wide", "k_verify")),
    # searches with further exact phases: k_exact at k > 0; Hamming distance: k_hbfs.  On the index that never switches to in-text
    # verification (with the default switch point one read x strand in ten leaves such a search: 25 000 reads for three trips at cap 3)
    ("kuch1", "edit", "dynamic", 4, "exact_phases", ("k_parts", "k_exact", "k_bfs_start", "k_bfs_pass")),
    ("kuch1", "hamming", "uniform", 4, "exact_phases", ("k_parts", "k_exact", "k_hbfs_start", "k_hbfs_pass")),
    ("kuch2", "edit", "static", 3, "exact_phases", ("k_parts", "k_exact", "k_bfs_start", "k_bfs_pass")),
    # k = 0: one lane of k_exact per read x strand runs the whole search
    ("kuch1", "edit", "dynamic", 0, "k0", ("k_exact",)),
]
_FM_ID = lambda c: "-".join(map(str, c[:4]))  # noqa: E731


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("case", FM_CASES, ids=_FM_ID)
def test_fm_batch_under_the_cap(world, capped, capfd, case, cap):
    spec, metric, partition, k, reads, need = case
    capped(cap)
    _compare(world["in_index"] if reads == "exact_phases" else world, spec, metric, partition, k, _fm(world, reads), dups_rare=False)
    guard(capfd, cap, need)


@pytest.mark.parametrize("cap", CAPS)
def test_overflowing_queues_under_the_cap(world, capped, capfd, cap):
    """CMB_TEST_SMALL_POOLS: every queue starts from almost nothing, overflows and is grown — the run that is repeated takes its
    chunks across the trips again"""
    capped(cap, CMB_TEST_SMALL_POOLS="1")
    _compare(world, "multiple_opt", "edit", "dynamic", 4, _fm(world, "k4"), dups_rare=False)
    err = capfd.readouterr().err
    assert "[retry] queues too small" in err
    lines = grid_lines(err)
    for kern in EDIT_PIPELINE:
        assert any(i >= 3 * l for i, l in lines[kern]), (kern, lines[kern])
    assert len(lines["k_parts"]) >= 2, "the prologue ran once: nothing overflowed"


# narrow k_cigar; wide k_cigar, also at the 9 errors up to which its match words reach; beyond them k_cigar_wide on slab slots
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("spec,k,reads,kernel", [("multiple_opt", 4, "k4_aligned", "k_cigar"), ("columba", 7, "k7", "k_cigar"), ("columba", 9, "k9", "k_cigar"),
                                                 ("columba", 10, "k10", "k_cigar_wide")])
def test_alignments_under_the_cap(world, oracle_built, capped, capfd, spec, k, reads, kernel, cap):
    capped(cap)
    rd = _fm(world, reads)
    _compare(world, spec, "edit", "dynamic", k, rd, dups_rare=False)
    capfd.readouterr()
    n_occ = _check_alignments(world, oracle_built, spec, "edit", k, rd, 3 * 256 * cap)
    most = guard(capfd, cap, (kernel, "k_parts"))
    assert most[kernel] * 256 * cap >= n_occ   # (the line is the launch over every final occurrence)


# ------------------------------------------------------------------------------------------------ the verification hook
def hook_input(g):
    """one pattern of 100 characters, a copy of text[pos, pos + 100) with a substitution, a deletion and an insertion, and 5200 start positions:
    2500 distinct ones all over the text (a distinct key each for the staged path), every position around pos, pos - 1 ... pos + 1 850 times
    each (2550 candidates that end in a traceback at 4 errors), the ends of the text"""
    rng = np.random.default_rng(88)
    pos = 100_000
    t = g[pos:pos + 101].tobytes()
    pat = t[:20] + (b"A" if t[20:21] != b"A" else b"C") + t[21:50] + t[51:80] + (b"G" if t[80:81] != b"G" else b"T") + t[80:100]
    assert len(pat) == 100
    starts = np.concatenate([rng.choice(len(g), 2500, replace=False), np.arange(pos - 60, pos + 60), np.repeat(np.arange(pos - 1, pos + 2), 850),
                             [len(g) - 5, len(g), 0]]).astype(np.uint32)
    rng.shuffle(starts)
    return pat, starts


def _hook_world(world):
    if "hook" not in world["reads"]:
        world["reads"]["hook"] = hook_input(world["genome"])
    return world["reads"]["hook"]


def hook_truth(gt, text, pat, starts, k):
    """groundtruth.c for a fixed start s: D(s) = min over e of the edit distance of the pattern and text[s, e) (a window within k is at most
    k longer or shorter than the pattern).  Returns {s: D(s)} of the distinct starts with D(s) <= k."""
    m, n, out = len(pat), len(text), {}
    for s in np.unique(starts).tolist():
        ds = [gt.gt_edit_distance(pat, m, text[s:e], e - s) for e in range(max(s, s + m - k), min(n, s + m + k) + 1)]
        if ds and min(ds) <= k:
            out[s] = min(ds)
    return out


_HOOK_TRUTH = {}


def _hook_against_truth(gt, text, pat, starts, occ, k, staged):
    """one record per candidate within k, at D(start) (the record's begin is the start or, where the alignment opens with deleted text
    characters, behind it: its window aligns at no more than the reported distance); the staged path verifies identical candidates once"""
    D = _HOOK_TRUTH[k] if k in _HOOK_TRUTH else _HOOK_TRUTH.setdefault(k, hook_truth(gt, text, pat, starts, k))   # (once per k)
    want = sorted(D.values()) if staged else sorted(D[s] for s in starts.tolist() if s in D)
    got = sorted({(int(o["begin"]), int(o["end"]), int(o["distance"])) for o in occ}) if staged else [(int(o["begin"]), int(o["end"]), int(o["distance"])) for o in occ]
    assert sorted(d for _, _, d in got) == want and len(want) > 0
    for b, e, d in set(got):
        assert gt.gt_edit_distance(pat, len(pat), text[b:e], e - b) <= d <= k, (b, e, d)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("k,staged,need", [(4, False, ("k_verify", "k_traceback")), (4, True, ("k_verify", "k_verify_stage")),
                                           (9, False, ("k_verify_wide",)), (9, True, ("k_verify", "k_wide_filter"))],
                         ids=["direct-4", "staged-4", "dp-9", "staged-9"])
def test_verification_hook_under_the_cap(world, gt, capped, capfd, k, staged, need, cap):
    """cmb_verify_batch (k_verify<false> + k_traceback; beyond 7 errors k_verify_wide<false> on its own slab) and cmb_verify_batch_staged
    (the batch's own path over given candidates) with fixed start positions: the oracle's records and counters, and every window's
    distance is groundtruth.c's edit distance of the pattern and the best window at that start"""
    pat, starts = _hook_world(world)
    capped(cap)
    d, dc = world["dev"].verify(pat, starts, k, 0, True, staged=staged)
    o, oc = world["op"].once((id(world["orc"]), "verify", k), [pat, starts.tobytes()], lambda: world["orc"].verify(pat, starts, k, 0, True))
    key = lambda a: sorted((int(x["begin"]), int(x["end"]), int(x["distance"])) for x in a)  # noqa: E731
    if staged:   # (identical candidates are verified once; the counters are scaled by the multiplicity)
        assert sorted(set(key(d))) == sorted(set(key(o)))
    else:
        assert key(d) == key(o)
    for n in ("IN_TEXT_STARTED", "ABORTED_IN_TEXT_VERIF", "CIGARS_IN_TEXT_VERIFICATION", "MATRIX_ROWS"):
        assert dc[n] == oc[n], (n, dc[n], oc[n])
    assert oc["IN_TEXT_STARTED"] >= 3 * 256 * cap and oc["CIGARS_IN_TEXT_VERIFICATION"] >= 3 * 256 * cap
    _hook_against_truth(gt, world["genome"].tobytes(), clean(pat), starts, d, k, staged)
    guard(capfd, cap, need)


# ------------------------------------------------------------------------------------------------ b-move
MVS_EDIT = ("k_mvs_parts", "k_mvs_exact", "k_mvs_start", "k_mvs_pass")
MOVE_CASES = [("multiple_opt", "edit", "dynamic", 4, "k4", MVS_EDIT), ("columba", "edit", "dynamic", 9, "k9", MVS_EDIT),
              ("kuch1", "hamming", "dynamic", 3, "hamming", ("k_mvs_parts", "k_mvs_exact", "k_mvs_hbfs_start", "k_mvs_hbfs_pass"))]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("case", MOVE_CASES, ids=_FM_ID)
def test_bmove_batch_under_the_cap(world, capped, capfd, case, cap):
    spec, metric, partition, k, reads, need = case
    capped(cap)
    tms._compare(world["move"], spec, partition, k, _mv(world, reads), metric=metric)
    guard(capfd, cap, need)


@pytest.mark.parametrize("cap", CAPS)
def test_bmove_alignments_under_the_cap(world, oracle_built, capped, capfd, cap):
    """moveCigarsOnText: k_cigar over the occurrences of a b-move batch, on the text beside the index — the occurrences are the oracle's
    (the case above), every CIGAR is the oracle's findCIGAR of (read on its strand, text[begin, end), distance)"""
    w = world["move"]
    reads = _mv(world, "k4")
    capped(cap)
    o_occ, o_off, _ = w["orc"].match_batch(w["op"].OracleStrategy(__import__("schemes_py").BY_NAME["multiple_opt"], "edit", "dynamic"), 4, reads,
                                            threads=8, word_size=8)
    mb = ca.MoveBatch(w["dev"], ca.SearchStrategy("multiple_opt", "edit", "dynamic"), 4, reads=reads, kmer_size=8)
    mb.want_alignments()
    mb.run()
    occ, offs, _ = mb.results()
    aln, ops = mb.alignments()
    assert np.array_equal(offs, o_off) and len(aln) == len(occ) >= 3 * 256 * cap
    for f in ("begin", "end", "distance"):
        assert np.array_equal(occ[f].astype(np.uint64), o_occ[f].astype(np.uint64)), f
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    cmds = []
    for i, r in enumerate(reads):
        fw = clean(r)
        rc = fw.translate(comp)[::-1]
        for j in range(int(offs[i]), int(offs[i + 1])):
            o = occ[j]
            cmds.append(f"findcigar {(rc if o['strand'] else fw).decode()} {w['text'][int(o['begin']):int(o['end'])].decode()} {int(o['distance'])}")
    res = subprocess.run([os.path.join(oracle_built, "oracle_driver")], input="\n".join(cmds) + "\n", capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(res) == len(cmds) == len(occ)
    gaps = 0
    for j, want in enumerate(res):
        a = aln[j]
        got = ca.cigar_string(ops[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["cigar_len"])])
        assert got == want, (j, occ[j], got, want)
        gaps += ("I" in got) or ("D" in got)
    assert gaps > 20
    starts = np.asarray(MOVE_STARTS + (len(w["g"]),), dtype=np.int64)
    idx = np.searchsorted(starts, occ["begin"].astype(np.int64), side="right") - 1
    assert np.array_equal(aln["seq_id"], idx.astype(np.uint32))
    assert np.array_equal(aln["seq_begin"].astype(np.int64), occ["begin"].astype(np.int64) - starts[idx])
    mb.close()
    guard(capfd, cap, ("k_cigar",) + MVS_EDIT)


# ------------------------------------------------------------------------------------------------ BEST mode
BEST_CFG = ("columba", "edit", 1, 94)


def best_reads():
    """the chunk of that configuration and those of nine other identities (other seeds and edit counts; the cut-offs are this
    configuration's).  A stratum's batch holds the reads that are searched at its k: the largest, about 0.65 of the reads on both
    strands, has to hold 3 x 768 read x strands for three trips of k_parts at cap 3"""
    return sum((tbg.chunk(("columba", "edit", 1, i)) for i in (94, 95, 91, 93, 92, 96, 97, 90, 89, 98)), [])


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("path", ["host", "device"])
def test_best_mode_under_the_cap(gpu_world, gt, capped, capfd, path, cap):
    """the strata of BEST mode run as batches at growing k over the same buffers, the later ones over preset items: slots are reused
    across runs as well as across trips.  Judge: plain dynamic programming (test_best_ground_truth.check_best)."""
    spec, metric, x, min_identity = BEST_CFG
    reads = best_reads()
    capped(cap)
    fn = ca.match_best if path == "host" else ca.match_best_device
    res = fn(gpu_world["dev"], ca.SearchStrategy(spec, metric, "dynamic"), reads, x=x, min_identity=min_identity)
    tbg.check_best(gt, BEST_CFG, reads, tbg.norm_lib(res), "match_best under cap %d (%s)" % (cap, path))
    lines = grid_lines(capfd.readouterr().err)
    assert any(i >= 3 * l for i, l in lines["k_parts"]), lines["k_parts"]
    assert any(i >= 3 * l for i, l in lines["k_verify"]), lines["k_verify"]
    assert len(lines["k_parts"]) >= 3, "fewer than three strata ran"


# ------------------------------------------------------------------------------------------------ the knobs that change no result
KNOBS = [{"CMB_BFS_GRID": "1", "CMB_BFS_GRID_EV": "1"}, {"CMB_BFS_CHAIN": "1"}, {"CMB_BFS_CHAIN": "64"}, {"CMB_BFS_CHECK": "1"},
         {"CMB_STAGE_BLOCKS": "1"}, {"CMB_STAGE_BLOCKS": "8"}, {"CMB_P_SLOTS": "256", "CMB_V_SLOTS": "256", "CMB_TB_SLOTS": "256"},
         {"CMB_STAGE_GRID": "1"},
         {"CMB_SUBBATCHES": "4", "CMB_MAX_CONCURRENT": "1"}, {"CMB_SUBBATCHES": "4", "CMB_MAX_CONCURRENT": "4"},
         {"CMB_SUBBATCHES": "4", "CMB_SERIAL_SUBBATCHES": "1"}]
_KNOB_ID = lambda e: ",".join("%s=%s" % (k[4:], v) for k, v in e.items())  # noqa: E731


@pytest.mark.parametrize("env", KNOBS, ids=_KNOB_ID)
@pytest.mark.parametrize("case", FM_CASES[:2], ids=_FM_ID)
def test_geometry_knobs_change_no_result(world, monkeypatch, case, env):
    spec, metric, partition, k, reads, _ = case
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    _compare(world, spec, metric, partition, k, _fm(world, reads), dups_rare=False)


@pytest.mark.parametrize("env", [{"CMB_VW_SLOTS": "256"}, {"CMB_VW_SLOTS": "100"}], ids=_KNOB_ID)
def test_wide_verification_slots_change_no_result(world, monkeypatch, capfd, env):
    """(100 slots once gave a launch of 0 blocks: it is one block now)"""
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    monkeypatch.setenv("CMB_VERBOSE", "1")
    capfd.readouterr()
    _compare(world, "columba", "edit", "uniform", 9, _fm(world, "k9"), dups_rare=False)
    lines = grid_lines(capfd.readouterr().err)
    assert all(l == 256 for _, l in lines["k_verify_wide"]) and any(i >= 3 * l for i, l in lines["k_verify_wide"])


_MVS_KNOBS = [{"CMB_MVS_GRID": "1"}, {"CMB_MVS_CHAIN": "1"}, {"CMB_MVS_CHAIN": "64"}]


@pytest.mark.parametrize("env", _MVS_KNOBS + [dict(e, CMB_MOVE_POS64="1") for e in _MVS_KNOBS], ids=_KNOB_ID)
def test_bmove_knobs_change_no_result(world, monkeypatch, env):
    """one block that makes many trips, no walk, and a walk that crosses blocks of match words: on both arms of the expansion (32-bit
    positions with the children in slots, and with CMB_MOVE_POS64=1 the general 40-bit positions with one child per character)"""
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    tms._compare(world["move"], "multiple_opt", "dynamic", 4, _mv(world, "k4"))
