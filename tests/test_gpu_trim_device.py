"""Occurrences over a sequence end trimmed by the run itself (Batch.trim_on_device -> cmb_batch_trim_on_device; dev_trim.hpp).

Worlds and chunks are those of tests/test_gpu_contigs.py (contigs.contig_world: 60 000 characters in 383 sequences, a quarter of all
occurrences over a sequence end; contigs.dense_world: sequences of 6).  The bar is never the new stage against itself:
  text     Batch.sam_device of the batch with the switch == Batch.sam (the host path: samOfRead -> trimOccurrence per occurrence) of a
           second batch WITHOUT it == the oracle's text, byte for byte, with and without unmapped records; host_reads == 0
  records  every occurrence that has spans == 1 in the plain batch, through cmb_trim_occurrence with the read's strand pattern and k:
           found -> cmb_occ, seq_id, seq_begin and CIGAR runs are the switched batch's entry at the same index, spans == 2; not found ->
           the original record with spans == 4.  Every other entry, all offsets and all search counters bit for bit; trim_stats == the
           counts derived that way
Vacuity: spanning occurrences are at least a tenth of all; under edit distance at least one is trimmed and one dropped; under Hamming
distance none is trimmed.

The mixed chunk (reads of 12 ... 250 characters, reads with N) holds 40 reads of every length at k = 2; at k = 10 two each of 12 and 17
characters beside 40 of every longer length: such a read lies within 10 errors of almost every window of the text, so two of them are
thousands of occurrences, each a host round trip in the plain batch.  At k = 12 (chunk_of) the reads are those of 60 characters and more:
k_verify_wide<WxThirteen> on patterns shorter than that is not run here (DESIGN.md §4.7 says so).

Run with `pytest -m gpu` on an MI355X.  Observed there (printed by the tests): see DESIGN.md §4.7.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # (the child process of test_under_the_grid_cap has no conftest.py)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import columba_amd as ca  # noqa: E402
from columba_amd import indexbuild as ib, synth  # noqa: E402
import contigs  # noqa: E402
import samcheck  # noqa: E402

pytestmark = pytest.mark.gpu

# (strategy, metric, k, XA tag): k = 7 the 64-bit in-text matrix, k = 10 k_verify_wide<WxTen> + k_cigar_wide, k = 12 WxThirteen
CONFIGS = [("columba", "edit", 2, False), ("columba", "edit", 7, False), ("columba", "edit", 10, False), ("columba", "edit", 12, False),
           ("multiple_opt", "edit", 4, True), ("kuch1", "hamming", 2, False)]
_ID = lambda c: f"{c[0]}-{c[1]}-k{c[2]}" + ("-xa" if c[3] else "")  # noqa: E731


def edge_reads(every_end=False):
    """16 reads of 60 characters cut from the text so that they hang over a sequence end by one or two characters, at four ends with 70
    characters and more on either side (every_end: at all 164 such ends, 656 reads): the two options of findSeqName at every k >= 2.
    (contigs.chunk(2) by itself has 73 occurrences over an end and cmb_trim_occurrence finds none of them again: no window lies within 2
    characters of an end.)"""
    w = contigs.contig_world()
    g, st = w["genome"], w["starts"]
    ends = [s for a, s, b in zip(st, st[1:], st[2:]) if s - a >= 70 and b - s >= 70]
    assert len(ends) == 164
    if not every_end:
        ends = ends[3:40:10]
    reads = []
    for s in ends:
        reads += [g[s - over:s - over + 60].tobytes() for over in (1, 2)]  # option 1: the begin just before the end of a sequence
        reads += [g[s + over - 60:s + over].tobytes() for over in (1, 2)]  # option 2: the end just over the start of the next
    return reads


def chunk_of(k, per_length=50, every_end=False):
    """contigs.chunk as tests/test_gpu_contigs.py takes it (from 10 errors on, reads of 40 instead of 30 characters) and edge_reads; at 12
    errors the reads of 60 characters and more: shorter ones lie within 12 errors of every window of the text"""
    reads, ids, quals = contigs.chunk(k, per_length, (40, 60, 100, 150) if k >= 10 else (30, 60, 100, 150))
    extra = edge_reads(every_end)
    reads = reads + extra
    ids = ids + [f"@edge{i} over an end" for i in range(len(extra))]
    quals = quals + ["".join(chr(35 + (i + j) % 38) for j in range(60)) for i in range(len(extra))]
    if k >= 12:
        keep = [i for i, r in enumerate(reads) if len(r) >= 60]
        reads, ids, quals = [reads[i] for i in keep], [ids[i] for i in keep], [quals[i] for i in keep]
    return reads, ids, quals


def mixed_chunk(k):
    """reads of 12 ... 250 characters with 0 ... k edits, a sixth of them with one to three N"""
    g = contigs.contig_world()["genome"]
    reads = []
    for length in (12, 17, 40, 64, 151, 250):
        # (at 10 errors two reads each of 12 and 17 characters: such a read lies within 10 errors of almost every window of the text)
        reads += synth.sample_reads(g, 2 if k >= 10 and length < 40 else 40, length, seed=300 + length + k, edit_choices=(0, 0, 1, 2, k))
    rng = np.random.default_rng(5 + k)
    for i in range(0, len(reads), 6):
        r = bytearray(reads[i])
        for p in rng.integers(0, len(r), int(rng.integers(1, 4))).tolist():
            r[p] = ord("N")
        reads[i] = bytes(r)
    ids = [f"@mixed{i} len={len(r)}" for i, r in enumerate(reads)]
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    return reads, ids, quals


def open_world(op=None):
    out = {"op": op}
    for w in (contigs.contig_world(), contigs.dense_world()):
        ix = ib.build_index(w["text"], seq_starts=np.asarray(w["starts"], np.uint32), device="cuda")
        out[w["label"]] = dict(w, ix=ix, dev=ca.Index(ix), orc=op.OracleIndex(ix) if op else None)
    return out


@pytest.fixture(scope="module")
def world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    return open_world(op)


def _same(a, b, what):
    if a != b:
        n = min(len(a), len(b))
        i = next((j for j in range(n) if a[j] != b[j]), n)
        raise AssertionError(f"{what}: lengths {len(a)} / {len(b)}, first difference at {i}: {a[max(0, i - 120):i + 60]!r} / {b[max(0, i - 120):i + 60]!r}")


def run_batch(w, spec, metric, k, reads, trim, per_strand=False, first=None):
    """a batch that has run on `reads` (first: the chunk it is created with and runs on before — `reads` is then staged)"""
    b = ca.Batch(w["dev"], ca.SearchStrategy(spec, metric, "dynamic"), k, first if first is not None else reads)
    b.want_alignments()
    if per_strand:
        ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
    if trim:
        b.trim_on_device()
    if first is not None:
        b.stage(ca.pack_reads(reads))
        b.run()
    b.run()
    return b


def oracle_text(world, w, spec, metric, k, reads, ids, quals, unmapped, xa):
    import schemes_py as sp
    op = world["op"]
    return op.match_batch_sam(w["orc"], op.OracleStrategy(sp.BY_NAME[spec], metric, "dynamic"), k, reads, ids, quals, w["names"], unmapped=unmapped, xa=xa)


def check_text(plain, trimmed, w, reads, ids, quals, xa, oracle=None, label=""):
    """oracle: {unmapped: text} or None"""
    for unmapped in (True, False):
        host = plain.sam(ids, quals, w["names"], unmapped=unmapped, xa=xa)
        got, host_reads = trimmed.sam_device(ids, quals, w["names"], unmapped=unmapped, xa=xa)
        print(f"{label} unmapped={unmapped}: {len(got)} bytes, host_reads={host_reads}")
        _same(got, host, "device text with the switch / host text without")
        _same(trimmed.sam(ids, quals, w["names"], unmapped=unmapped, xa=xa), host, "host text with the switch / host text without")
        assert host_reads == 0
        if oracle is not None:
            _same(got, oracle[unmapped], "device text with the switch / oracle text")


def check_records(plain, trimmed, w, metric, k, reads, label=""):
    """-> (occurrences, spanning, trimmed, dropped), derived from the plain batch and cmb_trim_occurrence"""
    occ_p, offs_p, cnt_p = plain.results()
    occ_t, offs_t, cnt_t = trimmed.results()
    aln_p, ops_p = plain.alignments()
    aln_t, ops_t = trimmed.alignments()
    assert np.array_equal(offs_p, offs_t) and len(occ_p) == len(occ_t) == len(aln_p) == len(aln_t)
    assert cnt_p == cnt_t, {n: (cnt_p[n], cnt_t[n]) for n in cnt_p if cnt_p[n] != cnt_t[n]}
    assert not (aln_t["spans"] == 1).any() and np.isin(aln_t["spans"], (0, 2, 4)).all()
    runs = lambda aln, ops, j: ops[int(aln["cigar_off"][j]):int(aln["cigar_off"][j]) + int(aln["cigar_len"][j])].tolist()  # noqa: E731
    n_span = n_trim = n_drop = 0
    L = ca.lib()
    for i, r in enumerate(reads):
        fw = samcheck.clean(r)
        pats = (fw, samcheck.revcomp(fw))
        for j in range(int(offs_p[i]), int(offs_p[i + 1])):
            if aln_p["spans"][j] != 1:
                assert occ_p[j] == occ_t[j] and aln_p["spans"][j] == aln_t["spans"][j] == 0, (i, j, occ_p[j], occ_t[j], aln_t[j])
                assert (aln_p["seq_id"][j], aln_p["seq_begin"][j]) == (aln_t["seq_id"][j], aln_t["seq_begin"][j])
                assert runs(aln_p, ops_p, j) == runs(aln_t, ops_t, j), (i, j)
                continue
            n_span += 1
            oc1, al1 = occ_p[j:j + 1].copy(), aln_p[j:j + 1].copy()
            ops1 = np.zeros(2 * k + 8, np.uint16)
            nops, found = C.c_uint32(), C.c_int32()
            pat = pats[int(occ_p["strand"][j])]
            ca._chk(L.cmb_trim_occurrence(w["dev"].h, pat, len(pat), k, ca.METRIC[metric], ca._p(oc1), ca._p(al1), ca._p(ops1), ops1.shape[0],
                                          C.byref(nops), C.byref(found)))
            if found.value:
                n_trim += 1
                assert aln_t["spans"][j] == 2, (i, j, aln_t[j], oc1, occ_t[j])
                assert occ_t[j] == oc1[0], (i, j, occ_p[j], oc1[0], occ_t[j])
                assert (aln_t["seq_id"][j], aln_t["seq_begin"][j]) == (al1["seq_id"][0], al1["seq_begin"][0]), (i, j, aln_t[j], al1[0])
                assert runs(aln_t, ops_t, j) == ops1[:nops.value].tolist(), (i, j, ca.cigar_string(runs(aln_t, ops_t, j)), ca.cigar_string(ops1[:nops.value]))
            else:
                n_drop += 1
                assert aln_t["spans"][j] == 4, (i, j, occ_p[j], aln_t[j], occ_t[j])
                assert occ_t[j] == occ_p[j] and (aln_p["seq_id"][j], aln_p["seq_begin"][j]) == (aln_t["seq_id"][j], aln_t["seq_begin"][j])
                assert runs(aln_p, ops_p, j) == runs(aln_t, ops_t, j), (i, j)
    st = trimmed.trim_stats()
    print(f"{label}: {len(occ_p)} occurrences, {n_span} over a sequence end, {n_trim} trimmed, {n_drop} dropped; trim_stats {st}; "
          f"stage {dict((n, round(v, 3)) for n, v in trimmed.timings().items() if n.startswith('k_trim'))}")
    assert st == {"spanning": n_span, "trimmed": n_trim, "dropped": n_drop}
    assert plain.trim_stats() == {"spanning": 0, "trimmed": 0, "dropped": 0}
    return len(occ_p), n_span, n_trim, n_drop


def not_vacuous(metric, n, n_span, n_trim, n_drop, tenth=True):
    """tenth=False (the mixed chunk): a read of 12 characters runs over an end at one begin in thirteen (12 of the 157 characters of a mean
    sequence) and has thousands of occurrences, so the share of spanning occurrences follows the read lengths there; a hundred of them"""
    assert n_span * 10 >= n if tenth else n_span >= 100, (n, n_span)
    if metric == "edit":
        assert n_trim >= 1 and n_drop >= 1, (n_trim, n_drop)
    else:
        assert n_trim == 0 and n_drop == n_span


def check_pair(world, w, cfg, chunk, oracle=True, label="", tenth=True, **how):
    spec, metric, k, xa = cfg
    reads, ids, quals = chunk
    plain, trimmed = run_batch(w, spec, metric, k, reads, False, **how), run_batch(w, spec, metric, k, reads, True, **how)
    try:
        orc = {u: oracle_text(world, w, spec, metric, k, reads, ids, quals, u, xa) for u in (True, False)} if oracle else None
        check_text(plain, trimmed, w, reads, ids, quals, xa, orc, label)
        counts = check_records(plain, trimmed, w, metric, k, reads, label)
    finally:
        plain.close()
        trimmed.close()
    not_vacuous(metric, *counts, tenth=tenth)
    return counts


# ------------------------------------------------------------------------------------------------ 1. text, 2. records
@pytest.fixture(scope="module")
def pairs(world):
    """cfg -> the plain and the switched batch of a configuration, run once for the two tests below and closed after the module"""
    cache = {}

    def pair_of(cfg):
        if cfg not in cache:
            spec, metric, k, xa = cfg
            reads = chunk_of(k)[0]
            cache[cfg] = (run_batch(world["contig"], spec, metric, k, reads, False), run_batch(world["contig"], spec, metric, k, reads, True))
        return cache[cfg]

    yield pair_of
    for plain, trimmed in cache.values():
        plain.close()
        trimmed.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_text(world, pairs, cfg):
    spec, metric, k, xa = cfg
    w = world["contig"]
    reads, ids, quals = chunk_of(k)
    plain, trimmed = pairs(cfg)
    orc = {u: oracle_text(world, w, spec, metric, k, reads, ids, quals, u, xa) for u in (True, False)}
    check_text(plain, trimmed, w, reads, ids, quals, xa, orc, _ID(cfg))
    st = trimmed.trim_stats()
    n = len(trimmed.results()[0])
    not_vacuous(metric, n, st["spanning"], st["trimmed"], st["dropped"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_records(world, pairs, cfg):
    spec, metric, k, xa = cfg
    plain, trimmed = pairs(cfg)
    not_vacuous(metric, *check_records(plain, trimmed, world["contig"], metric, k, chunk_of(k)[0], _ID(cfg)))
    timed = trimmed.timings()
    assert "k_trim_plan" in timed and (metric != "edit" or {"k_trim_verify", "k_trim_pick", "k_trim_commit"} <= set(timed)), timed


# ------------------------------------------------------------------------------------------------ 3. dense world
def test_dense_world(world):
    """60 reads of 30 characters on sequences of 6: every occurrence runs over an end and none can be trimmed — all dropped by the plan
    kernel, 60 unmapped records written by the device"""
    w = world["dense"]
    d = contigs.dense_world()
    rng = np.random.default_rng(3)
    reads = [d["text"][p:p + 30] for p in rng.integers(0, 120_000 - 30, 60).tolist()]
    ids, quals = [f"@dense{i} x" for i in range(60)], ["".join(chr(40 + (i + j) % 30) for j in range(30)) for i in range(60)]
    plain, trimmed = run_batch(w, "columba", "edit", 2, reads, False), run_batch(w, "columba", "edit", 2, reads, True)
    try:
        orc = {u: oracle_text(world, w, "columba", "edit", 2, reads, ids, quals, u, False) for u in (True, False)}
        check_text(plain, trimmed, w, reads, ids, quals, False, orc, "dense")
        n, n_span, n_trim, n_drop = check_records(plain, trimmed, w, "edit", 2, reads, "dense")
        assert n >= 60 and n_span == n_drop == n and n_trim == 0
        got, host_reads = trimmed.sam_device(ids, quals, w["names"], unmapped=True)
        lines = got.splitlines()
        assert host_reads == 0 and len(lines) == 60 and all(x.split("\t")[1:4] == ["4", "*", "0"] for x in lines)
        assert trimmed.sam_device(ids, quals, w["names"], unmapped=False) == ("", 0)
    finally:
        plain.close()
        trimmed.close()


# ------------------------------------------------------------------------------------------------ 4. loops and shapes
SHAPE_CONFIGS = [("columba", "edit", 2, False), ("columba", "edit", 10, False)]


@pytest.mark.parametrize("cfg", SHAPE_CONFIGS, ids=_ID)
def test_composite_batch(world, monkeypatch, cfg):
    """three sub-batches, each with its own stage on its own stream; the statistics are their sum"""
    monkeypatch.setenv("CMB_SUBBATCHES", "3")
    check_pair(world, world["contig"], cfg, chunk_of(cfg[2]), label=f"3 sub-batches {_ID(cfg)}")


@pytest.mark.parametrize("cfg", SHAPE_CONFIGS, ids=_ID)
def test_staged_chunk(world, cfg):
    """the batch is created with another chunk of as many reads and runs on it first; the chunk under test is staged (Batch.stage)"""
    reads, ids, quals = chunk_of(cfg[2])
    check_pair(world, world["contig"], cfg, (reads, ids, quals), label=f"staged {_ID(cfg)}", first=reads[7:] + reads[:7])


@pytest.mark.parametrize("cfg", SHAPE_CONFIGS, ids=_ID)
def test_filter_per_strand(world, cfg):
    """every strand filtered by itself: two groups per read.  (The oracle's ALL-mode text filters the strands together: the bars are
    the host path and cmb_trim_occurrence.)"""
    check_pair(world, world["contig"], cfg, chunk_of(cfg[2]), oracle=False, label=f"per strand {_ID(cfg)}", per_strand=True)


@pytest.mark.parametrize("cfg", SHAPE_CONFIGS, ids=_ID)
def test_mixed_lengths_and_n(world, cfg):
    check_pair(world, world["contig"], cfg, mixed_chunk(cfg[2]), label=f"mixed {_ID(cfg)}", tenth=False)


def test_small_pools_retry(world, monkeypatch, capfd):
    """CMB_TEST_SMALL_POOLS: the record queue of the stage starts below one chunk of a wavefront, overflows, is grown to what the kernels
    asked for and the verification runs again — at 2 errors through k_verify + k_traceback, at 10 through k_verify_wide"""
    monkeypatch.setenv("CMB_TEST_SMALL_POOLS", "1")
    monkeypatch.setenv("CMB_VERBOSE", "1")
    for cfg in SHAPE_CONFIGS:
        capfd.readouterr()
        check_pair(world, world["contig"], cfg, chunk_of(cfg[2]), oracle=False, label=f"small pools {_ID(cfg)}")
        assert "[retry] trim:" in capfd.readouterr().err


CHILD_CHUNK = dict(per_length=100, every_end=True)  # the child's chunk: more than a thousand occurrences and more than 256 windows


def _child(cap, oracle_file):
    """(a fresh process) k = 2 and k = 10 under CMB_TEST_GRID_CAP=cap on a chunk large enough for several trips of every loop"""
    os.environ["CMB_TEST_GRID_CAP"] = str(cap)
    os.environ["CMB_VERBOSE"] = "1"
    world = open_world()
    orc = json.load(open(oracle_file))
    for cfg in SHAPE_CONFIGS:
        spec, metric, k, xa = cfg
        reads, ids, quals = chunk_of(k, **CHILD_CHUNK)
        w = world["contig"]
        plain, trimmed = run_batch(w, spec, metric, k, reads, False), run_batch(w, spec, metric, k, reads, True)
        check_text(plain, trimmed, w, reads, ids, quals, xa, {True: orc[str(k)]["1"], False: orc[str(k)]["0"]}, f"cap {cap} {_ID(cfg)}")
        counts = check_records(plain, trimmed, w, metric, k, reads, f"cap {cap} {_ID(cfg)}")
        not_vacuous(metric, *counts)
        print("CHILD-COUNTS", k, *counts)
    print("CHILD-OK")


@pytest.mark.parametrize("cap", [1, 3])
def test_under_the_grid_cap(world, tmp_path, cap):
    """every launch of the stage with more work than lanes (CMB_TEST_GRID_CAP, read per run: host_grid.hpp), in a process of its own.
    The parent hands over the oracle's texts; the child prints `[grid] <kernel> <items> items, <lanes> lanes` per capped launch"""
    import re
    w = world["contig"]
    orc = {}
    for spec, metric, k, xa in SHAPE_CONFIGS:
        reads, ids, quals = chunk_of(k, **CHILD_CHUNK)
        orc[str(k)] = {"1": oracle_text(world, w, spec, metric, k, reads, ids, quals, True, xa),
                       "0": oracle_text(world, w, spec, metric, k, reads, ids, quals, False, xa)}
    f = tmp_path / "oracle.json"
    f.write_text(json.dumps(orc))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(cap), str(f)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "CHILD-OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    lines = {}
    for m in re.finditer(r"\[grid\] (k_trim_\w+|k_\w+ \(trim\)) (\d+) items, (\d+) lanes", res.stderr):
        lines.setdefault(m.group(1), []).append((int(m.group(2)), int(m.group(3))))
    print({k: sorted(set(v))[-3:] for k, v in lines.items()})
    for kernel in ("k_trim_plan", "k_verify (trim)", "k_traceback (trim)", "k_verify_wide (trim)", "k_trim_keys", "k_trim_pick", "k_trim_commit"):
        assert kernel in lines, (kernel, sorted(lines))
        assert all(0 < l <= cap * 256 for _, l in lines[kernel]), (kernel, lines[kernel])
    # at cap 1 a first, a middle and a last trip of the plan, and more than one trip of the kernels that run over what it found
    assert any(i >= (3 if cap == 1 else 1) * l + 1 for i, l in lines["k_trim_plan"]), lines["k_trim_plan"]
    if cap == 1:
        for kernel in ("k_verify (trim)", "k_verify_wide (trim)", "k_trim_keys", "k_trim_pick"):
            assert any(i > l for i, l in lines[kernel]), (kernel, lines[kernel])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(world):
    w = world["contig"]
    reads, ids, quals = chunk_of(2)
    b = ca.Batch(w["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), 2, reads)
    with pytest.raises(ca.CmbError) as e:
        b.trim_on_device()
    assert e.value.code == -1 and "cmb_batch_want_alignments" in str(e.value)  # CMB_ERR_INVALID
    b.close()
    pair = []
    for _ in range(2):
        b = run_batch(w, "columba", "edit", 2, reads, True, per_strand=True)
        pair.append(b)
    with pytest.raises(ca.CmbError) as e:
        ca.pair_batches_sam_device(pair[0], pair[1], ids, ids, quals, quals, w["names"])
    assert e.value.code == -1 and "cmb_batch_trim_on_device" in str(e.value)
    for b in pair:
        b.close()


# ------------------------------------------------------------------------------------------------ 6. the command-line aligner
def test_cli_writes_the_same_file(world, tmp_path):
    """columba_align (examples/) on a FASTA of contig_world: CMB_TRIM_DEVICE=1 changes no record of the SAM file (without it the stage
    does not run: the switch is opt-in)"""
    from test_cpp_adapter import _build_align
    w = contigs.contig_world()
    exe = _build_align(str(tmp_path))
    ix = ib.build_index(w["text"], seq_starts=np.asarray(w["starts"], np.uint32), seq_names=w["names"], device="cuda")
    ib.save_index(ix, str(tmp_path / "idx"))
    reads, ids, _ = chunk_of(4)
    with open(tmp_path / "reads.fa", "w") as f:
        for i, r in enumerate(reads):
            f.write(f">{ids[i][1:]}\n{r.decode()}\n")
    texts = []
    for trim in (False, True):
        env = {k: v for k, v in os.environ.items() if k != "CMB_TRIM_DEVICE"}
        env["CMB_VERBOSE"] = "1"
        if trim:
            env["CMB_TRIM_DEVICE"] = "1"
        out = tmp_path / f"all{int(trim)}.sam"
        r = subprocess.run([exe, "-r", str(tmp_path / "idx"), "-f", str(tmp_path / "reads.fa"), "-o", str(out), "-a", "all", "-e", "4", "-S", "columba",
                            "-b", "100"], check=True, capture_output=True, text=True, env=env)
        assert ("[trim]" in r.stderr) == trim  # (the stage ran, or did not)
        texts.append(out.read_text())
    body = lambda t: "\n".join(x for x in t.splitlines() if not x.startswith("@PG"))  # noqa: E731  (@PG holds the command line: the output's name)
    _same(body(texts[1]), body(texts[0]), "columba_align with CMB_TRIM_DEVICE=1 / without")
    records = [x for x in texts[0].splitlines() if not x.startswith("@")]
    assert len(records) >= len(reads) and sum(x.split("\t")[1] != "4" for x in records) >= 100


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "child":
    _child(int(sys.argv[2]), sys.argv[3])
