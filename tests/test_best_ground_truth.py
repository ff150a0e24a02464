"""BEST (+x strata) mode against textbook dynamic programming, on chunks whose reads have DIFFERENT cut-offs.

The other BEST-mode tests compare code written from one reading of the reference with more code written from the same reading
(`cmb_match_best`, `cmb_match_best_device`, `oracle/`).  Here the judge is `oracle/groundtruth.c` (Sellers' semi-global alignment,
plain O(mn) edit distance; for Hamming distance a sliding mismatch count): per read and strand "the true distance of the best alignment
ending at j", d* its minimum over both strands.  The cut-off is per read, min(13, max supported, len * (100 - I) / 100)
(searchstrategy.h:1797), and every chunk mixes reads of 12, 19, 40, 64, 100, 151 and 250 characters, so that reads with different k, maxED
and cutOff share a stratum's batch.

Per read that lies away from the inner sequence ends (trimming changes distances there):
  x = 0                    best == d* if d* <= cut-off, else unmapped with an empty list
  x > 0, cut-off < x       unmapped: findBestAlignments starts at k = max(x, 1) and never enters its loop (searchstrategy.cpp:676)
  x > 0, d* == 0           stratum 0 is never examined (searchstrategy.cpp:686 starts at prevK + 1): only "unmapped or
                           best in [1, cut-off]" and sound records
  x > 0 otherwise          as x = 0
Records of every mapped read: distances in [best, top = min(best + x, cut-off)], one at `best`, n_hits >= the records at `best`, keys
(distance, strand, seq_id, seq_begin) strictly increasing, begin == seq_start[seq_id] + seq_begin, end inside that sequence, the CIGAR
consumes read and text[begin, end) and shows the window's true edit distance, which is at most the reported one (Hamming: width = read
length, mismatches = distance).  Completeness inside the reported strata: every end position j with true distance d_j in [best, top] has
a record of distance <= d_j ending within 4 * top (8 * top, the filter's chain, for at most 2 % of them).

Five paths get these assertions: the oracle (CPU, runs everywhere), cmb_match_best, cmb_match_best_device, cmb_move_match_best, and
cmb_match_best_device over composite batches (CMB_SUBBATCHES=3).  The GPU paths must also return the oracle's lists on these chunks,
host and device path bit for bit.
"""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

from columba_amd import synth  # noqa: E402
from test_ground_truth import clean, gt  # noqa: E402,F401
import samcheck  # noqa: E402

NONE = 0xFFFFFFFF
# (strategy, metric, x, minimal identity): cut-offs from 1 to 13; the last one walks the strata 1, 3, 5, 9, 13
CONFIGS = [("columba", "edit", 0, 95), ("columba", "edit", 1, 94), ("minU", "edit", 2, 96), ("columba", "hamming", 1, 93),
           ("kuch1", "hamming", 0, 97), ("columba", "edit", 0, 91)]
EDIT_CONFIGS = [c for c in CONFIGS if c[1] == "edit"]
LENGTHS = (40, 64, 100, 151, 250)
_ID = lambda c: "-".join(map(str, c))  # noqa: E731

_W = {}


def _world():
    """text, truth cache and chunks: one per process, shared by the CPU and the GPU tests"""
    if not _W:
        g, starts = synth.genome_rep(seed=23, n=120_000, scale=4.0)
        _W.update(genome=g, text=g.tobytes(), starts=[int(s) for s in starts], truth={}, chunks={}, oracle={}, runs={})
    return _W


def max_supported(spec):
    import schemes_py as sp
    k = 0
    while (k + 1) in sp.BY_NAME[spec]["schemes"]:
        k += 1
    return min(k, 13)


def cutoff(spec, min_identity, length):
    """getMaxED, searchstrategy.h:1797-1806"""
    return min(13, max_supported(spec), length * (100 - min_identity) // 100)


def chunk(cfg):
    w = _world()
    if cfg in w["chunks"]:
        return w["chunks"][cfg]
    spec, metric, x, min_identity = cfg
    g, starts = w["genome"], w["starts"]
    model = dict(p_sub=1.0, p_ins=0.0) if metric == "hamming" else {}
    reads = []
    for li, length in enumerate(LENGTHS):
        c = cutoff(spec, min_identity, length)
        # edits up to beyond the read's own cut-off (for the longest reads: beyond the largest one); with x > 0 no unedited read is drawn
        choices = [1, max(c // 2, 1), max(c - 1, 1), max(c, 1), max(c, 1), c + 1, c + 2, c + 4] + ([0] if x == 0 else [])
        reads += synth.sample_reads(g, 38, length, seed=1000 * min_identity + 10 * x + li, n_frac=0.02, edit_choices=tuple(choices), **model)
    reads.append(g[500:519].tobytes())  # 19 characters: cut-off 0 at 95 %
    reads.append(g[900:912].tobytes())  # 12 characters: cut-off 0 from 92 % on, also where x > 0
    for s in starts[1:-1]:  # reads across every inner sequence end: trimmed or dropped
        reads += [g[s - 50:s + 50].tobytes(), g[s - 3:s + 97].tobytes(), g[s - 97:s + 3].tobytes()]
    reads.append(b"N" * 100)
    if x > 0:  # five deliberately unedited reads: stratum 0 is never looked at
        for li, length in enumerate(LENGTHS):
            r = g[7000 + 20_000 * li:7000 + 20_000 * li + length].tobytes()
            reads.append(synth.revcomp(r) if li % 2 else r)
    assert 200 <= len(reads) <= 250
    w["chunks"][cfg] = reads
    return reads


def fill_truth(gt, reads, cuts, metric):
    """per (read, cut-off): for each strand the end positions j whose best alignment is within the cut-off, and its distance there"""
    w = _world()
    text, n = w["text"], len(w["text"])
    ta = np.frombuffer(text, dtype=np.uint8)
    todo = sorted({(r, c) for r, c in zip(reads, cuts) if (r, c, metric) not in w["truth"]})

    def one(rc):
        rd, cut = rc
        fw = clean(rd)
        out = []
        for p in (fw, synth.revcomp(fw)):
            if metric == "hamming":
                pa = np.frombuffer(p, dtype=np.uint8)
                m = len(pa)
                mism = np.zeros(n - m + 1, np.uint8)  # (reads are shorter than 256 characters)
                for c in range(m):
                    if pa[c] == ord("N"):
                        mism += 1
                    else:
                        mism += ta[c:n - m + 1 + c] != pa[c]
                b = np.flatnonzero(mism <= cut)
                out.append((b + m, mism[b].copy()))
            else:
                best = np.zeros(n + 1, np.uint8)
                gt.gt_semiglobal_ends(text, n, p, len(p), cut, best.ctypes.data_as(C.c_void_p), None)
                j = np.flatnonzero(best <= cut)
                out.append((j, best[j].copy()))
        return (rd, cut, metric), tuple(out)

    with ThreadPoolExecutor(8) as ex:  # (ctypes and numpy release the interpreter lock)
        for key, val in ex.map(one, todo):
            w["truth"][key] = val
    return w["truth"]


def norm_oracle(res):
    occ, sid, sb, cig, off, best, hits, _ = res
    return {"occ": occ, "seq_id": np.asarray(sid), "seq_begin": np.asarray(sb), "cigar": list(cig), "offs": np.asarray(off).astype(np.int64),
            "best": np.asarray(best), "hits": np.asarray(hits)}


def norm_lib(res):
    import columba_amd as ca
    occ, aln, ops, off, best, hits = res[:6]
    cig = [ca.cigar_string(ops[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["cigar_len"])]) for a in aln]
    return {"occ": occ, "seq_id": aln["seq_id"].copy(), "seq_begin": aln["seq_begin"].copy(), "cigar": cig,
            "offs": np.asarray(off).astype(np.int64), "best": np.asarray(best), "hits": np.asarray(hits)}


def check_best(gt, cfg, reads, R, label):
    """every assertion of the module docstring on one result; returns the counts it prints"""
    w = _world()
    spec, metric, x, min_identity = cfg
    text, starts = w["text"], w["starts"]
    inner = np.asarray(starts[1:-1], np.int64)
    cuts = [cutoff(spec, min_identity, len(r)) for r in reads]
    truth = fill_truth(gt, reads, cuts, metric)
    occ, offs = R["occ"], R["offs"]
    assert len(offs) == len(reads) + 1 and offs[0] == 0 and (np.diff(offs) >= 0).all() and offs[-1] == len(occ), "offsets"
    assert len(R["best"]) == len(R["hits"]) == len(reads)
    c = {"reads": len(reads), "near_end": 0, "zero_skipped": 0, "mapped": 0, "unmapped": 0, "records": 0, "loose": 0, "positions": 0, "chain": 0}
    cut_seen = set()
    for i, rd in enumerate(reads):
        fw = clean(rd)
        pats = (fw, synth.revcomp(fw))
        cut = cuts[i]
        lo, hi = int(offs[i]), int(offs[i + 1])
        best = int(R["best"][i])
        mapped = best != NONE
        assert mapped == (hi > lo), (label, i, best, lo, hi, "an unmapped read has an empty list, a mapped one has records")
        dist = occ["distance"][lo:hi].astype(np.int64)
        ends = occ["end"][lo:hi].astype(np.int64)
        top = min(best + x, cut) if mapped else None
        if mapped:
            assert best <= cut, (label, i, best, cut)
            assert ((dist >= best) & (dist <= top)).all(), (label, i, best, top, dist.tolist(), "distances in [best, top]")
            at_best = int((dist == best).sum())
            assert at_best >= 1, (label, i, best, dist.tolist(), "a record at the best distance")
            assert int(R["hits"][i]) >= at_best, (label, i, int(R["hits"][i]), at_best, "n_hits counts at least the records at best")
            keys = list(zip(dist.tolist(), occ["strand"][lo:hi].tolist(), R["seq_id"][lo:hi].tolist(), R["seq_begin"][lo:hi].tolist()))
            assert all(a < b for a, b in zip(keys, keys[1:])), (label, i, keys, "keys strictly increasing")
            for j in range(lo, hi):
                b, e, d, s = int(occ["begin"][j]), int(occ["end"][j]), int(occ["distance"][j]), int(occ["strand"][j])
                sid = int(R["seq_id"][j])
                assert s in (0, 1) and 0 <= sid < len(starts) - 1, (label, i, j)
                assert b == starts[sid] + int(R["seq_begin"][j]) and b < e <= starts[sid + 1], (label, i, j, b, e, sid, int(R["seq_begin"][j]))
                p, win = pats[s], text[b:e]
                ops = samcheck.cigar_ops(R["cigar"][j])
                qi, ti, edits = samcheck.cigar_walk(ops, p, win)
                assert qi == len(p) and ti == len(win), (label, i, j, R["cigar"][j], "the CIGAR consumes the read and text[begin, end)")
                true = gt.gt_edit_distance(p, len(p), win, len(win))
                if metric == "hamming":
                    assert e - b == len(p) and len(ops) == 1 and edits == d, (label, i, j, R["cigar"][j], edits, d)
                else:
                    assert edits == true <= d, (label, i, j, edits, true, d, "the CIGAR's edits are the window's edit distance")
                    c["loose"] += true < d
                c["records"] += 1
        tr = truth[(rd, cut, metric)]
        all_pos = np.concatenate([tr[0][0], tr[1][0]])
        all_d = np.concatenate([tr[0][1], tr[1][1]])
        dstar = int(all_d.min()) if len(all_d) else cut + 1
        reach = len(fw) + 2 * cut
        if len(all_pos) and len(inner) and (np.abs(all_pos[:, None] - inner[None, :]) <= reach).any():
            c["near_end"] += 1
            continue
        if x > 0 and cut < x:
            assert not mapped, (label, i, best, cut, "cut-off below x: the strata loop is never entered")
            c["unmapped"] += 1
            continue
        if x > 0 and dstar == 0:
            assert not mapped or 1 <= best <= cut, (label, i, best, cut)
            c["zero_skipped"] += 1
            continue
        if dstar > cut:
            assert not mapped, (label, i, best, dstar, cut, "no alignment within the cut-off, yet mapped")
            c["unmapped"] += 1
            continue
        assert mapped and best == dstar, (label, i, len(fw), cut, "best", None if not mapped else best, "true minimal distance", dstar)
        c["mapped"] += 1
        cut_seen.add(cut)
        for strand in (0, 1):
            pos, dj = tr[strand]
            sel = (dj >= best) & (dj <= top)
            pos, dj = pos[sel], dj[sel].astype(np.int64)
            for o in range(0, len(pos), 2048):
                pp, dd = pos[o:o + 2048, None], dj[o:o + 2048, None]
                ok = dist[None, :] <= dd
                gap = np.abs(ends[None, :] - pp)
                near = (ok & (gap <= 4 * top)).any(axis=1)
                far = (ok & (gap <= 8 * top)).any(axis=1)
                assert far.all(), (label, i, strand, int(pos[o + int(np.argmin(far))]), int(dj[o + int(np.argmin(far))]), best, top,
                                   list(zip(ends.tolist(), dist.tolist())), "an end position inside the reported strata is not covered")
                c["positions"] += len(near)
                c["chain"] += int((~near).sum())
    left_out = c["near_end"] + c["zero_skipped"]
    c["cutoffs"] = sorted(cut_seen)
    print(f"{label} {_ID(cfg)}: {c['reads']} reads, left out {left_out} ({100.0 * left_out / c['reads']:.1f} %: {c['near_end']} near an end, "
          f"{c['zero_skipped']} with d*=0), checked {c['mapped']} mapped / {c['unmapped']} unmapped, cut-offs {c['cutoffs']}, "
          f"{c['records']} records, loose {c['loose']}, {c['positions']} end positions, chain {c['chain']}")
    # conditions that keep the test from hiding failures
    assert left_out * 10 <= c["reads"], c
    assert c["mapped"] >= 60 and c["unmapped"] >= 20, c
    assert len(cut_seen) >= 3, c
    assert c["loose"] * 50 <= c["records"], c
    assert c["chain"] * 50 <= c["positions"], c
    if metric == "edit":
        assert c["near_end"] >= 1, c
    return c


def assert_oracle_parity(O, D, strand_tolerance=False):
    assert np.array_equal(O["best"], D["best"]), np.flatnonzero(O["best"] != D["best"])[:10]
    assert np.array_equal(O["hits"], D["hits"]), np.flatnonzero(O["hits"] != D["hits"])[:10]
    assert np.array_equal(O["offs"], D["offs"])
    for f in ("begin", "end", "distance"):
        assert np.array_equal(O["occ"][f], D["occ"][f]), f
    same = O["occ"]["strand"] == D["occ"]["strand"]
    if strand_tolerance:  # (the strand label of an occurrence found on both strands: unstable sort in the reference)
        assert (~same).sum() <= max(1, len(same) // 500)
    else:
        assert same.all()
    assert np.array_equal(O["seq_id"], D["seq_id"]) and np.array_equal(O["seq_begin"], D["seq_begin"])
    for j in range(len(same)):
        assert not same[j] or O["cigar"][j] == D["cigar"][j], (j, D["occ"][j], O["cigar"][j], D["cigar"][j])


def oracle_result(op, orc, cfg, key="fm", **kw):
    import schemes_py as sp
    w = _world()
    if (key, cfg) not in w["oracle"]:
        spec, metric, x, min_identity = cfg
        res = op.match_best(orc, op.OracleStrategy(sp.BY_NAME[spec], metric, "dynamic"), chunk(cfg), x=x, min_identity=min_identity,
                            max_supported=max_supported(spec), threads=8, **kw)
        w["oracle"][(key, cfg)] = norm_oracle(res)
    return w["oracle"][(key, cfg)]


# ------------------------------------------------------------------------------------------------ CPU: the oracle
@pytest.fixture(scope="module")
def cpu_world(oracle_built):
    import oracle_py as op
    from columba_amd import indexbuild as ib
    w = _world()
    ix = ib.build_index(w["text"], seq_starts=np.asarray(w["starts"], np.uint32), device="cpu")
    return {"op": op, "orc": op.OracleIndex(ix)}


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_oracle_best_mode_against_ground_truth(cpu_world, gt, cfg):
    """the reference's behaviour as the oracle restates it satisfies every rule: what the GPU paths are then held to"""
    R = oracle_result(cpu_world["op"], cpu_world["orc"], cfg, key="cpu")
    check_best(gt, cfg, chunk(cfg), R, "oracle")


def test_cutoff_below_x_leaves_the_read_unmapped(cpu_world):
    """the smallest input for the quirk of searchstrategy.cpp:676: an exact copy of the text, 40 characters at 96 % identity (cut-off 1),
    x = 2 — unmapped; with x = 1 it maps (at distance 1: stratum 0 is not examined)"""
    import schemes_py as sp
    op = cpu_world["op"]
    w = _world()
    rd = [w["genome"][61_000:61_040].tobytes()]
    st = op.OracleStrategy(sp.BY_NAME["minU"], "edit", "dynamic")
    two = norm_oracle(op.match_best(cpu_world["orc"], st, rd, x=2, min_identity=96, max_supported=max_supported("minU")))
    assert two["best"][0] == NONE and two["offs"][1] == 0
    one = norm_oracle(op.match_best(cpu_world["orc"], st, rd, x=1, min_identity=96, max_supported=max_supported("minU")))
    assert one["best"][0] in (NONE, 1)


# ------------------------------------------------------------------------------------------------ GPU: the HIP paths
@pytest.fixture(scope="module")
def gpu_world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import columba_amd as ca
    import oracle_py as op
    from columba_amd import indexbuild as ib, movebuild
    w = _world()
    starts = np.asarray(w["starts"], np.uint32)
    ix = ib.build_index(w["text"], seq_starts=starts, device="cuda")
    mv = movebuild.build_move(w["text"], device="cuda")
    mdev, morc = ca.MoveIndex(mv), op.OracleMoveIndex(mv)
    mdev.attach_text(w["text"], starts)
    morc.attach_text(w["text"], starts, word_size=8)
    return {"ca": ca, "op": op, "ix": ix, "dev": ca.Index(ix), "orc": op.OracleIndex(ix), "mdev": mdev, "morc": morc}


def _host(gw, cfg):
    w = _world()
    if ("host", cfg) not in w["runs"]:
        ca = gw["ca"]
        spec, metric, x, min_identity = cfg
        w["runs"][("host", cfg)] = ca.match_best(gw["dev"], ca.SearchStrategy(spec, metric, "dynamic"), chunk(cfg), x=x, min_identity=min_identity)
    return w["runs"][("host", cfg)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_host_bookkeeping_against_ground_truth(gpu_world, gt, cfg):
    """cmb_match_best: the strata as device batches, the bookkeeping on the host"""
    R = norm_lib(_host(gpu_world, cfg))
    check_best(gt, cfg, chunk(cfg), R, "match_best")
    assert_oracle_parity(oracle_result(gpu_world["op"], gpu_world["orc"], cfg), R)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_device_bookkeeping_against_ground_truth(gpu_world, gt, cfg):
    """cmb_match_best_device: reads with different k, maxED and cut-off in one stratum batch (runStratum, bestSelected in dev_best.hpp)"""
    from test_gpu_best_device import _assert_same
    ca = gpu_world["ca"]
    spec, metric, x, min_identity = cfg
    res = ca.match_best_device(gpu_world["dev"], ca.SearchStrategy(spec, metric, "dynamic"), chunk(cfg), x=x, min_identity=min_identity)
    R = norm_lib(res)
    check_best(gt, cfg, chunk(cfg), R, "match_best_device")
    assert_oracle_parity(oracle_result(gpu_world["op"], gpu_world["orc"], cfg), R)
    _assert_same(_host(gpu_world, cfg), res)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_device_bookkeeping_over_composite_batches(gpu_world, gt, cfg):
    """the same with every stratum split into three sub-batches"""
    from test_gpu_best_device import _assert_same, _env
    ca = gpu_world["ca"]
    spec, metric, x, min_identity = cfg
    with _env(CMB_SUBBATCHES="3"):
        res = ca.match_best_device(gpu_world["dev"], ca.SearchStrategy(spec, metric, "dynamic"), chunk(cfg), x=x, min_identity=min_identity)
    R = norm_lib(res)
    check_best(gt, cfg, chunk(cfg), R, "match_best_device/3")
    assert_oracle_parity(oracle_result(gpu_world["op"], gpu_world["orc"], cfg), R)
    _assert_same(_host(gpu_world, cfg), res)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", EDIT_CONFIGS, ids=_ID)
def test_bmove_best_mode_against_ground_truth(gpu_world, gt, cfg):
    """cmb_move_match_best: the strata as b-move batches, CIGARs and trimming from the text beside the index"""
    ca = gpu_world["ca"]
    spec, metric, x, min_identity = cfg
    res = ca.match_best(gpu_world["mdev"], ca.SearchStrategy(spec, metric, "dynamic"), chunk(cfg), x=x, min_identity=min_identity, kmer_size=8)
    R = norm_lib(res)
    check_best(gt, cfg, chunk(cfg), R, "b-move match_best")
    assert_oracle_parity(oracle_result(gpu_world["op"], gpu_world["morc"], cfg, key="move", word_size=8), R, strand_tolerance=True)
