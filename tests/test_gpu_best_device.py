"""BEST (+x strata) mode with the strata bookkeeping and the SAM text on the device (cmb_match_best_device, cmb_best_sam_device;
csrc/dev_best.hpp, k_sam_plan_best) against the host path of the same library (cmb_match_best: bit for bit) and the oracle's
restatement of matchApproxBestPlusX.

Run with `pytest -m gpu` on an MI355X.
"""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF

# (strategy, metric, x, minimal identity)
CONFIGS = [("columba", "edit", 0, 95), ("columba", "edit", 1, 96), ("minU", "edit", 2, 97), ("kuch1", "hamming", 0, 98),
           ("columba", "hamming", 1, 90), ("multiple_opt", "edit", 0, 97), ("columba", "edit", 0, 91), ("kuch1", "edit", 0, 50)]


@pytest.fixture(scope="module")
def best_world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    g, starts = synth.genome_rep(seed=11, n=2_000_000, scale=1.5)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    return {"genome": g, "ix": ix, "dev": ca.Index(ix), "orc": op.OracleIndex(ix), "op": op, "runs": {}}


def _reads(w, cfg):
    spec, metric, x, min_identity = cfg
    g = w["genome"]
    reads = synth.sample_reads(g, 600, 150, seed=800 + x, n_frac=0.01,
                               edit_choices=(0, 0, 1, 2, 3, 5, 6, 9) + ((11, 13) if min_identity < 95 else ()))
    starts = np.asarray(w["ix"].seq_starts, dtype=np.int64)
    for s in starts[1:-1][:10]:  # reads across sequence boundaries: trimmed or dropped (findSeqName)
        reads.append(g[int(s) - 75:int(s) + 75].tobytes())
        reads.append(g[int(s) - 3:int(s) + 147].tobytes())
        reads.append(g[int(s) - 147:int(s) + 3].tobytes())
    reads += [b"ACGT" * 37 + b"AC", b"N" * 150]
    if (metric, min_identity) == ("edit", 91):  # strata up to 13 errors: a smaller chunk (the oracle walks them on the CPU)
        reads = reads[:160] + reads[600:]
    if min_identity == 50:  # reads not longer than the number of parts: naive backtracking inside a stratum's batch
        reads = reads + [b"A", b"AC", b"ACG", b"ACGTA", b"GATTACA", b""]
    return reads


def _run(w, cfg):
    """host path and device path of one configuration, computed once for all tests"""
    if cfg not in w["runs"]:
        spec, metric, x, min_identity = cfg
        reads = _reads(w, cfg)
        st = ca.SearchStrategy(spec, metric, "dynamic")
        host = ca.match_best(w["dev"], st, reads, x=x, min_identity=min_identity)
        dev = ca.match_best_device(w["dev"], st, reads, x=x, min_identity=min_identity)
        w["runs"][cfg] = {"reads": reads, "host": host, "dev": dev}
    return w["runs"][cfg]


def _assert_same(host, dev):
    h_occ, h_aln, h_ops, h_off, h_best, h_hits, h_cnt = host
    d_occ, d_aln, d_ops, d_off, d_best, d_hits, d_cnt = dev[:7]
    assert np.array_equal(h_off, d_off)
    assert np.array_equal(h_best, d_best)
    assert np.array_equal(h_hits, d_hits)
    for f in ("begin", "end", "distance", "strand"):
        assert np.array_equal(h_occ[f], d_occ[f]), f
    for f in ("seq_id", "seq_begin", "spans", "cigar_off", "cigar_len"):
        assert np.array_equal(h_aln[f], d_aln[f]), f
    assert np.array_equal(h_ops, d_ops)
    assert h_cnt == d_cnt, {k: (h_cnt[k], d_cnt[k]) for k in h_cnt if h_cnt[k] != d_cnt[k]}


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_parity_with_host_path_and_oracle(best_world, cfg):
    """1: every array and every counter of cmb_match_best, bit for bit; and the oracle's matchApproxBestPlusX"""
    import schemes_py as sp
    w = best_world
    op = w["op"]
    spec, metric, x, min_identity = cfg
    r = _run(w, cfg)
    reads = r["reads"]
    _assert_same(r["host"], r["dev"])
    d_occ, d_aln, d_ops, d_off, d_best, d_hits, d_cnt, flagged = r["dev"]
    print(f"{cfg}: {len(reads)} reads, {len(d_occ)} records, mapped {(d_best != NONE).sum()}, host reads {int(flagged.sum())}")
    assert (d_best != NONE).sum() > 0 and (d_best == NONE).sum() > 0
    spec_tables = sp.BY_NAME[spec]
    max_sup = 0
    while (max_sup + 1) in spec_tables["schemes"]:
        max_sup += 1
    max_sup = min(max_sup, 13)  # (MAX_K)
    o_occ, o_sid, o_sb, o_cig, o_off, o_best, o_hits, o_cnt = op.match_best(
        w["orc"], op.OracleStrategy(spec_tables, metric, "dynamic"), reads, x=x, min_identity=min_identity, max_supported=max_sup, threads=8)
    assert np.array_equal(o_best, d_best)
    assert np.array_equal(o_hits, d_hits)
    assert np.array_equal(o_off, d_off)
    for f in ("begin", "end", "distance", "strand"):
        assert np.array_equal(o_occ[f], d_occ[f]), f
    assert np.array_equal(o_sid, d_aln["seq_id"]) and np.array_equal(o_sb, d_aln["seq_begin"])
    for j in range(len(d_occ)):
        a = d_aln[j]
        got = ca.cigar_string(d_ops[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["cigar_len"])])
        assert got == o_cig[j], (j, d_occ[j], got, o_cig[j])
    for n in ("NODE_COUNTER", "IN_TEXT_STARTED", "SEARCH_STARTED", "EXPANSIONS", "IMMEDIATE_SWITCH"):
        assert o_cnt[n] == d_cnt[n], (n, o_cnt[n], d_cnt[n])


def _cutoff(spec, min_identity, length=150):
    import schemes_py as sp
    max_sup = 0
    while (max_sup + 1) in sp.BY_NAME[spec]["schemes"]:
        max_sup += 1
    return min(13, max_sup, length * (100 - min_identity) // 100)


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[1], CONFIGS[2], CONFIGS[3], CONFIGS[4]], ids=lambda c: "-".join(map(str, c)))
def test_host_reads(best_world, cfg):
    """2: the reads whose bookkeeping went through the host have an occurrence over a sequence end; few under edit distance (the reads
    constructed across a sequence end and what the sampling puts there: at most 5 % of the chunk), none under Hamming distance"""
    w = best_world
    spec, metric, x, min_identity = cfg
    r = _run(w, cfg)
    reads, flagged = r["reads"], r["dev"][7]
    n_flagged = int(flagged.sum())
    print(f"{cfg}: {n_flagged} host reads of {len(reads)}")
    if metric == "hamming":
        assert n_flagged == 0
        return
    assert 1 <= n_flagged <= 0.05 * len(reads)
    k = _cutoff(spec, min_identity)
    b = ca.Batch(w["dev"], ca.SearchStrategy(spec, metric, "dynamic"), k, reads)
    assert ca.lib().cmb_batch_filter_per_strand(b.h, 1) == 0
    b.want_alignments()
    b.run()
    _, offs, _ = b.results()
    aln, _ = b.alignments()
    for i in np.flatnonzero(flagged):
        assert (aln["spans"][int(offs[i]):int(offs[i + 1])] != 0).any(), i
    b.close()


@pytest.mark.parametrize("cfg", [CONFIGS[1], CONFIGS[2]], ids=lambda c: "-".join(map(str, c)))
def test_both_continuations(best_world, cfg):
    """3: with x > 0 the final stratum min(best + x, cut-off) is a new search for some reads and one both strands have been
    through for others (findBestAlignments, searchstrategy.cpp:623-712): the chunk holds both kinds"""
    w = best_world
    spec, metric, x, min_identity = cfg
    r = _run(w, cfg)
    best = r["dev"][4]
    cut = _cutoff(spec, min_identity)
    strata, k = [], max(x, 1)
    while True:  # the strata a read walks until it finds its best distance
        strata.append(k)
        if k == cut:
            break
        k = min(k + x + (2 if k < 5 else 4), cut)
    fresh = stale = 0
    for b in best:
        if b == NONE:
            continue
        found_at = next(s for s in strata if s >= b)
        if min(int(b) + x, cut) > found_at:
            fresh += 1
        else:
            stale += 1
    print(f"{cfg}: strata {strata}, final stratum a new search for {fresh} reads, already searched for {stale}")
    assert fresh >= 10 and stale >= 10


def _wide_text(seed=78):
    """a 150 bp unit 1300 times exactly and 100 times with one substitution, 60 random characters between copies; then a second unit
    and, further on, its reverse complement"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    unit = acgt[rng.integers(0, 4, 150)]
    parts = []
    for c in range(1400):
        u = unit.copy()
        if c % 14 == 13:
            p = int(rng.integers(10, 140))
            u[p] = acgt[(int(np.where(acgt == u[p])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]
        parts.append(u)
        parts.append(acgt[rng.integers(0, 4, 60)])
    unit2 = acgt[rng.integers(0, 4, 150)]
    parts += [unit2, acgt[rng.integers(0, 4, 500)], np.frombuffer(synth.revcomp(unit2.tobytes()), np.uint8), acgt[rng.integers(0, 4, 350)]]
    return unit.tobytes(), unit2.tobytes(), np.concatenate(parts)


@pytest.mark.parametrize("x", [0, 1])
def test_wide_lists(oracle_built, x):
    """4: a read with more than 1200 occurrences in its best stratum, and one that matches on both strands there: the order is
    distance, forward before reverse complement, position"""
    unit, unit2, g = _wide_text()
    starts = [0, 210 * 476 + 180, 210 * 952 + 180, len(g)]  # (sequence ends between two copies: no occurrence runs over one)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    dev = ca.Index(ix)
    changed = bytearray(unit)
    changed[5] = ord("A") if changed[5] != ord("A") else ord("C")
    changed2 = bytearray(unit2)
    changed2[7] = ord("A") if changed2[7] != ord("A") else ord("C")
    reads = [unit, unit2, bytes(changed), bytes(changed2), synth.revcomp(unit)]
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    host = ca.match_best(dev, st, reads, x=x, min_identity=95)
    got = ca.match_best_device(dev, st, reads, x=x, min_identity=95)
    _assert_same(host, got)
    occ, aln, _, offs, best, hits, _, flagged = got
    assert flagged.sum() == 0  # (the lists below come from the device's bookkeeping)
    wide, both = (0, 1) if x == 0 else (2, 3)
    for i in range(len(reads)):
        lo, hi = int(offs[i]), int(offs[i + 1])
        key = list(zip(occ["distance"][lo:hi].tolist(), occ["strand"][lo:hi].tolist(), aln["seq_id"][lo:hi].tolist(),
                       aln["seq_begin"][lo:hi].tolist()))
        assert key == sorted(set(key)), i
        if best[i] != NONE:
            assert hits[i] >= (occ["distance"][lo:hi] == best[i]).sum() > 0
    lo, hi = int(offs[wide]), int(offs[wide + 1])
    at_best = int((occ["distance"][lo:hi] == best[wide]).sum())
    print(f"x={x}: best {best[wide]}, {at_best} records at it, n_hits {hits[wide]}, {hi - lo} records in all")
    assert best[wide] == x and at_best > 1200 and hits[wide] >= at_best
    lo, hi = int(offs[both]), int(offs[both + 1])
    at = occ["distance"][lo:hi] == best[both]
    assert best[both] == x and set(occ["strand"][lo:hi][at].tolist()) == {0, 1} and hits[both] >= 2


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_grid_edges(best_world, n):
    """5a: chunks around the sizes of a wavefront and of a block (the boundary reads first)"""
    w = best_world
    reads = _reads(w, CONFIGS[0])
    reads = (reads[590:] + reads[:590])[:n]
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    for x in (0, 1):
        host = ca.match_best(w["dev"], st, reads, x=x, min_identity=95)
        got = ca.match_best_device(w["dev"], st, reads, x=x, min_identity=95)
        _assert_same(host, got)
        assert len(got[3]) == n + 1 and len(got[7]) == n


def test_no_read_maps_and_composite_strata(best_world):
    """5b: a chunk of uniform random reads; 5c: strata that run as composite batches of three sub-batches"""
    w = best_world
    rng = np.random.default_rng(99)
    junk = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150)) for _ in range(70)]
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    host = ca.match_best(w["dev"], st, junk, x=0, min_identity=95)
    got = ca.match_best_device(w["dev"], st, junk, x=0, min_identity=95)
    _assert_same(host, got)
    assert len(got[0]) == 0 and (got[4] == NONE).all() and got[7].sum() == 0
    cfg = CONFIGS[1]
    r = _run(w, cfg)
    with _env(CMB_SUBBATCHES="3"):
        comp = ca.match_best_device(w["dev"], ca.SearchStrategy(cfg[0], cfg[1], "dynamic"), r["reads"], x=cfg[2], min_identity=cfg[3])
    _assert_same(r["host"], comp)
    assert np.array_equal(comp[7], r["dev"][7])


def _first_difference(a, b):
    n = min(len(a), len(b))
    i = next((j for j in range(n) if a[j] != b[j]), n)
    return f"lengths {len(a)} / {len(b)}, first difference at {i}: {a[max(0, i - 80):i + 40]!r} / {b[max(0, i - 80):i + 40]!r}"


def _sam_of_best(result, reads, ids, quals, names, unmapped, xa):
    """samOfBest (include/columba_amd_best.hpp) with the record builders of the C-ABI"""
    occ, aln, ops, offs, best, hits = result[:6]
    out = []
    for i, r in enumerate(reads):
        q = quals[i] if quals is not None else "*"
        sid, seq, rc, rq = ca.read_prepare(ids[i], r.decode(), q)
        lo, hi = int(offs[i]), int(offs[i + 1])
        if lo == hi:
            if unmapped:
                out.append(ca.sam_unmapped_se(sid, seq, q))
            continue
        hs = [(names[int(aln["seq_id"][j])], int(aln["seq_begin"][j]), int(occ["distance"][j]), bool(occ["strand"][j]),
               ops[int(aln["cigar_off"][j]):int(aln["cigar_off"][j]) + int(aln["cigar_len"][j])]) for j in range(lo, hi)]
        first_rc = bool(occ["strand"][lo])
        ps, pq = (rc, rq) if first_rc else (seq, q)
        if xa:
            out.append(ca.sam_se_xa(sid, hs, int(hits[i]), ps, pq))
        else:
            out.append(ca.sam_se(sid, hs[0], True, int(hits[i]), int(best[i]), ps, pq))
            out += [ca.sam_se(sid, h, False, int(hits[i]), int(best[i]), "*", "*") for h in hs[1:]]
    return "".join(out)


@pytest.mark.parametrize("cfg,xa,unmapped", [(CONFIGS[0], False, True), (CONFIGS[1], True, True), (CONFIGS[2], True, False),
                                             (CONFIGS[4], False, False)], ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_sam_text(best_world, cfg, xa, unmapped):
    """6: the text written on the device is, byte for byte, the one samOfBest assembles from cmb_match_best's result; the reads the
    host formatted are the flagged ones.  Quirks: no qualities, empty qualities beside an XA tag, lower-case reads, a one-character
    identifier"""
    w = best_world
    spec, metric, x, min_identity = cfg
    r = _run(w, cfg)
    reads = list(r["reads"])
    reads[3] = reads[3].lower()
    rng = np.random.default_rng(17)
    ids = [("@" if i % 2 else ">") + f"read{i}/1 some description" for i in range(len(reads))]
    ids[0], ids[1], ids[2] = "@", "@nospace", ">x"
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(rd))) for rd in reads]
    some_empty = [("" if i % 3 == 0 else q) for i, q in enumerate(quals)]
    names = [f"chr{j + 1}" for j in range(len(w["ix"].seq_starts) - 1)]
    st = ca.SearchStrategy(spec, metric, "dynamic")
    host = ca.match_best(w["dev"], st, reads, x=x, min_identity=min_identity)
    b = ca.BestDevice(w["dev"], st, reads, x=x, min_identity=min_identity)
    flagged = int(b.host_reads().sum())
    for q in (quals, some_empty, None):
        want = _sam_of_best(host, reads, ids, q, names, unmapped, xa)
        got, host_reads = b.sam_device(ids, q, names, unmapped=unmapped, xa=xa)
        print(f"{cfg} xa={xa} unmapped={unmapped}: {len(got)} bytes, host_reads={host_reads}")
        assert got == want, _first_difference(got, want)
        assert host_reads == flagged
        assert len(got) > 10_000
    # packed inputs give the same text
    packed, _ = b.sam_device(ca.pack_fields(ids), ca.pack_fields(quals), ca.pack_fields(names), unmapped=unmapped, xa=xa)
    assert packed == _sam_of_best(host, reads, ids, quals, names, unmapped, xa)
    _assert_same(host, b.results())  # (the lists are still what they were)
    b.close()


def test_cpp_adapter_paths_agree(best_world, tmp_path):
    """7: columba_align in its default mode on case 1's chunk: the host path (CMB_BEST_HOST=1), the default and the device path
    (CMB_BEST_DEVICE=1) write the same file"""
    w = best_world
    ca.build_library()
    exe = str(tmp_path / "columba_align")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_align.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "columba_amd"), "-lcolumba_amd", "-lz",
                           "-Wl,-rpath," + os.path.join(ROOT, "columba_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    ib.save_index(w["ix"], str(tmp_path / "idx"))
    reads = _reads(w, CONFIGS[0])
    rng = np.random.default_rng(4)
    with open(tmp_path / "reads.fq", "w") as f:
        for i, r in enumerate(reads):
            q = "".join(chr(33 + int(v)) for v in rng.integers(0, 41, len(r)))
            f.write(f"@read{i} len={len(r)}\n{r.decode()}\n+\n{q}\n")
    texts = {}
    for name, env in (("host", {"CMB_BEST_HOST": "1"}), ("default", {}), ("device", {"CMB_BEST_DEVICE": "1"})):
        e = {k: v for k, v in os.environ.items() if k not in ("CMB_BEST_HOST", "CMB_BEST_DEVICE")}
        e.update(env)
        os.makedirs(tmp_path / name)  # (the header names the command line: the same relative file name in a directory per path)
        subprocess.run([exe, "-r", str(tmp_path / "idx"), "-f", str(tmp_path / "reads.fq"), "-o", "out.sam", "-I", "95", "-b", "400"],
                       check=True, capture_output=True, text=True, env=e, cwd=str(tmp_path / name))
        texts[name] = (tmp_path / name / "out.sam").read_bytes()
    assert texts["host"] == texts["default"] == texts["device"]
    assert sum(1 for x in texts["device"].splitlines() if not x.startswith(b"@")) >= len(reads)
