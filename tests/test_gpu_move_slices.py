"""The b-move batch across its slices and halves, and its refusals.

moveBatchRunOne cuts a chunk into equal slices of at most 2^18 / 2^19 / 2^20 reads (k >= 5 / k >= 3 / below), rebases
every slice's offsets onto the records before it and copies its records out on a second stream while the next slice is
matched; cmb_move_batch_create matches a chunk of 2^19 reads and more as two concurrent halves when most of the HBM is free.
The other b-move tests never put more than a few thousand reads in a batch, so they only ever ran one slice.

* forced slices (CMB_MOVE_SLICE) on `sworld`: occurrences, offsets, counters, alignments and BEST-mode filtering per strand
  are byte-identical to the same batch as one slice (k >= 1: a batch at k = 0 is never cut);
* natural boundaries on a pan-genome of 16 x 4 Mbp at 0.5 % SNPs: the edge reads (first, last, both sides of every slice or
  half boundary the batch may take) equal the same reads in a small batch, and those agree with `oracle/`;
* refusals: 2^23 reads per batch, 2^31 text positions per slice (at k >= 1 and on the k = 0 path), before any work of that
  size, with the index usable afterwards.

Also here: build_move_resident on the device gives the host builder's parts for `sworld`'s text and for the pan-genome
(there with the PLCP of plcp_gpu).  The oracle/ index of the low-complexity text takes the parts of build_move_resident: its
PLCP is not checked by another builder (plcp_gpu compares one character per round, too slow on a 3 Mbp run).
"""
import resource
import time

import numpy as np
import pytest

from columba_amd import movebuild, synth
from test_gpu_move_search import _compare, _reads, sworld  # noqa: F401  (sworld: the fixture)

pytestmark = pytest.mark.gpu

EDGE = 384
N_ORACLE = 48   # edge reads per boundary also run through oracle/


def _expand_plcp(mv):
    mv.plcp = movebuild.plcp_from_runs(mv.plcp_pos, mv.plcp_sum, mv.n)   # (oracle/ takes the PLCP by position)
    return mv


@pytest.fixture(scope="module")
def mid(oracle_built):
    import torch
    import columba_amd as ca
    import oracle_py as op
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    t_module = time.time()
    g = movebuild.pangenome(4_000_000, 16, 0.005, seed=21)
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    mv = _expand_plcp(movebuild.build_move_resident(g.tobytes(), device="cuda"))
    torch.cuda.synchronize()
    print(f"\n[move slices] {len(g) + 1} characters, {mv.runs_fwd} runs: built in {time.time() - t0:.1f} s, peak "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB device, {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GiB host")
    text = torch.from_numpy(g).cuda()
    reads = {100: synth.sample_reads_fast(text, (1 << 23) - 1, 100, seed=5, device="cuda", edit_choices=(0, 1, 2, 3, 4))[0],
             250: synth.sample_reads_fast(text, (1 << 18) + 1, 250, seed=6, device="cuda", edit_choices=(0, 1, 2, 4, 6, 7))[0]}
    del text
    torch.cuda.empty_cache()
    w = {"g": g, "mv": mv, "dev": ca.MoveIndex(mv), "orc": op.OracleMoveIndex(mv), "ca": ca, "op": op, "reads": reads}
    yield w
    w["dev"].close()
    print(f"\n[move slices] pan-genome tests: {time.time() - t_module:.1f} s with the fixture")


def test_resident_build_on_the_device_is_the_host_build(sworld):
    mv = sworld["mv"]
    d = movebuild.build_move_resident(sworld["text"], device="cuda", n_random_rows=4096)
    for f in ("lfbp_fwd", "lfbp_rev", "smpf", "smpl", "rev_smpf", "rev_smpl", "pred_first", "first_to_run", "pred_last", "last_to_run",
              "text"):
        assert np.array_equal(getattr(mv, f), getattr(d, f)), f
    pos, sm = mv.plcp_run_form()
    assert np.array_equal(pos, d.plcp_pos) and np.array_equal(sm, d.plcp_sum)
    assert np.array_equal(mv.sa[d.sa_rows.astype(np.int64)], d.sa_at_rows)


def test_resident_build_is_the_host_build_on_the_pan_genome(mid):
    """the parts the pan-genome tests (and their oracle/ index) use, from the host builder with plcp_gpu's PLCP"""
    h = movebuild.build_move(mid["g"].tobytes(), device="cuda", with_locate=False)
    h.plcp = movebuild.plcp_gpu(h)
    d = mid["mv"]
    for f in ("lfbp_fwd", "lfbp_rev", "smpf", "smpl", "rev_smpf", "rev_smpl", "pred_first", "first_to_run", "pred_last", "last_to_run",
              "text", "plcp"):
        assert np.array_equal(getattr(h, f), getattr(d, f)), f
    assert np.array_equal(h.sa[d.sa_rows.astype(np.int64)], d.sa_at_rows)


# ------------------------------------------------------------------------------------------------ forced slices
def _run_move(w, spec, k, reads=None, packed=None, aln=False, per_strand=False, metric="edit", kmer_size=8):
    ca = w["ca"]
    b = ca.MoveBatch(w["dev"], ca.SearchStrategy(spec, metric, "dynamic"), k, reads=reads, packed=packed, kmer_size=kmer_size)
    try:
        if aln:
            b.want_alignments()
        if per_strand:
            b.filter_per_strand()
        b.run()
        occ, offs, cnt = b.results()
        out = (occ, offs, cnt) + (b.alignments() if aln else ())
        return out
    finally:
        b.close()


def _same_runs(a, b, what):
    assert np.array_equal(a[1], b[1]), (what, "offsets")
    assert a[0].tobytes() == b[0].tobytes(), (what, "occurrences")
    assert a[2] == b[2], (what, {n: (a[2][n], b[2][n]) for n in a[2] if a[2][n] != b[2][n]})
    for x, y, name in zip(a[3:], b[3:], ("alignment records", "CIGAR pool")):
        assert x.tobytes() == y.tobytes(), (what, name)


SLICE_CASES = [("multiple_opt", "edit", 6, 250, True, False), ("multiple_opt", "edit", 2, 100, True, False),
               ("columba", "edit", 4, 150, True, True), ("kuch1", "hamming", 3, 150, True, False),
               ("columba", "edit", 9, 150, True, False)]


@pytest.mark.parametrize("spec,metric,k,length,aln,per_strand", SLICE_CASES)
def test_forced_slices_are_byte_identical(sworld, monkeypatch, spec, metric, k, length, aln, per_strand):
    g = sworld["g"]
    sworld["dev"].attach_text(sworld["text"], np.array([0, 250_000, 640_000, len(g)], dtype=np.uint64))
    reads = _reads(g, k, 300, length, seed=900 + k + length)
    monkeypatch.delenv("CMB_MOVE_SLICE", raising=False)
    monkeypatch.setenv("CMB_MOVE_SUBBATCHES", "1")
    one = _run_move(sworld, spec, k, reads=reads, aln=aln, per_strand=per_strand, metric=metric)
    assert len(one[0]) > len(reads) // 2
    for sl in ("1", "7", "1000"):
        monkeypatch.setenv("CMB_MOVE_SLICE", sl)
        _same_runs(one, _run_move(sworld, spec, k, reads=reads, aln=aln, per_strand=per_strand, metric=metric), f"CMB_MOVE_SLICE={sl}")
    monkeypatch.setenv("CMB_MOVE_SUBBATCHES", "3")
    monkeypatch.setenv("CMB_MOVE_SLICE", "5")
    _same_runs(one, _run_move(sworld, spec, k, reads=reads, aln=aln, per_strand=per_strand, metric=metric), "3 halves of slices of 5")


# ------------------------------------------------------------------------------------------------ natural boundaries
def _slice_bounds(n, k):
    """moveBatchRunOne's slice starts of a batch of n reads (and its end)"""
    sl = (1 << 18) if k >= 5 else (1 << 19) if k >= 3 else (1 << 20)
    if n > sl:
        sl = -(-n // -(-n // sl))
    return list(range(0, n, sl)) + [n]


def _possible_bounds(n, k, halves):
    b = set(_slice_bounds(n, k))
    if halves:   # (cmb_move_batch_create's halves, each cut into its own slices)
        for j in range(2):
            lo, hi = n * j // 2, n * (j + 1) // 2
            b |= {lo + x for x in _slice_bounds(hi - lo, k)}
    return sorted(b)


def _segments(n, bounds):
    segs = sorted((max(a, 0), min(b, n)) for a, b in [(0, EDGE), (n - EDGE, n)] + [(x - EDGE, x + EDGE) for x in bounds[1:-1]])
    out = [list(segs[0])]
    for a, b in segs[1:]:
        if a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def _check_edges(w, spec, k, buf, length, n, occ, off, bounds):
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    oracle_reads = []
    for a, b in _segments(n, bounds):
        o2, f2, _ = _run_move(w, spec, k, packed=(buf[a * length:b * length], offs[:b - a + 1]), kmer_size=10)
        got = off[a:b + 1] - off[a]
        if not np.array_equal(f2, got):
            i = int(np.flatnonzero(f2 != got)[0]) - 1
            raise AssertionError(("read", a + i, "alone:", o2[int(f2[i]):int(f2[i + 1])].tolist(),
                                  "in the batch:", occ[int(off[a + i]):int(off[a + i + 1])].tolist()))
        part = occ[int(off[a]):int(off[b])]
        assert part.tobytes() == o2.tobytes(), ("reads", a, b)
        sel = np.unique(np.linspace(a, b - 1, N_ORACLE).astype(np.int64))
        oracle_reads += [buf[i * length:(i + 1) * length].tobytes() for i in sel]
    _compare(w, spec, "dynamic", k, oracle_reads, kmer_size=10)


BOUNDARY_CASES = [("250bp_k6_2^18+1", "multiple_opt", 6, 250, (1 << 18) + 1, "1"),
                  ("k2_2^20+1", "multiple_opt", 2, 100, (1 << 20) + 1, "1"),
                  ("k4_2^19", "multiple_opt", 4, 100, 1 << 19, None),
                  ("k1_2^23-1", "kuch1", 1, 100, (1 << 23) - 1, None)]


@pytest.mark.parametrize("name,spec,k,length,n,subs", BOUNDARY_CASES, ids=[c[0] for c in BOUNDARY_CASES])
def test_batch_across_natural_slice_and_half_boundaries(mid, monkeypatch, name, spec, k, length, n, subs):
    monkeypatch.delenv("CMB_MOVE_SLICE", raising=False)
    if subs:
        monkeypatch.setenv("CMB_MOVE_SUBBATCHES", subs)
    else:   # (the automatic halves: taken only with 160 GB of HBM free, so either path must pass)
        monkeypatch.delenv("CMB_MOVE_SUBBATCHES", raising=False)
    import torch
    buf = mid["reads"][length][:n * length]
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    free = torch.cuda.mem_get_info()[0]
    t0 = time.time()
    occ, off, cnt = _run_move(mid, spec, k, packed=(buf, offs), kmer_size=10)
    halves = subs is None and n >= 1 << 19 and free >= 160 << 30   # (cmb_move_batch_create's test, just before)
    print(f"\n[move slices] {name}: {len(occ)} occurrences in {time.time() - t0:.1f} s, {free / 2 ** 30:.0f} GiB HBM free: "
          f"{'two halves' if halves else 'one batch'}, slices {_slice_bounds(n // 2 if halves else n, k)[:-1]}")
    assert off.shape[0] == n + 1 and int(off[-1]) == len(occ) and np.all(off[1:] >= off[:-1])
    assert len(occ) > n and int(occ["end"].max()) < mid["mv"].n and int(occ["distance"].max()) <= k
    bounds = _possible_bounds(n, k, halves=subs is None and n >= 1 << 19)
    assert len(bounds) >= 3, bounds
    monkeypatch.setenv("CMB_MOVE_SUBBATCHES", "1")
    _check_edges(mid, spec, k, buf, length, n, occ, off, bounds)


# ------------------------------------------------------------------------------------------------ refusals
def test_batch_of_2_23_reads_is_refused(mid):
    ca = mid["ca"]
    n = 1 << 23
    buf = np.concatenate([mid["reads"][100], mid["reads"][100][:100]])
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(100)
    with pytest.raises(ca.CmbError) as e:
        ca.MoveBatch(mid["dev"], ca.SearchStrategy("kuch1", "edit", "dynamic"), 1, packed=(buf, offs))
    assert e.value.code == ca.CMB_ERR_UNSUPPORTED and "2^23" in str(e.value)


@pytest.fixture(scope="module")
def lowc(oracle_built):
    """a pan-genome with 3 Mbp of one character in the middle: a read from there has ~3 M occurrences per range"""
    import columba_amd as ca
    import oracle_py as op
    rng = np.random.default_rng(8)
    g = np.concatenate([movebuild.pangenome(200_000, 8, 0.005, seed=8), np.full(3_000_000, ord("A"), np.uint8),
                        np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100_000)]])
    mv = _expand_plcp(movebuild.build_move_resident(g.tobytes(), device="cuda"))
    w = {"g": g, "mv": mv, "dev": ca.MoveIndex(mv), "orc": op.OracleMoveIndex(mv), "ca": ca, "op": op}
    yield w
    w["dev"].close()


@pytest.mark.parametrize("spec,k", [("kuch1", 0), ("kuch1", 1), ("kuch1", 3)])
def test_batch_past_2_31_text_positions_is_refused(lowc, monkeypatch, spec, k):
    ca = lowc["ca"]
    monkeypatch.setenv("CMB_MOVE_SUBBATCHES", "1")
    monkeypatch.delenv("CMB_MOVE_SLICE", raising=False)
    occ, offs, _ = lowc["dev"].match_exact([b"A" * 100])
    assert len(occ) >= 2_900_000, len(occ)   # (one read from the stretch: ~3 M exact occurrences)
    reads = [b"A" * 100] * 1500 + [b"A" * 60 + b"C" + b"A" * 39] * 500   # (together ~4.5 G text positions and more)
    try:
        got = _run_move(lowc, spec, k, reads=reads, kmer_size=10)
    except ca.CmbError as e:
        assert e.code == ca.CMB_ERR_UNSUPPORTED and "2^31" in str(e), str(e)
    else:
        raise AssertionError(("accepted", len(got[0]), got[1][:4].tolist(), got[2]))
    # the index answers normally afterwards
    g = lowc["g"][:1_600_000]
    _compare(lowc, spec, "dynamic", max(k, 1), _reads(g, max(k, 1), 200, 100, seed=60 + k), kmer_size=10)
