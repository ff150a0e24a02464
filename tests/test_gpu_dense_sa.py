"""The dense suffix array that cmb_index_create and cmb_index_validate derive on the device (one word per row, so that a locate
is one load instead of the sparse walk).  CMB_SA_SPARSE=1 keeps the walk: the array must hold the suffix array, and the search must
return the same occurrences, counters (LF steps included) and SAM records on either layout.  Run with `pytest -m gpu`."""
import contextlib
import os

import numpy as np
import pytest
import torch

import columba_amd as ca
from columba_amd import indexbuild as ib, synth

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kv):
    """environment variables that cmb_index_create reads, set for the duration (None: unset)"""
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


def _index(ix, sparse=False, min_free_gb=None, **kw):
    with _env(CMB_SA_SPARSE="1" if sparse else None, CMB_TEST_SA_MIN_FREE_GB=min_free_gb):
        return ca.Index(ix, **kw)


@pytest.fixture(scope="module")
def genome():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g, starts = synth.genome_rep(seed=31, n=300_000, scale=2.0)
    full = ib.build_index(g.tobytes(), sparseness=1, seq_starts=starts, device="cuda")   # (every row sampled: the samples ARE the SA)
    return {"g": g, "starts": starts, "sa": full.sa_samples.astype(np.uint32), "ix4": ib.build_index(g.tobytes(), seq_starts=starts,
                                                                                                      device="cuda")}


@pytest.mark.parametrize("s", [1, 2, 4, 8, 32])
def test_dense_array_is_the_suffix_array(genome, s):
    ix = genome["ix4"] if s == 4 else ib.build_index(genome["g"].tobytes(), sparseness=s, seq_starts=genome["starts"], device="cuda")
    sa = genome["sa"]
    n = ix.n
    assert sa.shape[0] == n
    dense, sparse = _index(ix), _index(ix, sparse=True)
    try:
        assert dense.device_bytes() - sparse.device_bytes() == 4 * n
        rows = np.arange(n, dtype=np.uint32)
        pos_d, lf_d = dense.locate(rows)
        pos_s, lf_s = sparse.locate(rows)
        assert np.array_equal(pos_s, sa) and np.array_equal(pos_d, sa)
        # the walk takes SA[row] % s steps on every row: the LF counter of the dense path is that sum
        assert lf_d == lf_s == int((sa.astype(np.int64) % s).sum())
        assert (lf_d > 0) == (s > 1)
        rng = np.random.default_rng(s)
        some = rng.integers(0, n, 5000).astype(np.uint32)   # (repeated and unordered rows)
        p1, l1 = dense.locate(some)
        p2, l2 = sparse.locate(some)
        assert np.array_equal(p1, sa[some]) and np.array_equal(p2, sa[some]) and l1 == l2
    finally:
        dense.close()
        sparse.close()


def _run(index, names, spec, metric, k, reads):
    b = ca.Batch(index, ca.SearchStrategy(spec, metric, "dynamic"), k, reads)
    try:
        b.want_alignments()
        b.run()
        occ, offs, cnt = b.results()
        aln, ops = b.alignments()
        sam = b.sam([f"r{i}" for i in range(len(reads))], ["I" * len(r) for r in reads], names)
        return occ, offs, cnt, aln, ops, sam
    finally:
        b.close()


@pytest.mark.parametrize("spec,metric,k", [
    ("multiple_opt", "edit", 4),   # the headline's strategy: k_verify<true> + k_verify_stage, k_fmocc
    ("columba", "edit", 0),        # exact candidates only
    ("columba", "hamming", 3),
    ("columba", "edit", 9),        # k >= 8: k_verify_wide
])
def test_search_equal_on_dense_and_sparse_layout(genome, spec, metric, k):
    g = genome["g"]
    edits = tuple(sorted({0, k // 2, k, k + 1}))
    reads = synth.sample_reads(g, 1500, 150, seed=50 + k, n_frac=0.01, edit_choices=edits)
    reads += [g[0:150].tobytes(), g[-151:-1].tobytes()]
    dense, sparse = _index(genome["ix4"]), _index(genome["ix4"], sparse=True)
    try:
        assert dense.device_bytes() > sparse.device_bytes()
        names = genome["ix4"].seq_names
        d, s = _run(dense, names, spec, metric, k, reads), _run(sparse, names, spec, metric, k, reads)
    finally:
        dense.close()
        sparse.close()
    occ, offs, cnt, aln, ops, sam = d
    assert len(occ) > 500 and cnt["LOCATED_ROWS"] > 500
    assert cnt["LF_STEPS"] > 0
    assert np.array_equal(occ, s[0]) and np.array_equal(offs, s[1])
    assert cnt == s[2]
    assert np.array_equal(aln, s[3]) and np.array_equal(ops, s[4])
    assert sam == s[5] and sam.count("\n") >= len(reads)


def test_not_enough_memory_keeps_the_sparse_walk(genome):
    ix, sa = genome["ix4"], genome["sa"]
    sparse = _index(ix, sparse=True)
    tight = _index(ix, min_free_gb="1e9")   # (more free memory demanded after the array than any device has)
    roomy = _index(ix, min_free_gb="0")
    try:
        assert tight.device_bytes() == sparse.device_bytes()
        assert roomy.device_bytes() == sparse.device_bytes() + 4 * ix.n
        rows = np.arange(ix.n, dtype=np.uint32)
        pos, lf = tight.locate(rows)
        assert np.array_equal(pos, sa) and lf == int((sa.astype(np.int64) % 4).sum())
        reads = synth.sample_reads(genome["g"], 500, 150, seed=77)
        st = ca.SearchStrategy("multiple_opt", "edit", "dynamic")
        a, b = ca.match_batch(tight, st, 4, reads), ca.match_batch(roomy, st, 4, reads)
        assert len(a[0]) > 300 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    finally:
        for x in (sparse, tight, roomy):
            x.close()


def test_replica_builds_its_own_dense_array_when_validated(genome):
    """create_empty + device_arrays + validate (what columba_amd.dist.broadcast_device_index does across ranks), on one GPU: the dense
    array is not one of the replicated arrays; the replica derives it in validate, and works on the sparse walk until then"""
    ix, sa = genome["ix4"], genome["sa"]
    orig = _index(ix)
    sparse = _index(ix, sparse=True)
    rep = ca.Index.empty_like(orig.layout(), orig.seq_starts(), device=0)
    try:
        lay = orig.layout()
        assert sum(int(b) for b in lay.bytes) == sparse.device_bytes() == rep.device_bytes()
        for src, dst in zip(orig.device_tensors(), rep.device_tensors()):
            assert (src is None) == (dst is None)
            if src is not None:
                dst.copy_(src)
        torch.cuda.synchronize()
        reads = synth.sample_reads(genome["g"], 800, 150, seed=91, n_frac=0.01)
        st = ca.SearchStrategy("multiple_opt", "edit", "dynamic")
        want = ca.match_batch(orig, st, 4, reads)
        rows = np.arange(ix.n, dtype=np.uint32)
        for validated in (False, True):
            if validated:
                rep.validate()
            assert rep.device_bytes() == (orig if validated else sparse).device_bytes()
            pos, lf = rep.locate(rows)
            assert np.array_equal(pos, sa) and lf == int((sa.astype(np.int64) % 4).sum())
            got = ca.match_batch(rep, st, 4, reads)
            assert len(got[0]) > 300 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        rep.validate()   # (again: the array is rebuilt, not added twice)
        assert rep.device_bytes() == orig.device_bytes()
    finally:
        for x in (rep, sparse, orig):
            x.close()
