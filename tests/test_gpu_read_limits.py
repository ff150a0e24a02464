"""Read numbers at the sub-batch edges.

The filter key holds the group of an occurrence — the read, or read x strand when every strand is filtered by itself
(BEST mode) — in 24 bits (22 in the wide layout from 8 errors), the verification keys hold read x strand.  A batch is
cut into sub-batches of at most 2^23 reads (2^20 from 8 errors, 2^11 from 11) so that these fields never overflow; the
other GPU tests never put more than 120 000 reads in a batch.  Every batch here sits exactly at such a limit, or one
read past it, and is compared, at its edges (its first and last reads, the reads on both sides of every sub-batch
boundary), with the same reads run alone in a small batch, and those with `oracle/`.

A sub-batch made larger than its keys hold (CMB_SUBBATCH_SPLIT) is refused before any work: at creation when the read
does not fit, by cmb_batch_filter_per_strand when read x strand does not.
"""
import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

EDGE = 4096
SPLIT_ONE = (1 << 24) - 1   # one sub-batch of 2^24 - 1 reads (and one of a single read)


@pytest.fixture(scope="module")
def small(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    g, starts = synth.genome_human_like(16_000_000, seed=31, device="cuda")
    ix = ib.build_index(g, seq_starts=starts, device="cuda", with_bwt=True)
    del g
    text = torch.from_numpy(ix.text[:-1]).cuda()
    reads = {100: synth.sample_reads_fast(text, 1 << 24, 100, seed=7, device="cuda")[0],
             150: synth.sample_reads_fast(text, (1 << 20) + 1, 150, seed=8, device="cuda", edit_choices=(0, 1, 2, 4, 6, 8))[0],
             151: synth.sample_reads_fast(text, (1 << 11) + 1, 150, seed=9, device="cuda", edit_choices=(0, 2, 5, 9, 11))[0]}
    del text
    torch.cuda.empty_cache()
    w = {"ix": ix, "dev": ca.Index(ix), "orc": op.OracleIndex(ix), "op": op, "reads": reads}
    yield w
    w["dev"].close()
    del w["orc"]


def _packed(w, key, n):
    length = 150 if key != 100 else 100
    buf = w["reads"][key][:n * length]
    return buf, np.arange(n + 1, dtype=np.uint64) * np.uint64(length), length


def _bounds(n, S, wts=None):
    """cmb_batch_create's sub-batch bounds (the same double arithmetic)"""
    wts = wts or [1.0] * S
    wsum, acc, b = float(sum(wts)), 0.0, [0]
    for j in range(S):
        acc += wts[j]
        b.append(n if j + 1 == S else int(float(n) * (acc / wsum)))
    return b


def _edges(n, bounds):
    segs = [(0, EDGE), (n - EDGE, n)] + [(x - EDGE, x + EDGE) for x in bounds[1:-1]]
    segs = sorted((max(a, 0), min(b, n)) for a, b in segs)
    out = [list(segs[0])]
    for a, b in segs[1:]:
        if a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(s) for s in out]


def _run(w, st, k, buf, offs, per_strand):
    b = ca.Batch(w["dev"], st, k, packed=(buf, offs))
    try:
        if per_strand:
            ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
        b.run()
        return b.results()
    finally:
        b.close()


def _check_offsets(occ, offs, n, k, text_n):
    assert offs.shape[0] == n + 1 and int(offs[0]) == 0 and int(offs[-1]) == len(occ)
    assert np.all(offs[1:] >= offs[:-1])
    assert np.all(occ["begin"] < occ["end"]) and int(occ["end"].max()) <= text_n
    assert int(occ["distance"].max()) <= k and int(occ["strand"].max()) <= 1


# (name, strategy, metric, k, reads, read set, CMB_SUBBATCHES, CMB_SUBBATCH_SPLIT, per strand, reads through oracle/ per edge)
CASES = [
    ("k4_2^23", "multiple_opt", "edit", 4, 1 << 23, 100, 1, None, False, EDGE),
    ("k4_2^23+1", "multiple_opt", "edit", 4, (1 << 23) + 1, 100, 1, None, False, EDGE),
    ("best_k4_2^23", "multiple_opt", "edit", 4, 1 << 23, 100, 1, None, True, 0),
    ("best_k4_2^23+1", "multiple_opt", "edit", 4, (1 << 23) + 1, 100, 1, None, True, 0),
    ("hamming_k2_2^23", "kuch1", "hamming", 2, 1 << 23, 100, 1, None, False, EDGE),
    ("k8_2^20", "columba", "edit", 8, 1 << 20, 150, 1, None, False, 512),
    ("k8_2^20+1", "columba", "edit", 8, (1 << 20) + 1, 150, 1, None, False, 512),
    ("k11_2^11", "columba", "edit", 11, 1 << 11, 151, 1, None, False, 64),
    ("k11_2^11+1", "columba", "edit", 11, (1 << 11) + 1, 151, 1, None, False, 64),
    ("split_2^24-1", "multiple_opt", "edit", 4, 1 << 24, 100, 2, [float(SPLIT_ONE), 1.0], False, EDGE),
]


@pytest.mark.parametrize("name,spec,metric,k,n,key,subs,split,per_strand,n_oracle", CASES, ids=[c[0] for c in CASES])
def test_batch_at_a_sub_batch_edge(small, monkeypatch, name, spec, metric, k, n, key, subs, split, per_strand, n_oracle):
    monkeypatch.setenv("CMB_SUBBATCHES", str(subs))
    if split:
        monkeypatch.setenv("CMB_SUBBATCH_SPLIT", ",".join(str(int(x)) for x in split))
    maxsub = 1 << 23 if metric != "edit" or k <= 7 else (1 << 20 if k <= 10 else 1 << 11)
    S = max(subs, -(-n // maxsub))
    bounds = _bounds(n, S, split)
    assert max(b - a for a, b in zip(bounds, bounds[1:])) <= (SPLIT_ONE if split else maxsub)
    if split:
        assert bounds[1] == SPLIT_ONE
    buf, offs, length = _packed(small, key, n)
    st = ca.SearchStrategy(spec, metric, "dynamic")
    occ, off, _ = _run(small, st, k, buf, offs, per_strand)
    _check_offsets(occ, off, n, k, small["ix"].n)
    assert len(occ) > n // 4
    monkeypatch.delenv("CMB_SUBBATCHES")
    monkeypatch.delenv("CMB_SUBBATCH_SPLIT", raising=False)
    oracle_reads = []
    for a, b in _edges(n, bounds):
        o2, f2, _ = _run(small, st, k, buf[a * length:b * length], offs[:b - a + 1], per_strand)
        got = off[a:b + 1] - off[a]
        if not np.array_equal(f2, got):
            i = int(np.flatnonzero(f2 != got)[0]) - 1
            raise AssertionError((name, "read", a + i, "alone:", o2[int(f2[i]):int(f2[i + 1])].tolist(),
                                  "in the batch:", occ[int(off[a + i]):int(off[a + i + 1])].tolist()))
        part = occ[int(off[a]):int(off[b])]
        for f in ("begin", "end", "distance", "strand"):
            bad = np.flatnonzero(o2[f] != part[f])
            if bad.size:
                j = int(bad[0])
                i = int(np.searchsorted(f2, j, "right")) - 1
                raise AssertionError((name, "read", a + i, "(begin, end, distance, strand) alone:", o2[j].tolist(),
                                      "in the batch:", part[j].tolist()))
        if n_oracle:
            sel = np.unique(np.linspace(a, b - 1, min(n_oracle, b - a)).astype(np.int64))
            oracle_reads += [buf[i * length:(i + 1) * length].tobytes() for i in sel]
    if oracle_reads:
        _compare({"op": small["op"], "orc": small["orc"], "dev": small["dev"]}, spec, metric, "dynamic", k, oracle_reads,
                 counters=True)


def test_oversized_sub_batches_are_refused_before_any_work(small, monkeypatch):
    """CMB_SUBBATCH_SPLIT can make one sub-batch of 2^24 - 1 reads.  In BEST mode its group is read x strand, 25 bits
    where layout 0 holds 24: cmb_batch_filter_per_strand refuses it (before, the batch failed at its filter, after the
    search).  From 8 errors (22 group bits) a sub-batch of 2^22 reads is refused at creation.  Sub-batches at the limit
    are accepted."""
    st = ca.SearchStrategy("multiple_opt", "edit", "dynamic")
    monkeypatch.setenv("CMB_SUBBATCHES", "2")
    monkeypatch.setenv("CMB_SUBBATCH_SPLIT", f"{SPLIT_ONE},1")
    buf, offs, _ = _packed(small, 100, 1 << 24)
    b = ca.Batch(small["dev"], st, 4, packed=(buf, offs))
    try:
        with pytest.raises(ca.CmbError) as e:
            ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
        assert e.value.code == ca.CMB_ERR_UNSUPPORTED and "read x strand" in str(e.value)
    finally:
        b.close()
    # at the limit: 2^23 reads in one sub-batch, read x strand up to 2^24 - 1
    monkeypatch.setenv("CMB_SUBBATCHES", "1")
    monkeypatch.delenv("CMB_SUBBATCH_SPLIT")
    buf, offs, _ = _packed(small, 100, 1 << 23)
    b = ca.Batch(small["dev"], st, 4, packed=(buf, offs))
    ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
    b.close()
    # wide keys: a sub-batch of 2^22 reads at 8 errors (five sub-batches of at most 2^20 reads, the first one made larger)
    n = (1 << 22) + 8
    wts = [float(1 << 22), 1.0, 1.0, 1.0, 1.0]
    assert -(-n // (1 << 20)) == len(wts) and _bounds(n, len(wts), wts)[1] >= 1 << 22
    monkeypatch.setenv("CMB_SUBBATCHES", str(len(wts)))
    monkeypatch.setenv("CMB_SUBBATCH_SPLIT", ",".join(str(int(x)) for x in wts))
    buf, offs, _ = _packed(small, 100, n)
    with pytest.raises(ca.CmbError) as e:
        ca.Batch(small["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), 8, packed=(buf, offs))
    assert e.value.code == ca.CMB_ERR_UNSUPPORTED and "2^22" in str(e.value)
