"""bench.py builds its reference's index with suffix arrays of its own (prefix doubling that re-sorts only the open groups);
the arrays must be those of columba_amd.indexbuild.build_index, which every other caller uses."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from columba_amd import indexbuild as ib, synth  # noqa: E402


def _texts():
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    g, _ = synth.genome_human_like(300_000, seed=7)
    yield "human_like", g
    yield "homopolymer", torch.full((3000,), ord("A"), dtype=torch.uint8)
    unit = acgt[rng.integers(0, 4, 7)]
    yield "tandem", torch.from_numpy(np.concatenate([acgt[rng.integers(0, 4, 500)], np.tile(unit, 400), acgt[rng.integers(0, 4, 500)]]))
    yield "random", torch.from_numpy(acgt[rng.integers(0, 4, 20_000)])
    for t in (b"A", b"AC", b"GATTACA"):
        yield t.decode(), torch.from_numpy(np.frombuffer(t, np.uint8).copy())


@pytest.mark.parametrize("name,text", list(_texts()), ids=lambda v: v if isinstance(v, str) else "")
def test_suffix_array_is_indexbuilds(name, text):
    tc = torch.from_numpy(ib.CODE)[torch.cat([text, torch.tensor([ord("$")], dtype=torch.uint8)]).long()]
    assert torch.equal(bench.suffix_array(tc), ib.suffix_array(tc)), name
    assert torch.equal(bench.suffix_array(torch.flip(tc, dims=[0])), ib.suffix_array(torch.flip(tc, dims=[0]))), name


@pytest.mark.parametrize("with_bwt", [False, True])
def test_bench_index_is_indexbuilds(with_bwt):
    g, starts = synth.genome_human_like(300_000, seed=7)
    mine = bench.build_fm_index(g, starts, 4, "cpu", with_bwt=with_bwt)
    ref = ib.build_index(g, sparseness=4, seq_starts=starts, device="cpu", with_bwt=with_bwt)
    for f in ("text", "counts", "bv_fwd", "cnt_fwd", "bv_rev", "cnt_rev", "bwt_words", "sa_bv", "sa_bv_counts", "sa_samples",
              "seq_starts"):
        a, b = getattr(mine, f), getattr(ref, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    for f in ("dollar_pos_fwd", "dollar_pos_rev", "sparseness", "seq_names"):
        assert getattr(mine, f) == getattr(ref, f), f
