"""movebuild.build_move_resident (the b-move parts derived where the suffix arrays are, only O(r) arrays and the PLCP runs
brought to the host) against the host builder movebuild.build_move, with torch on the CPU: the same .LFBP bytes, samples,
predecessors and PLCP, at text lengths on both sides of powers of two (the field widths of the packed rows change there)."""
import numpy as np
import pytest

from columba_amd import movebuild

FIELDS = ("lfbp_fwd", "lfbp_rev", "smpf", "smpl", "rev_smpf", "rev_smpl", "pred_first", "first_to_run", "pred_last", "last_to_run", "text")


def _same(text):
    a = movebuild.build_move(text, device="cpu")
    b = movebuild.build_move_resident(text, device="cpu", n_random_rows=256)
    assert a.n == b.n and b.plcp is None and b.sa is None and b.rev_sa is None
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), (f, a.n)
    pos, sm = a.plcp_run_form()
    assert np.array_equal(pos, b.plcp_pos) and np.array_equal(sm, b.plcp_sum), a.n
    assert np.array_equal(movebuild.plcp_from_runs(b.plcp_pos, b.plcp_sum, b.n), a.plcp), a.n
    assert b.sa_rows.shape[0] >= min(a.n, 1 << 10)
    assert np.array_equal(a.sa[b.sa_rows.astype(np.int64)], b.sa_at_rows), a.n


@pytest.mark.parametrize("j", range(2, 14))
def test_resident_build_is_the_host_build_around_powers_of_two(j):
    rng = np.random.default_rng(j)
    for n in ((1 << j) - 1, (1 << j) + 1):   # (n counts the '$'; a power of two cannot be packed)
        _same(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n - 1)].tobytes())


def test_resident_build_is_the_host_build_on_repetitive_texts():
    g = movebuild.pangenome(3000, 8, 0.01, seed=3)
    _same(g.tobytes())
    rng = np.random.default_rng(5)
    tail = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 700)].tobytes()
    _same(b"A" * 3000 + tail)             # long common prefixes: the compared blocks grow
    _same(b"ACGT" * 700 + b"AC" + tail)
    _same(tail + b"C" * 2000)             # the homopolymer just before the '$'


def test_resident_build_keeps_the_top_rows():
    text = movebuild.pangenome(50_000, 4, 0.01, seed=9).tobytes()
    b = movebuild.build_move_resident(text, device="cpu", n_random_rows=100)
    rows = b.sa_rows.astype(np.int64)
    assert np.array_equal(rows, np.unique(rows)) and rows[-1] == b.n - 1 and rows[0] == 0
    assert np.isin(np.arange(max(0, b.n - (1 << 16)), b.n), rows).all() and rows.shape[0] < b.n
