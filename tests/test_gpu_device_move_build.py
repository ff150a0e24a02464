"""The device builder of the b-move index (cmb_build_move_*, columba_amd/csrc/dev_move_build.hpp) against the harness builder on the CPU
(movebuild.build_move(device="cpu"), movebuild._pack_rows), code it does not share a line with.

  * every array of MoveArrays and the PLCP's run form on the tiny texts of tests/tinytexts.py whose length is no power of two;
  * where the field widths change: n = 2^j +- 1, the first text whose row straddles a 64-bit word (2^20 + 1), and through
    cmb_build_pack_lfbp rows of texts of 2^31 + 1, 2^32 - 2 and 2^39 + 5 characters (offsets of 64 bits and more, 40-bit fields);
  * repetitive texts: a pan-genome, homopolymers and a tandem repeat before and after a random tail, polyA of 5000 (one pair with an
    LCP of 4999: the wavefront pass);
  * the same under CMB_TEST_GRID_CAP = 1 and 3, with the vacuity guard of tests/test_gpu_grid_trips.py;
  * the resident index (cmb_build_move_index) against cmb_move_create on the CPU builder's arrays: layout, device arrays byte for
    byte, locate, a batch of reads, alignments with the text beside it, and its independence of the handle;
  * the refusals.

Run with `pytest -m gpu` on an MI355X.
"""
import ctypes as C
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import columba_amd as ca  # noqa: E402
from columba_amd import movebuild, synth  # noqa: E402
import tinytexts as tt  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAY_FIELDS = ("lfbp_fwd", "lfbp_rev", "smpf", "smpl", "rev_smpf", "rev_smpl", "pred_first", "first_to_run", "pred_last", "last_to_run", "text")
assert set(ARRAY_FIELDS) | {"n", "plcp", "sa", "rev_sa", "plcp_pos", "plcp_sum", "sa_rows", "sa_at_rows"} == \
    {f.name for f in dataclasses.fields(movebuild.MoveArrays)}
# every kernel of the move build that loops over rows, runs or pairs (columba_amd/csrc/dev_move_build.hpp)
CAPPED = ("k_bld_bwt", "k_mvb_flags", "k_mvb_heads", "k_mvb_lens", "k_mvb_lf", "k_mvb_out_run", "k_mvb_pack", "k_mvb_rows", "k_mvb_pred_keys",
          "k_mvb_lcp_prefix", "k_mvb_lcp_wave", "k_mvb_plcp_keep")


def grid_lines(err):
    """kernel -> [(items, lanes)] from the CMB_VERBOSE output (as tests/test_gpu_grid_trips.py)"""
    out = {}
    for m in re.finditer(r"\[grid\] (\w+) (\d+) items, (\d+) lanes", err):
        out.setdefault(m.group(1), []).append((int(m.group(2)), int(m.group(3))))
    return out


def _same_move(got: movebuild.MoveArrays, want: movebuild.MoveArrays, where):
    assert got.n == want.n, (where, got.n, want.n)
    assert got.plcp is None and got.sa is None and got.rev_sa is None, where
    pairs = [(f, getattr(got, f), getattr(want, f)) for f in ARRAY_FIELDS]
    pairs += [("plcp_pos", got.plcp_pos, want.plcp_run_form()[0]), ("plcp_sum", got.plcp_sum, want.plcp_run_form()[1])]
    for f, g, w in pairs:
        assert g.dtype == w.dtype and g.shape == w.shape, (where, f, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (where, f, np.flatnonzero(g != w)[:8])


def _check(text: bytes, where):
    want = movebuild.build_move(text, device="cpu")
    b = ca.DeviceBuild(text)
    try:
        _same_move(b.move_arrays(), want, where)
    finally:
        b.close()
    return want


def _random_text(n: int, seed: int) -> bytes:
    """n characters, the final '$' among them"""
    return tt.ACGT[np.random.default_rng(seed).integers(0, 4, n - 1)].tobytes() + b"$"


def _power_of_two(n: int) -> bool:
    return n & (n - 1) == 0


# ------------------------------------------------------------------------------------------------ 1. tiny texts
@pytest.mark.parametrize("kind", tt.KINDS)
def test_tiny_texts_equal_the_cpu_builder(kind):
    seen = 0
    for n in tt.LENGTHS:
        text = tt.text_of(kind, n) + b"$"
        if _power_of_two(len(text)):
            continue
        _check(text, (kind, n))
        seen += 1
    assert seen >= 8


# ------------------------------------------------------------------------------------------------ 2. field widths
@pytest.mark.parametrize("j", range(2, 14))
def test_field_widths_around_powers_of_two(j):
    for n in ((1 << j) - 1, (1 << j) + 1):
        _check(_random_text(n, seed=n), n)


def test_a_row_that_straddles_the_64_bit_word():
    n = (1 << 20) + 1
    want = _check(_random_text(n, seed=20), n)
    r = want.runs_fwd
    assert 3 + 2 * movebuild._bits(n) + movebuild._bits(r) > 64 and 3 + 2 * movebuild._bits(n) < 64   # the run field crosses the word


@pytest.mark.parametrize("n", [(1 << 31) + 1, (1 << 32) - 2, (1 << 39) + 5], ids=["2^31+1", "2^32-2", "2^39+5"])
@pytest.mark.parametrize("r", [2, 3, 700])
def test_the_packing_kernel_at_wide_fields(n, r):
    """rows no text a test can build reaches: offsets of 64 bits and more (3 + 2 bitsN >= 64 from bitsN = 31 on) and 40-bit fields.
    Values use every bit of their field; run numbers beyond r - 1 and positions beyond n - 1 are cut to the field as the reference cuts"""
    rng = np.random.default_rng(n % 1000 + r)
    bits_n = movebuild._bits(n)
    head = rng.integers(0, 5, r).astype(np.uint64)
    starts = np.sort(rng.integers(0, 1 << bits_n, r, dtype=np.uint64))
    starts[0], starts[-1] = 0, (1 << bits_n) - 1
    out = rng.integers(0, 1 << bits_n, r, dtype=np.uint64)
    out[0] = (1 << bits_n) - 1
    out_run = rng.integers(0, max(r, 2), r, dtype=np.uint64)
    out_run[-1] = r - 1
    zero = int(rng.integers(0, n))
    rows = np.stack([head, starts, out, out_run], axis=1)
    for bits in (64, 32) if n < (1 << 32) else (64,):
        got = ca.device_pack_lfbp(n, rows, zero, bits)
        want = movebuild._pack_rows(n, head, starts, out, out_run, zero, bits)
        assert got.dtype == want.dtype and got.shape == want.shape, (n, r, bits, got.shape, want.shape)
        assert np.array_equal(got, want), (n, r, bits, np.flatnonzero(got != want)[:8])


# ------------------------------------------------------------------------------------------------ 3. repetitive texts
def _tail() -> bytes:
    return tt.ACGT[np.random.default_rng(5).integers(0, 4, 700)].tobytes()


REPETITIVE = {
    "pangenome": lambda: movebuild.pangenome(3000, 8, 0.01, seed=3).tobytes(),
    "polyA-then-tail": lambda: b"A" * 3000 + _tail(),
    "tandem-then-tail": lambda: b"ACGT" * 700 + b"AC" + _tail(),
    "tail-then-polyC": lambda: _tail() + b"C" * 2000,
    "polyA-5000": lambda: b"A" * 5000,
}


@pytest.mark.parametrize("name", sorted(REPETITIVE))
def test_repetitive_texts_equal_the_cpu_builder(name):
    text = REPETITIVE[name]() + b"$"
    want = _check(text, name)
    if name == "polyA-5000":
        assert want.runs_fwd == 2 and int(want.plcp.max()) == 4999   # one pair, compared by a wavefront to the end of the text


# ------------------------------------------------------------------------------------------------ 4. grid trips
def _long_pairs() -> bytes:
    """48 random units of 48 characters, each twice, with 20 random characters between them: every unit gives one irreducible pair with
    an LCP of 48 or more, so k_mvb_lcp_wave (64 lanes per pair whose LCP reaches 32) has 48 * 64 = 3072 items, three trips of three
    blocks.  The slice of genome_rep has 17 such pairs (three trips of one block) and no slice of 5000 characters has 36"""
    rng = np.random.default_rng(41)
    units = [tt.ACGT[rng.integers(0, 4, 48)] for _ in range(48)]
    parts = []
    for _ in range(2):
        for j in rng.permutation(48):
            parts += [units[j], tt.ACGT[rng.integers(0, 4, 20)]]
    return np.concatenate(parts).tobytes()


@pytest.fixture(scope="module")
def mid_texts():
    g, _ = synth.genome_rep(seed=29, n=40_000, scale=16.0)
    texts = {"polyA": b"A" * 5000 + b"$", "genome_rep": g.tobytes()[30_000:35_000] + b"$", "long_pairs": _long_pairs() + b"$"}
    return {k: (t, movebuild.build_move(t, device="cpu")) for k, t in texts.items()}


@pytest.fixture(scope="module")
def capped_lines():
    return {}


@pytest.mark.parametrize("cap", (1, 3))
@pytest.mark.parametrize("kind", ("polyA", "genome_rep", "long_pairs"))
def test_move_build_under_the_grid_cap(mid_texts, capped_lines, monkeypatch, capfd, kind, cap):
    text, want = mid_texts[kind]
    monkeypatch.setenv("CMB_VERBOSE", "1")
    monkeypatch.setenv("CMB_TEST_GRID_CAP", str(cap))
    b = ca.DeviceBuild(text)
    try:
        capfd.readouterr()
        got = b.move_arrays()
        ix = b.move_index()
        ix.close()
    finally:
        b.close()
    lines = grid_lines(capfd.readouterr().err)
    monkeypatch.delenv("CMB_TEST_GRID_CAP")
    _same_move(got, want, (kind, cap))
    for k, v in lines.items():
        assert all(0 < lanes <= cap * 256 and lanes % 256 == 0 for _, lanes in v), (k, v)
    for k in CAPPED:
        assert k in lines, (k, "no [grid] line", sorted(lines))
    capped_lines[(kind, cap)] = lines


def test_every_loop_of_the_move_build_had_three_trips(capped_lines):
    """items >= 3 * lanes for every looping kernel: on polyA or the slice of genome_rep under some cap, and under either cap on one of
    the three texts"""
    kinds = ("polyA", "genome_rep", "long_pairs")
    assert sorted(capped_lines) == sorted((kind, cap) for kind in kinds for cap in (1, 3))
    assert int(capped_lines[("long_pairs", 3)]["k_mvb_lcp_wave"][0][0]) == 48 * 64
    for k in CAPPED:
        two = [il for kind in kinds[:2] for cap in (1, 3) for il in capped_lines[(kind, cap)][k]]
        assert any(i >= 3 * lanes for i, lanes in two), (k, two)
        for cap in (1, 3):
            seen = [il for kind in kinds for il in capped_lines[(kind, cap)][k]]
            assert any(i >= 3 * lanes for i, lanes in seen), (k, cap, seen)


# ------------------------------------------------------------------------------------------------ 5. resident index
@pytest.fixture(scope="module")
def resident_world():
    g = movebuild.pangenome(50_000, 4, 0.01, seed=9)
    text = g.tobytes() + b"$"
    starts = np.array([0, 50_000, 100_000, 150_000, len(text) - 1], dtype=np.uint32)
    reads = synth.sample_reads(g, 300, 100, seed=77)
    return text, starts, reads, movebuild.build_move(text, device="cpu")


def _batch(ix, reads, alignments: bool):
    st = ca.SearchStrategy("multiple_opt", "edit", "dynamic")
    b = ca.MoveBatch(ix, st, 2, reads)
    try:
        if alignments:
            b.want_alignments()
        b.run()
        return b.results() + (b.alignments() if alignments else ())
    finally:
        b.close()


def test_resident_index_equals_the_uploaded_one(resident_world):
    text, starts, reads, mv = resident_world
    want_ix = ca.MoveIndex(mv)
    b = ca.DeviceBuild(text)
    try:
        got_ix = b.move_index()
        with_text = b.move_index(attach_text=True, seq_starts=starts)
        no_locate = b.move_index(with_locate=False)
    finally:
        b.close()   # (the indexes do not depend on the handle)
    try:
        lw, lg = want_ix.layout(), got_ix.layout()
        for f, _ in ca.MoveLayout._fields_:
            w, g = getattr(lw, f), getattr(lg, f)
            if hasattr(w, "__len__"):
                w, g = list(w), list(g)
            assert w == g, (f, w, g)
        assert lg.has_locate == 1 and no_locate.layout().has_locate == 0
        assert (got_ix.n, got_ix.runs, got_ix.rev_runs) == (want_ix.n, want_ix.runs, want_ix.rev_runs)
        assert want_ix.device_bytes() == got_ix.device_bytes()
        tw, tg = want_ix.device_tensors(), got_ix.device_tensors()
        for i in range(ca.MOVE_DEV_ARRAYS):
            assert (tw[i] is None) == (tg[i] is None) and tw[i] is not None, i
            w, g = tw[i].cpu().numpy(), tg[i].cpu().numpy()
            if i in (0, 3):   # the rows: the word behind the terminating row is padding (0xFF)
                assert np.array_equal(w[-16:], g[-16:]) and (g[-16:] == 0xFF).all(), i
            assert w.shape == g.shape and np.array_equal(w, g), (i, np.flatnonzero(w != g)[:8])   # (rows: the gap bits among them)
        tn = no_locate.device_tensors()
        for i in range(6):
            assert np.array_equal(tn[i].cpu().numpy(), tw[i].cpu().numpy()), i
        assert all(t is None for t in tn[6:])
        assert np.array_equal(want_ix.rows(0), got_ix.rows(0)) and np.array_equal(want_ix.rows(1), got_ix.rows(1))
        kw, kg = want_ix.kmer_table(6), got_ix.kmer_table(6)
        assert np.array_equal(kw, kg)
        ranges = kw[kw["end"] > kw["begin"]]
        assert len(ranges) > 1000
        (pw, ow), (pg, og) = want_ix.locate(ranges), got_ix.locate(ranges)
        assert np.array_equal(ow, og) and np.array_equal(pw, pg) and len(pw) > 100_000
        (wo, woff, wc), (go, goff, gc) = _batch(want_ix, reads, False), _batch(got_ix, reads, False)
        assert np.array_equal(woff, goff) and np.array_equal(wo, go) and len(wo) > len(reads)
        assert wc == gc
        # alignments: the handle's own text against the text attached by the caller
        want_ix.attach_text(text, starts)
        aw, ag = _batch(want_ix, reads, True), _batch(with_text, reads, True)
        assert np.array_equal(aw[0], ag[0]) and np.array_equal(aw[1], ag[1]) and aw[2] == ag[2]
        assert np.array_equal(aw[3], ag[3]) and np.array_equal(aw[4], ag[4]) and len(aw[3]) == len(aw[0]) > len(reads)
        with pytest.raises(ca.CmbError):
            _batch(got_ix, reads, True)   # (no text beside this one)
    finally:
        for ix in (want_ix, got_ix, with_text, no_locate):
            ix.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("n", [2, 4, 64, 4096])
def test_a_power_of_two_is_refused_with_the_reason(n):
    b = ca.DeviceBuild(_random_text(n, seed=n))
    try:
        for call in (b.move_sizes, b.move_arrays, b.move_index):
            with pytest.raises(ca.CmbError) as e:
                call()
            assert e.value.code == ca.CMB_ERR_UNSUPPORTED and "power of two" in str(e.value) and "terminating row" in str(e.value)
        assert b.suffix_array().shape[0] == n   # (the handle is as good as before)
    finally:
        b.close()


CAPS = ("lfbp_cap", "rev_lfbp_cap", "runs_cap", "rev_runs_cap", "plcp_cap")


def test_small_output_buffers_overflow_with_the_needed_sizes():
    text = movebuild.pangenome(600, 3, 0.02, seed=2).tobytes() + b"$"
    want = movebuild.build_move(text, device="cpu")
    b = ca.DeviceBuild(text)
    try:
        L = ca.lib()
        for bits in (64, 32):
            z = b.move_sizes(bits)
            sizes = [z.lfbp_bytes, z.rev_lfbp_bytes, z.runs, z.rev_runs, z.n_plcp]
            assert sizes == [len(want.lfbp_fwd) - (0 if bits == 64 else 12), len(want.lfbp_rev) - (0 if bits == 64 else 12), want.runs_fwd,
                             want.runs_rev, len(want.plcp_run_form()[0])] and z.text_length == len(text)
            per_run = ("samples_first", "samples_last", "pred_first", "first_to_run", "pred_last", "last_to_run")
            bufs = {"lfbp": np.zeros(z.lfbp_bytes, np.uint8), "rev_lfbp": np.zeros(z.rev_lfbp_bytes, np.uint8)}
            bufs.update({k: np.zeros(z.runs, np.uint64) for k in per_run})
            bufs.update({k: np.zeros(z.rev_runs, np.uint64) for k in ("rev_samples_first", "rev_samples_last")})
            bufs.update({k: np.zeros(z.n_plcp, np.uint64) for k in ("plcp_pos", "plcp_sum")})
            for short in CAPS:
                a = ca._BuildMoveArrays()
                for k, v in bufs.items():
                    setattr(a, k, ca._p(v))
                a.length_bits = bits
                for k, s in zip(CAPS, sizes):
                    setattr(a, k, s - 1 if k == short else s)
                needed = np.zeros(5, np.uint64)
                assert L.cmb_build_move_arrays(b.h, C.byref(a), ca._p(needed)) == ca.CMB_ERR_OVERFLOW, (bits, short)
                assert needed.tolist() == sizes and not any(v.any() for v in bufs.values()), (bits, short)
                assert L.cmb_build_move_arrays(b.h, C.byref(a), None) == ca.CMB_ERR_OVERFLOW   # (needed may be NULL)
        _same_move(b.move_arrays(), want, "after the overflows")
    finally:
        b.close()


def test_a_second_call_returns_the_same_arrays(monkeypatch, capfd):
    text = REPETITIVE["pangenome"]() + b"$"
    b = ca.DeviceBuild(text)
    try:
        first = b.move_arrays()
        phases = [k for k in b.timings() if k.startswith("move ")]
        assert any("PLCP" in k for k in phases) and any(k.startswith("move rev: ") for k in phases), phases
        monkeypatch.setenv("CMB_VERBOSE", "1")
        capfd.readouterr()
        second = b.move_arrays()
        third = b.move_arrays(32)
        lines = grid_lines(capfd.readouterr().err)
        assert set(lines) == {"k_mvb_pack"}, sorted(lines)   # the O(runs) arrays are kept in the handle: only the packing runs again
        assert [k for k in b.timings() if k.startswith("move ")] == phases
        _same_move(second, first, "second call")
        for f in ARRAY_FIELDS[2:] + ("plcp_pos", "plcp_sum"):
            assert np.array_equal(getattr(third, f), getattr(first, f)), f
        # 32-bit length_t: the header alone differs
        assert np.array_equal(third.lfbp_fwd[12:], first.lfbp_fwd[24:]) and np.array_equal(third.lfbp_rev[12:], first.lfbp_rev[24:])
        assert third.lfbp_fwd[:12].view(np.uint32).tolist() == first.lfbp_fwd[:24].view(np.uint64).tolist()
    finally:
        b.close()
