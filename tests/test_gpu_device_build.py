"""The device index builder (cmb_build_*, columba_amd/csrc/build.hip) against code it does not share a line with.

  * suffix arrays of the text and of the reversed text against plain Python sorting, on the tiny texts of tests/tinytexts.py: shorter
    than a wavefront, a sort tile or the 20 symbols of the initial key; polyA and the tandem keep every group open for log2 n rounds,
    `copies` closes its groups in different rounds;
  * every field of IndexArrays against the harness builder on the CPU (indexbuild.build_index(device="cpu")), at the lengths where a
    layout has a seam, at sparseness factors larger than some of the texts, on a repeat-rich text and on a small pan-genome whose long
    repeats need many doubling rounds; repeated sparse suffix arrays from one handle;
  * the same under CMB_TEST_GRID_CAP = 1 and 3, with the vacuity guard of tests/test_gpu_grid_trips.py: every capped kernel of the
    build shows a launch with at least three trips per lane;
  * the resident index (cmb_build_index) against cmb_index_create on the CPU builder's arrays: layout, k-mer table, and a batch of
    reads with identical occurrences and counters, once more through the sparse samples the build produced;
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
from columba_amd import indexbuild as ib, movebuild, synth  # noqa: E402
import tinytexts as tt  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAY_FIELDS = ("text", "counts", "bv_fwd", "cnt_fwd", "bv_rev", "cnt_rev", "bwt_words", "sa_bv", "sa_bv_counts", "sa_samples", "seq_starts")
SCALAR_FIELDS = ("dollar_pos_fwd", "dollar_pos_rev", "sparseness", "seq_names")
assert set(ARRAY_FIELDS + SCALAR_FIELDS) == {f.name for f in dataclasses.fields(ib.IndexArrays)}
SPARSENESS = (1, 4, 16, 128)
# every kernel of the build that loops over rows or positions (columba_amd/csrc/dev_build.hpp)
CAPPED = ("k_bld_check", "k_bld_key20", "k_bld_heads", "k_bld_ranks", "k_bld_round_keys", "k_bld_bwt", "k_bld_bitvectors", "k_bld_sa_mark")


def grid_lines(err):
    """kernel -> [(items, lanes)] from the CMB_VERBOSE output (as tests/test_gpu_grid_trips.py)"""
    out = {}
    for m in re.finditer(r"\[grid\] (\w+) (\d+) items, (\d+) lanes", err):
        out.setdefault(m.group(1), []).append((int(m.group(2)), int(m.group(3))))
    return out


def _plain_sa(t: bytes) -> np.ndarray:
    return np.array(sorted(range(len(t)), key=lambda i: t[i:]), dtype=np.uint32)


def _check_suffix_arrays(text: bytes, where):
    b = ca.DeviceBuild(text)
    try:
        assert np.array_equal(b.suffix_array(), _plain_sa(text)), (where, "text")
        assert np.array_equal(b.suffix_array(reverse=True), _plain_sa(text[::-1])), (where, "reversed text")
    finally:
        b.close()


def _same_arrays(got: ib.IndexArrays, want: ib.IndexArrays, where):
    for f in SCALAR_FIELDS:
        assert getattr(got, f) == getattr(want, f), (where, f, getattr(got, f), getattr(want, f))
    for f in ARRAY_FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (where, f, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (where, f, np.flatnonzero(g != w)[:8])


def _random_text(n: int, seed: int) -> bytes:
    """n characters, the final '$' among them"""
    return tt.ACGT[np.random.default_rng(seed).integers(0, 4, n - 1)].tobytes() + b"$"


# ------------------------------------------------------------------------------------------------ 1. suffix arrays
@pytest.mark.parametrize("kind", tt.KINDS)
def test_suffix_arrays_equal_plain_sorting(kind):
    for n in tt.LENGTHS:
        _check_suffix_arrays(tt.text_of(kind, n) + b"$", (kind, n))


def test_suffix_array_of_the_sentinel_alone():
    _check_suffix_arrays(b"$", "$")


# ------------------------------------------------------------------------------------------------ 2. arrays
# n + 1 around one 512-bit count block; the host builder's own cases; the 3-bit words; the shortest text with a character
SEAM_LENGTHS = (510, 511, 512, 513, 64 * 512 - 1, 64 * 512, 21, 22, 43, 64, 2)


@pytest.mark.parametrize("n", SEAM_LENGTHS)
def test_arrays_equal_the_cpu_builder_at_the_seams(n):
    text = _random_text(n, seed=n)
    b = ca.DeviceBuild(text)
    try:
        for s in SPARSENESS:
            _same_arrays(b.arrays(s), ib.build_index(text, sparseness=s, device="cpu"), (n, s))
    finally:
        b.close()


@pytest.fixture(scope="module")
def rep_text():
    g, starts = synth.genome_rep(seed=29, n=200_000, scale=4.0)
    return g.tobytes() + b"$", starts


def test_arrays_of_a_repeat_rich_text(rep_text):
    text, starts = rep_text
    starts = np.concatenate([starts[:-1], [len(text) - 1]]).astype(np.uint32)
    names = ["chr%d" % i for i in range(len(starts) - 1)]
    b = ca.DeviceBuild(text)
    try:
        _same_arrays(b.arrays(4, seq_starts=starts, seq_names=names), ib.build_index(text, sparseness=4, seq_starts=starts, seq_names=names, device="cpu"),
                     "genome_rep")
        assert len([k for k in b.timings() if "round" in k]) >= 4   # (the repeats are longer than 20 symbols)
    finally:
        b.close()


def test_arrays_of_a_pangenome():
    text = movebuild.pangenome(3000, 8, 0.01).tobytes() + b"$"
    b = ca.DeviceBuild(text)
    try:
        _same_arrays(b.arrays(16), ib.build_index(text, sparseness=16, device="cpu"), "pangenome")
        assert len([k for k in b.timings() if k.startswith("fwd: round")]) >= 5   # repeats of hundreds of characters
    finally:
        b.close()


def test_every_sparse_suffix_array_from_one_handle(rep_text):
    text = rep_text[0][:50_000] + b"$"
    b = ca.DeviceBuild(text)
    try:
        for s in (1, 2, 4, 8, 16, 32, 64, 128, 4, 1):   # (and again: nothing of an earlier call is left behind)
            want = ib.build_index(text, sparseness=s, device="cpu", with_bwt=False)
            bv, cnt, samples = b.sparse_sa(s)
            for name, g, w in (("sa_bv", bv, want.sa_bv), ("sa_bv_counts", cnt, want.sa_bv_counts), ("sa_samples", samples, want.sa_samples)):
                assert g.dtype == w.dtype and np.array_equal(g, w), (s, name)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ 3. grid trips
def _mid_texts(rep_text):
    return {"polyA": b"A" * 5000 + b"$", "genome_rep": rep_text[0][100_000:105_000] + b"$"}


@pytest.mark.parametrize("cap", (1, 3))
@pytest.mark.parametrize("kind", ("polyA", "genome_rep"))
def test_build_under_the_grid_cap(rep_text, monkeypatch, capfd, kind, cap):
    """every loop of the build with at least three trips: items >= 3 * lanes for every capped kernel.  On the repeat-rich text few
    rows stay open after the sort of 20 symbols, so k_bld_round_keys has its three trips on polyA alone (every row open in every round)."""
    text = _mid_texts(rep_text)[kind]
    monkeypatch.setenv("CMB_VERBOSE", "1")
    monkeypatch.setenv("CMB_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    b = ca.DeviceBuild(text)
    try:
        assert np.array_equal(b.suffix_array(), _plain_sa(text))
        assert np.array_equal(b.suffix_array(reverse=True), _plain_sa(text[::-1]))
        got = b.arrays(4)
    finally:
        b.close()
    lines = grid_lines(capfd.readouterr().err)
    monkeypatch.delenv("CMB_TEST_GRID_CAP")
    _same_arrays(got, ib.build_index(text, sparseness=4, device="cpu"), (kind, cap))
    for k, v in lines.items():
        assert all(0 < lanes <= cap * 256 and lanes % 256 == 0 for _, lanes in v), (k, v)
    for k in CAPPED:
        if k == "k_bld_round_keys" and kind != "polyA":
            continue
        assert k in lines, (k, "no [grid] line", sorted(lines))
        assert any(i >= 3 * lanes for i, lanes in lines[k]), (k, lines[k])


# ------------------------------------------------------------------------------------------------ 4. resident index
@pytest.fixture(scope="module")
def resident_world(rep_text):
    g = np.frombuffer(rep_text[0][:20_000], dtype=np.uint8)
    text = g.tobytes() + b"$"
    starts = np.array([0, 6_000, 13_000, 20_000], dtype=np.uint32)
    reads = synth.sample_reads(g, 200, 100, seed=77)
    return text, starts, reads


@pytest.mark.parametrize("sparseness,sparse_walk", [(4, False), (16, True)])
def test_resident_index_equals_the_uploaded_one(resident_world, monkeypatch, sparseness, sparse_walk):
    text, starts, reads = resident_world
    if sparse_walk:
        monkeypatch.setenv("CMB_SA_SPARSE", "1")   # locates walk the sparse samples the build produced
    want_ix = ca.Index(ib.build_index(text, sparseness=sparseness, seq_starts=starts, device="cpu"))
    b = ca.DeviceBuild(text)
    try:
        got_ix = b.index(sparseness=sparseness, kmer_size=10, in_text_switch=4, seq_starts=starts)
    finally:
        b.close()   # (the index does not depend on the handle)
    try:
        lw, lg = want_ix.layout(), got_ix.layout()
        for f, _ in ca.IndexLayout._fields_:
            w, g = getattr(lw, f), getattr(lg, f)
            if hasattr(w, "__len__"):
                w, g = list(w), list(g)
            assert w == g, (f, w, g)
        assert np.array_equal(want_ix.seq_starts(), got_ix.seq_starts())
        assert want_ix.device_bytes() == got_ix.device_bytes()
        assert np.array_equal(want_ix.kmer_table(), got_ix.kmer_table())
        st = ca.SearchStrategy("multiple_opt", "edit", "dynamic")
        (wo, woff, wc), (go, goff, gc) = ca.match_batch(want_ix, st, 4, reads), ca.match_batch(got_ix, st, 4, reads)
        assert np.array_equal(woff, goff) and np.array_equal(wo, go) and len(wo) > 200
        assert wc == gc
        assert wc["LF_STEPS"] > 0 if sparse_walk else True
    finally:
        want_ix.close(), got_ix.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("text", [b"ACGTaCGT$", b"ACGTNCGT$", b"ACG$ACGT$", b"ACGTACGT", b"ACGTACG$A", b""],
                         ids=["lower-case", "N", "sentinel-inside", "no-sentinel", "sentinel-not-last", "empty"])
def test_malformed_texts_are_refused_before_any_sort(text, monkeypatch, capfd):
    monkeypatch.setenv("CMB_VERBOSE", "1")
    capfd.readouterr()
    with pytest.raises(ca.CmbError) as e:
        ca.DeviceBuild(text)
    assert e.value.code == ca.CMB_ERR_INVALID
    assert "k_bld_key20" not in capfd.readouterr().err


def test_small_output_buffers_overflow_with_the_needed_size():
    text = _random_text(1000, seed=5)
    b = ca.DeviceBuild(text)
    try:
        L, z = ca.lib(), b.sizes()
        out = np.zeros(len(text), np.uint32)
        assert L.cmb_build_suffix_array(b.h, 0, ca._p(out), len(text) - 1) == ca.CMB_ERR_OVERFLOW
        assert str(len(text)).encode() in L.cmb_last_error() and not out.any()
        nb, nc, ns = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.cmb_build_sparse_sa_sizes(b.h, 4, C.byref(nb), C.byref(nc), C.byref(ns)) == ca.CMB_OK
        bv, cnt, smp, got = np.zeros(nb.value, np.uint64), np.zeros(nc.value, np.uint64), np.zeros(ns.value, np.uint32), C.c_uint64()
        assert L.cmb_build_sparse_sa(b.h, 4, ca._p(bv), nb.value, ca._p(cnt), nc.value, ca._p(smp), ns.value - 1, C.byref(got)) == ca.CMB_ERR_OVERFLOW
        assert got.value == ns.value == 250 and not bv.any() and not smp.any()
        a, bufs = b.bwt_arrays()
        a.cnt_cap = z.cnt_words - 1
        for v in bufs.values():
            v[:] = 0
        needed = np.zeros(3, np.uint64)
        assert L.cmb_build_bwt_arrays(b.h, C.byref(a), ca._p(needed)) == ca.CMB_ERR_OVERFLOW
        assert needed.tolist() == [z.bv_words, z.cnt_words, z.bwt_words] and not any(v.any() for v in bufs.values())
        assert L.cmb_build_sparse_sa(b.h, 3, ca._p(bv), nb.value, ca._p(cnt), nc.value, ca._p(smp), ns.value, C.byref(got)) == ca.CMB_ERR_INVALID
    finally:
        b.close()
