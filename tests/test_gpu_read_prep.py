"""Read preparation in one kernel (k_prep): the codes of both strands, the eight match bit-strings, the read records and the match
words of the full reads, every word of them written by the launch itself — nothing is zeroed beforehand.

A block of k_prep takes 256 / chunks reads per pass (chunks = 32-character words of the longest read of the batch: 51 reads at 150 bp,
17 at 480) and one thread per (read, chunk); it writes G, rec and the match words of a pass from an LDS copy of the strings.  What can go
wrong is therefore a matter of lengths around the 16- and 32-character edges, of batches that end inside a pass, of a block's second
pass, of the header bit for N, and of words that an earlier, longer chunk left behind in the buffers of a batch.

Bar: the CPU oracle, occurrences and counters bit for bit (test_gpu_parity._compare), on a 150 kbp text — reads of one to seventeen
characters match all over it at four and more errors, and the oracle's time for them grows with the text.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 255, 256, 257, 320, 480)


@pytest.fixture(scope="module")
def world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    g, starts = synth.genome_rep(seed=17, n=150_000, scale=2.0)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    return {"genome": g, "ix": ix, "op": op, "dev": ca.Index(ix), "orc": op.OracleIndex(ix), "dev4": ca.Index(ix, kmer_size=4),
            "orc4": op.OracleIndex(ix, kmer_size=4), "built": oracle_built}


def _with_n(read, at):
    return read[:at] + b"N" + read[at + 1:]


def mixed_reads(g, shortest=1, empty=True):
    """every length of LENGTHS from `shortest` on in one batch (the rows are padded to 480): one read each up to 17 characters (they match
    all over the text), six each beyond with up to four edits, half of them reverse-complemented; lower-case reads; reads with N
    at the first position, at the last and on both sides of a 32-character boundary; an all-N read and an empty one"""
    reads = []
    for ln in LENGTHS:
        if ln < shortest:
            continue
        if ln <= 17:
            reads.append(g[4000 + 37 * ln:4000 + 38 * ln].tobytes())
        else:
            reads += synth.sample_reads(g, 6, ln, seed=3000 + ln, edit_choices=(0, 1, 2, 4))
    for ln in (33, 65, 150, 257):
        r = g[9000 + ln:9000 + 2 * ln].tobytes()
        reads += [r.lower(), _with_n(r, 0), _with_n(r, ln - 1), _with_n(r, 31), _with_n(r, 32), _with_n(r.lower(), ln // 2).replace(b"N", b"n")]
    reads += [b"N" * 40, g[0:150].tobytes(), g[-151:-1].tobytes()] + ([b""] if empty else [])
    return reads


# edit distance at 1 and 4 errors (32-bit matrix words) and at 5 (64-bit), Hamming distance, exact matching, and beyond 7 errors the
# wide verification that takes its match words from G itself: all of them read seq, G and — but for the last three — the match words
METRICS = [("columba", "edit", "dynamic", 1, 1), ("multiple_opt", "edit", "dynamic", 4, 1), ("columba", "edit", "dynamic", 5, 1),
           ("kuch1", "hamming", "dynamic", 2, 1), ("pigeon", "edit", "dynamic", 0, 1), ("columba", "edit", "dynamic", 8, 15)]


@pytest.mark.parametrize("spec,metric,partition,k,shortest", METRICS, ids=lambda v: str(v))
def test_lengths_around_chunk_edges_in_one_batch(world, spec, metric, partition, k, shortest):
    # (the single character is left out at 8 errors: every window of up to nine characters is an occurrence of it.  The empty read is
    # left out under the Hamming distance: its occurrences are the oracle's, but the device has always counted fewer nodes for it — 120
    # against 288 at two errors, before this kernel as after it; the edit-distance cases hold its zero-header record to the oracle)
    _compare(world, spec, metric, partition, k, mixed_reads(world["genome"], shortest, empty=metric != "hamming"), dups_rare=False)


def test_a_block_takes_several_passes(world, monkeypatch):
    """one block for the whole batch: 17 reads per pass at rows of 480 characters, the last pass ragged"""
    monkeypatch.setenv("CMB_TEST_GRID_CAP", "1")
    _compare(world, "multiple_opt", "edit", "dynamic", 4, mixed_reads(world["genome"]), dups_rare=False)


@pytest.fixture(scope="module")
def reads150(world):
    return synth.sample_reads(world["genome"], 257, 150, seed=41, n_frac=0.05)


# (51 reads of 150 characters to a pass, 64 of 100: batches that end inside a pass, on its edge and one read beyond)
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 50, 51, 52, 102, 103, 255, 256, 257])
def test_batch_sizes(world, reads150, n):
    _compare(world, "multiple_opt", "edit", "dynamic", 4, reads150[:n], dups_rare=False)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_batch_sizes_at_100_characters(world, reads150, n):
    _compare(world, "multiple_opt", "edit", "dynamic", 2, [r[:100] for r in reads150[:n]], dups_rare=False)


@pytest.mark.parametrize("spec,metric,k", [("multiple_opt", "edit", 4), ("columba", "edit", 5), ("kuch1", "hamming", 2), ("columba", "edit", 8)])
def test_a_shorter_chunk_finds_no_stale_words(world, spec, metric, k):
    """a batch of 150 bp reads runs; then a chunk of reads of 20 ... 149 characters, some with N, is staged into the same buffers and
    runs: the words of G, rec and the match words behind the shorter reads are zeros again, the N bits of the headers are gone —
    results and counters are those of a fresh batch on that chunk, which are the oracle's"""
    g = world["genome"]
    n = 300
    first = synth.sample_reads(g, n, 150, seed=51, n_frac=0.3)
    rng = np.random.default_rng(52)
    second = []
    for i in range(n):
        ln = 20 + (i * 7) % 130
        r = synth.sample_reads(g, 1, ln, seed=6000 + i, edit_choices=(0, 1, 2))[0]
        second.append(_with_n(r, int(rng.integers(0, ln))) if i % 9 == 0 else r)
    assert min(map(len, second)) == 20 and max(map(len, second)) == 149
    _compare(world, spec, metric, "dynamic", k, second, dups_rare=False)       # fresh batch == oracle
    st = ca.SearchStrategy(spec, metric, "dynamic")
    want = ca.match_batch(world["dev"], st, k, second)
    batch = ca.Batch(world["dev"], st, k, reads=first)
    batch.stage(ca.pack_reads(second))
    batch.run()                                                                # the 150 bp reads; the chunk travels
    one = batch.results()
    batch.run()                                                                # the chunk, over the words of the first run
    got = batch.results()
    batch.close()
    w1 = ca.match_batch(world["dev"], st, k, first)
    assert np.array_equal(one[0], w1[0]) and np.array_equal(one[1], w1[1]) and one[2] == w1[2]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("length", [16, 33, 150])
@pytest.mark.parametrize("k", [2, 4, 9])
def test_single_pattern_verification_hooks(world, length, k):
    """cmb_verify_batch (its own k_prep launch for one pattern: k_verify + k_traceback, k_verify_wide beyond 7 errors) and
    cmb_verify_batch_staged (the batch path over given candidates)"""
    g = world["genome"]
    pos = 70_000
    pat = bytearray(g[pos:pos + length].tobytes())
    pat[length // 2] = ord("A") if pat[length // 2] != ord("A") else ord("C")
    pat = bytes(pat)
    rng = np.random.default_rng(length + k)
    starts = np.concatenate([rng.integers(0, len(g), 40), np.arange(pos - 12, pos + 12), [0, len(g) - 5, len(g)]]).astype(np.uint32)
    key = lambda a: sorted((int(x["begin"]), int(x["end"]), int(x["distance"])) for x in a)  # noqa: E731
    for fixed in (True, False):
        o, oc = world["orc"].verify(pat, starts, k, 0, fixed)
        assert len(o) > 0
        for staged in (False, True):
            d, dc = world["dev"].verify(pat, starts, k, 0, fixed, staged=staged)
            assert key(d) == key(o), (fixed, staged)
            for n in ("IN_TEXT_STARTED", "ABORTED_IN_TEXT_VERIF", "CIGARS_IN_TEXT_VERIFICATION", "MATRIX_ROWS"):
                assert dc[n] == oc[n], (fixed, staged, n, dc[n], oc[n])


def test_single_pattern_cigar_hook(world):
    """cmb_cigar_windows (the other single-pattern k_prep launch) at 16, 33 and 150 characters, against the oracle's findCIGAR"""
    g = world["genome"]
    L = ca.lib()
    cmds, got = [], []
    for length in (16, 33, 150):
        for pos, cut, d in ((20_000, 0, 2), (0, 5, 3), (len(g) - length - 1, length // 2, 4), (50_000, length - 3, 9)):
            text = g[pos:pos + length + 1].tobytes()
            read = text[:cut] + text[cut + 1:]          # one text character missing from the read
            assert len(read) == length
            bb, ee, dd = np.array([pos], np.uint32), np.array([pos + length + 1], np.uint32), np.array([d], np.uint32)
            ops, nops = np.zeros(40, np.uint16), np.zeros(1, np.uint32)
            rc = L.cmb_cigar_windows(world["dev"].h, read, len(read), bb.ctypes.data_as(C.c_void_p), ee.ctypes.data_as(C.c_void_p),
                                     dd.ctypes.data_as(C.c_void_p), 1, ops.ctypes.data_as(C.c_void_p), 40, nops.ctypes.data_as(C.c_void_p))
            assert rc == 0, (length, pos, d, L.cmb_last_error())
            got.append(ca.cigar_string(ops[:int(nops[0])]))
            cmds.append(f"findcigar {read.decode()} {text.decode()} {d}")
    res = subprocess.run([os.path.join(world["built"], "oracle_driver")], input="\n".join(cmds) + "\n", capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert res == got
    assert sum("D" in c for c in got) >= 6
