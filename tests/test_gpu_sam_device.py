"""The SAM text of a single-end chunk in ALL mode written on the device (cmb_batch_sam_device, csrc/dev_sam.hpp) against the host
formatter of the same batch (cmb_batch_sam: byte for byte) and against the oracle's restatement of generateOutputSingleEnd.

Run with `pytest -m gpu` on an MI355X.
"""
import contextlib
import os

import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chunk_world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    g, starts = synth.genome_rep(seed=11, n=2_000_000, scale=1.5)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    return {"genome": g, "ix": ix, "dev": ca.Index(ix), "orc": op.OracleIndex(ix), "op": op}


def _chunk(w, k):
    """the read set of test_gpu_parity.test_sam_records_of_a_chunk"""
    g = w["genome"]
    rng = np.random.default_rng(5 + k)
    reads = synth.sample_reads(g, 600, 150, seed=950 + k, n_frac=0.01, edit_choices=(0, 1, 2, 4, 9))
    starts = np.asarray(w["ix"].seq_starts, dtype=np.int64)
    for s in starts[1:-1][:10]:
        reads.append(g[int(s) - 75:int(s) + 75].tobytes())
        reads.append(g[int(s) - 2:int(s) + 148].tobytes())
    ids = [("@" if i % 2 else ">") + f"read{i}/1 some description" for i in range(len(reads))]
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    names = [f"chr{j + 1}" for j in range(len(starts) - 1)]
    return reads, ids, quals, names


def _batch(dev, spec, metric, k, reads):
    b = ca.Batch(dev, ca.SearchStrategy(spec, metric, "dynamic"), k, reads)
    b.want_alignments()
    b.run()
    return b


def _first_difference(a, b):
    n = min(len(a), len(b))
    i = next((j for j in range(n) if a[j] != b[j]), n)
    return f"lengths {len(a)} / {len(b)}, first difference at {i}: {a[max(0, i - 80):i + 40]!r} / {b[max(0, i - 80):i + 40]!r}"


def _same(dev_text, host_text):
    assert dev_text == host_text, _first_difference(dev_text, host_text)


def _norm_k0(lines):
    # (the normalisation of test_sam_records_of_a_chunk: which of several exact matches is the primary one may differ at k = 0)
    out = []
    for x in lines:
        f = x.split("\t")
        f[1] = str(int(f[1]) & ~256)
        f[9] = f[10] = "."
        out.append("\t".join(f))
    return sorted(out)


CONFIGS = [("columba", "edit", 4, False), ("multiple_opt", "edit", 2, True), ("kuch1", "hamming", 2, False),
           ("kuch1", "edit", 0, False), ("columba", "edit", 9, False), ("columba", "edit", 13, True)]


@pytest.mark.parametrize("spec,metric,k,xa", CONFIGS)
def test_device_text_equals_host_text_and_oracle(chunk_world, spec, metric, k, xa):
    """1 + 2: byte for byte the host path's text (also at k = 0), line for line the oracle's; the reads the host formatted are
    exactly those with an occurrence over the end of its sequence, and at most 5 % of the chunk"""
    import schemes_py as sp
    w = chunk_world
    op = w["op"]
    reads, ids, quals, names = _chunk(w, k)
    assert len(reads) == 606
    b = _batch(w["dev"], spec, metric, k, reads)
    _, offs, _ = b.results()
    aln, _ = b.alignments()
    spanning = sum(1 for i in range(len(reads)) if (aln["spans"][int(offs[i]):int(offs[i + 1])] == 1).any())
    for unmapped in (True, False):
        host = b.sam(ids, quals, names, unmapped=unmapped, xa=xa)
        got, host_reads = b.sam_device(ids, quals, names, unmapped=unmapped, xa=xa)
        print(f"{spec} {metric} k={k} xa={xa} unmapped={unmapped}: {len(got)} bytes, host_reads={host_reads}, spanning={spanning}")
        _same(got, host)
        assert host_reads == spanning
        assert host_reads <= 0.05 * len(reads)
        want = op.match_batch_sam(w["orc"], op.OracleStrategy(sp.BY_NAME[spec], metric, "dynamic"), k, reads, ids, quals, names,
                                  unmapped=unmapped, xa=xa)
        gl, wl = got.splitlines(), want.splitlines()
        assert len(wl) >= (len(reads) if unmapped else 1)  # (with unmapped records every read has at least one line)
        if k == 0:
            gl, wl = _norm_k0(gl), _norm_k0(wl)
        for a, x in zip(gl, wl):
            assert a == x
        assert len(gl) == len(wl)
    b.close()


def test_quirks(chunk_world):
    """3: no qualities; empty qualities (plain and XA path); lower-case reads; identifiers without a space and of one character;
    a 30 bp and a 480 bp read; a chunk without any occurrence"""
    w = chunk_world
    g = w["genome"]
    reads = synth.sample_reads(g, 200, 150, seed=31, n_frac=0.01, edit_choices=(0, 1, 2, 4, 9))
    reads[3] = reads[3].lower()
    reads[4] = bytes(c + 32 if i % 3 else c for i, c in enumerate(reads[4]))
    reads.append(g[70_000:70_030].tobytes())
    reads.append(g[90_000:90_480].tobytes())
    reads.append(synth.revcomp(g[120_000:120_480].tobytes()))
    n = len(reads)
    ids = [f"@r{i} d{i} e" for i in range(n)]
    ids[0], ids[1], ids[2], ids[5], ids[6] = "@nospace", "@", ">x", "@ lead", ""
    rng = np.random.default_rng(8)
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    some_empty = [("" if i % 3 == 0 else q) for i, q in enumerate(quals)]
    names = [f"chr{j + 1}" for j in range(len(w["ix"].seq_starts) - 1)]
    b = _batch(w["dev"], "columba", "edit", 4, reads)
    for xa in (False, True):
        for unmapped in (True, False):
            for q in (quals, some_empty):
                got, _ = b.sam_device(ids, q, names, unmapped=unmapped, xa=xa)
                _same(got, b.sam(ids, q, names, unmapped=unmapped, xa=xa))
            got, _ = b.sam_device(ids, None, names, unmapped=unmapped, xa=xa)
            _same(got, b.sam(ids, ["*"] * n, names, unmapped=unmapped, xa=xa))
    text, _ = b.sam_device(ids, quals, names)
    lines = text.splitlines()
    assert lines[0].startswith("nospace\t") and any("\t4\t*\t0\t0\t*" in x for x in lines)
    assert all(x.split("\t")[9] == x.split("\t")[9].upper() for x in lines)
    b.close()
    # a chunk whose reads all lack occurrences
    rng = np.random.default_rng(99)
    junk = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150)) for _ in range(70)]
    b = _batch(w["dev"], "columba", "edit", 2, junk)
    occs, _, _ = b.results()
    assert len(occs) == 0
    jid = [f"@j{i}" for i in range(70)]
    for unmapped in (True, False):
        got, host_reads = b.sam_device(jid, None, names, unmapped=unmapped)
        _same(got, b.sam(jid, ["*"] * 70, names, unmapped=unmapped))
        assert host_reads == 0 and (got == "") == (not unmapped)
    b.close()


def _heavy_text(seed=77):
    """a 150 bp unit 1200 times, every third copy with one substitution, 60 random characters between copies"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    unit = acgt[rng.integers(0, 4, 150)]
    parts = []
    for c in range(1200):
        u = unit.copy()
        if c % 3 == 2:
            p = int(rng.integers(0, 150))
            u[p] = acgt[(int(np.where(acgt == u[p])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]
        parts.append(u)
        parts.append(acgt[rng.integers(0, 4, 60)])
    return unit.tobytes(), np.concatenate(parts)


@pytest.mark.parametrize("k", [2, 4])
def test_a_heavy_read(oracle_built, k):
    """4: a read with more than a thousand occurrences — its XA line is far longer than what a wavefront stages at once"""
    import oracle_py as op
    import schemes_py as sp
    unit, g = _heavy_text()
    starts = [0, 84_000, 168_000, len(g)]  # (three sequences, and the end of the last)
    assert len(g) == 252_000
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    dev = ca.Index(ix)
    reads = [unit, unit[:100], synth.revcomp(unit)]
    ids = ["@heavy first", "@part", "@back"]
    quals = ["I" * len(r) for r in reads]
    names = [f"s{j}" for j in range(len(ix.seq_starts) - 1)]
    b = _batch(dev, "columba", "edit", k, reads)
    occs, offs, _ = b.results()
    d = occs["distance"][int(offs[0]):int(offs[1])]
    print(f"k={k}: {len(d)} occurrences, {(d == d.min()).sum()} at the minimal distance {d.min()}")
    assert len(d) >= 1000 and (d == d.min()).sum() >= 10
    for xa in (False, True):
        got, host_reads = b.sam_device(ids, quals, names, xa=xa)
        _same(got, b.sam(ids, quals, names, xa=xa))
        assert host_reads == 0
        want = op.match_batch_sam(op.OracleIndex(ix), op.OracleStrategy(sp.BY_NAME["columba"], "edit", "dynamic"), k, reads, ids, quals,
                                  names, unmapped=True, xa=xa)
        assert got.splitlines() == want.splitlines()
        if xa:
            assert max(len(x) for x in got.splitlines()) > 16_000
    b.close()


def test_mapq_table():
    """5: the MAPQ the device prints for 1 ... 64 occurrences of minimal distance is the one in cmb_sam_se's line"""
    dev = ca.sam_device_mapq(64)
    for n_hits in range(1, 65):
        line = ca.sam_se("r", ("chr1", 10, 1, False, np.array([150 << 2], np.uint16)), True, n_hits, 1, "ACGT", "IIII")
        assert int(line.split("\t")[4]) == int(dev[n_hits - 1]), n_hits


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


def test_composite_batch(chunk_world):
    """6a: three sub-batches, every one formats its reads on its own stream; the text is in read order"""
    w = chunk_world
    g = w["genome"]
    reads = synth.sample_reads(g, 3000, 150, seed=41, n_frac=0.01, edit_choices=(0, 1, 2, 4, 9))
    starts = np.asarray(w["ix"].seq_starts, dtype=np.int64)
    for j, s in enumerate(starts[1:-1]):
        reads[700 * (j + 1)] = g[int(s) - 75:int(s) + 75].tobytes()
    ids = [f"@c{i} x" for i in range(len(reads))]
    quals = ["".join(chr(40 + (i + j) % 30) for j in range(len(r))) for i, r in enumerate(reads)]
    names = [f"chr{j + 1}" for j in range(len(starts) - 1)]
    with _env(CMB_SUBBATCHES="3"):
        b = _batch(w["dev"], "columba", "edit", 4, reads)
    for xa in (False, True):
        got, host_reads = b.sam_device(ids, quals, names, xa=xa)
        _same(got, b.sam(ids, quals, names, xa=xa))
        assert 1 <= host_reads <= 30
    b.close()
    single = _batch(w["dev"], "columba", "edit", 4, reads)
    _same(single.sam_device(ids, quals, names)[0], single.sam(ids, quals, names))
    single.close()


def _text_of(entry, obj, ids, quals, names, xa):
    """the text `entry` (cmb_batch_sam_device / cmb_best_sam_device) writes for the handle of `obj` from (bytes, offsets) pairs.
    SamInputs is filled here, not by the package's wrapper: offsets that do not start at 0 must reach the C ABI untouched"""
    import ctypes as C
    (bi, oi), (bq, oq), (bn, on) = ids, quals, names
    inp = ca.SamInputs(ca._p(obj._packed[0]), ca._p(bi), ca._p(oi), ca._p(bq), ca._p(oq), ca._p(bn), ca._p(on), on.shape[0] - 1)
    text, n, host = C.c_void_p(), C.c_uint64(), C.c_uint64()
    ca._chk(entry(obj.h, C.byref(inp), 1, int(xa), C.byref(text), C.byref(n), C.byref(host)))
    return (C.string_at(text.value, n.value) if n.value else b"").decode(), int(host.value)


def test_packed_inputs_that_do_not_start_at_zero(chunk_world):
    """8: identifiers and qualities whose offsets begin at 7 and 5 (the driver subtracts id_offs[r0] / qual_offs[r0] as a base, which
    only a sub-batch exercises otherwise) give the text of the zero-based packing, in ALL and in BEST mode, with a host-formatted
    read among the 65 (one more than a wavefront has lanes, five pieces of SAM_READS_PER_WAVE)"""
    w = chunk_world
    g = w["genome"]
    reads = synth.sample_reads(g, 63, 150, seed=71, n_frac=0.01, edit_choices=(0, 1, 2))
    s = int(np.asarray(w["ix"].seq_starts, dtype=np.int64)[1])
    reads += [g[s - 75:s + 75].tobytes(), g[s - 2:s + 148].tobytes()]  # (the sequence-boundary reads of _chunk)
    assert len(reads) == 65 and all(len(r) == 150 for r in reads)
    rng = np.random.default_rng(72)
    ids = ca.pack_fields([("@" if i % 2 else ">") + f"read{i}/1 some description" for i in range(65)])
    quals = ca.pack_fields(["".join(chr(33 + int(q)) for q in rng.integers(0, 41, 150)) for _ in reads])
    names = ca.pack_fields([f"chr{j + 1}" for j in range(len(w["ix"].seq_starts) - 1)])
    shifted_ids = (np.concatenate([np.frombuffer(b"\tjunk \n", np.uint8), ids[0]]), ids[1] + np.uint64(7))
    shifted_quals = (np.concatenate([np.frombuffer(b"~~~~\n", np.uint8), quals[0]]), quals[1] + np.uint64(5))
    assert shifted_ids[0].shape[0] == ids[0].shape[0] + 7 and shifted_quals[0].shape[0] == quals[0].shape[0] + 5
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    b = _batch(w["dev"], "columba", "edit", 2, reads)
    best = ca.BestDevice(w["dev"], st, reads, x=0, min_identity=95)
    for entry, obj in ((ca.lib().cmb_batch_sam_device, b), (ca.lib().cmb_best_sam_device, best)):
        for xa in (False, True):
            want, host_reads = _text_of(entry, obj, ids, quals, names, xa)
            got, host_shifted = _text_of(entry, obj, shifted_ids, shifted_quals, names, xa)
            _same(got, want)
            assert host_shifted == host_reads >= 1 and want.count("\n") >= 65
    _same(_text_of(ca.lib().cmb_batch_sam_device, b, ids, quals, names, False)[0], b.sam_device(ids, quals, names)[0])
    b.close()
    best.close()


def test_run_format_stage_run_format(chunk_world):
    """6b: a batch that is run, formatted, fed a staged chunk and formatted again (a staged chunk travels during the next run
    and is matched by the one after it)"""
    w = chunk_world
    g = w["genome"]
    names = [f"chr{j + 1}" for j in range(len(w["ix"].seq_starts) - 1)]
    first = synth.sample_reads(g, 500, 150, seed=51, edit_choices=(0, 1, 2, 4))
    second = synth.sample_reads(g, 500, 140, seed=52, edit_choices=(0, 1, 3, 9))
    ids1, ids2 = [f"@a{i}" for i in range(500)], [f"@b{i} second" for i in range(500)]
    q1, q2 = ["F" * len(r) for r in first], ["".join(chr(35 + j % 40) for j in range(len(r))) for r in second]
    b = _batch(w["dev"], "columba", "edit", 4, first)
    t1 = b.sam_device(ids1, q1, names)[0]  # (a copy: the library's buffer is not read after the next run)
    _same(t1, b.sam(ids1, q1, names))
    b.stage(ca.pack_reads(second))
    b.run()  # (matches the first chunk once more while the second travels to the device)
    _same(b.sam_device(ids1, q1, names)[0], t1)
    b.run()  # (the staged chunk)
    t2 = b.sam_device(ids2, q2, names, xa=True)[0]
    _same(t2, b.sam(ids2, q2, names, xa=True))
    assert t1 != t2 and t2.startswith("b0\t")
    b.close()


def test_refusals(chunk_world):
    """7: before run, or without alignments: CMB_ERR_INVALID, as cmb_batch_sam"""
    w = chunk_world
    reads = synth.sample_reads(w["genome"], 20, 150, seed=61)
    ids, quals, names = [f"@r{i}" for i in range(20)], ["I" * 150] * 20, ["a", "b", "c", "d"]
    b = ca.Batch(w["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), 2, reads)
    b.want_alignments()
    with pytest.raises(ca.CmbError) as e:
        b.sam_device(ids, quals, names)
    assert e.value.code == -1  # CMB_ERR_INVALID: not run
    with pytest.raises(ca.CmbError) as e2:
        b.sam(ids, quals, names)
    assert e2.value.code == e.value.code
    b.close()
    b = ca.Batch(w["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), 2, reads)
    b.run()
    with pytest.raises(ca.CmbError) as e:
        b.sam_device(ids, quals, names)
    assert e.value.code == -1  # alignments were not requested
    b.close()
