"""The HIP path on tiny, low-complexity texts (tests/tinytexts.py: 1 ... 1 000 characters, six kinds, one and three sequences)
and at the two ends of a text.

Texts shorter than a wavefront, a rank block, a suffix-array sample interval or a k-mer of the seed table were reached only by
tools/soak_tiny_texts.py and tools/soak_move_tiny.py, outside pytest and before the device built its dense suffix array,
started searches from k_parts, wrote SAM text, kept BEST-mode bookkeeping or returned b-move lists.  Here:

  * the FM flavour against the oracle (what tools/soak_tiny_texts.py compares: offsets, begin / end / distance, counters) on
    every world, at sparseness 1 / 4 / 16, seed sizes 4 and 10, dense and sparse locate;
  * the device lists through the judge of tests/tinytexts.py, on the FM index (default switch point and 0) and through
    `MoveIndex.match_batch`;
  * `Batch.sam` = `Batch.sam_device` = the oracle's text; `match_best` = `match_best_device` = the oracle, and the BEST-mode
    text written on the device — on every world as well;
  * `pair_chunk_sam` = `pair_chunk_sam_device` on a text of 257 characters in three sequences;
  * the b-move backend: `one_text` of tools/soak_move_tiny.py (rows, every extension of the walks, locate, the refused
    toeholds, exact matching) on its seven fixed texts and 24 generated ones;
  * the b-move search on texts of 16 ... 1 000 characters against the oracle's b-move search, `MoveBatch.sam` =
    `MoveBatch.sam_device`, and BEST mode on the host and device paths of that backend.

Run with `pytest -m gpu` on an MI355X.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import columba_amd as ca  # noqa: E402
from columba_amd import indexbuild as ib, movebuild, synth  # noqa: E402
import tinytexts as tt  # noqa: E402
from test_ground_truth import gt  # noqa: E402,F401
from test_gpu_dense_sa import _index  # noqa: E402
from test_gpu_best_device import _assert_same, _sam_of_best  # noqa: E402
from test_gpu_sam_device import _norm_k0, _same  # noqa: E402
from test_tiny_texts import SHAPES, f1_reads  # noqa: E402

pytestmark = pytest.mark.gpu

STRATEGIES = (("multiple_opt", "edit", "dynamic", 4), ("columba", "edit", "dynamic", 7), ("kuch1", "hamming", "dynamic", 2),
              ("pigeon", "edit", "uniform", 1), ("multiple_opt", "edit", "dynamic", 0))
# (suffix-array sparseness, seed size, sparse locate): every value of each on every world; 16 and 10 exceed the smallest texts
VARIANTS = ((1, 4, False), (4, 10, True), (16, 4, True), (16, 10, False))
COUNTERS = ("NODE_COUNTER", "IN_TEXT_STARTED", "MATRIX_ROWS", "CIGARS_IN_TEXT_VERIFICATION", "EXPANSIONS")
# every world of tests/tinytexts.py: each length with one sequence, and with three where n >= 200
WORLDS = tuple((n, three) for n in tt.LENGTHS for three in ((False, True) if n >= 200 else (False,)))


@pytest.fixture(scope="module")
def op(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py
    return oracle_py


def _ost(op, spec, metric, partition):
    import schemes_py as sp
    return op.OracleStrategy(sp.BY_NAME[spec], metric, partition)


def _without_empty_under_hamming(reads, metric):
    """The empty read under Hamming distance is outside what the reference defines: its naive backtracking
    (indexinterface.cpp:1143-1209) writes `vec[1]` of a one-element vector and reads `pattern[size - 1]` of an empty pattern for
    every character whose range is wider than the switch point, and reports a zero-width occurrence per suffix for the others —
    so on texts of a few characters the oracle lists zero-width occurrences, on larger ones nothing.  The device reports nothing
    for it on any text (asserted where this is used); chunks compared with the oracle under Hamming distance leave it out."""
    return [r for r in reads if r] if metric == "hamming" else reads


def _tuples(occ, offs, i, fields=("begin", "end", "distance")):
    return [tuple(int(occ[f][j]) for f in fields) for j in range(int(offs[i]), int(offs[i + 1]))]


def _assert_parity(o, d, k, reads, where):
    (o_occ, o_off, o_cnt), (d_occ, d_off, d_cnt) = o, d
    assert np.array_equal(o_off, d_off), where
    if k == 0:  # (exact matches: suffix-array order in the reference, sorted by the C-ABI)
        for i in range(len(reads)):
            assert sorted(_tuples(o_occ, o_off, i)) == sorted(_tuples(d_occ, d_off, i)), (where, i, reads[i])
    else:
        for f in ("begin", "end", "distance"):
            if not np.array_equal(o_occ[f], d_occ[f]):
                i = next(i for i in range(len(reads)) if _tuples(o_occ, o_off, i) != _tuples(d_occ, d_off, i))
                raise AssertionError((where, f, reads[i], _tuples(o_occ, o_off, i), _tuples(d_occ, d_off, i)))
    for c in COUNTERS + (("ABORTED_IN_TEXT_VERIF",) if k else ()):
        assert o_cnt[c] == d_cnt[c], (where, c, o_cnt[c], d_cnt[c])


@pytest.mark.parametrize("n", tt.LENGTHS)
@pytest.mark.parametrize("kind", tt.KINDS)
def test_fm_search_equals_the_oracle(op, kind, n):
    text = tt.text_of(kind, n)
    records = beyond = 0
    for three in ((False, True) if n >= 200 else (False,)):
        for sparseness, kmer, sparse_locate in (VARIANTS[:2] if three else VARIANTS):
            ix = ib.build_index(text, sparseness=sparseness, seq_starts=tt.seq_starts(n, three), device="cuda")
            dev, orc = _index(ix, sparse=sparse_locate, kmer_size=kmer), op.OracleIndex(ix, kmer_size=kmer)
            try:
                for spec, metric, partition, k in STRATEGIES:
                    reads = _without_empty_under_hamming(tt.world_reads(text, k, seed=n + k), metric)
                    assert len(reads) <= 300
                    o = op.match_batch(orc, _ost(op, spec, metric, partition), k, reads, threads=8)
                    st = ca.SearchStrategy(spec, metric, partition)
                    d = ca.match_batch(dev, st, k, reads)
                    if metric == "hamming":  # (the device reports nothing for the empty read, alone or between other reads)
                        e_occ, e_off, _ = ca.match_batch(dev, st, k, [b"", reads[-1], b""])
                        assert e_off[1] == e_off[0] and e_off[3] == e_off[2], (kind, n, e_off)
                        assert _tuples(e_occ, e_off, 1) == _tuples(d[0], d[1], len(reads) - 1)
                    st.close()
                    _assert_parity(o, d, k, reads, (kind, n, three, sparseness, kmer, sparse_locate, spec, k))
                    records += len(d[0])
                    beyond += int((d[0]["end"] > n).sum())
            finally:
                dev.close()
    print(f"{kind} n={n}: {records} records identical to the oracle's, {beyond} of them end beyond the text")
    assert records > 0


@pytest.mark.parametrize("n", (64, 257, 1000))
@pytest.mark.parametrize("kind", tt.KINDS)
def test_device_lists_are_sound_and_complete(op, gt, kind, n):
    """the judge of tests/tinytexts.py on what the device returns: FM index with the default switch point and with 0 (no in-text
    verification), and the b-move index"""
    text = tt.text_of(kind, n)
    ix = ib.build_index(text, sparseness=4, seq_starts=tt.seq_starts(n), device="cuda")
    assert tt.move_text(text) == text
    backends = [("fm", ca.Index(ix, kmer_size=4)), ("fm switch 0", ca.Index(ix, in_text_switch=0, kmer_size=4)),
                ("b-move", ca.MoveIndex(movebuild.build_move(text)))]
    try:
        for name, dev in backends:
            for spec, k, length in SHAPES:
                if n <= length + 8:
                    continue
                reads = tt.sampled_reads(text, 40, length, k, seed=n + k)
                st = ca.SearchStrategy(spec, "edit", "dynamic")
                if name == "b-move":
                    occ, offs, _ = dev.match_batch(st, k, reads, kmer_size=4)
                else:
                    occ, offs, _ = ca.match_batch(dev, st, k, reads)
                st.close()
                assert tt.beyond_text(text, reads, occ, offs, k, spec) == []
                checked, _ = tt.check_soundness_pinned(gt, text, reads, occ, offs, k, "edit", spec)
                judged, exempt, misses = tt.check_completeness(gt, text, reads, occ, offs, k)
                print(f"{kind} n={n} {name} {spec} k={k} L={length}: {len(occ)} records, {judged} ends judged, {exempt} exempt "
                      f"({100.0 * exempt / judged:.1f} %), {len(misses)} misses")
                assert misses == [], misses[:5]
                assert judged - exempt >= 50 and checked == len(occ)
    finally:
        for _, dev in backends:
            dev.close()


@pytest.mark.parametrize("spec,k", [("columba", 4), ("columba", 7), ("columba", 10), ("multiple_opt", 4), ("kuch1", 2)])
def test_device_alignments_over_a_text_end(op, spec, k):
    """F1 of tests/test_tiny_texts.py on the device: found by in-text verification, lost with switch point 0 and on b-move"""
    n = 3000
    text = tt.text_of("random", n)
    ix = ib.build_index(text, seq_starts=tt.seq_starts(n), device="cuda")
    reads, want = f1_reads(text, k)
    st = ca.SearchStrategy(spec, "edit", "dynamic")
    backends = [("fm", ca.Index(ix)), ("fm switch 0", ca.Index(ix, in_text_switch=0)), ("b-move", ca.MoveIndex(movebuild.build_move(text)))]
    try:
        for name, dev in backends:
            occ, offs, cnt = dev.match_batch(st, k, reads) if name == "b-move" else ca.match_batch(dev, st, k, reads)
            assert (cnt["IN_TEXT_STARTED"] > 0) == (name == "fm")
            for i, w in enumerate(want):
                recs = _tuples(occ, offs, i, ("begin", "end", "distance", "strand"))
                if name == "fm" or w[2] == 0:
                    assert w in recs, (name, w, recs)
                else:
                    assert recs == [], (name, w, recs)
    finally:
        st.close()
        for _, dev in backends:
            dev.close()


def test_device_reports_the_pinned_occurrence_beyond_the_text(op):
    """F2 of tests/test_tiny_texts.py on the device: the same six records, the last one ending at 64 of 60; its CIGAR is read from
    the text's padding, and the SAM writers trim it at the end of the sequence as the oracle does"""
    pin = tt.F2_PIN
    text, n = pin["text"], len(pin["text"])
    ix = ib.build_index(text, sparseness=1, seq_starts=tt.seq_starts(n), device="cuda")
    orc = op.OracleIndex(ix, kmer_size=4)
    st = ca.SearchStrategy(pin["spec"], "edit", "dynamic")
    for sparse_locate in (False, True):
        dev = _index(ix, sparse=sparse_locate, kmer_size=4)
        b = ca.Batch(dev, st, pin["k"], [pin["read"]])
        try:
            b.want_alignments()
            b.run()
            occ, offs, _ = b.results()
            assert _tuples(occ, offs, 0, ("begin", "end", "distance", "strand")) == pin["records"]
            aln, _ = b.alignments()
            assert aln["spans"].tolist() == [0, 0, 0, 0, 0, 1]
            host = b.sam(["@r"], ["I" * 12], ["s1"])
            got, host_reads = b.sam_device(["@r"], ["I" * 12], ["s1"])
            _same(got, host)
            assert host_reads == 1
            want = op.match_batch_sam(orc, _ost(op, pin["spec"], "edit", "dynamic"), pin["k"], [pin["read"]], ["@r"], ["I" * 12], ["s1"])
            assert got == want
        finally:
            b.close()
            dev.close()
    st.close()


def _chunk(text, k, seed, metric):
    reads = _without_empty_under_hamming(tt.world_reads(text, k, seed=seed, per_length=6), metric)
    rng = np.random.default_rng(seed)
    ids = [("@" if i % 2 else ">") + f"r{i}/1 tiny" for i in range(len(reads))]
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    return reads, ids, quals


@pytest.mark.parametrize("spec,metric,k,xa", [("columba", "edit", 4, False), ("multiple_opt", "edit", 2, True), ("kuch1", "hamming", 2, False),
                                              ("kuch1", "edit", 0, False)])
@pytest.mark.parametrize("kind", tt.KINDS)
def test_sam_text_of_host_device_and_oracle(op, kind, spec, metric, k, xa):
    for n, three in WORLDS:
        text = tt.text_of(kind, n)
        starts = tt.seq_starts(n, three)
        names = [f"s{j + 1}" for j in range(len(starts) - 1)]
        ix = ib.build_index(text, sparseness=4, seq_starts=starts, device="cuda")
        dev, orc = ca.Index(ix, kmer_size=4), op.OracleIndex(ix, kmer_size=4)
        reads, ids, quals = _chunk(text, k, n + k, metric)
        st = ca.SearchStrategy(spec, metric, "dynamic")
        b = ca.Batch(dev, st, k, reads)
        try:
            b.want_alignments()
            b.run()
            for unmapped in (True, False):
                host = b.sam(ids, quals, names, unmapped=unmapped, xa=xa)
                got, host_reads = b.sam_device(ids, quals, names, unmapped=unmapped, xa=xa)
                _same(got, host)
                want = op.match_batch_sam(orc, _ost(op, spec, metric, "dynamic"), k, reads, ids, quals, names, unmapped=unmapped, xa=xa)
                gl, wl = got.splitlines(), want.splitlines()
                if k == 0:
                    gl, wl = _norm_k0(gl), _norm_k0(wl)
                for a, x in zip(gl, wl):
                    assert a == x, (kind, n, a, x)
                assert len(gl) == len(wl)
            print(f"{kind} n={n} {spec} {metric} k={k}: {len(reads)} reads, {len(gl)} lines, host_reads={host_reads}")
        finally:
            b.close()
            st.close()
            dev.close()


@pytest.mark.parametrize("spec,metric,x,min_identity", [("columba", "edit", 0, 90), ("columba", "edit", 1, 95), ("kuch1", "hamming", 0, 90)])
@pytest.mark.parametrize("kind", tt.KINDS)
def test_best_mode_of_host_device_and_oracle(op, kind, spec, metric, x, min_identity):
    import schemes_py as sp
    max_sup = 0
    while (max_sup + 1) in sp.BY_NAME[spec]["schemes"]:
        max_sup += 1
    max_sup = min(max_sup, 13)
    for n, three in WORLDS:
        text = tt.text_of(kind, n)
        starts = tt.seq_starts(n, three)
        names = [f"s{j + 1}" for j in range(len(starts) - 1)]
        ix = ib.build_index(text, sparseness=4, seq_starts=starts, device="cuda")
        dev, orc = ca.Index(ix, kmer_size=4), op.OracleIndex(ix, kmer_size=4)
        reads, ids, quals = _chunk(text, 3, n + x, metric)
        st = ca.SearchStrategy(spec, metric, "dynamic")
        try:
            host = ca.match_best(dev, st, reads, x=x, min_identity=min_identity)
            got = ca.match_best_device(dev, st, reads, x=x, min_identity=min_identity)
            _assert_same(host, got)
            d_occ, d_aln, d_ops, d_off, d_best, d_hits, d_cnt, flagged = got
            o_occ, o_sid, o_sb, o_cig, o_off, o_best, o_hits, o_cnt = op.match_best(
                orc, _ost(op, spec, metric, "dynamic"), reads, x=x, min_identity=min_identity, max_supported=max_sup, threads=8)
            assert np.array_equal(o_best, d_best) and np.array_equal(o_hits, d_hits) and np.array_equal(o_off, d_off), (kind, n)
            for f in ("begin", "end", "distance", "strand"):
                assert np.array_equal(o_occ[f], d_occ[f]), (kind, n, f)
            assert np.array_equal(o_sid, d_aln["seq_id"]) and np.array_equal(o_sb, d_aln["seq_begin"])
            for j in range(len(d_occ)):
                a = d_aln[j]
                assert ca.cigar_string(d_ops[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["cigar_len"])]) == o_cig[j], (kind, n, j, d_occ[j])
            for c in ("NODE_COUNTER", "IN_TEXT_STARTED", "SEARCH_STARTED", "EXPANSIONS", "IMMEDIATE_SWITCH"):
                assert o_cnt[c] == d_cnt[c], (kind, n, c, o_cnt[c], d_cnt[c])
            text_dev, host_reads = ca.best_sam_device(dev, st, reads, ids, quals, names, x=x, min_identity=min_identity, xa=bool(x))
            _same(text_dev, _sam_of_best(host, reads, ids, quals, names, True, bool(x)))
            assert host_reads == int(flagged.sum())
            print(f"{kind} n={n} {spec} {metric} x={x} identity={min_identity}: {len(d_occ)} records, host_reads={host_reads}")
        finally:
            st.close()
            dev.close()


def test_read_pairs_on_a_tiny_text_of_three_sequences(op):
    """pair_chunk_sam = pair_chunk_sam_device: pairs whose fragment is the whole text (the mates lie in different sequences),
    a whole sequence, inside one sequence, over a sequence end; pairs with one and with no mate mapped"""
    n, k = 257, 2
    text = tt.text_of("random", n)
    starts = tt.seq_starts(n, True)
    names = ["s1", "s2", "s3"]
    ix = ib.build_index(text, sparseness=4, seq_starts=starts, device="cuda")
    dev = ca.Index(ix, kmer_size=4)
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    rng = np.random.default_rng(9)
    s1, s2 = int(starts[1]), int(starts[2])
    frags = [(0, n), (s1, s2), (s1 + 10, s2 - 10), (0, s1), (s2, n), (s1 - 30, s1 + 60), (5, n - 5), (s2 - 20, n)]
    try:
        for orientation in (ca.ORIENTATION_FR, ca.ORIENTATION_RF, ca.ORIENTATION_FF):
            r1, r2 = [], []
            for length in (20, 40):
                for b, e in frags:
                    up, down = text[b:b + length], text[e - length:e]
                    for swapped in (False, True):
                        if orientation == ca.ORIENTATION_FR:
                            a, c = up, synth.revcomp(down)
                        elif orientation == ca.ORIENTATION_RF:
                            a, c = synth.revcomp(up), down
                        else:
                            a, c = (synth.revcomp(down), synth.revcomp(up)) if swapped else (up, down)
                        if swapped and orientation != ca.ORIENTATION_FF:
                            a, c = c, a
                        r1.append(a)
                        r2.append(c)
                # one substitution in a mate; one mate unmapped; no mate mapped; an empty mate
                sub = bytearray(text[s1:s1 + length])
                sub[length // 2] = ord("A") if sub[length // 2] != ord("A") else ord("C")
                r1 += [bytes(sub), text[s1:s1 + length], tt.junk(rng, length), b""]
                r2 += [synth.revcomp(text[s2 - length:s2]), tt.junk(rng, length), tt.junk(rng, length), text[:length]]
            ids1 = [f"@p{i}/1 x" for i in range(len(r1))]
            ids2 = [f"@p{i}/2 x" for i in range(len(r2))]
            q1 = ["I" * len(r) for r in r1]
            q2 = ["5" * len(r) for r in r2]
            for max_frag in (500, 120):
                host, mapped = ca.pair_chunk_sam(dev, st, k, r1, r2, ids1, ids2, q1, q2, names, orientation, max_frag=max_frag)
                got, mapped_d, stats = ca.pair_chunk_sam_device(dev, st, k, r1, r2, ids1, ids2, q1, q2, names, orientation, max_frag=max_frag)
                _same(got, host)
                assert mapped == mapped_d and mapped > 0
                print(f"orientation {orientation} max_frag {max_frag}: {len(r1)} pairs, {mapped} mapped, {stats}")
    finally:
        st.close()
        dev.close()


@pytest.mark.parametrize("kind", tt.KINDS)
def test_bmove_search_sam_and_best_on_tiny_texts(op, kind):
    """the b-move search against the oracle's b-move search (lists, NODE_COUNTER, EXPANSIONS), `MoveBatch.sam` =
    `MoveBatch.sam_device` from the kept device lists, `match_best` = `match_best_device` — texts of 16 characters and more
    (below, the oracle itself refuses searches that meet the wrapped toehold of bmove.cpp:262)"""
    for n, three in ((16, False), (17, False), (65, False), (257, True), (1000, True)):
        text = tt.move_text(tt.text_of(kind, n))
        starts = tt.seq_starts(n, three)
        starts[-1] = len(text)
        names = [f"s{j + 1}" for j in range(len(starts) - 1)]
        mv = movebuild.build_move(text)
        dev, orc = ca.MoveIndex(mv), op.OracleMoveIndex(mv)
        dev.attach_text(text, starts)
        try:
            for spec, metric, partition, k in STRATEGIES:
                reads = _without_empty_under_hamming(tt.world_reads(text, k, seed=n + k, per_length=6), metric)
                kmer = 4 if k % 2 == 0 else 10
                o_occ, o_off, o_cnt = orc.match_batch(_ost(op, spec, metric, partition), k, reads, threads=8, word_size=kmer)
                st = ca.SearchStrategy(spec, metric, partition)
                b = ca.MoveBatch(dev, st, k, reads=reads, kmer_size=kmer)
                try:
                    b.want_alignments()
                    b.keep_device_lists()
                    b.run()
                    d_occ, d_off, d_cnt = b.results()
                    where = (kind, n, spec, metric, k)
                    assert np.array_equal(o_off, d_off), where
                    for i in range(len(reads)):
                        a, c = _tuples(o_occ, o_off, i), _tuples(d_occ, d_off, i)
                        if k == 0:  # (exact matches: the order they were located in)
                            a, c = sorted(a), sorted(c)
                        assert a == c, (where, reads[i], a, c)
                    for c in ("NODE_COUNTER", "EXPANSIONS"):
                        assert o_cnt[c] == d_cnt[c], (where, c, o_cnt[c], d_cnt[c])
                    ids = [f"@m{i} x" for i in range(len(reads))]
                    quals = ["F" * len(r) for r in reads]
                    for unmapped in (True, False):
                        host = b.sam(ids, quals, names, unmapped=unmapped, xa=(k == 4), metric=metric)
                        got, host_reads = b.sam_device(ids, quals, names, unmapped=unmapped, xa=(k == 4))
                        _same(got, host)
                finally:
                    b.close()
                    st.close()
            reads = tt.world_reads(text, 3, seed=n, per_length=6)
            st = ca.SearchStrategy("columba", "edit", "dynamic")
            for x in (0, 1):
                _assert_same(ca.match_best(dev, st, reads, x=x, min_identity=90, kmer_size=4),
                             ca.match_best_device(dev, st, reads, x=x, min_identity=90, kmer_size=4))
            st.close()
            print(f"{kind} n={n}: b-move lists identical to the oracle's, SAM text and BEST mode identical on host and device paths")
        finally:
            dev.close()


def _move_texts():
    import soak_move_tiny as smt
    return list(smt.texts(np.random.default_rng(11), 24))


@pytest.mark.parametrize("i", range(7 + 24))
def test_bmove_backend_on_tiny_texts(op, i):
    """tools/soak_move_tiny.py in the suite: rows of both tables, every extension of three walks, locate of every range met,
    toeholds outside the text refused, exact matching — device against oracle"""
    import soak_move_tiny as smt
    text = _move_texts()[i]
    children, located, exact = smt.one_text(text, np.random.default_rng(100 + i))
    print(f"text {i} ({len(text)} characters): {children} children, {located} ranges located, {exact} exact occurrences")
    assert children > 0 and exact > 0
