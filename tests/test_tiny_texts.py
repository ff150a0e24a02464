"""The CPU oracle on tiny, low-complexity texts and at the two ends of a text, against plain dynamic programming.

The ground-truth layer (tests/test_ground_truth.py and its siblings) runs on texts of 120 000 characters and more and reaches
a text end only through `text[:100]` / `text[-100:]`.  Here the texts have 64 ... 3 000 characters (tests/tinytexts.py), and
three things are held:

  F3  away from the text ends the completeness rule holds exactly (zero misses, no chain rule), with and without in-text
      verification, on all six kinds of text; every configuration prints (ends judged, ends exempt, misses);
  F1  at a text end the in-index search loses every alignment that hangs over the end, in-text verification finds it: pinned as
      the reference does it (indexinterface.cpp:506-526, :544-560);
  F2  the reference reports occurrences that end beyond the text (stale ranges of descendants after a direction switch,
      indexinterface.cpp:468-478 with :486-487, indexhelpers.h:1743-1761, indexinterface.cpp:1410-1416): the reproducer is pinned,
      and the judge fails every other record outside [0, n].
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from columba_amd import indexbuild as ib, movebuild, synth  # noqa: E402
import tinytexts as tt  # noqa: E402
from test_ground_truth import gt  # noqa: E402,F401

# (spec, k, read length) of F3: L >= 5k/2 everywhere.  Other shapes are not judged: at L = 12 and 30 with k = 4 ... 7 roughly
# 1 of 500 occurrences of the oracle ends beyond the text (F2).
SHAPES = (("columba", 2, 20), ("multiple_opt", 4, 36), ("columba", 7, 60))


@pytest.fixture(scope="module")
def op(oracle_built):
    import oracle_py
    return oracle_py


def _strategy(op, spec, metric="edit", partition="dynamic"):
    import schemes_py as sp
    return op.OracleStrategy(sp.BY_NAME[spec], metric, partition)


@pytest.mark.parametrize("n", (64, 257, 1000))
@pytest.mark.parametrize("kind", tt.KINDS)
def test_oracle_is_complete_away_from_the_text_ends(op, gt, kind, n):
    text = tt.text_of(kind, n)
    ix = ib.build_index(text, sparseness=4, seq_starts=tt.seq_starts(n), device="cpu")
    for switch in (4, 0):
        orc = op.OracleIndex(ix, kmer_size=4, switch_point=switch)
        for spec, k, length in SHAPES:
            if n <= length + 8:
                continue
            reads = tt.sampled_reads(text, 40, length, k, seed=n + k)
            occ, offs, _ = op.match_batch(orc, _strategy(op, spec), k, reads, threads=4)
            assert tt.beyond_text(text, reads, occ, offs, k, spec) == []
            checked, _ = tt.check_soundness_pinned(gt, text, reads, occ, offs, k, "edit", spec)
            judged, exempt, misses = tt.check_completeness(gt, text, reads, occ, offs, k)
            print(f"{kind} n={n} switch={switch} {spec} k={k} L={length}: {len(occ)} records, {judged} ends judged, "
                  f"{exempt} exempt ({100.0 * exempt / judged:.1f} %), {len(misses)} misses")
            assert misses == [], misses[:5]
            assert judged - exempt >= 50 and checked == len(occ)


@pytest.fixture(scope="module")
def f1_world(op):
    n = 3000
    text = tt.text_of("random", n)
    ix = ib.build_index(text, seq_starts=tt.seq_starts(n), device="cpu")
    return {"text": text, "n": n, "default": op.OracleIndex(ix), "switch0": op.OracleIndex(ix, switch_point=0),
            "move": op.OracleMoveIndex(movebuild.build_move(text))}


def f1_reads(text, k):
    """(reads, the record each read has if its overhanging alignment is found) for o = 0 ... k, L = 40 and 100, both strands"""
    n = len(text)
    reads, want = [], []
    for length in (40, 100):
        for o in range(k + 1):
            a, b = tt.overhang_reads(text, length, o, seed=100 * length + o)
            for r, (begin, end) in ((a, (n - (length - o), n)), (b, (0, length - o))):
                reads += [r, synth.revcomp(r)]
                want += [(begin, end, o, 0), (begin, end, o, 1)]
    return reads, want


@pytest.mark.parametrize("spec,k", [("columba", 4), ("columba", 7), ("columba", 10), ("multiple_opt", 4), ("kuch1", 2)])
def test_alignments_over_a_text_end_need_in_text_verification(op, f1_world, spec, k):
    """F1.  A read whose last (first) o characters hang over the end (begin) of the text aligns with the text's last (first)
    L - o characters at distance o.  In-text verification clamps its window to the text and finds it.  The in-index search does
    not: `goDeeper` is called only from `branchAndBound` when `!validED || onlyVerticalGapsLeft(row)`
    (indexinterface.cpp:544-560), and the loop over the stack (:506-526) ends silently when the node on the last character of
    the text has no children, so the cluster that holds the alignment is never reported.  The b-move flavour has no in-text
    verification (indexinterface.cpp:345-348) and always behaves like switch point 0."""
    text = f1_world["text"]
    reads, want = f1_reads(text, k)
    st = _strategy(op, spec)

    def lists(occ, offs):
        return [[tuple(int(x) for x in r) for r in occ[int(offs[i]):int(offs[i + 1])]] for i in range(len(reads))]

    occ, offs, cnt = op.match_batch(f1_world["default"], st, k, reads, threads=4)
    assert cnt["IN_TEXT_STARTED"] > 0
    assert tt.beyond_text(text, reads, occ, offs, k, spec) == []
    for recs, w in zip(lists(occ, offs), want):
        assert w in recs, (w, recs)
    for name in ("switch0", "move"):
        if name == "move":
            occ, offs, cnt = f1_world["move"].match_batch(st, k, reads, threads=4)
        else:
            occ, offs, cnt = op.match_batch(f1_world[name], st, k, reads, threads=4)
        assert cnt["IN_TEXT_STARTED"] == 0
        lost = 0
        for recs, w in zip(lists(occ, offs), want):
            if w[2] == 0:
                assert w in recs, (name, w, recs)
            else:
                assert recs == [], (name, w, recs)
                lost += 1
        assert lost == 8 * k


def test_occurrence_beyond_the_text_is_the_pinned_one(op, gt):
    """F2.  After a direction switch the reference walks the descendants of the earlier phase in this direction with the ranges
    they had THEN (indexinterface.cpp:468-478; only the last one's range is replaced for the extension, :486-487), stores them
    in the cluster (:546-548), and `reportCentersAtEnd` (indexhelpers.h:1743-1761) reports such a node with the depth of the
    current start match plus its row: a range of suffixes that were never extended by the characters of the phases in between.
    The conversion to text occurrences (indexinterface.cpp:1410-1416) only asserts `startPos < textLength`.  On polyA every
    suffix of 5 characters or more is in such a range, and the occurrence of depth 9 at position 55 of 60 ends at 64."""
    pin = tt.F2_PIN
    text, n = pin["text"], len(pin["text"])
    ix = ib.build_index(text, sparseness=1, seq_starts=tt.seq_starts(n), device="cpu")
    for switch in (4, 0):
        orc = op.OracleIndex(ix, kmer_size=4, switch_point=switch)
        occ, offs, _ = op.match_batch(orc, _strategy(op, pin["spec"]), pin["k"], [pin["read"]], threads=1)
        assert [tuple(int(x) for x in r) for r in occ] == pin["records"]
        assert tt.beyond_text(text, [pin["read"]], occ, offs, pin["k"], pin["spec"]) == []
        # every record inside the text is a true alignment; the pinned one alone is let through
        checked, _ = tt.check_soundness_pinned(gt, text, [pin["read"]], occ, offs, pin["k"], "edit", pin["spec"])
        assert checked == len(pin["records"]) - 1
        # ... and only in exactly this setting: the same list under another k, or a record moved by one, fails the judge
        assert len(tt.beyond_text(text, [pin["read"]], occ, offs, pin["k"] + 1, pin["spec"])) == 1
        moved = occ.copy()
        moved["end"][-1] += 1
        assert len(tt.beyond_text(text, [pin["read"]], moved, offs, pin["k"], pin["spec"])) == 1
        with pytest.raises(AssertionError):
            tt.check_soundness_pinned(gt, text, [pin["read"]], moved, offs, pin["k"], "edit", pin["spec"])


def test_the_judge_sees_a_lost_interior_record_and_exempts_the_text_ends(op, gt):
    n, k, length, spec = 1000, 4, 36, "multiple_opt"
    text = tt.text_of("random", n)
    ix = ib.build_index(text, sparseness=4, seq_starts=tt.seq_starts(n), device="cpu")
    reads = [text[400:400 + length], text[n - length:], text[:length]]
    occ, offs, _ = op.match_batch(op.OracleIndex(ix, kmer_size=4), _strategy(op, spec), k, reads, threads=1)
    recs = [tuple(int(x) for x in r) for r in occ]
    assert recs == [(400, 400 + length, 0, 0), (n - length, n, 0, 0), (0, length, 0, 0)]
    judged, exempt, misses = tt.check_completeness(gt, text, reads, occ, offs, k)
    print(f"judge: three exact reads on random n={n}, k={k}: {judged} ends judged, {exempt} exempt ({100.0 * exempt / judged:.1f} %), "
          f"{len(misses)} misses")
    assert misses == [] and judged > exempt > 0
    # the interior record: every end within k of its end is a truth end that nothing else covers
    occ1, offs1 = tt.drop_record(occ, offs, 0)
    assert len(occ1) == 2 and offs1.tolist() == [0, 0, 1, 2]
    _, exempt1, misses1 = tt.check_completeness(gt, text, reads, occ1, offs1, k)
    assert exempt1 == exempt and (0, 0, 400 + length, 0) in misses1 and all(m[0] == 0 for m in misses1)
    # the record at the end of the text, and the one at its begin: their truth ends are exempt (j >= n - 2k; Sellers begin <= 2k)
    for j in (1, 2):
        occ2, offs2 = tt.drop_record(occ, offs, j)
        _, exempt2, misses2 = tt.check_completeness(gt, text, reads, occ2, offs2, k)
        assert exempt2 == exempt and misses2 == []
    # the exemption ends 2k from the text ends: a record that ends 2k + 1 before the end of the text is missed
    reads3 = [text[n - length - 2 * k - 1:n - 2 * k - 1], text[2 * k + 1:2 * k + 1 + length]]
    occ3, offs3, _ = op.match_batch(op.OracleIndex(ix, kmer_size=4), _strategy(op, spec), k, reads3, threads=1)
    judged3, exempt3, misses3 = tt.check_completeness(gt, text, reads3, occ3, offs3, k)
    print(f"judge: two reads 2k + 1 from the text ends: {judged3} ends judged, {exempt3} exempt ({100.0 * exempt3 / judged3:.1f} %), "
          f"{len(misses3)} misses")
    assert misses3 == []
    for j, end in ((0, n - 2 * k - 1), (1, 2 * k + 1 + length)):
        occ4, offs4 = tt.drop_record(occ3, offs3, j)
        assert (j, 0, end, 0) in tt.check_completeness(gt, text, reads3, occ4, offs4, k)[2]
    assert tt.exempt(n, k, n - 2 * k, 500) and not tt.exempt(n, k, n - 2 * k - 1, 2 * k + 1) and tt.exempt(n, k, 500, 2 * k)


@pytest.mark.parametrize("kind", tt.KINDS)
def test_oracle_on_every_tiny_world_stays_inside_the_text(op, gt, kind):
    """every length of tests/tinytexts.py, one sequence and three, sparseness and seed size larger than the text: the oracle's
    lists are sound and stay inside [0, n] at the judged shapes (reads longer than the text are built from its repetitions)"""
    total = 0
    for n in tt.LENGTHS:
        text = tt.text_of(kind, n)
        for three in ((False, True) if n >= 200 else (False,)):
            ix = ib.build_index(text, sparseness=16, seq_starts=tt.seq_starts(n, three), device="cpu")
            orc = op.OracleIndex(ix, kmer_size=10)
            for spec, k, length in SHAPES:
                if n > length + 8:
                    reads = tt.sampled_reads(text, 6, length, k, seed=n + k, extra_random=2)
                else:
                    reads = [(text * (length // n + 2))[j:j + length] for j in range(min(n, 4))] + [tt.junk(np.random.default_rng(n), length)]
                reads += [text[:length], text[-length:], b"", b"N" * length]
                occ, offs, _ = op.match_batch(orc, _strategy(op, spec), k, reads, threads=4)
                assert tt.beyond_text(text, reads, occ, offs, k, spec) == [], (n, three, spec)
                total += tt.check_soundness_pinned(gt, text, reads, occ, offs, k, "edit", spec)[0]
    assert total > 100
