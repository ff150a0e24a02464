"""Read pairs that start from the inference phase — the path a default paired run takes first: the first chunk matched single-end, orientation
and insert bounds inferred from the pairs whose mates both map unambiguously, the chunk then paired from those single-end results
(cmb_pair_best_seed) — held to plain dynamic programming and to what was planted (tests/pairtruth.py): no occurrence array, no oracle
result and no second reading of the reference aligner takes part.

The world has places to be wrong in: 120 000 characters of uniform ACGT in two sequences (the second one plays the second reference
file), mates of 80, 100 and 150 characters (cut-offs 4, 5 and 7 at 95 % identity) in one chunk, fragments of 250 ... 450 from both strands,
and eleven classes of twelve pairs each (CLASSES).  A verbatim decoy makes a mate's true place a NON-best stratum; a decoy in the second
file, or a near copy in the first, sets the reference's rule for the sample (one hit in the first file among ALL hits within the cut-off,
parallel.cpp:236-262) apart from "one hit in the best stratum".

Layout, where the text is too short for a 1 kb slot per pair and decoy: the pairs of the classes that must stay out of the sample although
every mate of theirs is unique (`far`, `short_cutoff`) live in the second sequence — a unique pair in the first file IS sampled by the
reference's rule — all others side by side in the first one, fragment after fragment; decoys of the first sequence follow more than 5 kb
after the last fragment that has one, 200 apart; those of the second sequence 500 apart.  Reads of different pairs share nothing, and
before anything else runs the world checks itself: the DP finds exactly the planted locations of every mate, at the planted distances.

What this world showed while the phase still ran in BEST mode at x = 0 (FR, FM-index): read2done wrong in decoy1, both, decoy_file2,
decoy_pair and near_copy; 72 sampled pairs against 36 (decoy1, decoy2, decoy_pair and near_copy wrongly in, decoy_file2 wrongly out);
no proper pair in any pair of decoy1, decoy2, both and decoy_file2 nor in the three short_cutoff pairs whose read 1 has the decoy —
e.g. pair 1 (decoy1): mate 1 at its decoy (first:42430, NM 0) with mate 2 at first:501 as a discordant pair, the true place first:857 at
2 edits never searched; pair 4 (decoy_file2): mate 1 at second:32501, mate 2 at first:24275, TLEN 0.  plain, far, junk, n_mate, near_copy
and decoy_pair paired as they should.
"""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import columba_amd as ca  # noqa: E402
from test_ground_truth import gt  # noqa: E402,F401
import pairtruth  # noqa: E402
import samcheck  # noqa: E402

NAMES = ["first", "second"]
STARTS = [0, 60_000, 120_000]
LENGTHS = (80, 100, 150)
PER_CLASS = 12
CLASSES = ["plain", "decoy1", "decoy2", "both", "decoy_file2", "near_copy", "decoy_pair", "far", "junk", "n_mate", "short_cutoff"]
SAMPLED = {"plain", "decoy_file2", "n_mate"}
IN_SECOND_SEQUENCE = {"far", "short_cutoff"}
WITH_DECOY_IN_FIRST = ("decoy1", "decoy2", "both", "near_copy", "decoy_pair")
MIX2 = ("SI", "SD", "ID", "SS")          # two edits: substitutions, insertions and deletions
MIX4 = ("SSID", "SIDS", "SSSS", "DSIS")  # four edits on 80 characters: the cut-off itself
ORIENTATIONS = [ca.ORIENTATION_FR, ca.ORIENTATION_RF, ca.ORIENTATION_FF]
ORI_NAME = {ca.ORIENTATION_FR: "FR", ca.ORIENTATION_RF: "RF", ca.ORIENTATION_FF: "FF"}
SC_ORI = {ca.ORIENTATION_FR: samcheck.ORIENTATION_FR, ca.ORIENTATION_RF: samcheck.ORIENTATION_RF, ca.ORIENTATION_FF: samcheck.ORIENTATION_FF}
_ori_id = lambda o: ORI_NAME[o]  # noqa: E731


def cutoff(length, min_identity=95):
    """getMaxED (searchstrategy.h:1797-1806) where the strategy supports 13 errors"""
    return min(13, length * (100 - min_identity) // 100)


def _edit(g, p0, length, kinds, rng):
    """(the `length` characters a read shows of the text from p0 on after the edits `kinds` — S substitution, I insertion, D deletion, N an
    N — at least 8 characters from either end and 10 from each other, the width of the text they cover)"""
    ext = bytearray(g[p0:p0 + length + kinds.count("D")].tobytes())
    ne = len(kinds)
    pos = [8 + int((length - 16) * (t + 0.5) / ne) + int(rng.integers(-3, 4)) for t in range(ne)]
    for p, kind in sorted(zip(pos, kinds), reverse=True):
        if kind == "S":
            ext[p] = b"ACGT"[(b"ACGT".index(ext[p]) + int(rng.integers(1, 4))) % 4]
        elif kind == "N":
            ext[p] = ord("N")
        elif kind == "I":
            ext.insert(p, b"ACGT"[int(rng.integers(0, 4))])
        else:
            del ext[p]
    return bytes(ext[:length]), length + kinds.count("D") - kinds.count("I")


_TEXT = {}


def world(orientation, seed=7):
    """the text (the same for every orientation), the reads of the chunk and, per pair and mate, what was planted: [(sequence, strand, begin,
    end, distance, begin and end are exact)] in text coordinates"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, STARTS[-1])].copy()
    n = PER_CLASS * len(CLASSES)
    pairs = []
    for i in range(n):
        cls, j = CLASSES[i % len(CLASSES)], i // len(CLASSES)
        pairs.append({"cls": cls, "j": j, "length": 80 if cls == "short_cutoff" else LENGTHS[j % 3], "frag": int(rng.integers(250, 451)),
                      "swapped": i % 2})
    # homes: the first sequence fragment after fragment, the classes with a decoy there first; the second sequence 1 kb apart
    at = 500
    for p in sorted((p for p in pairs if p["cls"] not in IN_SECOND_SEQUENCE), key=lambda p: p["cls"] not in WITH_DECOY_IN_FIRST):
        p["home"], p["gap"] = at, 0
        at += p["frag"] + 30
        if p["cls"] in WITH_DECOY_IN_FIRST:
            last_with_decoy = at
    slot = {0: at + 200, "frag": 0, 1: 92_000}
    assert slot[0] >= last_with_decoy + 5000
    at = STARTS[1] + 1000
    for p in (p for p in pairs if p["cls"] == "far"):
        p["home"], p["gap"] = at, 5400  # (mates 5 kb apart; the downstream ends lie between the upstream ends of later pairs)
        at += 1000
    at += 6000
    for p in (p for p in pairs if p["cls"] == "short_cutoff"):
        p["home"], p["gap"] = at, 0
        at += 1000
    assert at <= slot[1] - 1000

    def take(where, width=0):
        s = slot[where]
        slot[where] += {0: 200, 1: 500}[where] if not width else width
        return s

    singles_in_first = sum(1 for p in pairs if p["cls"] in ("decoy1", "decoy2", "both", "near_copy"))
    first_frag = slot["frag"] = slot[0] + 200 * singles_in_first + 200
    r1, r2 = [], []
    for i, p in enumerate(pairs):
        cls, j, length, sw = p["cls"], p["j"], p["length"], p["swapped"]
        few = lambda: "S" * int(rng.integers(0, 2))  # noqa: E731
        kinds, decoy = [few(), few()], [None, None]   # per MATE; decoy: the sequence a verbatim copy of the read goes to
        if cls == "plain":
            kinds = ["S" * int(rng.integers(0, 3)), "S" * int(rng.integers(0, 3))]
        elif cls == "decoy1":
            kinds[0], decoy[0] = MIX2[j % 4], 0
        elif cls == "decoy2":
            kinds[1], decoy[1] = MIX2[j % 4], 0
        elif cls == "both":
            kinds, decoy = [MIX2[j % 4], MIX2[(j + 1) % 4]], [0, 1]
        elif cls == "decoy_file2":
            kinds[0], decoy[0] = "SS", 1
        elif cls == "near_copy":
            kinds[0] = ""
        elif cls == "decoy_pair":
            kinds, decoy = [MIX2[j % 4], MIX2[(j + 2) % 4]], ["frag", "frag"]
        elif cls == "n_mate":
            kinds[(j // 2) % 2] = "N" + few()
        elif cls == "short_cutoff":
            e = (j // 2) % 2
            kinds[e] = MIX4[j % 4]
            decoy[e] = 1 if j % 2 == 0 else None
        sid = 1 if cls in IN_SECOND_SEQUENCE else 0
        # (the decoy fragment's ends are two texts of their own: they must not overlap)
        frag_slot = take("frag", int(rng.integers(max(250, 2 * length + 10), 451)) + 50) if cls == "decoy_pair" else None
        reads, planted = [], []
        for m in (0, 1):
            side = m ^ sw  # 0: the upstream end of the fragment, 1: the downstream one
            begin = p["home"] + (p["gap"] + p["frag"] - length if side else 0)
            strand = {ca.ORIENTATION_FR: side, ca.ORIENTATION_RF: 1 - side, ca.ORIENTATION_FF: sw}[orientation]
            piece, width = _edit(g, begin, length, kinds[m], rng)
            here = [(sid, strand, begin, begin + width, len(kinds[m]), not set(kinds[m]) & set("ID"))]
            if cls == "junk" and m == (j // 2) % 2:
                piece, here = bytes(b"ACGT"[int(c)] for c in rng.integers(0, 4, length)), []
            if decoy[m] is not None:
                d = take(decoy[m]) if decoy[m] != "frag" else frag_slot + (slot["frag"] - 50 - frag_slot - length if side else 0)
                g[d:d + length] = np.frombuffer(piece, np.uint8)
                here.append((0 if decoy[m] == "frag" else decoy[m], strand, d, d + length, 0, True))
            if cls == "near_copy" and m == 0:
                d = take(0)
                copy, _ = _edit(g, begin, length, "SS", rng)
                g[d:d + length] = np.frombuffer(copy, np.uint8)
                here.append((0, strand, d, d + length, 2, True))
            reads.append(samcheck.revcomp(piece) if strand else piece)
            planted.append(sorted(here))
        p["planted"] = planted
        r1.append(reads[0])
        r2.append(reads[1])
    assert slot[0] <= first_frag - 200 and slot["frag"] <= STARTS[1] - 500 and slot[1] <= STARTS[2] - 500
    text = g.tobytes()
    assert _TEXT.setdefault(seed, text) == text, "every orientation reads the same text"
    q = np.random.default_rng(5)
    ids1, ids2 = [f"@pair{i}/1 {pairs[i]['cls']}" for i in range(n)], [f"@pair{i}/2 {pairs[i]['cls']}" for i in range(n)]
    q1 = ["".join(chr(33 + int(c)) for c in q.integers(0, 41, len(r))) for r in r1]
    q2 = ["".join(chr(33 + int(c)) for c in q.integers(0, 41, len(r))) for r in r2]
    return {"text": text, "pairs": pairs, "cls": [p["cls"] for p in pairs], "r1": r1, "r2": r2, "ids1": ids1, "ids2": ids2, "q1": q1, "q2": q2,
            "cut": [(cutoff(len(a)), cutoff(len(b))) for a, b in zip(r1, r2)], "orientation": orientation}


def _truth_of(gt, w, k=None):
    """per pair (locations of mate 1, of mate 2) at the mates' cut-offs (or at k)"""
    return [(pairtruth.mate_locations(gt, w["text"], STARTS, a, c1 if k is None else k), pairtruth.mate_locations(gt, w["text"], STARTS, b, c2 if k is None else k))
            for a, b, (c1, c2) in zip(w["r1"], w["r2"], w["cut"])]


def _self_check(w, truth, k=None):
    """the DP finds exactly the planted locations of every mate (those within k where the truth was computed at k)"""
    for i, (p, locs) in enumerate(zip(w["pairs"], truth)):
        for m in (0, 1):
            want = [t for t in p["planted"][m] if k is None or t[4] <= k]
            got = sorted(locs[m], key=lambda l: (l.seq, l.strand, l.begin))
            assert len(got) == len(want), ("locations found and planted", i, p["cls"], m, got, want)
            for l, (sid, strand, b, e, d, exact) in zip(got, want):
                assert (l.seq, l.strand, l.distance) == (sid, strand, d), (i, p["cls"], m, l, want)
                slack = 0 if exact else w["cut"][i][m]
                assert abs(l.begin - b) <= slack and abs(l.end - e) <= slack, (i, p["cls"], m, l, want)


@pytest.fixture(scope="module")
def truths(gt):
    """world and truth per orientation (and per k of an ALL-mode run), computed once and left unchanged"""
    cache = {}

    def get(orientation, k=None):
        if (orientation, k) not in cache:
            w = world(orientation)
            t0 = time.process_time()
            truth = _truth_of(gt, w, k)
            _self_check(w, truth, k)
            print(f"truth of the {ORI_NAME[orientation]} world{'' if k is None else f' at k = {k}'}: {len(truth)} pairs, "
                  f"{time.process_time() - t0:.1f} s of CPU")
            cache[(orientation, k)] = (w, truth)
        return cache[(orientation, k)]
    return get


def _reference(gt, w):
    return samcheck.Reference(w["text"], NAMES, STARTS, gt)


def _judge_best(gt, w, truth, text, orientation, min_frag, max_frag, label):
    t0 = time.perf_counter()
    st, groups = samcheck.check_paired(text, _reference(gt, w), w["r1"], w["r2"], w["ids1"], w["ids2"], w["q1"], w["q2"], limit=w["cut"],
                                       orientation=SC_ORI[orientation], min_frag=min_frag, max_frag=max_frag)
    print(f"{label}: " + ", ".join(f"{k} {v}" for k, v in st.items()) + f" ({time.perf_counter() - t0:.1f} s to check)")
    pairtruth.check_best_pairs(groups, truth, NAMES, STARTS, w["cut"], SC_ORI[orientation], min_frag, max_frag, label=w["cls"])
    return st, groups


# ------------------------------------------------------------------------------------------------ CPU: the judge, the walk, the sample
def _lists(gt, w, truth):
    """occurrence lists written down from the locations: per pair and mate [(Location, CIGAR operations)]"""
    out = []
    for a, b, locs in zip(w["r1"], w["r2"], truth):
        per = []
        for read, ls in ((a, locs[0]), (b, locs[1])):
            fw = samcheck.clean(read)
            items = []
            for l in ls:
                ops, d = pairtruth.traceback_ops(gt, samcheck.revcomp(fw) if l.strand else fw, w["text"][l.begin:l.end])
                assert d == l.distance
                items.append((l, ops))
            per.append(items)
        out.append(per)
    return out


def _arrays(items):
    occ, aln, ops = np.zeros(len(items), ca.OCC_DTYPE), np.zeros(len(items), ca.ALN_DTYPE), []
    for q, (l, o) in enumerate(items):
        occ[q] = (l.begin, l.end, l.distance, l.strand)
        aln[q] = (l.seq, l.begin - STARTS[l.seq], len(ops), len(o), 0, 0)
        ops += o
    return occ, aln, np.asarray(ops, np.uint16)


def _prepared(w):
    mates = []
    for reads, ids, quals in ((w["r1"], w["ids1"], w["q1"]), (w["r2"], w["ids2"], w["q2"])):
        prep = []
        for i in range(len(reads)):
            sid, seq, rc, rq = ca.read_prepare(ids[i], reads[i].decode(), quals[i])
            prep.append((sid, seq, rc, quals[i], rq))
        mates.append(prep)
    return mates


def _walk(w, lists, seeds, read2done, orientation, min_frag, max_frag, disc):
    """cmb_pair_best_* from seeds (host code of the library); the reads 2 that are not done are served from `lists`"""
    mates = _prepared(w)
    pb = ca.PairBest(mates[0], mates[1], 0, 95, 13, orientation, max_frag, min_frag, disc, True)
    for i in range(len(lists)):
        assert (pb.cutoff(i, 0), pb.cutoff(i, 1)) == w["cut"][i]
        pb.seed(i, _arrays(seeds[i][0]), _arrays(seeds[i][1] if read2done[i] else []), read2done[i])
    for _ in range(200):
        req = pb.advance()
        if req.shape[0] == 0:
            break
        for r in req:
            i, m, s, k = int(r["pair"]), int(r["mate"]), int(r["strand"]), int(r["max_distance"])
            assert m == 1 and not read2done[i], "only a read 2 that was not matched is ever searched"
            pb.supply(i, m, s, k, *_arrays([it for it in lists[i][m] if it[0].strand == s and it[0].distance <= k]))
    else:
        raise AssertionError("the walk does not end")
    text = "".join(pb.sam(i, NAMES)[0] for i in range(len(lists)))
    pb.close()
    return text


def _inferred_from(truth, sample):
    s = [(a.begin, a.end, a.strand, b.begin, b.end, b.strand) for a, b in ((next(l for l in truth[i][0] if l.seq < 1), next(l for l in truth[i][1] if l.seq < 1))
                                                                              for i in sample)]
    return ca.pair_infer(s)


def test_sample_truth_on_the_world(truths):
    """by the reference's rule the sample holds exactly the classes plain, decoy_file2 and n_mate — near_copy, unique in its best stratum,
    is out; read 2 counts as done where read 1 has one location in the first file"""
    for orientation in ORIENTATIONS:
        w, truth = truths(orientation)
        sample, done = pairtruth.sample_truth(truth, 1)
        assert {w["cls"][i] for i in sample} == SAMPLED and len(sample) == PER_CLASS * len(SAMPLED)
        done_classes = {c: {done[i] for i in range(len(done)) if w["cls"][i] == c} for c in CLASSES}
        assert all(done_classes[c] == {True} for c in ("plain", "decoy2", "decoy_file2", "n_mate"))
        assert all(done_classes[c] == {False} for c in ("decoy1", "both", "near_copy", "decoy_pair", "far", "short_cutoff"))
        assert done_classes["junk"] == {True, False}  # (the random mate is read 1 in half of them)
        every, _ = pairtruth.sample_truth(truth, 2)   # one reference file: the second sequence counts
        assert {w["cls"][i] for i in every} == {"plain", "n_mate", "far", "short_cutoff"}
        inf = _inferred_from(truth, sample)
        assert inf.orientation == orientation and inf.n_pairs == len(sample)
        assert all(inf.min_insert <= w["pairs"][i]["frag"] <= inf.max_insert for i in sample)


@pytest.mark.parametrize("orientation", ORIENTATIONS, ids=_ori_id)
def test_judge_accepts_the_walk_from_complete_seeds(truths, gt, orientation):
    """seeds that hold every stratum up to the cut-off, read2done by the reference's rule: every class comes out as the DP says"""
    w, truth = truths(orientation)
    lists = _lists(gt, w, truth)
    sample, done = pairtruth.sample_truth(truth, 1)
    inf = _inferred_from(truth, sample)
    lo, hi = int(inf.min_insert), int(inf.max_insert)
    for disc in (True, False):
        text = _walk(w, lists, lists, done, orientation, lo, hi, disc)
        st, _ = _judge_best(gt, w, truth, text, orientation, lo, hi, f"complete seeds, {ORI_NAME[orientation]}, discordant pairs {'' if disc else 'not '}allowed")
        assert st["proper"] >= 2 * PER_CLASS * 9 and st["unmapped"] >= PER_CLASS
        assert (st["discordant"] >= 2 * PER_CLASS and st["unpaired"] == 0) if disc else (st["discordant"] == 0 and st["unpaired"] >= 2 * PER_CLASS)


@pytest.mark.parametrize("orientation", ORIENTATIONS, ids=_ori_id)
def test_judge_rejects_seeds_of_the_best_stratum_only(truths, gt, orientation):
    """the defect: each mate's best stratum as the seed, every stratum counting as looked at — the partner in a non-best stratum is never
    searched.  The judge names pairs of decoy1, decoy2, both and of short_cutoff with a decoy, and nothing of plain."""
    w, truth = truths(orientation)
    lists = _lists(gt, w, truth)
    best = [[[it for it in items if it[0].distance == min(x[0].distance for x in items)] for items in per] for per in lists]
    done = [sum(1 for it in per[0] if it[0].seq < 1) == 1 for per in best]  # "unambiguous" within the best stratum
    sample, _ = pairtruth.sample_truth(truth, 1)
    inf = _inferred_from(truth, sample)
    lo, hi = int(inf.min_insert), int(inf.max_insert)
    text = _walk(w, lists, best, done, orientation, lo, hi, True)
    _, groups = samcheck.check_paired(text, _reference(gt, w), w["r1"], w["r2"], w["ids1"], w["ids2"], w["q1"], w["q2"], limit=w["cut"],
                                      orientation=SC_ORI[orientation], min_frag=lo, max_frag=hi)
    faults = pairtruth.best_pair_faults(groups, truth, NAMES, STARTS, w["cut"], SC_ORI[orientation], lo, hi)
    named = {i for i, _ in faults}
    classes = {w["cls"][i] for i in named}
    print("best-only seeds: faults in", {c: sum(1 for i in named if w["cls"][i] == c) for c in sorted(classes)})
    assert {"decoy1", "decoy2", "both"} <= classes and "plain" not in classes
    assert any(w["cls"][i] == "short_cutoff" and len(truth[i][0]) + len(truth[i][1]) == 3 for i in named)
    assert all(i in named for i in range(len(truth)) if w["cls"][i] in ("decoy1", "decoy2", "both"))
    with pytest.raises(AssertionError):
        pairtruth.check_best_pairs(groups, truth, NAMES, STARTS, w["cut"], SC_ORI[orientation], lo, hi, label=w["cls"])


def test_all_mode_judge_on_lists_built_by_hand(truths, gt):
    """cmb_pair_sam (host code) on the complete lists: every concordant combination is a proper pair and no proper pair lies outside them;
    a dropped concordant pair and an added proper pair outside the combinations are each rejected"""
    orientation = ca.ORIENTATION_FR
    w, truth = truths(orientation)
    lists = _lists(gt, w, truth)
    mates = _prepared(w)
    text = []
    for i, per in enumerate(lists):
        rd = [mates[m][i] + ([(l.seq, l.begin - STARTS[l.seq], l.end - STARTS[l.seq], l.begin, l.distance, l.strand, np.asarray(o, np.uint16)) for l, o in per[m]],)
              for m in (0, 1)]
        text.append(ca.pair_sam(rd[0], rd[1], NAMES, orientation, 600, 100, True, True)[0])
    st, groups = samcheck.check_paired("".join(text), _reference(gt, w), w["r1"], w["r2"], w["ids1"], w["ids2"], w["q1"], w["q2"], limit=w["cut"],
                                       orientation=SC_ORI[orientation], min_frag=100, max_frag=600)
    args = (truth, NAMES, STARTS, w["cut"], SC_ORI[orientation], 100, 600)
    pairtruth.check_all_pairs(groups, *args, label=w["cls"])
    two = next(i for i, c in enumerate(w["cls"]) if c == "decoy_pair")
    assert sum(1 for r in groups[two] if r["flag"] & 2) == 4  # the decoy pair and the true place
    keys = [{samcheck.qname(a), samcheck.qname(b)} for a, b in zip(w["ids1"], w["ids2"])]
    parsed = lambda lines: samcheck._groups(lines, keys, "corrupted")  # noqa: E731
    lines = "".join(text).splitlines()
    mine = [q for q, ln in enumerate(lines) if ln.split("\t")[0] in keys[two]]
    dropped = [ln for q, ln in enumerate(lines) if q not in mine[2:]]  # its second proper pair is gone
    with pytest.raises(AssertionError, match="is not reported"):
        pairtruth.check_all_pairs(parsed(dropped), *args)
    far = next(i for i, c in enumerate(w["cls"]) if c == "far")
    added = list(lines)
    for q, ln in enumerate(lines):
        if ln.split("\t")[0] in keys[far]:
            f = ln.split("\t")
            assert not int(f[1]) & (2 | 4 | 8)
            added[q] = "\t".join([f[0], str(int(f[1]) | 2)] + f[2:])
    with pytest.raises(AssertionError, match="although no two locations of the mates are concordant"):
        pairtruth.check_all_pairs(parsed(added), *args)


# ------------------------------------------------------------------------------------------------ GPU: the drivers
@pytest.fixture(scope="module")
def gpu_world(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from columba_amd import indexbuild as ib, movebuild
    text = world(ca.ORIENTATION_FR)["text"]
    starts = np.asarray(STARTS, np.uint32)
    ix = ib.build_index(text, seq_starts=starts, device="cuda")
    ix.seq_names = NAMES
    mdev = ca.MoveIndex(movebuild.build_move(text, device="cuda"))
    mdev.attach_text(text, starts)
    return {"ix": ix, "dev": ca.Index(ix), "mdev": mdev, "runs": {}}


def _python_layer(gw, gt, w, truth, index, flavour, kmer_size=10):
    """inference phase and seeded walk of the Python layer on one index flavour, every assertion of the issue; returns the texts"""
    orientation = w["orientation"]
    strategy = ca.SearchStrategy("columba", "edit", "dynamic")
    t0 = time.perf_counter()
    inf = ca.infer_paired_end_best(index, strategy, w["r1"], w["r2"], min_identity=95, seqs_in_first_file=1, kmer_size=kmer_size)
    t_inf = time.perf_counter() - t0
    sample, done = pairtruth.sample_truth(truth, 1)
    got = inf["inferred"]
    print(f"{flavour} {ORI_NAME[orientation]}: {inf['unambiguous_pairs']} unambiguous pairs (truth {len(sample)}), orientation {ORI_NAME.get(int(got.orientation))}, "
          f"insert {got.mean_insert:.1f} +- {got.stddev_insert:.1f}, bounds [{got.min_insert}, {got.max_insert}], inference phase {t_inf:.2f} s")
    wrong_done = [(i, w["cls"][i]) for i in range(len(done)) if bool(inf["read2done"][i]) != done[i]]
    assert not wrong_done, ("read2done differs from the truth", wrong_done[:8])
    wrong_sample = [(i, w["cls"][i]) for i in sorted(set(inf["sample"]) ^ set(sample))]
    assert not wrong_sample, ("the sample differs from the truth", wrong_sample[:8])
    assert inf["unambiguous_pairs"] == len(sample)
    rebuilt = []
    for i in sample:
        row = []
        for m, read in ((0, w["r1"][i]), (1, w["r2"][i])):
            occ, aln, _ops = inf["single"][m][i]
            b, e, d, s = int(occ["begin"][0]), int(occ["end"][0]), int(occ["distance"][0]), int(occ["strand"][0])
            fw = samcheck.clean(read)
            win = w["text"][b:e]
            assert gt.gt_edit_distance(samcheck.revcomp(fw) if s else fw, len(fw), win, len(win)) <= d <= w["cut"][i][m], (i, m, b, e, d)
            here = next(l for l in truth[i][m] if l.seq < 1)
            assert (b, e, s, d) == (here.begin, here.end, here.strand, here.distance), ("a sampled alignment away from its planted place", i, w["cls"][i], m)
            sb = int(aln["seq_begin"][0])
            assert int(aln["seq_id"][0]) == 0 and sb == b - STARTS[0]
            row += [sb, sb + e - b, s]
        rebuilt.append(row)
    want = ca.pair_infer(rebuilt)
    fields = [f for f, _ in ca.PairInferred._fields_]
    assert [getattr(got, f) for f in fields] == [getattr(want, f) for f in fields]
    assert got.inferred == 1 and int(got.orientation) == orientation
    lo, hi = int(got.min_insert), int(got.max_insert)
    assert all(lo <= w["pairs"][i]["frag"] <= hi for i in sample)
    texts = {}
    for disc in (True, False):
        t0 = time.perf_counter()
        text, mapped, batches = ca.pair_chunk_sam_best(index, strategy, w["r1"], w["r2"], w["ids1"], w["ids2"], w["q1"], w["q2"], NAMES, x=0, min_identity=95,
                                                       orientation=int(got.orientation), max_frag=hi, min_frag=lo, discordant_allowed=disc,
                                                       kmer_size=kmer_size, start_from=inf)
        print(f"seeded walk: {batches} device batches, {time.perf_counter() - t0:.2f} s")
        _judge_best(gt, w, truth, text, orientation, lo, hi, f"{flavour}, {ORI_NAME[orientation]}, discordant pairs {'' if disc else 'not '}allowed")
        texts[disc] = text
    gw["runs"][(flavour, orientation)] = {"inf": inf, "texts": texts, "bounds": (lo, hi)}
    return gw["runs"][(flavour, orientation)]


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", ORIENTATIONS, ids=_ori_id)
def test_python_layer_from_the_inference_phase(gpu_world, truths, gt, orientation):
    """ca.infer_paired_end_best + ca.pair_chunk_sam_best(start_from=...) on the FM-index: sample, read2done, the sampled alignments, the
    inferred parameters and every pair of every class"""
    w, truth = truths(orientation)
    _python_layer(gpu_world, gt, w, truth, gpu_world["dev"], "FM-index")


@pytest.mark.gpu
def test_bmove_from_the_inference_phase(gpu_world, truths, gt):
    """the same on the b-move index with its text attached; its records equal the FM-index flavour's"""
    w, truth = truths(ca.ORIENTATION_FR)
    run = _python_layer(gpu_world, gt, w, truth, gpu_world["mdev"], "b-move", kmer_size=8)
    fm = gpu_world["runs"].get(("FM-index", ca.ORIENTATION_FR)) or _python_layer(gpu_world, gt, w, truth, gpu_world["dev"], "FM-index")
    assert run["texts"] == fm["texts"] and run["bounds"] == fm["bounds"]


def _cli(tmp_path, gw, w, extra):
    from columba_amd import indexbuild as ib
    from test_cpp_adapter import _build_align
    exe = _build_align(str(tmp_path))
    base = str(tmp_path / "idx")
    ib.save_index(gw["ix"], base)
    np.asarray([0, 1], np.uint32).tofile(base + ".fsid")  # the second sequence is the second reference file
    for name, ids, reads, quals in (("r1.fq", w["ids1"], w["r1"], w["q1"]), ("r2.fq", w["ids2"], w["r2"], w["q2"])):
        (tmp_path / name).write_text("".join(f"{i}\n{r.decode()}\n+\n{q}\n" for i, r, q in zip(ids, reads, quals)))
    out = tmp_path / "o.sam"
    t0 = time.perf_counter()
    run = subprocess.run([exe, "-r", base, "-f", str(tmp_path / "r1.fq"), "-F", str(tmp_path / "r2.fq"), "-o", str(out), "-b", str(len(w["r1"]))] + extra,
                         capture_output=True, text=True, timeout=120)
    print(f"columba_align {' '.join(extra)}: {time.perf_counter() - t0:.2f} s")
    assert run.returncode == 0, run.stderr
    found = re.search(r"Found (\d+) unambiguous pairs while processing (\d+) reads", run.stderr)
    inferred = re.search(r"orientation (FR|RF|FF), insert size ([0-9.e+]+) \+- ([0-9.e+]+), bounds \[(\d+), (\d+)\]", run.stderr)
    assert found and inferred and int(found.group(2)) == 2 * len(w["r1"]), run.stderr
    body = "".join(ln for ln in out.read_text().splitlines(keepends=True) if not ln.startswith("@"))
    return int(found.group(1)), inferred, body


@pytest.mark.gpu
def test_cli_best_mode_from_the_inference_phase(gpu_world, truths, gt, tmp_path):
    """columba_align without -O / -X / -N, the whole world as its first chunk: what it reports equals the Python layer's values, and its
    records pass the judge"""
    w, truth = truths(ca.ORIENTATION_FR)
    n_sample, m, body = _cli(tmp_path, gpu_world, w, ["-I", "95", "-x", "0", "-S", "columba"])
    inf = ca.infer_paired_end_best(gpu_world["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), w["r1"], w["r2"], min_identity=95, seqs_in_first_file=1)
    got = inf["inferred"]
    assert n_sample == inf["unambiguous_pairs"] == len(pairtruth.sample_truth(truth, 1)[0])
    assert (m.group(1), m.group(2), m.group(3), int(m.group(4)), int(m.group(5))) == \
        (ORI_NAME[int(got.orientation)], f"{got.mean_insert:g}", f"{got.stddev_insert:g}", int(got.min_insert), int(got.max_insert)), (m.group(0), got.mean_insert)
    _judge_best(gt, w, truth, body, ca.ORIENTATION_FR, int(m.group(4)), int(m.group(5)), "columba_align, BEST mode")


@pytest.mark.gpu
@pytest.mark.parametrize("spec,k", [("columba", 3), ("multiple_opt", 4)])
def test_cli_all_mode_from_the_inference_phase(gpu_world, truths, gt, tmp_path, spec, k):
    """columba_align -a all -e k: inferPairedEndParametersAll + samOfChunkPairedAll(..., &inference) — the sample's size is the truth's
    at k, every concordant combination within k edits is a proper pair and no proper pair lies outside them.  k = 3 (every decoy is within
    3 edits of its read's true place) runs on the columba schemes: multiple_opt has schemes for 2, 4 and 6 errors only, here as in the
    reference aligner, so it runs at k = 4, where the mates of short_cutoff map as well."""
    w, truth = truths(ca.ORIENTATION_FR, k)
    sample, _ = pairtruth.sample_truth(truth, 1)
    assert {w["cls"][i] for i in sample} == SAMPLED
    n_sample, m, body = _cli(tmp_path, gpu_world, w, ["-a", "all", "-e", str(k), "-S", spec])
    lo, hi = int(m.group(4)), int(m.group(5))
    st, groups = samcheck.check_paired(body, _reference(gt, w), w["r1"], w["r2"], w["ids1"], w["ids2"], w["q1"], w["q2"], limit=k,
                                       orientation=samcheck.ORIENTATION_FR, min_frag=lo, max_frag=hi)
    print(f"columba_align, ALL mode, {spec} k = {k}: " + ", ".join(f"{a} {b}" for a, b in st.items()))
    assert n_sample == len(sample) and m.group(1) == "FR", (n_sample, len(sample), m.group(0))
    assert all(lo <= w["pairs"][i]["frag"] <= hi for i in sample)
    pairtruth.check_all_pairs(groups, truth, NAMES, STARTS, k, samcheck.ORIENTATION_FR, lo, hi, label=w["cls"])
