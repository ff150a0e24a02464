"""A judge for read pairs (helper of tests/test_pair_inference_ground_truth.py, no test in itself).

What goes in: the text that was indexed, the start positions of its sequences, the reads and the parameters of the run.  What never goes
in: an occurrence array, an oracle result or an index.  Where a mate can lie follows from Sellers' semi-global alignment by plain dynamic
programming (`oracle/groundtruth.c`, handed in as `gt`); which couples of such places are a proper pair, which of those BEST mode at x = 0
has to report, and which pairs belong in the sample the paired-end parameters are inferred from, is set logic over those places.

  location     a maximal run of end positions j with min_b ED(read, text[b, j)) <= cut-off, no two neighbours further than 4 * cut-off + 1
               apart, on one strand: its end of minimal distance (the first one), that distance, and the begin the DP returns for it
  concordant   two locations, one per mate, in one sequence, the strands of the upstream and the downstream one as the orientation asks
               (FR: forward then reverse; RF: reverse then forward; FF: the same strand, mate 1 upstream on the forward strand and mate 2
               on the reverse one), the fragment (end of the downstream location - begin of the upstream one) inside its bounds
  tolerance    a reported POS lies within 4 * cut-off of its location's begin: 2k for the filter's window, 2k for the width of an alignment
               with k indels (tests/test_ground_truth.py)
"""
import ctypes as C
from collections import namedtuple

import numpy as np

import samcheck

from samcheck import ORIENTATION_FF, ORIENTATION_FR, ORIENTATION_RF  # noqa: F401 (the checker's own numbering, not the library's)

Location = namedtuple("Location", "strand seq begin end distance")  # begin, end: text coordinates


def mate_locations(gt, text: bytes, starts, read: bytes, cutoff: int):
    """the locations of `read` (as given: it is cleaned here) on both strands within `cutoff` edits; starts: the begin of every sequence
    and, last, the end of the text"""
    n = len(text)
    best = np.zeros(n + 1, np.uint8)
    begin = np.zeros(n + 1, np.uint64)
    fw = samcheck.clean(read)
    bounds = np.asarray(starts[:-1], np.int64)
    out = []
    for strand, pat in enumerate((fw, samcheck.revcomp(fw))):
        gt.gt_semiglobal_ends(text, n, pat, len(pat), cutoff, best.ctypes.data_as(C.c_void_p), begin.ctypes.data_as(C.c_void_p))
        ends = np.flatnonzero(best <= cutoff)
        if ends.size == 0:
            continue
        for run in np.split(ends, np.flatnonzero(np.diff(ends) > 4 * cutoff + 1) + 1):
            j = int(run[np.argmin(best[run])])
            b = int(begin[j])
            out.append(Location(strand, int(np.searchsorted(bounds, b, side="right") - 1), b, j, int(best[j])))
    return out


def concordant(loc1: Location, loc2: Location, orientation: int, min_frag: int, max_frag: int) -> bool:
    """loc1: a location of mate 1, loc2: one of mate 2"""
    if loc1.seq != loc2.seq:
        return False
    ups = []  # (upstream, downstream, upstream is mate 1); equal begins: either one
    if loc1.begin <= loc2.begin:
        ups.append((loc1, loc2, True))
    if loc2.begin <= loc1.begin:
        ups.append((loc2, loc1, False))
    for up, down, first_up in ups:
        if orientation == ORIENTATION_FR:
            strands = (up.strand, down.strand) == (0, 1)
        elif orientation == ORIENTATION_RF:
            strands = (up.strand, down.strand) == (1, 0)
        else:
            strands = up.strand == down.strand and first_up == (up.strand == 0)
        if strands and min_frag <= down.end - up.begin <= max_frag:
            return True
    return False


def combinations(locs1, locs2, orientation: int, min_frag: int, max_frag: int):
    return [(a, b) for a in locs1 for b in locs2 if concordant(a, b, orientation, min_frag, max_frag)]


def _proper_couples(group, pair):
    """the proper pairs a group of records shows: (record of mate 1, record of mate 2) — every record with flag 2 in exactly the couples
    its RNEXT / PNEXT / flag 32 name"""
    first = [r for r in group if r["flag"] & 64 and r["flag"] & 2]
    second = [r for r in group if r["flag"] & 128 and r["flag"] & 2]
    couples, used = [], set()
    for a in first:
        mates = [j for j, b in enumerate(second) if b["rname"] == a["rname"] and b["pos"] == a["pnext"] and b["pnext"] == a["pos"]
                 and bool(b["flag"] & 16) == bool(a["flag"] & 32) and bool(a["flag"] & 16) == bool(b["flag"] & 32)]
        assert mates, ("a proper record of mate 1 without its mate's record", pair, a["line"])
        couples.append((a, second[mates[0]]))
        used.update(mates)
    assert len(used) == len(second), ("a proper record of mate 2 that no record of mate 1 names", pair)
    return couples


def _at(rec, loc: Location, starts, names, cutoff: int) -> bool:
    return (rec["rname"] == names[loc.seq] and ((rec["flag"] >> 4) & 1) == loc.strand
            and abs(rec["pos"] - 1 - (loc.begin - int(starts[loc.seq]))) <= 4 * cutoff)


def _faults(groups, truth, names, starts, cutoffs, orientation, min_frag, max_frag, best_only: bool):
    assert len(groups) == len(truth), "the judge leaves out no pair"
    faults = []
    for i, (g, (locs1, locs2)) in enumerate(zip(groups, truth)):
        c1, c2 = cutoffs[i] if hasattr(cutoffs, "__len__") else (cutoffs, cutoffs)
        comb = combinations(locs1, locs2, orientation, min_frag, max_frag)
        flagged = [r for r in g if r["flag"] & 2]
        if not comb:
            if flagged:
                faults.append((i, ("a proper pair although no two locations of the mates are concordant", flagged[0]["line"])))
            continue
        if best_only and len(flagged) != len(g):
            faults.append((i, ("a concordant combination exists, yet a record without flag 2", [r["line"] for r in g if not r["flag"] & 2][:2])))
            continue
        total = min(a.distance + b.distance for a, b in comb)
        want = [(a, b) for a, b in comb if a.distance + b.distance == total] if best_only else comb
        try:
            couples = _proper_couples(g, i)
        except AssertionError as e:
            faults.append((i, e.args[0]))
            continue
        hit = set()
        for ra, rb in couples:
            where = [j for j, (a, b) in enumerate(want) if _at(ra, a, starts, names, c1) and _at(rb, b, starts, names, c2)]
            if not where:
                other = [1 for a, b in comb if _at(ra, a, starts, names, c1) and _at(rb, b, starts, names, c2)]
                faults.append((i, ("a proper pair at a concordant combination above the minimal total distance" if other else
                                   "a proper pair outside the concordant combinations of the mates' locations", ra["line"], rb["line"])))
                continue
            hit.update(where)
            if best_only and ra["tags"]["NM"] + rb["tags"]["NM"] != total:
                faults.append((i, ("NM of a record and its mate do not sum to the minimal total distance", total, ra["line"], rb["line"])))
        for j, (a, b) in enumerate(want):
            if j not in hit:
                faults.append((i, ("a concordant combination" + (" of minimal total distance" if best_only else "") + " is not reported", a, b)))
    return faults


def best_pair_faults(groups, truth, names, starts, cutoffs, orientation: int, min_frag: int, max_frag: int):
    """BEST mode at x = 0 on the groups samcheck.check_paired returns (soundness of every record is its business).  truth: per pair
    (locations of mate 1, of mate 2) at the mates' cut-offs; cutoffs: per pair (mate 1, mate 2).  With C = the concordant combinations of a
    pair: C not empty — every record carries flag 2, the proper pairs are exactly the combinations of minimal total distance in C (each
    POS within 4 * cut-off of its location's begin) and NM of a record and its mate sum to that total; C empty — no record carries flag
    2.  Returns [(pair, what is wrong)]."""
    return _faults(groups, truth, names, starts, cutoffs, orientation, min_frag, max_frag, True)


def all_pair_faults(groups, truth, names, starts, k: int, orientation: int, min_frag: int, max_frag: int):
    """ALL mode at a fixed k: every combination in C is a proper pair and no proper pair lies outside C"""
    return _faults(groups, truth, names, starts, k, orientation, min_frag, max_frag, False)


def _raise(faults, label=None):
    assert not faults, (f"{len(faults)} faults in the pairs {sorted({i for i, _ in faults})}",
                        [(i, label[i] if label else None, what) for i, what in faults[:6]])


def check_best_pairs(groups, truth, names, starts, cutoffs, orientation: int, min_frag: int, max_frag: int, label=None):
    """label: per pair a name for the message (the class of the world it belongs to)"""
    _raise(best_pair_faults(groups, truth, names, starts, cutoffs, orientation, min_frag, max_frag), label)


def check_all_pairs(groups, truth, names, starts, k: int, orientation: int, min_frag: int, max_frag: int, label=None):
    _raise(all_pair_faults(groups, truth, names, starts, k, orientation, min_frag, max_frag), label)


def sample_truth(truth, seqs_in_first_file: int):
    """(the pairs that belong in the sample the paired-end parameters are inferred from, per pair whether read 2 counts as done): a read is
    unambiguous when exactly one of ALL its locations within the cut-off lies in a sequence of the first reference file; read 2 is matched
    (done) where read 1 is unambiguous; the sample holds the pairs whose reads both are"""
    def unambiguous(locs):
        return sum(1 for l in locs if l.seq < seqs_in_first_file) == 1

    done = [unambiguous(l1) for l1, _ in truth]
    return [i for i, (_, l2) in enumerate(truth) if done[i] and unambiguous(l2)], done


def traceback_ops(gt, pat: bytes, win: bytes):
    """run-length CIGAR operations (length << 2 | "MID".index(op)) of one optimal global alignment of the read with its window, by the
    plain O(mn) matrix; all-match when the window has the read's length and that many mismatches are optimal"""
    m, n = len(pat), len(win)
    d = gt.gt_edit_distance(pat, m, win, n)
    if m == n and gt.gt_hamming_distance(pat, win, m) == d:
        return [m << 2], d
    ok = lambda a, b: a == b and a in b"ACGT"  # noqa: E731
    D = np.zeros((m + 1, n + 1), np.int32)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(n + 1)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i, j] = min(D[i - 1, j - 1] + (0 if ok(pat[i - 1], win[j - 1]) else 1), D[i - 1, j] + 1, D[i, j - 1] + 1)
    assert int(D[m, n]) == d
    ops, i, j = [], m, n
    while i or j:
        if i and j and D[i, j] == D[i - 1, j - 1] + (0 if ok(pat[i - 1], win[j - 1]) else 1):
            ops.append(0)
            i, j = i - 1, j - 1
        elif i and D[i, j] == D[i - 1, j] + 1:
            ops.append(1)
            i -= 1
        else:
            ops.append(2)
            j -= 1
    ops.reverse()
    runs = []
    for o in ops:
        if runs and runs[-1][1] == o:
            runs[-1][0] += 1
        else:
            runs.append([1, o])
    return [(ln << 2) | o for ln, o in runs], d
