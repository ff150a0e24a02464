"""The pairs without a concordant combination, paired and written on the device (cmb_pair_sam_device_classes / cmb_move_pair_sam_device:
csrc/dev_pair.hpp, k_pair_plan and k_pair_class_write): one mate unmapped, discordant pairs up to the 10 000-combination rule and beyond
it, unpaired records.  The judge is the host path over the same C-ABI, ca.pair_chunk_sam(..., per_strand=True), i.e. cmb_pair_sam pair
by pair: the text byte for byte, the number of mapped pairs, and the class counters against a classifier written here from the host
lists.  Every test first asserts that its chunk holds the class it is about.

The world: 60 kbp of random text in three sequences, K = 2 with edit distance, reads of 40 - 100 characters.
  chrA  [0, 24 000)        plain fragments; at 20 000 a tandem of 35 copies of a 44-mer UD and then 35 copies of the reverse complement
                           of UD1 (UD with one substitution): a read of UD1 has 35 forward occurrences at distance 1 and, behind them in
                           its list, 35 reverse-complement ones at distance 0
  chrB  [24 000, 44 000)   at 26 000 a tandem of 130 copies of a 45-mer: 65 of UB, then 65 of VB (UB with substitutions at 5, 20, 35).
                           40 characters from 0 of either: 65 occurrences.  40 characters of VB from 6 ... 10 (over 20 and 35 only): 130
                           occurrences, the first 65 at distance 2 and the others at 0 — the primary is not the first
  chrC  [44 000, 60 000)   at 46 000 a tandem of 165 copies of a 50-mer: 100 of UC, one of YC (substitutions at 2, 4, 6), 64 of ZC
                           (at 10, 25, 38, 43, 45, 47).  UC from 0 or 1: 100 occurrences; UC from 8: 101; ZC from 0 or 2: 64
A maximal fragment size of 20, below every read's length, leaves no concordant combination, so pairs with both mates mapped become
discordant ones, or unpaired ones without discordant_allowed.  (Discordant / over the limit and unpaired exclude each other in one
call — discordant_allowed decides — so the mixed chunk, which holds all six device classes, shows five of them with the option and
four without it.)
"""
import numpy as np
import pytest

import columba_amd as ca
import samcheck
import test_gpu_pair_sam_device as base
from test_gpu_pair_sam_device import _concordant_pairs, _env, _groups, _ids, _mates, _quals, _random_read, _sub

pytestmark = pytest.mark.gpu

NAMES = ["chrA", "chrB", "chrC"]
STARTS = [0, 24_000, 44_000, 60_000]
K = 2
ALL = ca.PAIR_CLASS_ALL
D_AT, B_AT, C_AT = 20_000, 26_000, 46_000
ARRAYS = [(D_AT - 200, D_AT + 70 * 44 + 200), (B_AT - 200, B_AT + 130 * 45 + 200), (C_AT - 200, C_AT + 165 * 50 + 200)]
CLASSES = ("both_unmapped", "concordant", "one_unmapped", "discordant", "unpaired", "over_limit")
ORIENTATIONS = base.ORIENTATIONS
ORI_NAME = base.ORI_NAME
rc = samcheck.revcomp


def _with_subs(unit: bytes, at):
    b = bytearray(unit)
    for p in at:
        _sub(b, p)
    return bytes(b)


def _text():
    rng = np.random.default_rng(23)
    rnd = lambda n: bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())  # noqa: E731
    g = bytearray(rnd(STARTS[-1]))
    u = {"UD": rnd(44), "UB": rnd(45), "UC": rnd(50)}
    u["UD1"] = _with_subs(u["UD"], [17])
    u["VB"] = _with_subs(u["UB"], [5, 20, 35])
    u["YC"] = _with_subs(u["UC"], [2, 4, 6])
    u["ZC"] = _with_subs(u["UC"], [10, 25, 38, 43, 45, 47])
    for at, parts in ((D_AT, u["UD"] * 35 + rc(u["UD1"]) * 35), (B_AT, u["UB"] * 65 + u["VB"] * 65 + u["VB"][:10]), (C_AT, u["UC"] * 100 + u["YC"] + u["ZC"] * 64)):
        g[at:at + len(parts)] = parts
    return bytes(g), u


def _cyc(unit: bytes, at: int, n: int) -> bytes:
    return (unit * 3)[at:at + n]


def _tandem_reads(u):
    """the reads of the arrays, by the number of occurrences the world gives them (asserted from the lists where they are used)"""
    return {"b65": u["UB"][:40], "v65": u["VB"][:40], "b130": [_cyc(u["VB"], 6 + s, 40) for s in range(5)],
            "c100": u["UC"][:40], "c100b": u["UC"][1:41], "c101": u["UC"][8:48], "z64": u["ZC"][:42], "z64b": u["ZC"][2:44],
            "d70": u["UD1"][:40], "d70b": _cyc(u["UD1"], 2, 41)}


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from columba_amd import indexbuild as ib
    text, units = _text()
    ix = ib.build_index(text, seq_starts=np.asarray(STARTS, np.uint32), device="cuda")
    ix.seq_names = NAMES
    return {"text": text, "units": units, "reads": _tandem_reads(units), "dev": ca.Index(ix), "st": ca.SearchStrategy("columba", "edit", "dynamic"),
            "cache": {}}


@pytest.fixture(scope="module")
def move_world(world):
    from columba_amd import movebuild
    dev = ca.MoveIndex(movebuild.build_move(world["text"], device="cuda"))
    dev.attach_text(world["text"], np.asarray(STARTS, np.uint64))
    return dict(world, dev=dev, cache={})


def _place(rng, seq: int, n: int) -> int:
    """a begin in sequence `seq` for n characters, away from the arrays and the sequence's ends"""
    while True:
        p = int(rng.integers(STARTS[seq] + 300, STARTS[seq + 1] - 300 - n))
        if all(p + n < lo or p > hi for lo, hi in ARRAYS):
            return p


def _piece(w, rng, seq: int, lo: int = 40, hi: int = 101, edit: bool = False, reverse: bool = False) -> bytes:
    n = int(rng.integers(lo, hi))
    p = _place(rng, seq, n)
    r = bytearray(w["text"][p:p + n])
    if edit:
        _sub(r, int(rng.integers(8, n - 8)))
    return rc(bytes(r)) if reverse else bytes(r)


# ---------------------------------------------------------------------------------- the host lists, the classifier, the two paths
def _lists(w, reads, st=None):
    is_move = isinstance(w["dev"], ca.MoveIndex)
    b = (ca.MoveBatch if is_move else ca.Batch)(w["dev"], st or w["st"], K, reads=reads)
    b.want_alignments()
    b.filter_per_strand() if is_move else ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
    b.run()
    occ, offs, _ = b.results()
    aln, _ = b.alignments()
    b.close()
    return [[{"seq": int(aln["seq_id"][j]), "begin": int(occ["begin"][j]), "end": int(occ["end"][j]), "distance": int(occ["distance"][j]),
              "strand": int(occ["strand"][j]), "spans": int(aln["spans"][j]), "pos": int(aln["seq_begin"][j])}
             for j in range(int(offs[i]), int(offs[i + 1]))] for i in range(len(reads))]


def _class_of(a, b, orientation, min_frag, max_frag, discordant) -> str:
    """the class of a pair from its two host lists, as cmb_pair_sam decides it (pair_sam.hip: pairDiscordantly)"""
    if any(o["spans"] or o["seq"] >= len(NAMES) for o in a + b):
        return "host"
    if not a and not b:
        return "both_unmapped"
    if not a or not b:
        return "one_unmapped"
    if _concordant_pairs(a, b, orientation, min_frag, max_frag):
        return "concordant"
    if not discordant:
        return "unpaired"
    return "over_limit" if len(a) * len(b) > 10_000 else "discordant"


MASK = {"one_unmapped": ca.PAIR_CLASS_ONE_UNMAPPED, "discordant": ca.PAIR_CLASS_DISCORDANT, "unpaired": ca.PAIR_CLASS_UNPAIRED,
        "over_limit": ca.PAIR_CLASS_OVER_LIMIT}


def _expected_counts(l1, l2, orientation, min_frag, max_frag, discordant, classes=ALL):
    want = dict.fromkeys(CLASSES + ("host_pairs",), 0)
    for a, b in zip(l1, l2):
        c = _class_of(a, b, orientation, min_frag, max_frag, discordant)
        if c == "host" or (c in MASK and not classes & MASK[c]):
            want["host_pairs"] += 1
        else:
            want[c] += 1
    return want


def _judge(w, key, r1, r2, ids1, ids2, q1, q2, orientation, max_frag, min_frag, discordant, unmapped, st=None):
    """the host path's (text, mapped pairs), once per chunk and setting"""
    ck = (key, orientation, max_frag, min_frag, discordant, unmapped, None if q1 is None else (tuple(q1), tuple(q2)), st is not None)
    if ck not in w["cache"]:
        hq1, hq2 = (q1, q2) if q1 is not None else ([""] * len(r1), [""] * len(r2))
        w["cache"][ck] = ca.pair_chunk_sam(w["dev"], st or w["st"], K, r1, r2, ids1, ids2, hq1, hq2, NAMES, orientation, max_frag, min_frag, discordant,
                                           unmapped, per_strand=True)
    return w["cache"][ck]


def _chunk_lists(w, key, r1, r2, st=None):
    ck = ("lists", key, st is not None)
    if ck not in w["cache"]:
        w["cache"][ck] = (_lists(w, r1, st), _lists(w, r2, st))
    return w["cache"][ck]


def _check(w, key, r1, r2, q1, q2, orientation, max_frag, min_frag, discordant=True, unmapped=True, classes=ALL, st=None):
    """the device path against the judge and the classifier -> (device text, stats, the two host lists)"""
    n = len(r1)
    ids1, ids2 = _ids(n, 1), _ids(n, 2)
    want, want_mapped = _judge(w, key, r1, r2, ids1, ids2, q1, q2, orientation, max_frag, min_frag, discordant, unmapped, st)
    got, mapped, stats = ca.pair_chunk_sam_device(w["dev"], st or w["st"], K, r1, r2, ids1, ids2, q1, q2, NAMES, orientation, max_frag, min_frag, discordant,
                                                  unmapped, classes=classes)
    l1, l2 = _chunk_lists(w, key, r1, r2, st)
    counts = _expected_counts(l1, l2, orientation, min_frag, max_frag, discordant, classes)
    print(f"{key} {ORI_NAME[orientation]} disc={discordant} unmapped={unmapped} classes={classes}: {n} pairs, {len(got)} bytes, {stats}; expected {counts}")
    if got.encode() != want.encode():
        wl, gl = want.splitlines(), got.splitlines()
        at = next((i for i, (a, b) in enumerate(zip(wl, gl)) if a != b), min(len(wl), len(gl)))
        raise AssertionError(("the device text differs from the host text", len(want), len(got), at, wl[at:at + 2], gl[at:at + 2]))
    assert mapped == want_mapped == stats["mapped_pairs"]
    if len(stats) == 3:  # (classes = 0 on FM-index batches: cmb_pair_sam_device and its three fields)
        assert classes == 0 and stats["host_pairs"] == counts["host_pairs"]
        return got, stats, l1, l2
    assert {c: stats[c] for c in counts} == counts
    assert sum(stats[c] for c in CLASSES) + stats["host_pairs"] == n
    if stats["host_pairs"] == 0:
        assert stats["device_records"] == len(got.splitlines())
    return got, stats, l1, l2


def _first_is_not_best(lst) -> bool:
    return bool(lst) and lst[0]["distance"] > min(o["distance"] for o in lst)


# ---------------------------------------------------------------------------------- 1. one mate unmapped
def _one_unmapped_chunk(w):
    rng = np.random.default_rng(31)
    R = w["reads"]
    mapped = [_piece(w, rng, i % 3, edit=bool(i % 2), reverse=bool(i % 4 == 1)) for i in range(30)]
    mapped += [R["b65"], R["b130"][0], R["d70"], R["d70b"]] + R["b130"][1:] + [rc(R["b130"][2]), rc(R["d70"])]
    r1, r2 = [], []
    for i, m in enumerate(mapped):
        nowhere = _random_read(rng, int(rng.integers(40, 101)))
        r1.append(m if i % 2 == 0 else nowhere)
        r2.append(nowhere if i % 2 == 0 else m)
    return r1, r2


@pytest.mark.parametrize("with_quals", [True, False], ids=["quals", "noquals"])
@pytest.mark.parametrize("unmapped", [True, False], ids=["unmapped", "nounmapped"])
def test_one_mate_unmapped(world, unmapped, with_quals):
    r1, r2 = _one_unmapped_chunk(world)
    rng = np.random.default_rng(32)
    q1, q2 = (_quals(rng, r1), _quals(rng, r2)) if with_quals else (None, None)
    l1, l2 = _chunk_lists(world, "one", r1, r2)
    half = [a or b for a, b in zip(l1, l2) if bool(a) != bool(b) and not any(o["spans"] for o in a + b)]
    assert len(half) >= 40 and sum(bool(a) for a in l1) >= 15 and sum(bool(b) for b in l2) >= 15
    sizes = sorted(len(h) for h in half)
    assert sizes[0] == 1 and 65 in sizes and 130 in sizes, sizes
    assert sum(_first_is_not_best(h) for h in half) >= 5, "the swap"
    assert any({o["strand"] for o in h} == {0, 1} for h in half), "occurrences on both strands"
    got, stats, _, _ = _check(world, "one", r1, r2, q1, q2, ca.ORIENTATION_FR, 500, 100, True, unmapped)
    assert stats["one_unmapped"] == len(half) and stats["host_pairs"] == 0 and stats["mapped_pairs"] == 0
    for recs, a, b in zip(_groups(got, len(r1)), l1, l2):
        if bool(a) != bool(b):
            assert len(recs) == len(a or b) + 1 and int(recs[1][1]) & 4 and not int(recs[1][1]) & 8 and int(recs[0][1]) & 8


# ---------------------------------------------------------------------------------- 2. discordant pairs, 4. unpaired records
def _discordant_chunk(w, orientation):
    rng = np.random.default_rng(41 + orientation)
    R, t = w["reads"], w["text"]
    r1, r2 = [], []
    for i in range(40):  # mates in different sequences, every combination of strands
        s1 = i % 3
        r1.append(_piece(w, rng, s1, edit=bool(i % 3 == 1), reverse=bool(i & 1)))
        r2.append(_piece(w, rng, (s1 + 1 + i % 2) % 3, edit=bool(i % 5 == 1), reverse=bool(i & 2)))
    for i in range(12):  # the same sequence, too far apart for any fragment size used here; read 2 upstream in half of them
        p0 = _place(rng, 0, 3000)
        a, b = _mates(t[p0:p0 + 70], t[p0 + 2000:p0 + 2000 + 64 + i], orientation, bool(i % 2))
        r1.append(a)
        r2.append(b)
    for i in range(4):  # equal begins inside two different sequences: read 2's occurrence is up
        x = 1000 + 137 * i
        r1.append(t[STARTS[i % 2] + x:STARTS[i % 2] + x + 60])
        r2.append(rc(t[STARTS[2] + x:STARTS[2] + x + 75]) if i % 2 else t[STARTS[2] + x:STARTS[2] + x + 75])
    single = lambda s: _piece(w, rng, s)  # noqa: E731
    for a, b in ((single(0), R["b65"]), (R["v65"], single(2)), (R["z64"], R["z64b"]), (R["b130"][0], single(0)), (single(2), R["b130"][1]),
                 (R["b130"][2], rc(single(0))), (R["d70"], single(1)), (single(1), R["d70b"]), (R["b130"][3], R["d70"])):
        r1.append(a)
        r2.append(b)
    return r1, r2


def _assert_discordant_world(l1, l2):
    both = [(a, b) for a, b in zip(l1, l2) if a and b and not any(o["spans"] for o in a + b)]
    shapes = {(len(a), len(b)) for a, b in both}
    assert {(1, 1), (1, 65), (65, 1), (64, 64)} <= shapes, sorted(shapes)
    assert sum(len(a) == 1 == len(b) and a[0]["seq"] != b[0]["seq"] for a, b in both) >= 40
    same = [(a[0], b[0]) for a, b in both if len(a) == 1 == len(b) and a[0]["seq"] == b[0]["seq"]]
    assert sum(x["pos"] < y["pos"] for x, y in same) >= 5 and sum(y["pos"] < x["pos"] for x, y in same) >= 5
    assert sum(len(a) == 1 == len(b) and a[0]["seq"] != b[0]["seq"] and a[0]["pos"] == b[0]["pos"] for a, b in both) >= 4, "the tie"
    assert sum(_first_is_not_best(a) or _first_is_not_best(b) for a, b in both) >= 5, "the primary is not the first candidate"
    return both


@pytest.mark.parametrize("with_quals", [True, False], ids=["quals", "noquals"])
@pytest.mark.parametrize("orientation", ORIENTATIONS, ids=lambda o: ORI_NAME[o])
def test_discordant(world, orientation, with_quals):
    r1, r2 = _discordant_chunk(world, orientation)
    rng = np.random.default_rng(42)
    q1, q2 = (_quals(rng, r1), _quals(rng, r2)) if with_quals else (None, None)
    l1, l2 = _chunk_lists(world, ("disc", orientation), r1, r2)
    both = _assert_discordant_world(l1, l2)
    got, stats, _, _ = _check(world, ("disc", orientation), r1, r2, q1, q2, orientation, 20, 0, True, True)
    assert stats["discordant"] == len(both) >= 60 and stats["mapped_pairs"] == len(both)
    lines = [ln.split("\t") for ln in got.splitlines()]
    assert any(f[8] == "-0" for f in lines), "TLEN of the record behind its mate in another sequence"
    assert not any(int(f[1]) & 2 for f in lines) and not any(f[6] == "=" for f in lines)
    for recs, a, b in zip(_groups(got, len(r1)), l1, l2):
        if a and b:
            assert len(recs) == 2 * len(a) * len(b)


@pytest.mark.parametrize("quals", ["quals", "empty", "noquals"])
@pytest.mark.parametrize("orientation", [ca.ORIENTATION_FR, ca.ORIENTATION_FF], ids=lambda o: ORI_NAME[o])
def test_unpaired(world, orientation, quals):
    R = world["reads"]
    r1, r2 = _discordant_chunk(world, orientation)
    r1, r2 = r1 + [R["b130"][4], R["d70"]], r2 + [R["d70b"], R["b130"][0]]
    rng = np.random.default_rng(43)
    q1, q2 = (None, None) if quals == "noquals" else (_quals(rng, r1), _quals(rng, r2))
    if quals == "empty":
        q1, q2 = [q if i % 2 else "" for i, q in enumerate(q1)], [q if i % 3 else "" for i, q in enumerate(q2)]
    l1, l2 = _chunk_lists(world, ("unp", orientation), r1, r2)
    both = _assert_discordant_world(l1, l2)
    a, b = l1[-2], l2[-2]
    assert (len(a), len(b)) == (130, 70) and {o["strand"] for o in b} == {0, 1}
    for lst in (a, b):  # a stable sort by distance moves something
        assert [o["distance"] for o in lst] != sorted(o["distance"] for o in lst)
    fw, rv = [o["distance"] for o in b if not o["strand"]], [o["distance"] for o in b if o["strand"]]
    assert min(rv) < max(fw), "the reverse-complement part holds distances below the forward part's"
    got, stats, _, _ = _check(world, ("unp", orientation), r1, r2, q1, q2, orientation, 20, 0, False, True)
    assert stats["unpaired"] == len(both) >= 60 and stats["mapped_pairs"] == 0 and stats["discordant"] == 0
    for recs, x, y in zip(_groups(got, len(r1)), l1, l2):
        if x and y:
            assert len(recs) == len(x) + len(y) and [f[9] == "*" for f in recs] == [False] + [True] * (len(x) - 1) + [False] + [True] * (len(y) - 1)


# ---------------------------------------------------------------------------------- 3. the 10 000-combination rule
@pytest.mark.parametrize("unmapped", [True, False], ids=["unmapped", "nounmapped"])
def test_the_limit(world, unmapped):
    R = world["reads"]
    rng = np.random.default_rng(51)
    r1 = [_piece(world, rng, 0), R["c100"], _piece(world, rng, 1), R["c101"], _piece(world, rng, 0)]
    r2 = [_piece(world, rng, 1), R["c100b"], _piece(world, rng, 2), R["c100"], _piece(world, rng, 2)]
    l1, l2 = _chunk_lists(world, "limit", r1, r2)
    assert len(l1[1]) * len(l2[1]) == 10_000 and len(l1[3]) * len(l2[3]) == 10_100, [(len(a), len(b)) for a, b in zip(l1, l2)]
    got, stats, _, _ = _check(world, "limit", r1, r2, _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 20, 0, True, unmapped)
    assert stats["discordant"] == 4 and stats["over_limit"] == 1 and stats["host_pairs"] == 0
    groups = _groups(got, 5)
    assert len(groups[1]) == 20_000 and [int(f[1]) for f in groups[3]] == ([77, 141] if unmapped else [])
    assert len(got) > 100 * 8192, "many windows"


# ---------------------------------------------------------------------------------- 5. a mixed chunk
def _mixed_chunk(w, spanning: bool = True):
    rng = np.random.default_rng(61)
    R, t = w["reads"], w["text"]
    r1, r2 = [], []
    for i in range(203):
        c = i % 7
        if i == 100:
            a, b = R["c101"], R["c100"]  # over the limit (or 201 unpaired records)
        elif i == 101:
            a, b = R["z64"], R["z64b"]
        elif i == 102:
            a, b = R["b130"][0], _random_read(rng, 50)
        elif c in (0, 4):  # a true fragment
            p0 = _place(rng, i % 3, 600)
            a, b = base._fragment(w, p0, int(rng.integers(150, 501)), int(rng.integers(40, 101)), int(rng.integers(40, 101)), ca.ORIENTATION_FR, bool(i % 2))
        elif c == 1:  # one mate from nowhere
            a, b = _piece(w, rng, i % 3, edit=True), _random_read(rng, 70)
            a, b = (b, a) if i % 2 else (a, b)
        elif c == 2:  # mates in different sequences
            a, b = _piece(w, rng, 0, reverse=bool(i % 2)), _piece(w, rng, 1 + i % 2)
        elif c == 3:
            a, b = _random_read(rng, 64), _random_read(rng, 90)
        elif c == 5 and spanning:  # a read cut over a sequence end
            e = STARTS[1 + i % 2]
            a, b = t[e - 330:e - 260], rc(t[e - 40 - i % 9:e + 30])
            a, b = (b, a) if i % 2 else (a, b)
        else:  # too far apart
            p0 = _place(rng, 0, 1200)
            a, b = base._fragment(w, p0, 900 + i, 70, 70, ca.ORIENTATION_FR, bool(i % 2))
        r1.append(a)
        r2.append(b)
    return r1, r2


def _assert_mixed_world(l1, l2, discordant, spanning=True):
    cls = [_class_of(a, b, ca.ORIENTATION_FR, 100, 500, discordant) for a, b in zip(l1, l2)]
    need = {"both_unmapped", "concordant", "one_unmapped"} | ({"discordant", "over_limit"} if discordant else {"unpaired"})
    assert need <= set(cls), set(cls)
    assert cls.count("host") >= (10 if spanning else 0)
    assert all(len(set(cls[i:i + 8])) >= 3 for i in range(0, 200, 8)), "groups of eight consecutive pairs mix classes"
    return cls


@pytest.mark.parametrize("discordant", [True, False], ids=["disc", "nodisc"])
def test_mixed_chunk_as_a_composite_batch(world, discordant):
    r1, r2 = _mixed_chunk(world)
    assert len(r1) == 203
    rng = np.random.default_rng(62)
    q1, q2 = _quals(rng, r1), _quals(rng, r2)
    cls = _assert_mixed_world(*_chunk_lists(world, "mixed", r1, r2), discordant)
    _, whole, _, _ = _check(world, "mixed", r1, r2, q1, q2, ca.ORIENTATION_FR, 500, 100, discordant, True)
    assert whole["host_pairs"] == cls.count("host")
    with _env(CMB_SUBBATCHES="3"):
        _, parts, _, _ = _check(world, "mixed", r1, r2, q1, q2, ca.ORIENTATION_FR, 500, 100, discordant, True)
    assert parts == whole


@pytest.mark.parametrize("discordant", [True, False], ids=["disc", "nodisc"])
def test_mixed_chunk_class_by_class(world, discordant):
    r1, r2 = _mixed_chunk(world)
    rng = np.random.default_rng(62)
    q1, q2 = _quals(rng, r1), _quals(rng, r2)
    cls = _assert_mixed_world(*_chunk_lists(world, "mixed", r1, r2), discordant)
    for name, bit in MASK.items():
        _, stats, _, _ = _check(world, "mixed", r1, r2, q1, q2, ca.ORIENTATION_FR, 500, 100, discordant, True, classes=bit)
        assert stats["host_pairs"] == cls.count("host") + sum(cls.count(c) for c in MASK if c != name)
        assert stats[name] == cls.count(name)
    # classes = 0 is cmb_pair_sam_device
    n = len(r1)
    _, zero, _, _ = _check(world, "mixed", r1, r2, q1, q2, ca.ORIENTATION_FR, 500, 100, discordant, True, classes=0)
    assert set(zero) == {"host_pairs", "mapped_pairs", "device_records"}
    batches = []
    for reads in (r1, r2):
        b = ca.Batch(world["dev"], world["st"], K, reads=reads)
        b.want_alignments()
        ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
        b.run()
        batches.append(b)
    old_text, old = ca.pair_batches_sam_device(batches[0], batches[1], _ids(n, 1), _ids(n, 2), q1, q2, NAMES, ca.ORIENTATION_FR, 500, 100, discordant, True)
    new_text, new = ca.pair_batches_sam_device(batches[0], batches[1], _ids(n, 1), _ids(n, 2), q1, q2, NAMES, ca.ORIENTATION_FR, 500, 100, discordant, True,
                                               classes=ALL)
    for b in batches:
        b.close()
    assert old == zero and old_text == new_text and new["mapped_pairs"] == old["mapped_pairs"]
    assert old["host_pairs"] == cls.count("host") + sum(cls.count(c) for c in MASK)


# ---------------------------------------------------------------------------------- 6. Hamming distance
def test_hamming_distance(world):
    st = ca.SearchStrategy("kuch1", "hamming", "dynamic")
    r1, r2 = _mixed_chunk(world, spanning=False)
    rng = np.random.default_rng(63)
    for discordant in (True, False):
        _assert_mixed_world(*_chunk_lists(world, "mixed hamming", r1, r2, st), discordant, spanning=False)
        _check(world, "mixed hamming", r1, r2, _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 500, 100, discordant, True, st=st)


# ---------------------------------------------------------------------------------- 7. the b-move backend
def test_bmove_one_mate_unmapped(move_world):
    r1, r2 = _one_unmapped_chunk(move_world)
    rng = np.random.default_rng(71)
    _, stats, l1, l2 = _check(move_world, "one", r1, r2, _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 500, 100)
    assert stats["one_unmapped"] >= 40 and stats["host_pairs"] == 0
    assert {65, 130} <= {len(a or b) for a, b in zip(l1, l2)}


@pytest.mark.parametrize("discordant", [True, False], ids=["disc", "nodisc"])
def test_bmove_discordant_and_unpaired(move_world, discordant):
    r1, r2 = _discordant_chunk(move_world, ca.ORIENTATION_FR)
    rng = np.random.default_rng(72)
    l1, l2 = _chunk_lists(move_world, "disc", r1, r2)
    both = _assert_discordant_world(l1, l2)
    _, stats, _, _ = _check(move_world, "disc", r1, r2, _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 20, 0, discordant, True)
    assert stats["discordant" if discordant else "unpaired"] == len(both)


@pytest.mark.parametrize("discordant", [True, False], ids=["disc", "nodisc"])
def test_bmove_mixed_chunk(move_world, discordant):
    r1, r2 = _mixed_chunk(move_world)
    rng = np.random.default_rng(73)
    cls = _assert_mixed_world(*_chunk_lists(move_world, "mixed", r1, r2), discordant)
    _, stats, _, _ = _check(move_world, "mixed", r1, r2, _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 500, 100, discordant, True)
    assert stats["host_pairs"] == cls.count("host")


def test_bmove_refusals(move_world):
    from columba_amd import movebuild
    w = move_world
    r1, r2 = _mixed_chunk(w)
    r1, r2 = r1[:6], r2[:6]

    def batch(index, reads, per_strand=True, keep=True):
        b = ca.MoveBatch(index, w["st"], K, reads=reads)
        b.want_alignments()
        if per_strand:
            b.filter_per_strand()
        if keep:
            b.keep_device_lists()
        b.run()
        return b

    good = batch(w["dev"], r1)
    for what in ("no kept lists", "no per-strand filter"):
        bad = batch(w["dev"], r2, per_strand=what != "no per-strand filter", keep=what != "no kept lists")
        for first, second in ((good, bad), (bad, good)):
            with pytest.raises(ca.CmbError) as e:
                ca.pair_batches_sam_device(first, second, _ids(6, 1), _ids(6, 2), None, None, NAMES, classes=ALL)
            assert e.value.code == -1 and str(e.value), what
        bad.close()
    # no text beside the index: nothing with alignments can be asked of it, so no batch reaches the call
    bare = ca.MoveIndex(movebuild.build_move(w["text"][:20_000], device="cuda"))
    b = ca.MoveBatch(bare, w["st"], K, reads=r1)
    with pytest.raises(ca.CmbError) as e:
        b.want_alignments()
    assert e.value.code == -1
    b.run()
    with pytest.raises(ca.CmbError) as e:
        ca.pair_batches_sam_device(b, good, _ids(6, 1), _ids(6, 2), None, None, NAMES, classes=ALL)
    assert e.value.code == -1 and str(e.value)
    mate = batch(w["dev"], r2)
    text, stats = ca.pair_batches_sam_device(good, mate, _ids(6, 1), _ids(6, 2), None, None, NAMES, ca.ORIENTATION_FR, 500, 100, classes=ALL)
    want, _ = ca.pair_chunk_sam(w["dev"], w["st"], K, r1, r2, _ids(6, 1), _ids(6, 2), [""] * 6, [""] * 6, NAMES, ca.ORIENTATION_FR, 500, 100, True, True)
    assert text.decode() == want
    for x in (good, mate, b):
        x.close()
