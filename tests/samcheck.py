"""Validation of SAM text against the reference sequence alone (helper of tests/test_sam_ground_truth.py, no test in itself).

What goes in: the text that was indexed, the names and start positions of its sequences, and the reads, identifiers and qualities
the matcher was given.  What never goes in: an occurrence array, an oracle result or anything else a matcher computed.  Every
alignment a record (or an XA entry) claims is re-derived: its CIGAR is walked over read and reference window, and the number of edits
it shows must be the window's edit distance by plain dynamic programming (`oracle/groundtruth.c`, handed in as `gt`).

The record layout and the derived fields are the reference aligner's (indexhelpers.cpp:56-260, indexhelpers.h:321-421):
  MAPQ    60 for one hit at the minimal distance, round(-10 log10(1 - 1/nHits)) for more, 0 for a record above the minimum
          (getMapQ, indexhelpers.h:378-388)
  TLEN    end of the downstream record - begin of the upstream one, 0 across sequences (searchstrategy.cpp:1310, :1553-1556);
          negative on the record with the larger begin (indexhelpers.cpp:140-141)
"""
import math
import re

import numpy as np

MAX_MAPQ = 60
_CLEAN = bytes(c if chr(c) in "ACGT" else ord("N") for c in range(256))
_COMP = bytes({65: 84, 67: 71, 71: 67, 84: 65}.get(c, ord("N")) for c in range(256))
_CIGAR = re.compile(r"(\d+)([MID])")


def clean(read: bytes) -> bytes:
    """reads.h:43-58: upper case, everything outside ACGT becomes N"""
    return read.upper().translate(_CLEAN)


def revcomp(read: bytes) -> bytes:
    return read.translate(_COMP)[::-1]


def qname(identifier: str) -> str:
    """the identifier as a record shows it: without the leading '@' or '>', cut at the first blank"""
    s = identifier[1:] if identifier[:1] in ("@", ">") else identifier
    return s.split()[0] if s.split() else ""


def mapq(n_hits: int) -> int:
    assert n_hits >= 1
    return MAX_MAPQ if n_hits == 1 else int(math.floor(-10.0 * math.log10(1.0 - 1.0 / n_hits) + 0.5))


def cigar_ops(cigar: str):
    ops = _CIGAR.findall(cigar)
    assert ops and "".join(n + o for n, o in ops) == cigar, ("malformed CIGAR", cigar)
    ops = [(int(n), o) for n, o in ops]
    assert all(n > 0 for n, _ in ops), ("empty CIGAR operation", cigar)
    return ops


def cigar_walk(ops, pat: bytes, win: bytes):
    """(characters of the read consumed, characters of the window consumed, edits the CIGAR shows); a read's N never matches"""
    qi = ti = edits = 0
    for n, o in ops:
        if o == "M":
            a = np.frombuffer(pat[qi:qi + n], np.uint8)
            b = np.frombuffer(win[ti:ti + n], np.uint8)
            m = min(len(a), len(b))
            edits += int(((a[:m] != b[:m]) | (a[:m] == ord("N"))).sum())
            qi += n
            ti += n
        elif o == "I":
            qi += n
            edits += n
        else:
            ti += n
            edits += n
    return qi, ti, edits


def cigar_width(cigar: str) -> int:
    return sum(n for n, o in cigar_ops(cigar) if o in "MD")


class Reference:
    """the indexed text with its sequences: `starts` holds the begin of every sequence and, last, the end of the text"""

    def __init__(self, text: bytes, names, starts, gt):
        self.text, self.names, self.gt = text, list(names), gt
        self.starts = [int(s) for s in starts]
        assert len(self.starts) == len(self.names) + 1 and self.starts[-1] <= len(text)
        self.loose = self.alignments = 0

    def check_alignment(self, pat: bytes, rname: str, pos1: int, cigar: str, nm: int, limit: int, metric: str = "edit", ctx=None):
        """one claimed alignment of `pat` (the read as it aligns: its reverse complement on the other strand); returns the window
        (begin, end) in text coordinates"""
        assert rname in self.names, ("unknown RNAME", rname, ctx)
        sid = self.names.index(rname)
        assert pos1 >= 1, ("POS before the sequence", pos1, ctx)
        ops = cigar_ops(cigar)
        b = self.starts[sid] + pos1 - 1
        e = b + sum(n for n, o in ops if o in "MD")
        assert e <= self.starts[sid + 1], ("alignment runs past the end of its sequence", rname, pos1, cigar, ctx)
        win = self.text[b:e]
        qi, ti, edits = cigar_walk(ops, pat, win)
        assert qi == len(pat), ("CIGAR does not consume the read", cigar, len(pat), ctx)
        assert ti == len(win)
        true = self.gt.gt_edit_distance(pat, len(pat), win, len(win))
        if metric == "hamming":
            assert len(ops) == 1 and ops[0][1] == "M", ("Hamming distance: one run of M", cigar, ctx)
            assert edits == nm, ("mismatches of the window are not NM", edits, nm, ctx)
            assert true <= nm
        else:
            assert edits == true, ("the CIGAR's edits are not the window's edit distance", edits, true, rname, pos1, cigar, ctx)
            assert true <= nm, ("NM below the window's edit distance", true, nm, rname, pos1, cigar, ctx)
        assert nm <= limit, ("NM above the distance searched", nm, limit, ctx)
        self.alignments += 1
        self.loose += true < nm
        return b, e


def _fields(line: str, ctx):
    f = line.split("\t")
    assert len(f) >= 12, ("record with fewer than 11 fields and a tag", line, ctx)
    rec = {"qname": f[0], "flag": int(f[1]), "rname": f[2], "pos": int(f[3]), "mapq": int(f[4]), "cigar": f[5], "rnext": f[6],
           "pnext": int(f[7]), "tlen": int(f[8]), "seq": f[9], "qual": f[10], "tags": {}, "line": line}
    for t in f[11:]:
        name, typ, val = t.split(":", 2)
        assert name not in rec["tags"], ("tag twice", t, ctx)
        rec["tags"][name] = int(val) if typ == "i" else val
    assert rec["tags"].get("PG") == "Columba", ("PG tag", line, ctx)
    return rec


def _lines(text: str):
    if not text:
        return []
    assert text.endswith("\n"), "the text does not end with a line end"
    lines = text[:-1].split("\n")
    assert all(lines), "empty line"
    return lines


def _groups(lines, keys, ctx):
    """records in input order, one group per entry of `keys` (each a set of identifiers)"""
    out, p = [], 0
    for i, ks in enumerate(keys):
        g = []
        while p < len(lines) and lines[p].split("\t", 1)[0] in ks:
            g.append(_fields(lines[p], (ctx, i)))
            p += 1
        out.append(g)
    assert p == len(lines), ("record out of input order, or of an unknown read", lines[p].split("\t", 3)[:3], ctx)
    return out


def _unmapped_body(r, seq: bytes, qual, ctx):
    assert (r["rname"], r["pos"], r["mapq"], r["cigar"], r["rnext"], r["pnext"], r["tlen"]) == ("*", 0, 0, "*", "*", 0, 0), (r["line"], ctx)
    assert r["seq"] == seq.decode(), ("SEQ of an unmapped read", r["line"], ctx)
    assert r["qual"] == (qual or ""), ("QUAL of an unmapped read", r["line"], ctx)
    assert set(r["tags"]) == {"PG"}, (r["line"], ctx)


def _shown(r, fw: bytes, qual, strand: int, ctx):
    want_q = (qual[::-1] if strand else qual) if qual else "*"
    assert r["seq"] == (revcomp(fw) if strand else fw).decode(), ("SEQ", r["line"], ctx)
    assert r["qual"] == want_q, ("QUAL", r["line"], ctx)


def check_single_end(text: str, ref: Reference, reads, ids, quals, limit, unmapped: bool, xa: bool = False, best_mode: bool = False,
                     metric: str = "edit"):
    """every single-end rule on the SAM text of a chunk.  limit: the distance searched, one number or one per read (the cut-off of
    BEST mode); quals: a list (entries may be empty) or None; best_mode: nHits was counted before duplicates were removed, so it may
    exceed the records seen.  Returns counts."""
    names = [qname(s) for s in ids]
    assert len(set(names)) == len(names), "the checker needs distinct identifiers"
    groups = _groups(_lines(text), [{n} for n in names], "single-end")
    st = {"records": 0, "alignments": 0, "mapped": 0, "unmapped": 0, "absent": 0, "xa_entries": 0, "secondary": 0, "reverse": 0}
    a0, l0 = ref.alignments, ref.loose
    for i, g in enumerate(groups):
        fw = clean(reads[i])
        q = quals[i] if quals is not None else ""
        lim = int(limit[i]) if hasattr(limit, "__len__") else int(limit)
        st["records"] += len(g)
        if not g:
            assert not unmapped, ("no record for a read although unmapped records were asked for", i)
            st["absent"] += 1
            continue
        if g[0]["flag"] & 4:
            assert unmapped, ("unmapped record that was not asked for", i)
            assert len(g) == 1 and g[0]["flag"] == 4, ("an unmapped read has one record with flag 4", i)
            _unmapped_body(g[0], fw, q, i)
            st["unmapped"] += 1
            continue
        st["mapped"] += 1
        aln = []  # (rname, pos, cigar, nm, strand)
        for j, r in enumerate(g):
            assert r["flag"] in ((0, 16) if j == 0 else (256, 272)), ("flag", j, r["line"])
            assert (r["rnext"], r["pnext"], r["tlen"]) == ("*", 0, 0), r["line"]
            assert isinstance(r["tags"].get("NM"), int) and r["tags"]["AS"] == r["tags"]["NM"], ("AS and NM", r["line"])
            strand = (r["flag"] >> 4) & 1
            if j == 0:
                _shown(r, fw, q, strand, i)
            else:
                assert (r["seq"], r["qual"]) == ("*", "*"), ("a secondary record shows neither SEQ nor QUAL", r["line"])
            aln.append((r["rname"], r["pos"], r["cigar"], r["tags"]["NM"], strand))
        if xa:
            assert len(g) == 1, ("with the XA tag a read has one record", i)
            t = g[0]["tags"]
            assert set(t) == {"AS", "NM", "PG", "X0", "X1", "XA"}, g[0]["line"]
            entries = [e for e in t["XA"].split(";")]
            assert entries[-1] == "" and (len(entries) == 1 or t["XA"].endswith(";")), g[0]["line"]
            for e in entries[:-1]:
                name, pos, cig, nm = e.rsplit(",", 3)
                assert pos[0] in "+-", e
                aln.append((name, int(pos[1:]), cig, int(nm), int(pos[0] == "-")))
            st["xa_entries"] += len(entries) - 1
        else:
            assert all(set(r["tags"]) == {"AS", "NM", "PG"} for r in g), i
        for name, pos, cig, nm, strand in aln:
            ref.check_alignment(revcomp(fw) if strand else fw, name, pos, cig, nm, lim, metric, ctx=i)
            st["reverse"] += strand
        st["secondary"] += len(aln) - 1
        nms = [a[3] for a in aln]
        assert nms[0] == min(nms), ("the first alignment has the minimal NM of its group", i, nms)
        visible = nms.count(nms[0])
        for r in g:  # (MAPQ exists on records only)
            at_min = r["tags"]["NM"] == nms[0]
            if not at_min:
                assert r["mapq"] == 0, ("MAPQ above the minimal distance", r["line"])
            elif best_mode:
                assert 0 <= r["mapq"] <= mapq(visible), ("MAPQ", r["mapq"], visible, r["line"])
            else:
                assert r["mapq"] == mapq(visible), ("MAPQ", r["mapq"], visible, r["line"])
        if xa:
            x0, x1 = g[0]["tags"]["X0"], g[0]["tags"]["X1"]
            assert x0 + x1 == len(aln) - 1, ("X0 + X1 = XA entries", x0, x1, len(aln) - 1, i)
            assert x0 >= visible - 1 if best_mode else x0 == visible - 1, ("X0 = nHits - 1", x0, visible, i)
    st["alignments"], st["loose"] = ref.alignments - a0, ref.loose - l0
    return st


ORIENTATION_FF, ORIENTATION_FR, ORIENTATION_RF = 0, 1, 2


def _mate_of(r, others, ref: Reference):
    """a record of the other mate that r's RNEXT / PNEXT / flag 32 / TLEN describe, with the template length recomputed from POS and
    CIGAR of both"""
    rnext = r["rname"] if r["rnext"] == "=" else r["rnext"]
    for m in others:
        if m["flag"] & 4 or (m["rname"], m["pos"]) != (rnext, r["pnext"]) or bool(r["flag"] & 32) != bool(m["flag"] & 16):
            continue
        if abs(m["tlen"]) != abs(r["tlen"]):
            continue
        if (r["tlen"] < 0) != (r["pos"] > m["pos"]) and r["tlen"] != 0:
            continue
        if r["rname"] != m["rname"]:
            if r["tlen"] == 0:
                return m
            continue
        # searchstrategy.cpp:1310 (pairs), :1553-1556 (discordant pairs): index end of the downstream occurrence - begin of the upstream
        # one; upstream is the smaller begin (a tie: either end)
        ends = {x["pos"] - 1 + cigar_width(x["cigar"]) for x in ((m,) if m["pos"] > r["pos"] else (r,) if r["pos"] > m["pos"] else (r, m))}
        if any(e - (min(r["pos"], m["pos"]) - 1) == abs(r["tlen"]) for e in ends) and (r["tlen"] < 0) == (r["pos"] > m["pos"]):
            return m
    return None


def check_paired(text: str, ref: Reference, reads1, reads2, ids1, ids2, quals1, quals2, limit, orientation: int, min_frag: int,
                 max_frag: int, unmapped_records: bool = True, metric: str = "edit"):
    """every paired rule on the SAM text of a chunk of read pairs (records of cmb_sam_pe, cmb_sam_unpaired, cmb_sam_unmapped_pe).
    limit: one number, or per pair a (mate 1, mate 2) couple.  Returns (counts, per pair the records as dicts)."""
    n1, n2 = [qname(s) for s in ids1], [qname(s) for s in ids2]
    assert all(a != b for a, b in zip(n1, n2)) and len(set(n1 + n2)) == 2 * len(n1), "the checker needs distinct identifiers"
    groups = _groups(_lines(text), [{a, b} for a, b in zip(n1, n2)], "paired")
    st = {"records": 0, "proper": 0, "discordant": 0, "unpaired": 0, "unmapped": 0, "mate_unmapped": 0, "secondary": 0}
    a0, l0 = ref.alignments, ref.loose
    for i, g in enumerate(groups):
        st["records"] += len(g)
        per = ([r for r in g if r["qname"] == n1[i]], [r for r in g if r["qname"] == n2[i]])
        lims = limit[i] if hasattr(limit, "__len__") else (limit, limit)
        if unmapped_records:
            assert per[0] and per[1], ("a mate without a record", i)
        for m in (0, 1):
            fw = clean((reads1, reads2)[m][i])
            q = (quals1, quals2)[m][i] if (quals1, quals2)[m] is not None else ""
            mine, others = per[m], per[1 - m]
            mate_unmapped = bool(others) and all(o["flag"] & 4 for o in others)
            for r in mine:
                f = r["flag"]
                assert f & 1, ("flag 1", r["line"])
                assert bool(f & 64) != bool(f & 128) and bool(f & 64) == (m == 0), ("flags 64 / 128 name the file of the read", r["line"])
                assert not f & ~(1 | 2 | 4 | 8 | 16 | 32 | 64 | 128 | 256), ("unknown flag", r["line"])
                if f & 4:
                    assert len(mine) == 1 and not f & (2 | 16 | 256), ("an unmapped mate has one record", r["line"])
                    _unmapped_body(r, fw, q, i)
                    assert bool(f & 8) == mate_unmapped, ("flag 8 exactly when the mate's record carries flag 4", r["line"])
                    st["unmapped"] += 1
                    continue
                assert set(r["tags"]) == {"AS", "NM", "PG"} and r["tags"]["AS"] == r["tags"]["NM"], r["line"]
                st["secondary"] += bool(f & 256)
                if r["rnext"] == "*" and not f & 8:
                    # cmb_sam_unpaired (generateSAMUnpaired, indexhelpers.cpp:216-260): the mate is mapped but no pair was formed.  The
                    # record names no mate and carries no strand flag: the strand is the one SEQ shows (a secondary record shows none:
                    # either strand may hold the alignment)
                    assert not f & (2 | 16 | 32) and (r["pnext"], r["tlen"]) == (0, 0), r["line"]
                    assert others and not mate_unmapped, ("an unpaired record although the mate is unmapped", r["line"])
                    if f & 256:
                        assert (r["seq"], r["qual"]) == ("*", "*"), r["line"]
                        strands = (0, 1)
                    else:
                        strands = tuple(s for s in (0, 1) if r["seq"] == (revcomp(fw) if s else fw).decode())
                        assert strands, ("SEQ is neither the read nor its reverse complement", r["line"])
                        _shown(r, fw, q, strands[0], i)
                    err = None
                    for s in strands:
                        try:
                            ref.check_alignment(revcomp(fw) if s else fw, r["rname"], r["pos"], r["cigar"], r["tags"]["NM"], lims[m], metric, ctx=i)
                            err = None
                            break
                        except AssertionError as e:
                            err = e
                    if err is not None:
                        raise err
                    st["unpaired"] += 1
                    continue
                strand = (f >> 4) & 1
                _shown(r, fw, q, strand, i)   # (generateSAMPairedEnd shows SEQ and QUAL on every record)
                ref.check_alignment(revcomp(fw) if strand else fw, r["rname"], r["pos"], r["cigar"], r["tags"]["NM"], lims[m], metric, ctx=i)
                assert bool(f & 8) == mate_unmapped, ("flag 8 exactly when the mate's record carries flag 4", r["line"])
                if f & 8:
                    assert not f & (2 | 32) and (r["rnext"], r["pnext"], r["tlen"]) == ("*", 0, 0), r["line"]
                    st["mate_unmapped"] += 1
                    continue
                mate = _mate_of(r, others, ref)
                assert mate is not None, ("no record of the other mate fits RNEXT / PNEXT / flag 32 / TLEN", r["line"], [o["line"] for o in others])
                if f & 2:
                    assert mate["flag"] & 2 and r["rname"] == mate["rname"], ("proper pair across sequences", r["line"])
                    assert min_frag <= abs(r["tlen"]) <= max_frag, ("fragment outside its bounds", r["line"])
                    up, down = (r, mate) if (r["pos"], strand) <= (mate["pos"], (mate["flag"] >> 4) & 1) else (mate, r)
                    su, sd = (up["flag"] >> 4) & 1, (down["flag"] >> 4) & 1
                    want = {ORIENTATION_FR: (0, 1), ORIENTATION_RF: (1, 0)}.get(orientation)
                    if want is not None:
                        if up["pos"] == down["pos"]:
                            assert {su, sd} == {0, 1}, ("orientation", r["line"])
                        else:
                            assert (su, sd) == want, ("orientation", r["line"], mate["line"])
                    else:
                        assert su == sd, ("orientation", r["line"])
                    st["proper"] += 1
                else:
                    st["discordant"] += 1
    st["alignments"], st["loose"] = ref.alignments - a0, ref.loose - l0
    return st, groups
