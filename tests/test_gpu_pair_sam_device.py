"""Read pairs of an ALL-mode chunk paired and written on the device (cmb_pair_sam_device: csrc/dev_pair.hpp, k_pair_plan and k_pair_write)
against the host path over the same C-ABI: ca.pair_chunk_sam(..., per_strand=True), i.e. cmb_pair_sam pair by pair.  The comparison is
the text as bytes and the number of mapped pairs; what the world is built to show (a swapped primary, the MAPQ table, lists and pair
counts beyond a wavefront, host pairs between device pairs) is asserted on the text as well, so a world that lost it fails too.

The world: 40 kbp of random text in three sequences.
  chrA  [0, 20 000)        true fragments for the plain pairs; the pairs at the digit boundaries of POS and TLEN
  chrB  [20 000, 32 000)   four families: a 300 bp fragment planted once with a substitution under either mate (the copy at the lowest
                           position, so the FIRST concordant pair is not the best one) and then 1 ... 4 times exactly, 700 bp apart
  chrC  [32 000, 40 000)   a tandem of 76 copies of a 20 bp unit, three of them with a substitution
Reads are 60 - 100 characters, k = 2, strategy "columba" with edit distance.
"""
import contextlib
import os

import numpy as np
import pytest

import columba_amd as ca
import samcheck

pytestmark = pytest.mark.gpu

NAMES = ["chrA", "chrB", "chrC"]
STARTS = [0, 20_000, 32_000, 40_000]
K = 2
FAMILY_AT, FAMILY_LEN, FAMILY_STEP, FAMILY_READ = 20_500, 300, 700, 70
FAMILY_EXACT = (1, 2, 3, 4)  # exact copies per family, behind the edited one
UNIT, TANDEM_COPIES, TANDEM_AT = 20, 76, 33_000
ORIENTATIONS = [ca.ORIENTATION_FR, ca.ORIENTATION_RF, ca.ORIENTATION_FF]
ORI_NAME = {ca.ORIENTATION_FR: "FR", ca.ORIENTATION_RF: "RF", ca.ORIENTATION_FF: "FF"}


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


def _sub(b: bytearray, p: int):
    b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1) % 4]


def _text():
    rng = np.random.default_rng(11)
    g = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, STARTS[-1])].tobytes())
    families, at = [], FAMILY_AT
    for exact in FAMILY_EXACT:
        frag = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, FAMILY_LEN)].tobytes())
        homes = []
        for c in range(exact + 1):
            g[at:at + FAMILY_LEN] = frag
            if c == 0:  # the copy the first concordant pair lies on: one edit under either mate, summed distance 2
                _sub(g, at + 30)
                _sub(g, at + FAMILY_LEN - 30)
            homes.append(at)
            at += FAMILY_STEP
        families.append({"frag": frag, "homes": homes})
    assert at < STARTS[2]
    unit = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, UNIT)].tobytes())
    g[TANDEM_AT:TANDEM_AT + UNIT * TANDEM_COPIES] = unit * TANDEM_COPIES
    for c in (10, 30, 50):
        _sub(g, TANDEM_AT + UNIT * c + 5)
    return bytes(g), families, unit


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from columba_amd import indexbuild as ib
    text, families, unit = _text()
    ix = ib.build_index(text, seq_starts=np.asarray(STARTS, np.uint32), device="cuda")
    ix.seq_names = NAMES
    return {"text": text, "families": families, "unit": unit, "dev": ca.Index(ix), "st": ca.SearchStrategy("columba", "edit", "dynamic")}


def _mates(up: bytes, down: bytes, orientation: int, swapped: bool):
    """(read 1, read 2) of a pair whose upstream mate shows `up` and whose downstream mate shows `down` of the forward text; swapped: the
    second combination of the orientation (read 2 upstream)"""
    rc = samcheck.revcomp
    if orientation == ca.ORIENTATION_FR:
        a, b = up, rc(down)
    elif orientation == ca.ORIENTATION_RF:
        a, b = rc(up), down
    else:
        a, b = (rc(down), rc(up)) if swapped else (up, down)
        return a, b
    return (b, a) if swapped else (a, b)


def _fragment(w, p0: int, frag: int, l1: int, l2: int, orientation: int, swapped: bool):
    t = w["text"]
    return _mates(t[p0:p0 + l1], t[p0 + frag - l2:p0 + frag], orientation, swapped)


def _random_read(rng, n: int) -> bytes:
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())


def _quals(rng, reads):
    return ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]


def _ids(n: int, mate: int):
    return [f"@p{i}/{mate} len x" for i in range(n)]


# ---------------------------------------------------------------------------------- what the host lists say about a chunk
def _lists(w, reads):
    b = ca.Batch(w["dev"], w["st"], K, reads=reads)
    b.want_alignments()
    ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
    b.run()
    occ, offs, _ = b.results()
    aln, _ = b.alignments()
    b.close()
    return [[{"seq": int(aln["seq_id"][j]), "begin": int(occ["begin"][j]), "end": int(occ["end"][j]), "distance": int(occ["distance"][j]),
              "strand": int(occ["strand"][j]), "spans": int(aln["spans"][j])} for j in range(int(offs[i]), int(offs[i + 1]))]
            for i in range(len(reads))]


def _concordant_pairs(l1, l2, orientation: int, min_frag: int, max_frag: int) -> int:
    """pairOccurrences over the two combinations of the orientation (searchstrategy.cpp:1281-1344): the number of pairs"""
    def strand(lst, s):
        return sorted((o for o in lst if o["strand"] == s), key=lambda o: (o["begin"], o["distance"], o["end"] - o["begin"]))
    combos = {ca.ORIENTATION_FR: (((l1, 0), (l2, 1)), ((l2, 0), (l1, 1))), ca.ORIENTATION_RF: (((l1, 1), (l2, 0)), ((l2, 1), (l1, 0))),
              ca.ORIENTATION_FF: (((l1, 0), (l2, 0)), ((l2, 1), (l1, 1)))}[orientation]
    n = 0
    for (ul, us), (dl, ds) in combos:
        ups, downs = strand(ul, us), strand(dl, ds)
        for u in ups:
            for d in (d for d in downs if d["begin"] >= u["begin"]):
                frag = d["end"] - u["begin"]
                if frag > max_frag:
                    break
                n += frag >= min_frag and d["seq"] == u["seq"]
    return n


def _host_pairs(l1, l2, orientation: int, min_frag: int, max_frag: int):
    """the pairs the device leaves to the host: an occurrence over the end of its sequence, or lists that are not both empty and hold no
    concordant pair"""
    return [i for i, (a, b) in enumerate(zip(l1, l2))
            if any(o["spans"] for o in a + b) or ((a or b) and not _concordant_pairs(a, b, orientation, min_frag, max_frag))]


def _both(w, r1, r2, ids1, ids2, q1, q2, orientation, max_frag, min_frag, discordant=True, unmapped=True):
    """(text and mapped pairs of the host path, of the device path, the device path's stats); q1 / q2 None: no qualities"""
    hq1, hq2 = (q1, q2) if q1 is not None else ([""] * len(r1), [""] * len(r2))
    want, want_mapped = ca.pair_chunk_sam(w["dev"], w["st"], K, r1, r2, ids1, ids2, hq1, hq2, NAMES, orientation, max_frag, min_frag, discordant, unmapped,
                                          per_strand=True)
    got, mapped, stats = ca.pair_chunk_sam_device(w["dev"], w["st"], K, r1, r2, ids1, ids2, q1, q2, NAMES, orientation, max_frag, min_frag, discordant,
                                                  unmapped)
    return want, want_mapped, got, mapped, stats


def _same(want, want_mapped, got, mapped, stats):
    if got.encode() != want.encode():
        wl, gl = want.splitlines(), got.splitlines()
        at = next((i for i, (a, b) in enumerate(zip(wl, gl)) if a != b), min(len(wl), len(gl)))
        raise AssertionError(("the device text differs from the host text", len(want), len(got), at, wl[at:at + 2], gl[at:at + 2]))
    assert mapped == want_mapped == stats["mapped_pairs"]
    assert stats["device_records"] <= len(got.splitlines())


def _groups(text: str, n: int):
    """the records of every pair, by the pair's number in the identifier"""
    out = [[] for _ in range(n)]
    for line in text.splitlines():
        f = line.split("\t")
        out[int(f[0][1:].split("/")[0])].append(f)
    return out


# ---------------------------------------------------------------------------------- 1. orientations and options
def _plain_chunk(w, orientation: int, n: int = 203):
    rng = np.random.default_rng(100 + orientation)
    r1, r2 = [], []
    for i in range(n):
        frag = int(rng.integers(150, 501))
        l1, l2 = int(rng.integers(60, 101)), int(rng.integers(60, 101))
        p0 = int(rng.integers(300, STARTS[1] - 800))
        a, b = _fragment(w, p0, frag, l1, l2, orientation, bool(i % 2))
        a, b = bytearray(a), bytearray(b)
        if i % 3:
            _sub(a, int(rng.integers(8, len(a) - 8)))
        if i % 3 == 2:
            _sub(b, int(rng.integers(8, len(b) - 8)))
        if i % 11 == 0:
            b[12] = ord("N")
        r1.append(bytes(a))
        r2.append(bytes(b))
    return r1, r2


@pytest.mark.parametrize("with_quals", [True, False], ids=["quals", "noquals"])
@pytest.mark.parametrize("unmapped", [True, False], ids=["unmapped", "nounmapped"])
@pytest.mark.parametrize("discordant", [True, False], ids=["disc", "nodisc"])
@pytest.mark.parametrize("orientation", ORIENTATIONS, ids=lambda o: ORI_NAME[o])
def test_orientations_and_options(world, orientation, discordant, unmapped, with_quals):
    r1, r2 = _plain_chunk(world, orientation)
    n = len(r1)
    rng = np.random.default_rng(5)
    q1, q2 = (_quals(rng, r1), _quals(rng, r2)) if with_quals else (None, None)
    want, want_mapped, got, mapped, stats = _both(world, r1, r2, _ids(n, 1), _ids(n, 2), q1, q2, orientation, 500, 150, discordant, unmapped)
    key = ("plain lists", orientation)  # (the lists depend on the reads alone)
    if key not in world:
        world[key] = (_lists(world, r1), _lists(world, r2))
    host = _host_pairs(*world[key], orientation, 150, 500)
    print(f"{ORI_NAME[orientation]}: {n} pairs, {len(host)} for the host, {stats}")
    _same(want, want_mapped, got, mapped, stats)
    assert stats["host_pairs"] == len(host)
    assert n - stats["host_pairs"] >= 0.8 * n, "the device classes hold the chunk"
    assert stats["device_records"] >= 2 * (n - len(host)) and mapped >= n - len(host)


# ---------------------------------------------------------------------------------- 2. several concordant pairs per read pair
def test_several_concordant_pairs_and_the_swap(world):
    rc = samcheck.revcomp
    r1 = [f["frag"][:FAMILY_READ] for f in world["families"]]
    r2 = [rc(f["frag"][-FAMILY_READ:]) for f in world["families"]]
    n = len(r1)
    rng = np.random.default_rng(6)
    want, want_mapped, got, mapped, stats = _both(world, r1, r2, _ids(n, 1), _ids(n, 2), _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 500, 100)
    _same(want, want_mapped, got, mapped, stats)
    assert stats["host_pairs"] == 0 and mapped == n
    seen = set()
    for fam, exact, recs in zip(world["families"], FAMILY_EXACT, _groups(got, n)):
        assert len(recs) == 2 * (exact + 1)  # one pair per copy
        edited = fam["homes"][0] - STARTS[1] + 1
        prim = [f for f in recs if not int(f[1]) & 256]
        assert [int(f[1]) & 192 for f in prim] == [64, 128] and recs[:2] == prim
        assert int(prim[0][3]) != edited and int(prim[0][3]) == fam["homes"][1] - STARTS[1] + 1, "the primary is the first pair of minimal distance"
        for f in recs:
            on_edited = int(f[3]) in (edited, edited + FAMILY_LEN - FAMILY_READ)
            assert int(f[4]) == (0 if on_edited else samcheck.mapq(exact)), f
            assert f[12] == ("NM:i:1" if on_edited else "NM:i:0"), f
            seen.add(int(f[4]))
        # the swap: the first pair's records stand where the primary's would have stood — third and fourth line
        assert [int(f[3]) for f in recs[2:4]] == [edited, edited + FAMILY_LEN - FAMILY_READ]
    assert seen == {0, 60, 3, 2, 1}


# ---------------------------------------------------------------------------------- 3. more than a wavefront
def _tandem_chunk(w):
    unit, rc = w["unit"], samcheck.revcomp
    period = unit * 5
    r1, r2 = [], []
    rng = np.random.default_rng(8)
    for i in range(7):  # (not a multiple of the four wavefronts of a block of k_pair_plan, nor of the pairs per wavefront of k_pair_write)
        if i in (1, 3, 6):
            a, b = period[i:i + 60], rc(period[7 + i:7 + i + 64])
        else:
            p0 = int(rng.integers(300, STARTS[1] - 800))
            a, b = _fragment(w, p0, 320, 80, 75, ca.ORIENTATION_FR, False)
        r1.append(a if i != 3 else b)
        r2.append(b if i != 3 else a)
    return r1, r2


def test_lists_and_pairs_beyond_a_wavefront(world):
    """(k_pair_plan and k_pair_write are launched with a block per four and per eight pairs, on grids that are not capped: there is no
    second trip of a lane's loop for CMB_TEST_GRID_CAP to force, so no such variant)"""
    r1, r2 = _tandem_chunk(world)
    n = len(r1)
    max_frag = UNIT * TANDEM_COPIES + 80
    rng = np.random.default_rng(9)
    want, want_mapped, got, mapped, stats = _both(world, r1, r2, _ids(n, 1), _ids(n, 2), _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, max_frag, 60)
    l1, l2 = _lists(world, r1), _lists(world, r2)
    _same(want, want_mapped, got, mapped, stats)
    for i in (1, 3, 6):
        assert max(sum(o["strand"] == s for o in l[i]) for l in (l1, l2) for s in (0, 1)) > 64, "a strand list beyond a wavefront"
        assert _concordant_pairs(l1[i], l2[i], ca.ORIENTATION_FR, 60, max_frag) > 64
    groups = _groups(got, n)
    assert all(len(groups[i]) > 2 * 64 for i in (1, 3, 6)) and all(len(groups[i]) == 2 for i in (0, 2, 4, 5))
    assert stats["host_pairs"] == 0 and stats["device_records"] == len(got.splitlines())
    print(f"tandem: {[len(g) for g in groups]} records per pair, {len(got)} bytes")


# ---------------------------------------------------------------------------------- 4. host classes between device pairs
def _host_class_chunk(w):
    rng = np.random.default_rng(12)
    t, rc = w["text"], samcheck.revcomp
    plain = lambda p0: _fragment(w, p0, 300, 70, 80, ca.ORIENTATION_FR, False)  # noqa: E731
    pairs, cls = [], []
    def add(c, p):
        cls.append(c)
        pairs.append(p)
    add("plain", plain(1200))
    add("spans", (t[STARTS[1] - 330:STARTS[1] - 260], rc(t[STARTS[1] - 40:STARTS[1] + 30])))  # mate 2 lies over the end of chrA
    add("plain", plain(2500))
    add("two_sequences", (t[5000:5070], rc(t[STARTS[2] + 5000:STARTS[2] + 5080])))
    add("plain", plain(3100))
    add("one_unmapped", (t[6000:6075], _random_read(rng, 70)))
    add("both_unmapped", (_random_read(rng, 64), _random_read(rng, 90)))
    add("plain", plain(4100))
    add("too_far", _fragment(w, 8000, 900, 70, 70, ca.ORIENTATION_FR, False))
    add("plain", plain(9300))
    add("one_unmapped", (_random_read(rng, 61), t[12000:12100]))
    return [p[0] for p in pairs], [p[1] for p in pairs], cls


@pytest.mark.parametrize("unmapped", [True, False], ids=["unmapped", "nounmapped"])
@pytest.mark.parametrize("discordant", [True, False], ids=["disc", "nodisc"])
def test_host_classes_are_spliced_in_at_their_place(world, discordant, unmapped):
    r1, r2, cls = _host_class_chunk(world)
    n = len(r1)
    rng = np.random.default_rng(13)
    want, want_mapped, got, mapped, stats = _both(world, r1, r2, _ids(n, 1), _ids(n, 2), _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 500, 100,
                                                  discordant, unmapped)
    _same(want, want_mapped, got, mapped, stats)
    l1, l2 = _lists(world, r1), _lists(world, r2)
    assert any(o["spans"] for o in l2[cls.index("spans")]), "the world's mate over a sequence end"
    host = _host_pairs(l1, l2, ca.ORIENTATION_FR, 100, 500)
    assert [cls[i] for i in host] == ["spans", "two_sequences", "one_unmapped", "too_far", "one_unmapped"]
    assert stats["host_pairs"] == len(host)
    order = [int(line.split("\t")[0][1:].split("/")[0]) for line in got.splitlines()]
    assert order == sorted(order), "pair order"
    flags = {i: [int(f[1]) for f in g] for i, g in enumerate(_groups(got, n))}
    assert all(flags[i] and all(f & 2 for f in flags[i]) for i, c in enumerate(cls) if c == "plain")
    assert flags[cls.index("both_unmapped")] == ([77, 141] if unmapped else [])
    far = flags[cls.index("too_far")]
    assert far and not any(f & 2 for f in far) and all(bool(f & 1) for f in far)


def test_empty_qualities_among_present_ones(world):
    """an empty entry of a quality array that is there: "*" on a mapped record (device and host class), nothing on an unmapped one"""
    r1, r2, cls = _host_class_chunk(world)
    n = len(r1)
    rng = np.random.default_rng(16)
    q1, q2 = _quals(rng, r1), _quals(rng, r2)
    for i in range(n):  # read 1 of every second pair, read 2 of every third one; both reads of the pair without any occurrence
        if i % 2 == 0 or cls[i] == "both_unmapped":
            q1[i] = ""
        if i % 3 == 0 or cls[i] == "both_unmapped":
            q2[i] = ""
    want, want_mapped, got, mapped, stats = _both(world, r1, r2, _ids(n, 1), _ids(n, 2), q1, q2, ca.ORIENTATION_FR, 500, 100)
    _same(want, want_mapped, got, mapped, stats)
    groups = _groups(got, n)
    assert [f[10] for f in groups[cls.index("both_unmapped")]] == ["", ""]
    plain = groups[0]
    assert cls[0] == "plain" and [f[10] for f in plain] == ["*", "*"]
    mixed = groups[cls.index("plain", 1)]  # pair 2: read 1 without a quality, read 2 (reverse complement) with its quality reversed
    assert [f[10] for f in mixed] == ["*", q2[2][::-1]]


# ---------------------------------------------------------------------------------- 5. composite batches
def test_composite_batches(world):
    n = 50  # sub-batches [0, 16), [16, 33), [33, 50) (cmb_batch_create: equal shares, rounded down)
    bounds = [int(n * (j / 3.0)) for j in range(3)] + [n]
    assert bounds == [0, 16, 33, 50]
    at_host = {0, 15, 16, 32, 33, 49}  # first and last pair of every sub-batch
    rng = np.random.default_rng(14)
    t = world["text"]
    r1, r2 = [], []
    for i in range(n):
        p0 = 400 + 350 * i
        if i in at_host:  # (alternately: mates further apart than max_frag, and an unmapped mate)
            a, b = _fragment(world, p0, 900, 70, 70, ca.ORIENTATION_FR, False) if i % 2 else (t[p0:p0 + 80], _random_read(rng, 66))
        else:
            a, b = _fragment(world, p0, 280 + i, 60 + i % 40, 100 - i % 40, ca.ORIENTATION_FR, bool(i % 2))
        r1.append(a)
        r2.append(b)
    with _env(CMB_SUBBATCHES="3"):
        want, want_mapped, got, mapped, stats = _both(world, r1, r2, _ids(n, 1), _ids(n, 2), _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 500, 100)
        host = _host_pairs(_lists(world, r1), _lists(world, r2), ca.ORIENTATION_FR, 100, 500)
    _same(want, want_mapped, got, mapped, stats)
    assert set(host) == at_host and stats["host_pairs"] == len(at_host)
    assert stats["device_records"] == 2 * (n - len(at_host))


def test_counts_beyond_two_to_the_twenty_pairs(world):
    """more than 2^20 mapped pairs in one call, in one sub-batch (a batch is split from 2 * 10^6 reads on): the counts of the statistics
    are sums over the chunk and must not run into each other.  128 concordant pairs, held to the host path, 8200 times over under the
    same identifiers: pairs do not depend on their neighbours, so the text is the small one that many times."""
    r1, r2 = _plain_chunk(world, ca.ORIENTATION_FR, 128)
    ids1, ids2 = _ids(128, 1), _ids(128, 2)
    want, want_mapped, unit, mapped, stats = _both(world, r1, r2, ids1, ids2, None, None, ca.ORIENTATION_FR, 500, 150)
    _same(want, want_mapped, unit, mapped, stats)
    assert mapped == 128 and stats["device_records"] == 256 and stats["host_pairs"] == 0
    reps = 8200
    n = 128 * reps
    assert n > 1 << 20

    def tiled(fields):
        buf, offs = ca.pack_fields(fields)
        size = int(offs[-1])
        return np.tile(buf[:size], reps), np.concatenate([[0], (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(size) + offs[1:][None, :]).ravel()]).astype(np.uint64)

    batches = []
    for reads in (r1, r2):
        b = ca.Batch(world["dev"], world["st"], K, packed=tiled(reads))
        b.want_alignments()
        ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
        b.run()
        batches.append(b)
    text, stats = ca.pair_batches_sam_device(batches[0], batches[1], tiled(ids1), tiled(ids2), None, None, NAMES, ca.ORIENTATION_FR, 500, 150)
    for b in batches:
        b.close()
    assert stats == {"host_pairs": 0, "mapped_pairs": n, "device_records": 2 * n}
    assert len(text) == len(unit) * reps and text == unit.encode() * reps


# ---------------------------------------------------------------------------------- 6. lengths at the digit boundaries
def test_digit_boundaries_of_pos_and_tlen(world):
    """POS of 1 to 5 digits on either side of every boundary, TLEN of 2, 3 and 4 digits likewise (a fragment is at least as long as its
    downstream mate, so TLEN has two digits at least), the negative TLEN of every downstream record, identifiers cut at their space"""
    cases = [(pos, 300) for pos in (9, 10, 99, 100, 999, 1000, 9999, 10000)] + [(2000, frag) for frag in (99, 100, 999, 1000)]
    r1, r2, ids1, ids2 = [], [], [], []
    for i, (pos, frag) in enumerate(cases):
        a, b = _fragment(world, pos - 1, frag, 62, 60, ca.ORIENTATION_FR, bool(i % 2))
        r1.append(a)
        r2.append(b)
        ids1.append(f"@p{i}/1" + (" with a comment" if i % 3 else "") + (" " if i % 3 == 2 else ""))
        ids2.append(f"@p{i}/2 {i}" if i % 2 else f"@p{i}/2")
    n = len(cases)
    rng = np.random.default_rng(15)
    want, want_mapped, got, mapped, stats = _both(world, r1, r2, ids1, ids2, _quals(rng, r1), _quals(rng, r2), ca.ORIENTATION_FR, 1000, 60)
    _same(want, want_mapped, got, mapped, stats)
    assert stats["host_pairs"] == 0 and mapped == n
    for (pos, frag), recs, i1, i2 in zip(cases, _groups(got, n), ids1, ids2):
        assert len(recs) == 2
        up, down = recs
        assert {up[0], down[0]} == {samcheck.qname(i1), samcheck.qname(i2)}
        assert (int(up[3]), int(up[7]), int(up[8])) == (pos, pos + frag - 60, frag)
        assert (int(down[3]), int(down[7]), down[8]) == (pos + frag - 60, pos, f"-{frag}")


# ---------------------------------------------------------------------------------- 7. refusals
def _batch(w, reads, alignments=True, per_strand=True, run=True):
    b = ca.Batch(w["dev"], w["st"], K, reads=reads)
    if alignments:
        b.want_alignments()
    if per_strand:
        ca._chk(ca.lib().cmb_batch_filter_per_strand(b.h, 1))
    if run:
        b.run()
    return b


@pytest.mark.parametrize("what", ["read_counts", "no_alignments", "no_per_strand", "not_run"])
def test_refusals(world, what):
    r1, r2 = _plain_chunk(world, ca.ORIENTATION_FR, 6)
    good = _batch(world, r1)
    bad_reads = r2[:5] if what == "read_counts" else r2
    bad = _batch(world, bad_reads, alignments=what != "no_alignments", per_strand=what != "no_per_strand", run=what != "not_run")
    q = ["I" * len(r) for r in r1]
    for first, second, reads_a, reads_b in ((good, bad, r1, bad_reads), (bad, good, bad_reads, r1)):
        with pytest.raises(ca.CmbError) as e:
            ca.pair_batches_sam_device(first, second, _ids(len(reads_a), 1), _ids(len(reads_b), 2), None, None, NAMES)
        assert e.value.code == -1 and str(e.value), "CMB_ERR_INVALID with a message"
    # the device is as it was: the same batch pairs with a proper mate
    mate = _batch(world, r2)
    text, stats = ca.pair_batches_sam_device(good, mate, _ids(6, 1), _ids(6, 2), q, q, NAMES, ca.ORIENTATION_FR, 500, 150)
    want, _ = ca.pair_chunk_sam(world["dev"], world["st"], K, r1, r2, _ids(6, 1), _ids(6, 2), q, q, NAMES, ca.ORIENTATION_FR, 500, 150, True, True)
    assert text.decode() == want and stats["mapped_pairs"] == 6
    for b in (good, bad, mate):
        b.close()
