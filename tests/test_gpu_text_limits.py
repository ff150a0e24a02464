"""The FM path at the 32-bit text limit: one index over a text of 0xFFFFFFFE characters ('$' included), the longest
`cmb_index_create` accepts.

Every other GPU test builds texts of at most 48 Mbp, so only the low 26 bits of the 32-bit text positions and
suffix-array rows (filter keys, verification keys, packed-text loads, k_fmocc, rank blocks, SA samples) are ever set
there.  The text here is uniform ACGT with planted material that puts hits of both search paths at high positions:

  element   a 2 kb consensus copied 64 times at 2-5 % divergence (substitutions): half the copies below 2^31, half
            above, four of them in the last 2 Mbp; its SA ranges are wider than the in-text switch point
  stretch   an exact copy of 256 kbp from near position 0, placed so that it covers the first half of the last
            window: reads from there have hits almost 2^32 apart
  the rest  uniform, low-copy: found by in-text verification

Checks: the index primitives on rows at the top of the row space (A1), soundness / window completeness against textbook
dynamic programming and parity with `oracle/` for every key layout (A2), CIGARs, SAM positions and BEST mode at high
positions (A3).
"""
import bisect
import time

import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth
from test_ground_truth import check_completeness, check_soundness, clean, gt  # noqa: F401  (gt: the fixture)
from test_gpu_parity import _compare

N_TEXT = 0xFFFFFFFE       # characters, '$' included
L = N_TEXT - 1            # ACGT characters
TOP = 1 << 31
W = 1 << 18               # window length
WINDOWS = {"start": 0, "mid": TOP - W // 2, "last": L - W}
ELEM = 2000
STRETCH, STRETCH_SRC = 1 << 18, 1024
STRETCH_DST = L - W - W // 2
SEQ_STARTS = np.array([0, 1 << 30, TOP, 3 << 30, L - 10_000, L], np.uint64)   # (the last entry: the '$')
SEQ_NAMES = [f"chr{i + 1}" for i in range(len(SEQ_STARTS) - 1)]


def test_doubling_keys_fit_the_largest_accepted_text():
    """suffix_array's int64 doubling keys at the longest text cmb_index_create accepts (0xFFFFFFFE characters); its
    guard refused the last lengths below 2^32 although their keys fit"""
    assert ib.doubling_key_fits(N_TEXT) and ib.doubling_key_fits(N_TEXT - 1) and ib.doubling_key_fits(1 << 31)
    assert not ib.doubling_key_fits(1 << 32) and not ib.doubling_key_fits(1 << 33)
    n = N_TEXT
    half = n // 2
    lo, hi = (1 - half) * (n + 1), (n - half) * (n + 1) + n
    assert -(2 ** 63) <= lo and hi < 2 ** 63


def _element_positions(rng):
    below = [150_000] + [(1 << 26) * i + int(rng.integers(0, 1 << 20)) for i in range(1, 32)]
    above = [TOP + 30_000] + [TOP + (1 << 26) * i + int(rng.integers(0, 1 << 20)) for i in range(1, 28)]
    above += [L - 1_500_000, L - 900_000, L - 400_000, L - 60_000]   # the last 2 Mbp (the last one in the last window)
    return below + above


def _text_4g(device):
    """(uint8 ASCII tensor of L characters on `device`, element consensus, element positions): seeded, cheap"""
    import torch
    gen = torch.Generator(device=device)
    gen.manual_seed(4242)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)
    g = torch.empty(L, dtype=torch.uint8, device=device)
    for o in range(0, L, 1 << 28):
        m = min(1 << 28, L - o)
        g[o:o + m] = acgt[torch.randint(0, 4, (m,), generator=gen, device=device, dtype=torch.uint8).long()]
    rng = np.random.default_rng(4242)
    cons = synth.ACGT[rng.integers(0, 4, ELEM)]
    pos = _element_positions(rng)
    for p in pos:
        cp = synth._mutate(rng, cons, float(rng.uniform(0.02, 0.05)))
        g[p:p + ELEM] = torch.from_numpy(cp).to(device)
    g[STRETCH_DST:STRETCH_DST + STRETCH] = g[STRETCH_SRC:STRETCH_SRC + STRETCH].clone()
    return g, cons.tobytes(), pos


class _Text:
    """bytes-like view of the 4 G text for the ground-truth helpers (slices are copied, the whole never is)"""

    def __init__(self, a):
        self.a = a

    def __len__(self):
        return int(self.a.shape[0])

    def __getitem__(self, s):
        return self.a[s].tobytes()


@pytest.fixture(scope="module")
def top(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    g, cons, pos = _text_4g("cuda")
    ix = ib.build_index(g, seq_starts=SEQ_STARTS.astype(np.uint32), seq_names=SEQ_NAMES, device="cuda", with_bwt=True)
    del g
    torch.cuda.synchronize()
    build_s, peak = time.time() - t0, torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print(f"\n[text limits] index over {N_TEXT} characters built in {build_s:.1f} s, peak {peak / 2 ** 30:.1f} GiB allocated")
    assert ix.n == N_TEXT and ix.text[-1] == ord("$")
    w = {"ix": ix, "text": _Text(ix.text), "cons": cons, "pos": pos, "dev": ca.Index(ix), "orc": op.OracleIndex(ix), "op": op}
    yield w
    w["dev"].close()
    del w["orc"]


# ------------------------------------------------------------------------------------------------ A1: index primitives
def _rows(n, rng):
    blocks = [np.arange(0, 1 << 16), np.arange(TOP - (1 << 14), TOP + (1 << 14)), np.arange(n - (1 << 16), n)]
    return blocks, np.setdiff1d(rng.integers(0, n, 1 << 15), np.concatenate(blocks))


def _sampled_rank(ix, rows):
    """(sampled?, number of sampled rows before) of every row from the rank9 bit vector of the sparse SA"""
    words, cnt = ix.sa_bv, ix.sa_bv_counts
    rows = rows.astype(np.int64)
    w = rows >> 6
    bit = ((words[w] >> (rows & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    blk = rows >> 9
    rank = cnt[2 * blk].astype(np.int64)
    for j in range(8):
        wj = blk * 8 + j
        rank += np.where(wj < w, np.bitwise_count(words[np.minimum(wj, words.shape[0] - 1)]), 0).astype(np.int64)
    low = words[w] & ((np.uint64(1) << (rows & 63).astype(np.uint64)) - np.uint64(1))
    return bit, rank + np.bitwise_count(low).astype(np.int64)


def _suffix_less(T, p, q):
    """text[p:] < text[q:] for every pair, compared on the host up to the first difference ('$' is unique and smallest)"""
    n = T.shape[0]
    ar = np.arange(32)
    a = T[np.minimum(p[:, None] + ar, n - 1)]
    b = T[np.minimum(q[:, None] + ar, n - 1)]
    ne = a != b
    has = ne.any(1)
    first = ne.argmax(1)
    idx = np.flatnonzero(has)
    res = np.zeros(p.shape[0], bool)
    res[idx] = a[idx, first[idx]] < b[idx, first[idx]]
    for i in np.flatnonzero(~has):   # (long common prefixes: the planted repeats)
        x, y, o, step = int(p[i]), int(q[i]), 32, 1024
        while True:
            u, v = T[x + o:x + o + step], T[y + o:y + o + step]
            m = min(u.shape[0], v.shape[0])
            d = np.flatnonzero(u[:m] != v[:m])
            if d.size:
                res[i] = u[d[0]] < v[d[0]]
                break
            assert m == step, (x, y, "suffixes compare equal")
            o, step = o + step, step * 4
    return res


@pytest.mark.gpu
def test_locate_sorted_and_rank_steps_at_the_top_of_the_row_space(top):
    ix, dev, orc = top["ix"], top["dev"], top["orc"]
    n, T = ix.n, ix.text
    rng = np.random.default_rng(1)
    blocks, rnd = _rows(n, rng)
    rows = np.concatenate(blocks + [rnd]).astype(np.uint32)
    pos, lf = dev.locate(rows)
    opos, olf = orc.locate(rows)
    bad = np.flatnonzero(pos != opos)
    assert bad.size == 0, [(int(rows[i]), int(pos[i]), int(opos[i])) for i in bad[:8]]
    assert lf == olf
    assert int(pos.max()) < n and len(np.unique(pos)) == len(pos)
    sampled, before = _sampled_rank(ix, rows)
    assert np.array_equal(sampled, pos % ix.sparseness == 0)
    assert np.array_equal(pos[sampled], ix.sa_samples[before[sampled]])
    assert sampled.sum() > 10_000 and int(pos.max()) >= TOP
    # adjacent rows are sorted, and the rank step is the BWT character (neither needs oracle/)
    o = 0
    for blk in blocks:
        p = pos[o:o + blk.shape[0]].astype(np.int64)
        less = _suffix_less(T, p[:-1], p[1:])
        bad = np.flatnonzero(~less)
        assert bad.size == 0, [(int(blk[i]), int(p[i]), int(p[i + 1])) for i in bad[:8]]
        bwt = np.where(p > 0, T[np.maximum(p - 1, 0)], ord("$"))
        r = blk.astype(np.uint64)
        prev = np.zeros(r.shape[0], np.int64)
        for c, ch in enumerate(b"ACGT"):   # (rank(c, .) counts the characters A ... c: the cumulative BitvecIntl encoding)
            cc = np.full(r.shape[0], c, np.uint32)
            step = dev.rank(0, cc, r + np.uint64(1)).astype(np.int64) - dev.rank(0, cc, r).astype(np.int64)
            bad = np.flatnonzero(step - prev != (bwt == ch))
            assert bad.size == 0, [(int(blk[i]), chr(ch), int(step[i] - prev[i]), int(p[i])) for i in bad[:8]]
            prev = step
        o += blk.shape[0]


@pytest.mark.gpu
def test_rank_and_extend_at_the_top_of_the_row_space(top):
    ix, dev, orc = top["ix"], top["dev"], top["orc"]
    n = ix.n
    rng = np.random.default_rng(2)
    p = np.concatenate([[0, 1, n - 1, n], rng.integers(TOP, n + 1, 20_000), rng.integers(0, n + 1, 4000),
                        np.arange(TOP - 64, TOP + 64)]).astype(np.uint64)
    for rev in (0, 1):
        for c in range(4):
            cc = np.full(p.shape[0], c, np.uint32)
            d, o = dev.rank(rev, cc, p), orc.rank(rev, cc, p)
            bad = np.flatnonzero(d != o)
            assert bad.size == 0, [(rev, c, int(p[i]), int(d[i]), int(o[i])) for i in bad[:8]]
    b = np.concatenate([rng.integers(TOP, n, 6000), rng.integers(n - (1 << 20), n, 6000)])
    wd = np.minimum((2.0 ** rng.uniform(0, 31, b.shape[0])).astype(np.int64), n - b)
    b2 = np.concatenate([rng.integers(TOP, n, 6000), rng.integers(0, n, 6000)])
    r = np.stack([b, b + wd, b2, np.minimum(b2 + wd, n)], axis=1).astype(np.uint32)
    r[0] = [0, n, 0, n]
    r[1] = [n - 1, n, n - 1, n]
    r[2] = [TOP - 1, TOP + 1, 0, n]
    for mode in (0, 1, 2):
        do, dk = dev.extend(mode, r)
        oo, ok = orc.extend(mode, r)
        bad = np.flatnonzero((do != oo).any(axis=(1, 2)) | (dk != ok).any(axis=1))
        assert bad.size == 0, [(mode, r[i].tolist(), do[i].tolist(), oo[i].tolist()) for i in bad[:4]]


# ------------------------------------------------------------------------------------------------ A2: matching
CONFIGS = [("kuch1", "edit", "dynamic", 0), ("multiple_opt", "edit", "dynamic", 4), ("kuch1", "hamming", "dynamic", 2),
           ("columba", "edit", "dynamic", 8), ("columba", "edit", "dynamic", 11)]


def _reads(w, k):
    """{window: reads}: reads planted in each window with 0 ... k edits (reverse complements, N), a quarter of them from
    the element copy inside the window, the last window's with reads that end at the final character; 'element':
    reads of the consensus (their hits: many copies, above 2^31 too, through the in-index search)"""
    length = 100 if k <= 4 else 150
    count = 36 if k <= 4 else (24 if k <= 8 else 12)
    T = w["ix"].text
    out = {}
    for j, (name, o) in enumerate(WINDOWS.items()):
        win = T[o:o + W]
        edits = (0, 1, max(k - 1, 0), k) if k else (0,)
        rs = synth.sample_reads(win, count - count // 4, length, seed=100 * k + j, n_frac=0.05, edit_choices=edits)
        e = [p - o for p in w["pos"] if o <= p and p + ELEM <= o + W][0]
        rs += synth.sample_reads(win[e:e + ELEM], count // 4, length, seed=100 * k + j + 50, edit_choices=edits)
        if name == "last":
            tail = T[L - length:L].tobytes()
            rs += [tail, synth.revcomp(tail), tail[:40] + (b"A" if tail[40] != ord("A") else b"C") + tail[41:]]
        if name == "start":
            rs += [T[STRETCH_SRC + 5000:STRETCH_SRC + 5000 + length].tobytes()]   # (hits ~2^32 apart)
        out[name] = rs
    if k >= 2:   # (no copy holds the consensus exactly)
        cons = np.frombuffer(w["cons"], np.uint8)
        out["element"] = synth.sample_reads(cons, 6 if k >= 8 else 12, length, seed=700 + k, edit_choices=(0,))
    return out


def _shifted(occ, o):
    s = np.zeros(len(occ), [("begin", np.int64), ("end", np.int64), ("distance", np.int64)])
    s["begin"] = occ["begin"].astype(np.int64) - o
    s["end"] = occ["end"].astype(np.int64) - o
    s["distance"] = occ["distance"]
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("spec,metric,partition,k", CONFIGS)
def test_matching_at_high_positions(top, gt, spec, metric, partition, k):
    dev = top["dev"]
    groups = _reads(top, k)
    world = {"op": top["op"], "orc": top["orc"], "dev": dev}
    st = ca.SearchStrategy(spec, metric, partition)
    high = 0
    for name, reads in groups.items():
        t0 = time.time()
        _compare(world, spec, metric, partition, k, reads, counters=True)   # oracle/ on the same index (its rules)
        t_or = time.time() - t0
        occ, offs, cnt = ca.match_batch(dev, st, k, reads)
        try:
            checked, loose = check_soundness(gt, top["text"], reads, occ, offs, k, metric)
        except AssertionError as e:
            raise AssertionError(f"window {name}: (read, begin, end, distance[, ...]) {e}") from None
        assert checked >= len(reads) // 2 and loose * 50 <= checked, (name, checked, loose)
        high += int((occ["begin"] >= TOP).sum())
        if name == "element":
            # the consensus lies within a few % of 64 copies: wide SA ranges, in-index hits located above 2^31 (k_fmocc)
            above = [int(((occ["begin"][int(offs[i]):int(offs[i + 1])] >= TOP)).sum()) for i in range(len(reads))]
            assert max(above) > 4, (name, above)
            continue
        o = WINDOWS[name]
        try:
            hits, chain = check_completeness(gt, top["text"][o:o + W], reads, _shifted(occ, o), offs, k, metric)
        except AssertionError as e:
            raise AssertionError(f"window {name} at {o}: (read, strand, window end, distance[, occurrences]) {e}") from None
        assert hits >= len(reads) // 2 and chain * 50 <= hits, (name, hits, chain)
        if name == "mid":   # both paths of this window's reads: SA rows located and in-text verifications
            assert cnt["LOCATED_ROWS"] > 0 and (k == 0 or cnt["IN_TEXT_STARTED"] > 0), cnt
        if name == "start" and k == 0:
            lo, hi = int(offs[len(reads) - 1]), int(offs[len(reads)])
            b = occ["begin"][lo:hi].astype(np.int64)
            assert b.size >= 2 and b.max() - b.min() > (1 << 32) - (1 << 20), b.tolist()
        print(f"[text limits] {spec} {metric} k={k} {name}: {len(reads)} reads, {checked} occurrences sound, "
              f"{hits} window ends covered, oracle {t_or:.1f} s")
    print(f"[text limits] {spec} {metric} k={k}: {high} occurrences with begin >= 2^31 checked")
    assert high > 20


# ------------------------------------------------------------------------------------------------ A3: alignments, SAM, BEST
@pytest.mark.gpu
@pytest.mark.parametrize("spec,k", [("multiple_opt", 4), ("columba", 8)])
def test_cigars_and_sam_at_high_positions(top, gt, spec, k):
    dev, T, text = top["dev"], top["ix"].text, top["text"]
    groups = _reads(top, k)
    reads = groups["mid"] + groups["last"] + groups["element"]
    b = ca.Batch(dev, ca.SearchStrategy(spec, "edit", "dynamic"), k, reads)
    b.want_alignments()
    b.run()
    occ, offs, _ = b.results()
    aln, ops = b.alignments()
    ids = [f"@r{i}" for i in range(len(reads))]   # (QNAME: the identifier without its '@')
    sam = b.sam(ids, ["I" * len(r) for r in reads], SEQ_NAMES, unmapped=True, xa=False)
    b.close()
    starts = [int(s) for s in SEQ_STARTS]
    recs = {}
    for ln in sam.splitlines():
        f = ln.split("\t")
        if not int(f[1]) & 4:
            recs.setdefault(f[0], set()).add((f[2], int(f[3])))
    n_checked = n_sam = 0
    for i, rd in enumerate(reads):
        fw = clean(rd)
        for j in range(int(offs[i]), int(offs[i + 1])):
            bg, en, d, s = (int(occ[x][j]) for x in ("begin", "end", "distance", "strand"))
            o = ops[int(aln["cigar_off"][j]):int(aln["cigar_off"][j]) + int(aln["cigar_len"][j])]
            p = fw if s == 0 else synth.revcomp(fw)
            win = T[bg:en].tobytes()
            qi = ti = edits = 0
            for x in o.tolist():
                kind, ln = "MID?"[x & 3], x >> 2
                if kind == "M":
                    edits += sum(1 for a, c in zip(p[qi:qi + ln], win[ti:ti + ln]) if a != c or a == ord("N"))
                    qi += ln
                    ti += ln
                elif kind == "I":
                    qi += ln
                    edits += ln
                else:
                    assert kind == "D", (i, (bg, en, d, s), kind)
                    ti += ln
                    edits += ln
            assert qi == len(p) and ti == len(win), (i, (bg, en, d, s), qi, ti)
            true = gt.gt_edit_distance(p, len(p), win, len(win))
            assert edits == true <= d, (i, (bg, en, d, s), edits, true)
            n_checked += 1
            sq = bisect.bisect_right(starts, bg) - 1
            if sq < len(SEQ_NAMES) and en <= starts[sq + 1]:   # inside one sequence: RNAME and 1-based POS by bisect
                want = (SEQ_NAMES[sq], bg - starts[sq] + 1)
                assert want in recs.get(ids[i][1:], set()), (i, (bg, en, d, s), want, sorted(recs.get(ids[i][1:], set()))[:8])
                n_sam += 1
    assert n_checked > 50 and n_sam > 50
    assert int((occ["begin"] >= TOP).sum()) > 20


@pytest.mark.gpu
def test_best_mode_at_high_positions(top):
    import schemes_py as sp
    op = top["op"]
    groups = _reads(top, 4)
    reads = groups["mid"] + groups["last"] + groups["element"]
    tables = sp.BY_NAME["columba"]
    max_sup = 0
    while (max_sup + 1) in tables["schemes"] and max_sup < 13:
        max_sup += 1
    o_occ, o_sid, o_sb, o_cig, o_off, o_best, o_hits, o_cnt = op.match_best(
        top["orc"], op.OracleStrategy(tables, "edit", "dynamic"), reads, x=1, min_identity=95, max_supported=max_sup, threads=8)
    d_occ, d_aln, d_ops, d_off, d_best, d_hits, d_cnt = ca.match_best(
        top["dev"], ca.SearchStrategy("columba", "edit", "dynamic"), reads, x=1, min_identity=95)
    assert np.array_equal(o_best, d_best) and np.array_equal(o_hits, d_hits) and np.array_equal(o_off, d_off)
    assert (o_best != 0xFFFFFFFF).sum() > len(reads) // 2
    for f in ("begin", "end", "distance", "strand"):
        bad = np.flatnonzero(o_occ[f] != d_occ[f])
        assert bad.size == 0, (f, [(int(np.searchsorted(d_off, j, "right")) - 1, d_occ[j].tolist(), o_occ[j].tolist()) for j in bad[:4]])
    assert np.array_equal(o_sid, d_aln["seq_id"]) and np.array_equal(o_sb, d_aln["seq_begin"])
    for j in range(len(d_occ)):
        a = d_aln[j]
        got = ca.cigar_string(d_ops[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["cigar_len"])])
        assert got == o_cig[j], (j, d_occ[j], got, o_cig[j])
    assert int((d_occ["begin"] >= TOP).sum()) > 10
    for n in ("NODE_COUNTER", "IN_TEXT_STARTED", "SEARCH_STARTED", "EXPANSIONS", "IMMEDIATE_SWITCH"):
        assert o_cnt[n] == d_cnt[n], (n, o_cnt[n], d_cnt[n])
