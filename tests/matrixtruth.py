"""Cell-level truth for the bit-parallel matrices and trace rows (tests/test_matrix_truth.py, tests/test_gpu_matrix_probe.py).

Cases for tests/matrix_probe.hip are generated from seeds, screened with the plain dynamic programming of oracle/groundtruth.c
until the quotas below are full (the reference alone decides what a case exercises), written
as one binary case file, and the probe's result file is compared with what plain DP says:

  cells      a cell of at most maxED is exact on the device; a cell above maxED reads above maxED and nothing more
  verdict    a row is invalid iff the search for its rightmost active column finds none
  RAC        bitparallelmatrix.h:398-412 on integers: one column right if the diagonal step costs nothing, else the rightmost
             column >= i - Wv whose cell is at most maxED
  words      bit t of block b: character t - LEFT + BLOCK b of X equals the nucleotide; one left of X, zero beyond it
  walks      horizontal before diagonal before vertical over the integer matrix; run-length CIGAR, end row, flags == 0

`onlyVerticalGapsLeft(As)` reads cells above maxED, where plain DP says nothing: it is taken from the oracle's CPU matrices,
which the golden vectors pin to the reference, on valid rows only.
"""
import ctypes as C
import functools
import os
import random
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")
PROBE_SRC = os.path.join(HERE, "matrix_probe.hip")
# the flags of columba_amd.build_library, plus the include paths of a file outside csrc
PROBE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-variable",
               "-I", os.path.join(ROOT, "columba_amd", "csrc"), "-I", os.path.join(ROOT, "include")]

ROW_CELLS, MAX_WALKS, WALK_WORDS = 56, 32, 32
MAIN_LENGTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 47, 48, 49, 63, 64, 65]
LONG_LENGTHS = [150, 480]
LONG_CASES = 24  # per long length and geometry

# name, id in the probe, maxED served, in-text?, rows per block, LEFT, DIAG, largest Wv the geometry takes, the oracle matrix
# that answers onlyVerticalGapsLeft for it
GEOS = [
    dict(name="MX", id=0, ks=list(range(0, 11)), intext=False, block=32, left=21, diag=20, wvmax=20, ref=64),
    dict(name="MX32", id=1, ks=list(range(0, 5)), intext=True, block=8, left=14, diag=13, wvmax=13, ref=0),
    dict(name="MXW", id=2, ks=list(range(0, 8)), intext=True, block=16, left=22, diag=21, wvmax=21, ref=0),
    dict(name="MXX", id=3, ks=[8, 9, 10], intext=True, block=16, left=31, diag=30, wvmax=30, ref=0),
    dict(name="MXY", id=4, ks=[11, 12, 13], intext=True, block=8, left=40, diag=39, wvmax=39, ref=0),
    dict(name="MXN", id=5, ks=[11, 12, 13], intext=False, block=16, left=31, diag=30, wvmax=30, ref=128),
    # (a phase with Wv > DIAG - MXS_SLACK raises FLAG_NARROW_MATRIX and runs on MX: the small matrix never sees it)
    dict(name="MXS", id=6, ks=list(range(0, 7)), intext=False, block=8, left=15, diag=14, wvmax=12, ref=64),
]
GEO = {g["name"]: g for g in GEOS}
QUOTAS = dict(general=100, general_seam=10, invalid=200, diagonal=200)
TRACE_QUOTAS = dict(rel_lo=200, rel_hi=200, cross=200, row0=50)
SCREEN_CAP = 60000  # candidates screened per geometry / trace format before a quota counts as unreachable
CODE = {65: 0, 67: 1, 71: 2, 84: 3, 78: 4}
_CODE_LUT = np.full(256, 4, dtype=np.uint8)
for _c, _v in CODE.items():
    _CODE_LUT[_c] = _v


# ---------------------------------------------------------------- the plain reference
@functools.lru_cache(maxsize=None)
def lib():
    so, src = os.path.join(ORACLE, "libgroundtruth.so"), os.path.join(ORACLE, "groundtruth.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.gt_matrix_rows.restype = u32
    L.gt_matrix_rows.argtypes = [C.c_char_p, u32, C.c_char_p, u32, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp]
    L.gt_trace_walks.restype = u32
    L.gt_trace_walks.argtypes = [C.c_char_p, u32, C.c_char_p, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp]
    L.gt_match_word.restype = u64
    L.gt_match_word.argtypes = [C.c_char_p, u32, u32, u32, u32, C.c_uint8]
    L.gt_match_words.restype = None
    L.gt_match_words.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp]
    return L


def _p(a):
    return a.ctypes.data


_MAXROWS = 640
_buf = dict(v=np.zeros(_MAXROWS, np.uint8), rac=np.zeros(_MAXROWS, np.int32), ev=np.zeros(_MAXROWS, np.uint8),
            fc=np.zeros(_MAXROWS, np.uint32), nc=np.zeros(_MAXROWS, np.uint32), cells=np.zeros((_MAXROWS, ROW_CELLS), np.uint8))


def geometry(x_len, init, k):
    """n, m, Wv, Wh of bitparallelmatrix.cpp:77-103"""
    n = x_len + 1
    wv = len(init) - 1 + k - init[-1]
    wh = k - init[0]
    return n, max(wv + n, wv + wh + 1), wv, wh


def plain_rows(case):
    """what plain DP says about every row of a case, up to and including its first invalid row"""
    init = np.asarray(case["init"], dtype=np.uint32)
    b = _buf
    r = lib().gt_matrix_rows(case["x"], len(case["x"]), case["y"], len(case["y"]), _p(init), len(init), case["k"], ROW_CELLS,
                             _p(b["v"]), _p(b["rac"]), _p(b["ev"]), _p(b["fc"]), _p(b["nc"]), _p(b["cells"]))
    return dict(rows=r, v=b["v"][:r].copy(), rac=b["rac"][:r].copy(), ev=b["ev"][:r].copy(), fc=b["fc"][:r].copy(),
                nc=b["nc"][:r].copy(), cells=b["cells"][:r].copy())


# ---------------------------------------------------------------- windows and reads
def make_window(rng, length, kind):
    """kind 0 uniform four-letter, 1 two-letter, 2 homopolymer, 3 tandem (unit 1..8), 4 tandem with a few edits"""
    if kind == 0:
        return bytes(rng.choice(b"ACGT") for _ in range(length))
    if kind == 1:
        ab = rng.sample(list(b"ACGT"), 2)
        return bytes(rng.choice(ab) for _ in range(length))
    if kind == 2:
        return bytes([rng.choice(b"ACGT")]) * length
    unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 8)))
    w = bytearray((unit * (length // len(unit) + 1))[:length])
    if kind == 4:
        for _ in range(rng.randint(1, 3)):
            w[rng.randrange(length)] = rng.choice(b"ACGT")
    return bytes(w)


def make_read(rng, window, off, x_len, k, shape, with_n):
    """a read of x_len characters cut from the window at `off` and given 0 .. k + 2 edits: shape 0 spread out, 1 all insertions
    packed at one end, 2 all deletions packed at one end, 3 half deletions, half insertions at one end (the _edge_reads shape of
    tests/test_gpu_parity.py)"""
    ne = rng.randint(0, k + 2)
    seg = bytearray(window[off:off + x_len + ne + 2])
    if shape == 0:
        for _ in range(ne):
            if not seg:
                break
            at, what = rng.randrange(len(seg)), rng.randrange(3)
            if what == 0:
                seg[at] = rng.choice(b"ACGT")
            elif what == 1:
                seg.insert(at, rng.choice(b"ACGT"))
            else:
                del seg[at]
    else:
        nd = 0 if shape == 1 else ne if shape == 2 else ne // 2
        ni = ne - nd
        near = rng.randint(0, min(5, max(0, x_len - 1)))
        at = near if rng.random() < 0.5 else max(0, x_len - ni - near)
        seg[at:at + nd] = bytes(rng.choice(b"ACGT") for _ in range(ni))
    seg = seg[:x_len]
    while len(seg) < x_len:
        seg.append(rng.choice(b"ACGT"))
    if with_n and x_len:
        seg[rng.randrange(x_len)] = ord("N")
    return bytes(seg)


def intext_case(rng, geo, k, x_len, free, shape=None, kind=None, off=None):
    n_zeros = 2 * k + 1 if free else 1
    wv = n_zeros - 1 + k
    kind = rng.randrange(5) if kind is None else kind
    shape = rng.randrange(4) if shape is None else shape
    window = make_window(rng, x_len + wv + k + 4, kind)
    off = rng.randrange(n_zeros) if off is None else off
    x = make_read(rng, window, off, x_len, k, shape, rng.random() < 0.1)
    return dict(geo=geo["name"], k=k, x=x, src=x, xoff=0, y=window, init=[0] * n_zeros, raw=[0], increase=0, nzeros=n_zeros, off=off)


def first_column(rng, geo, k):
    """raw[] (a non-negative walk with steps -1, 0, +1, 1 .. LEFT + 1 long) and `increase` as the frontier passes them: first and
    last at most maxED, Wv within what the geometry takes"""
    for _ in range(20):
        n_init = min(rng.choice([1, 1, 2, 3, 4, rng.randint(1, geo["left"] + 1)]), geo["left"] + 1)
        increase = rng.choice([0, 0, 1, 2])
        raw = [rng.randint(0, max(0, k - increase))]
        for _ in range(n_init - 1):
            raw.append(max(0, raw[-1] + rng.choice([-1, 0, 1, 1])))
        first, last = raw[0] + increase, raw[-1] + increase
        if first <= k and last <= k and n_init - 1 + k - last <= geo["wvmax"]:
            return raw, increase
    return [min(k, 1)], 0


def inindex_case(rng, geo, k, x_len, shape=None, kind=None):
    raw, increase = first_column(rng, geo, k)
    init = [r + increase for r in raw]
    wv = len(init) - 1 + k - init[-1]
    kind = rng.randrange(5) if kind is None else kind
    shape = rng.randrange(4) if shape is None else shape
    xoff = rng.randrange(96)
    window = make_window(rng, xoff + x_len + wv + k + 8, kind)
    # the part X lies at bit xOff of its read's strings; the rows follow a text that is X with edits, entered up to nInit - 1
    # characters early
    x = window[xoff:xoff + x_len]
    if rng.random() < 0.1 and x_len:
        at = rng.randrange(x_len)
        x = x[:at] + b"N" + x[at + 1:]
    src = window[:xoff] + x + window[xoff + x_len:xoff + x_len + 5]
    lead = rng.randrange(len(init))
    y = make_read(rng, window, max(0, xoff - lead), x_len + wv + k + 2, k, shape, False)
    return dict(geo=geo["name"], k=k, x=x, src=src, xoff=xoff, y=y, init=init, raw=raw, increase=increase, nzeros=1)


def make_case(rng, geo, k, x_len, free=None, **kw):
    if geo["intext"]:
        return intext_case(rng, geo, k, x_len, rng.random() < 0.5 if free is None else free, **kw)
    return inindex_case(rng, geo, k, x_len, **kw)


def _strata(geo, case, exp):
    """what a case adds to each quota, as plain DP sees it"""
    i = np.arange(1, exp["rows"] + 1)
    valid = exp["v"] == 1
    general = valid & ((exp["ev"] & 1) != 0)
    return dict(general=int(general.sum()), general_seam=int((general & (i % geo["block"] == 0)).sum()),
                invalid=int(exp["rows"] > 0 and exp["v"][-1] == 0), diagonal=int((valid & ((exp["ev"] & 2) != 0)).sum()))


@functools.lru_cache(maxsize=None)
def matrix_cases(name):
    """(cases, expectations, per-k strata counts, candidates screened) of one geometry; deterministic by seed"""
    geo = GEO[name]
    rng = random.Random(1000 + geo["id"])
    cases, exps = [], []
    counts = {q: {k: 0 for k in geo["ks"]} for q in QUOTAS}

    def keep(case, exp, st):
        cases.append(case)
        exps.append(exp)
        for q, v in st.items():
            counts[q][case["k"]] += v

    # every length at every maxED the geometry serves, fixed and free start; then the long reads
    t = 0
    for k in geo["ks"]:
        for x_len in MAIN_LENGTHS:
            for free in ((False, True) if geo["intext"] else (None,)):
                case = make_case(rng, geo, k, x_len, free, shape=t % 4, kind=(t // 4) % 5)
                exp = plain_rows(case)
                keep(case, exp, _strata(geo, case, exp))
                t += 1
    if geo["intext"]:  # a free start at every offset below nZeros
        for k in geo["ks"]:
            for off in range(2 * k + 1):
                case = intext_case(rng, geo, k, MAIN_LENGTHS[3 + (off + k) % (len(MAIN_LENGTHS) - 3)], True, shape=off % 4, kind=(off // 4) % 5, off=off)
                exp = plain_rows(case)
                keep(case, exp, _strata(geo, case, exp))
    for x_len in LONG_LENGTHS:
        for t in range(LONG_CASES):
            case = make_case(rng, geo, geo["ks"][t % len(geo["ks"])], x_len, None if not geo["intext"] else bool(t & 1), shape=t % 4,
                             kind=(t // 4) % 5)
            exp = plain_rows(case)
            keep(case, exp, _strata(geo, case, exp))
    # screening: candidates at the short lengths, kept while they add to a quota that is not full
    screened = 0
    total = lambda q: sum(counts[q].values())
    while screened < SCREEN_CAP and any(total(q) < QUOTAS[q] for q in QUOTAS):
        screened += 1
        case = make_case(rng, geo, rng.choice(geo["ks"]), rng.choice(MAIN_LENGTHS))
        exp = plain_rows(case)
        st = _strata(geo, case, exp)
        if any(st[q] and total(q) < QUOTAS[q] for q in QUOTAS):
            keep(case, exp, st)
    return cases, exps, counts, screened


# ---------------------------------------------------------------- trace cases
def trace_params(narrow, k):
    """below, relLo, relHi, relHiAny, rows per line: narrow rows read their two implied bits at rel = 6 (HP) and rel = 22 (diagonal,
    read once HP is 0); wide rows are asked for steps at rel <= 1 and rel >= 3 maxED + maxED - 1"""
    return (18, 6, 22, 0, 16) if narrow else (21, 1, 4 * k - 1, 1, 8)


_walk_buf = np.zeros((MAX_WALKS, WALK_WORDS), np.uint16)
_strata_buf = np.zeros(5, np.uint64)


def plain_walks(case, narrow):
    below, lo, hi, hi_any, group = trace_params(narrow, case["k"])
    _walk_buf[:] = 0
    _strata_buf[:] = 0
    n = lib().gt_trace_walks(case["x"], len(case["x"]), case["y"], len(case["y"]), case["nzeros"], case["k"], below, lo, hi, hi_any, group,
                             WALK_WORDS, MAX_WALKS, _p(_walk_buf), _p(_strata_buf))
    s = _strata_buf
    return dict(n=n, walks=_walk_buf.copy(), valid=int(s[4])), dict(rel_lo=int(s[0]), rel_hi=int(s[1]), cross=int(s[2]), row0=int(s[3]))


@functools.lru_cache(maxsize=None)
def trace_cases(narrow):
    geo = GEO["MX32" if narrow else "MXW"]
    ks = [1, 2, 3, 4] if narrow else [1, 2, 3, 4, 5, 6, 7]
    rng = random.Random(2000 + int(narrow))
    cases, exps = [], []
    counts = {q: {k: 0 for k in ks} for q in TRACE_QUOTAS}

    def keep(case, exp, st):
        assert all(int(w[2]) <= WALK_WORDS - 4 for w in exp["walks"][:exp["n"]]), "a CIGAR of more runs than a record holds"
        cases.append(case)
        exps.append(exp)
        for q, v in st.items():
            counts[q][case["k"]] += v

    t = 0
    for k in ks:
        for x_len in MAIN_LENGTHS + [150]:
            for free in (False, True):
                case = intext_case(rng, geo, k, x_len, free, shape=t % 4, kind=(t // 4) % 5)
                keep(case, *plain_walks(case, narrow))
                t += 1
    for k in ks:  # a free start at every offset below nZeros
        for off in range(2 * k + 1):
            case = intext_case(rng, geo, k, MAIN_LENGTHS[3 + (off + k) % (len(MAIN_LENGTHS) - 3)], True, shape=off % 4, kind=(off // 4) % 5, off=off)
            keep(case, *plain_walks(case, narrow))
    for t in range(8):
        case = intext_case(rng, geo, ks[-1 - t % 2], 480, bool(t & 1), shape=t % 4, kind=0)
        keep(case, *plain_walks(case, narrow))
    screened = 0
    total = lambda q: sum(counts[q].values())
    while screened < SCREEN_CAP and any(total(q) < TRACE_QUOTAS[q] for q in TRACE_QUOTAS):
        screened += 1
        case = intext_case(rng, geo, rng.choice(ks), rng.choice(MAIN_LENGTHS), rng.random() < 0.5)
        exp, st = plain_walks(case, narrow)
        if any(st[q] and total(q) < TRACE_QUOTAS[q] for q in TRACE_QUOTAS):
            keep(case, exp, st)
    return cases, exps, counts, screened


# ---------------------------------------------------------------- match words
WORD_KINDS = [  # kind in the probe: LEFT, BLOCK of the word it stands for, rows per word of its source, shift base
    dict(name="matchWord<21,32>", left=21, block=32), dict(name="matchWord<23,32>", left=23, block=32),
    dict(name="matchWord<31,16>", left=31, block=16), dict(name="matchWord<40,8>", left=40, block=8),
    dict(name="matchWordW", left=22, block=16, shift0=1, word=64), dict(name="matchWord32", left=14, block=8, shift0=9, word=32),
    dict(name="matchWordSmall", left=15, block=8, shift0=6, word=32),
]
WORD_LENGTHS = sorted({m + d for m in range(8, 73, 8) for d in (-1, 0, 1)}) + LONG_LENGTHS


@functools.lru_cache(maxsize=None)
def word_queries():
    """sources (four strings of 600 characters) and the query table: kind, source, xOff, xLen, nucleotide, block (kinds 0..3) or row
    (the derived words, one row per block of theirs); xOff 0..95, every length of WORD_LENGTHS, every block the length has and one more"""
    rng = random.Random(3000)
    sources = [make_window(rng, 600, 0), make_window(rng, 600, 1), make_window(rng, 600, 4)]
    withn = bytearray(make_window(rng, 600, 0))
    for at in range(5, 600, 37):
        withn[at] = ord("N")
    sources.append(bytes(withn))
    parts = []
    for xoff in range(96):
        for x_len in WORD_LENGTHS:
            chs = [0, 1, 2, 3] if x_len < 100 else [(xoff + x_len) % 4]
            for kind, wk in enumerate(WORD_KINDS):
                nb = (x_len + wk["left"]) // wk["block"] + 2
                arg = np.arange(nb, dtype=np.uint32) * (wk["block"] if kind >= 4 else 1)
                for ch in chs:
                    q = np.zeros((nb, 8), np.uint32)
                    q[:, 0], q[:, 1], q[:, 2], q[:, 3], q[:, 4], q[:, 5] = kind, (xoff + x_len) % 4, xoff, x_len, ch, arg
                    parts.append(q)
    return sources, np.concatenate(parts)


def plain_words(sources, q):
    """every queried word as a character comparison; a derived word is a shift of a 64-bit block word, so only its low bits exist"""
    pool = np.frombuffer(b"".join(sources), dtype=np.uint8)
    starts = np.cumsum([0] + [len(s) for s in sources])[:-1].astype(np.uint32)
    kind, arg = q[:, 0], q[:, 5]
    left = np.array([w["left"] for w in WORD_KINDS], np.uint32)[kind]
    block = np.array([w["block"] for w in WORD_KINDS], np.uint32)[kind]
    b = np.where(kind >= 4, arg // block, arg).astype(np.uint32)
    x_start = (starts[q[:, 1]] + q[:, 2]).astype(np.uint32)
    x_len = np.ascontiguousarray(q[:, 3])
    ch = np.frombuffer(b"ACGT", np.uint8)[q[:, 4]].copy()
    out = np.zeros(len(q), np.uint64)
    lib().gt_match_words(_p(pool), _p(x_start), _p(x_len), _p(left), _p(block), _p(b), _p(ch), len(q), _p(out))
    shift0 = np.array([w.get("shift0", 0) for w in WORD_KINDS], np.uint64)[kind]
    word = np.array([w.get("word", 64) for w in WORD_KINDS], np.uint64)[kind]
    shift = np.where(kind >= 4, ((arg % 32) // block) * block + shift0, 0).astype(np.uint64)
    keep = np.minimum(word, np.uint64(64) - shift)
    mask = np.where(keep >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << keep) - np.uint64(1))
    return out & mask


# ---------------------------------------------------------------- the case file and the result file
def write_case_file(path):
    """all stages in one file (the formats of tests/matrix_probe.hip); returns what read_result_file needs"""
    sources, src_index = [], {}

    def src_of(s):
        if s not in src_index:
            src_index[s] = len(sources)
            sources.append(s)
        return src_index[s]

    ypool, raws, mc, geo_begin, row0 = [], [], [], [0], 0
    yoff = rawoff = 0
    layout = {}
    for geo in GEOS:
        cases, exps, _, _ = matrix_cases(geo["name"])
        first = row0
        for case, exp in zip(cases, exps):
            rows = min(len(case["y"]), geometry(len(case["x"]), case["init"], case["k"])[1] - 1)
            mc.append([src_of(case["src"]), case["xoff"], len(case["x"]), yoff, len(case["y"]), case["k"], case["nzeros"], len(case["raw"]),
                       rawoff, case["increase"], row0, rows, 0, 0, 0, 0])
            ypool.append(case["y"])
            yoff += len(case["y"])
            raws.extend(case["raw"])
            rawoff += len(case["raw"])
            row0 += rows
        layout[geo["name"]] = (geo_begin[-1], len(mc), first, row0)
        geo_begin.append(len(mc))
    wsources, wq = word_queries()
    wq = wq.copy()
    wq[:, 1] = np.array([src_of(s) for s in wsources], np.uint32)[wq[:, 1]]
    tcs, lines = [], []
    for narrow in (True, False):
        cases, _, _, _ = trace_cases(narrow)
        tc = []
        for case in cases:
            tc.append([src_of(case["x"]), len(case["x"]), yoff, len(case["y"]), case["k"], case["nzeros"], 0, 0])
            ypool.append(case["y"])
            yoff += len(case["y"])
        tcs.append(np.array(tc, np.uint32).reshape(-1, 8))
        group = 16 if narrow else 8
        lines.append(max((len(c["y"]) + group - 1) // group for c in cases) if cases else 0)
    srcs, off = [], 0
    for s in sources:
        srcs.append([off, len(s)])
        off += len(s)
    pool = _CODE_LUT[np.frombuffer(b"".join(sources), np.uint8)]
    ycodes = _CODE_LUT[np.frombuffer(b"".join(ypool), np.uint8)]
    header = [0x45424f5250424d43, len(sources), len(pool), len(mc), row0, len(ycodes), len(raws), len(wq), len(tcs[0]), len(tcs[1]),
              lines[0], lines[1]] + geo_begin
    header += [0] * (32 - len(header))
    with open(path, "wb") as f:
        f.write(struct.pack("<32Q", *header))
        for a in (np.array(srcs, np.uint32), pool, np.array(mc, np.uint32), ycodes, np.array(raws, np.uint16), wq, tcs[0], tcs[1]):
            f.write(np.ascontiguousarray(a).tobytes())
    return dict(layout=layout, n_mat=len(mc), rows=row0, n_words=len(wq), n_trace=(len(tcs[0]), len(tcs[1])))


ROW_DTYPE = np.dtype([("verdict", "u1"), ("ovgl", "u1"), ("score", "<u2"), ("rac", "<u2"), ("nc", "<u2"), ("cells", "u1", (ROW_CELLS,))])


def read_result_file(path, info):
    with open(path, "rb") as f:
        data = f.read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(data, dtype=dtype, count=n, offset=pos)
        pos += a.nbytes
        return a

    res = dict(done=take(np.uint32, info["n_mat"]), rows=take(ROW_DTYPE, info["rows"]), words=take(np.uint64, info["n_words"]))
    for name, n in zip(("narrow", "wide"), info["n_trace"]):
        res[name] = dict(n=take(np.uint32, n), valid=take(np.uint32, n), walks=take(np.uint16, n * MAX_WALKS * WALK_WORDS).reshape(n, MAX_WALKS, WALK_WORDS))
    assert pos == len(data), "the result file has another size than the case file implies"
    return res


def device_rows(name, res, info):
    """the probe's rows of one geometry in the shape of expected_rows: per case (rows done, row records)"""
    c0, c1, _, _ = info["layout"][name]
    cases, _, _, _ = matrix_cases(name)
    out, r0 = [], info["layout"][name][2]
    for ci, case in enumerate(cases):
        rows = min(len(case["y"]), geometry(len(case["x"]), case["init"], case["k"])[1] - 1)
        d = int(res["done"][c0 + ci])
        out.append(res["rows"][r0:r0 + min(d, rows)])
        r0 += rows
    assert c0 + len(cases) == c1
    return out


# ---------------------------------------------------------------- the oracle's CPU matrices
def oracle_rows(name):
    """every case of a geometry through oracle_driver's `matrix` (64-bit), `matrix128` (in-text) or `matrix128i`: per case the rows as
    (verdict, first column, onlyVerticalGapsLeft or None, cells)"""
    geo = GEO[name]
    cases, _, _, _ = matrix_cases(name)
    lines, has_ovgl = [], []
    for case in cases:
        x, y, k, init = case["x"].decode(), case["y"].decode(), case["k"], case["init"]
        wv = len(init) - 1 + k - init[-1]
        ini = " ".join(map(str, init))
        if geo["ref"] == 128:
            lines.append(f"matrix128i {x} {y} {k} {len(init)} {ini}")
            has_ovgl.append(True)
        elif k <= 10 and wv <= 20 and len(init) <= 22:
            lines.append(f"matrix {x} 0 {y} {k} {len(init)} {ini}")
            has_ovgl.append(True)
        else:
            assert geo["intext"]
            lines.append(f"matrix128 {x} {y} {k} {len(init)}")
            has_ovgl.append(False)
    out = subprocess.run([os.path.join(ORACLE, "oracle_driver")], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    res = []
    for line, ov in zip(out.stdout.splitlines(), has_ovgl):
        t = line.split()
        pos, rows = 4 if lines[len(res)].startswith("matrix ") else 3, []
        while pos < len(t):
            if ov:
                v, fc, o, nc = int(t[pos]), int(t[pos + 1]), int(t[pos + 3]), int(t[pos + 4])
                pos += 5
            else:
                v, fc, o, nc = int(t[pos]), int(t[pos + 1]), None, int(t[pos + 3])
                pos += 4
            rows.append((v, fc, o, np.array(t[pos:pos + nc], dtype=np.int64)))
            pos += nc
        res.append(rows)
    assert len(res) == len(cases)
    return res


# ---------------------------------------------------------------- the comparators
def compare_rows(geo, case, exp, dev, ovgl=None):
    """differences between plain DP (exp) and a device case (dev: ROW_DTYPE records): a list of (row, what); empty = equal.  `ovgl`:
    the oracle's predicate per row (None: not compared)."""
    bad = []
    k = case["k"]
    if len(dev) != exp["rows"]:
        bad.append((len(dev), "rows computed: %d, expected %d" % (len(dev), exp["rows"])))
    for r in range(min(len(dev), exp["rows"])):
        i, d = r + 1, dev[r]
        if int(d["verdict"]) != int(exp["v"][r]):
            bad.append((i, "verdict"))
            continue
        if exp["v"][r]:
            col = int(d["rac"]) - geo["diag"] + geo["block"] * (i // geo["block"])
            if col != int(exp["rac"][r]):
                bad.append((i, "RAC %d, expected %d" % (col, exp["rac"][r])))
            if ovgl is not None and ovgl[r] is not None and int(d["ovgl"]) != ovgl[r]:
                bad.append((i, "onlyVerticalGapsLeft"))
        nc = int(exp["nc"][r])
        if int(d["nc"]) != nc:
            bad.append((i, "number of cells"))
            continue
        e, c = exp["cells"][r, :nc].astype(np.int64), d["cells"][:nc].astype(np.int64)
        wrong = np.where(e <= k, c != e, c <= k)
        if wrong.any():
            bad.append((i, "cell at column %d: %d, expected %d" % (int(exp["fc"][r]) + int(np.argmax(wrong)), c[np.argmax(wrong)], e[np.argmax(wrong)])))
        fc = int(exp["fc"][r])
        if fc <= i < fc + nc:  # the score is the diagonal cell
            e0, s = int(e[i - fc]), int(d["score"])
            if (s != e0) if e0 <= k else (s <= k):
                bad.append((i, "score"))
    return bad


def as_device_rows(geo, exp):
    """the rows plain DP expects, written as the device would write them (the comparator's self-check starts from these)"""
    d = np.zeros(exp["rows"], ROW_DTYPE)
    i = np.arange(1, exp["rows"] + 1)
    d["verdict"] = exp["v"]
    d["rac"] = np.where(exp["v"] == 1, exp["rac"] + geo["diag"] - geo["block"] * (i // geo["block"]), 0)
    d["nc"] = exp["nc"]
    d["cells"] = exp["cells"]
    for r in range(exp["rows"]):
        fc = int(exp["fc"][r])
        d["score"][r] = exp["cells"][r, r + 1 - fc] if fc <= r + 1 < fc + int(exp["nc"][r]) else 255
    return d


def compare_walks(exp, dev_n, dev_valid, dev_walks):
    """differences between the plain walks of a case and the device's"""
    bad = []
    if int(dev_valid) != exp["valid"]:
        bad.append("valid rows %d, expected %d" % (dev_valid, exp["valid"]))
    if int(dev_n) != exp["n"]:
        bad.append("walks %d, expected %d" % (dev_n, exp["n"]))
        return bad
    for w in range(exp["n"]):
        e, d = exp["walks"][w], dev_walks[w]
        if int(d[3]) != 0:
            bad.append("walk %d: flags %d" % (w, d[3]))
        if int(d[0]) != int(e[0]) or int(d[1]) != int(e[1]):
            bad.append("walk %d: from row %d to row %d, expected %d to %d" % (w, d[0], d[1], e[0], e[1]))
        if int(d[2]) != int(e[2]) or not np.array_equal(d[4:4 + int(e[2])], e[4:4 + int(e[2])]):
            bad.append("walk %d: runs %s, expected %s" % (w, list(d[4:4 + int(d[2])]), list(e[4:4 + int(e[2])])))
    return bad


def compare_words(exp, dev):
    """indices of the queries whose word differs"""
    return np.nonzero(exp != dev)[0]


# ---------------------------------------------------------------- building and running the probe
def compile_probe(out_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + PROBE_FLAGS + ["-o", out_path, PROBE_SRC])
    return out_path


def format_counts(counts):
    return "; ".join("%s: %d (%s)" % (q, sum(c.values()), " ".join("k%d=%d" % kv for kv in sorted(c.items()))) for q, c in counts.items())
