"""Harness-side builder of the run-length compressed (b-move) index parts (test/bench tooling, not the hot path).

Produces, for a text over ACGT, what `columba_build` of the RUN_LENGTH_COMPRESSION flavour derives from the suffix
arrays of the text and of the reversed text (reference buildindex.cpp:1606-1686, 64-bit length_t, without PHI_MOVE):

* the move tables as the bytes of the reference's `.LFBP` / `.rev.LFBP` files (bmove/moverepr.cpp:145-181: three
  length_t header words, then nrOfRuns + 1 bit-packed rows) — the format `cmb_move_create` takes;
* the suffix array samples at run boundaries (buildindex.cpp:942-953), forward and reverse;
* the predecessor positions with their run mapping for phi / phi^-1 (buildindex.cpp:990-1013, :1044-1066) and the PLCP
  array (bmove/plcp.h:56-80, values; the reference stores them in sdsl sparse bit-vectors, whose file format is sdsl's
  and is not reproduced here).

`build_move` works on the host from the suffix arrays as int64 numpy arrays; `build_move_resident` derives the same parts
with torch on the arrays' device and brings only the O(r) arrays, the text and the PLCP in its run form to the host.  It has
run on texts of up to 64 Mbp; its time and peak memory on texts near 2^32 characters (two suffix arrays of int64 and the
temporaries of the BWT beside them) are not measured.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from .indexbuild import CODE, suffix_array


@dataclass
class MoveArrays:
    n: int                      # text length including '$'
    lfbp_fwd: np.ndarray        # uint8: bytes of <base>.LFBP
    lfbp_rev: np.ndarray        # uint8: bytes of <base>.rev.LFBP
    smpf: np.ndarray            # uint64 samplesFirst
    smpl: np.ndarray            # uint64 samplesLast
    rev_smpf: np.ndarray
    rev_smpl: np.ndarray
    pred_first: np.ndarray      # uint64, sorted marked positions of predFirst
    first_to_run: np.ndarray    # uint64
    pred_last: np.ndarray
    last_to_run: np.ndarray
    plcp: np.ndarray | None     # uint32 PLCP values by text position (None: only the run form below)
    sa: np.ndarray | None       # uint64 suffix array (kept for tests; None from build_move_resident)
    rev_sa: np.ndarray | None
    text: np.ndarray            # uint8 ASCII with the final '$'
    plcp_pos: np.ndarray | None = None    # uint64 run form of the PLCP (columba_amd.plcp_runs); None: derived from plcp
    plcp_sum: np.ndarray | None = None
    sa_rows: np.ndarray | None = None     # uint64 rows of the suffix array kept by build_move_resident ...
    sa_at_rows: np.ndarray | None = None  # ... and the suffix array at them

    def plcp_run_form(self):
        """(positions, PLCP + position there): what cmb_move_desc takes"""
        if self.plcp_pos is not None:
            return self.plcp_pos, self.plcp_sum
        from . import plcp_runs
        return plcp_runs(self.plcp)

    @property
    def runs_fwd(self) -> int:
        return int(np.frombuffer(self.lfbp_fwd[8:16].tobytes(), dtype=np.uint64)[0])

    @property
    def runs_rev(self) -> int:
        return int(np.frombuffer(self.lfbp_rev[8:16].tobytes(), dtype=np.uint64)[0])


def _bits(v: int) -> int:
    return int(math.ceil(math.log2(v)))  # moverepr.h:44-46


def pack_lfbp(bwt: np.ndarray, cum: np.ndarray, length_bits: int = 64) -> np.ndarray:
    """The bytes of a .LFBP file for BWT codes `bwt` (0..4) — buildindex.cpp:826-915 + moverepr.cpp:145-181."""
    n = int(bwt.shape[0])
    starts = np.flatnonzero(np.concatenate([[True], bwt[1:] != bwt[:-1]])).astype(np.uint64)
    head = bwt[starts.astype(np.int64)].astype(np.uint64)
    r = int(starts.shape[0])
    # LF of a run start = C[c] + number of c's before it
    out = np.zeros(r, dtype=np.uint64)
    for c in range(5):
        m = bwt == c
        before = np.cumsum(m) - m  # occurrences of c before position i
        sel = head == c
        out[sel] = np.uint64(int(cum[c])) + before[starts[sel].astype(np.int64)].astype(np.uint64)
    out_run = (np.searchsorted(starts, out, side="right") - 1).astype(np.uint64)
    zero_pos = int(np.flatnonzero(bwt == 0)[0])
    return _pack_rows(n, head, starts, out, out_run, zero_pos, length_bits)


def _pack_rows(n: int, head: np.ndarray, starts: np.ndarray, out: np.ndarray, out_run: np.ndarray, zero_pos: int,
               length_bits: int = 64) -> np.ndarray:
    """The bytes of a .LFBP file from its r rows (uint64: run head, start row, LF of the start row, run of that row)"""
    r = int(starts.shape[0])
    bits_n, bits_r, bits_c = _bits(n), _bits(r), 3
    total_bits = bits_c + 2 * bits_n + bits_r
    total_bytes = (total_bits + 7) // 8
    mask_n = np.uint64((1 << bits_n) - 1)
    mask_r = np.uint64((1 << bits_r) - 1)
    # rows 0..r-1 and the terminating row (0, n, n, r), every value cut to its field like setRowValue does
    h = np.concatenate([head, [np.uint64(0)]])
    a = np.concatenate([starts, [np.uint64(n)]]) & mask_n
    b = np.concatenate([out, [np.uint64(n)]]) & mask_n
    d = np.concatenate([out_run, [np.uint64(r)]]) & mask_r
    lo = np.zeros(r + 1, dtype=np.uint64)
    hi = np.zeros(r + 1, dtype=np.uint64)

    def place(val, off):
        nonlocal lo, hi
        if off < 64:
            lo |= val << np.uint64(off)
            if off > 0:
                hi |= val >> np.uint64(64 - off)
        else:
            hi |= val << np.uint64(off - 64)

    place(h, 0)
    place(a, bits_c)
    place(b, bits_c + bits_n)
    place(d, bits_c + 2 * bits_n)
    rows = np.stack([lo, hi], axis=1).view(np.uint8).reshape(r + 1, 16)[:, :total_bytes]
    header = np.array([n, r, zero_pos], dtype=np.uint64 if length_bits == 64 else np.uint32).view(np.uint8)
    return np.concatenate([header, rows.reshape(-1)])


def _samples(sa: np.ndarray, bwt: np.ndarray):
    chg = np.flatnonzero(bwt[1:] != bwt[:-1])
    first = np.concatenate([[sa[0]], sa[chg + 1]]).astype(np.uint64)
    last = np.concatenate([sa[chg], [sa[-1]]]).astype(np.uint64)
    return first, last


def _plcp(tc: np.ndarray, sa: np.ndarray) -> np.ndarray:
    """PLCP values (Kasai; bmove/plcp.h:56-80) — vectorised by prefix doubling on ranks is overkill for the harness sizes:
    LCP of neighbouring suffixes by chunked comparison."""
    n = int(sa.shape[0])
    isa = np.empty(n, dtype=np.int64)
    isa[sa.astype(np.int64)] = np.arange(n)
    plcp = np.zeros(n, dtype=np.uint32)
    pad = np.concatenate([tc, np.array([254, 253], dtype=np.uint8)])  # beyond the text: never equal
    cur = sa[1:].astype(np.int64)
    prv = sa[:-1].astype(np.int64)
    l = np.zeros(n - 1, dtype=np.int64)
    active = np.arange(n - 1)
    while active.size:
        a = cur[active] + l[active]
        b = prv[active] + l[active]
        a = np.minimum(a, n)
        b = np.minimum(b, n + 1)
        eq = pad[a] == pad[b]
        l[active[eq]] += 1
        active = active[eq]
    plcp[cur] = l.astype(np.uint32)
    return plcp


def build_move(text, device: str | torch.device = "cpu", with_locate: bool = True) -> MoveArrays:
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)
    if t.size == 0 or t[-1] != ord("$"):
        t = np.concatenate([t, np.array([ord("$")], dtype=np.uint8)])
    tc = CODE[t]
    if (tc[:-1] == 0).any() or (tc == 255).any():
        raise ValueError("text must consist of A,C,G,T followed by one final '$'")
    n = int(tc.shape[0])
    if n & (n - 1) == 0:
        raise ValueError("a text size that is a power of two cannot be packed (moverepr.cpp:75-77: the terminating row's "
                         "start position does not fit ceil(log2(n)) bits)")
    dev = torch.device(device)
    tt = torch.from_numpy(tc.copy()).to(dev)
    sa = suffix_array(tt).cpu().numpy().astype(np.int64)
    bwt = tc[np.where(sa > 0, sa - 1, n - 1)]
    rsa = suffix_array(torch.flip(tt, dims=[0])).cpu().numpy().astype(np.int64)
    rbwt = tc[np.where(rsa > 0, n - rsa, 0)]
    cnt = np.bincount(tc, minlength=5)
    cum = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    smpf, smpl = _samples(sa, bwt)
    rsmpf, rsmpl = _samples(rsa, rbwt)

    def pred(samples):  # buildindex.cpp:990-1013, :1044-1066 (stable order of equal keys cannot occur: keys are distinct)
        key = np.where(samples > 0, samples - np.uint64(1), np.uint64(n - 1))
        order = np.argsort(key, kind="stable")
        return key[order].astype(np.uint64), order.astype(np.uint64)

    pf, ftr = pred(smpf)
    pl, ltr = pred(smpl)
    return MoveArrays(n=n, lfbp_fwd=pack_lfbp(bwt, cum), lfbp_rev=pack_lfbp(rbwt, cum), smpf=smpf, smpl=smpl,
                      rev_smpf=rsmpf, rev_smpl=rsmpl, pred_first=pf, first_to_run=ftr, pred_last=pl, last_to_run=ltr,
                      plcp=_plcp(tc, sa) if with_locate else np.zeros(0, np.uint32), sa=sa.astype(np.uint64), rev_sa=rsa.astype(np.uint64), text=t)


def _nz(mask: torch.Tensor) -> torch.Tensor:
    return torch.nonzero(mask).flatten()


def _lcp_pairs(tt: torch.Tensor, a: torch.Tensor, b: torch.Tensor, budget: int = 1 << 26) -> torch.Tensor:
    """LCP of the suffixes a[j] and b[j] (distinct positions of `tt`, codes whose last one, '$', occurs once): blocks of
    characters compared per round, the block doubling while pairs stay equal (long common prefixes cost log rounds)"""
    n = int(tt.numel())
    lcp = torch.zeros(a.numel(), dtype=torch.int64, device=tt.device)
    active = torch.arange(a.numel(), device=tt.device)
    step = 8
    while active.numel():
        part = []
        for lo in range(0, active.numel(), max(1, budget // step)):   # (at most `budget` characters gathered at a time)
            idx = active[lo:lo + budget // step]
            off = torch.arange(step, device=tt.device)
            x = tt[(a[idx, None] + lcp[idx, None] + off).clamp_(max=n - 1)]
            y = tt[(b[idx, None] + lcp[idx, None] + off).clamp_(max=n - 1)]
            ne = x != y
            has = ne.any(1)
            first = ne.to(torch.uint8).argmax(1)
            lcp[idx] += torch.where(has, first, step)   # (the '$' is unique: every pair differs at or before it)
            part.append(idx[~has])
        active = torch.cat(part)
        step = min(step * 2, 1 << 16)
    return lcp


def _move_side(tt: torch.Tensor, cum: list, want_plcp: bool):
    """the O(r) parts of one side (the text's codes `tt` or the reversed text's): packed rows, samples at run boundaries and,
    for the forward side, the PLCP in its run form; and the suffix array (on the device)"""
    n = int(tt.numel())
    sa = suffix_array(tt)
    bwt = tt[torch.where(sa > 0, sa - 1, n - 1)]
    chg = _nz(bwt[1:] != bwt[:-1])
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device=tt.device), chg + 1])
    ends = torch.cat([chg, torch.full((1,), n - 1, dtype=torch.int64, device=tt.device)])
    head = bwt[starts].long()
    del bwt
    # LF of a run start = C[c] + the lengths of the earlier runs of c
    length = ends - starts + 1
    out = torch.empty_like(starts)
    for c in range(5):
        sel = _nz(head == c)
        before = torch.cumsum(length[sel], 0) - length[sel]
        out[sel] = int(cum[c]) + before
    out_run = torch.searchsorted(starts, out, right=True) - 1
    zero_pos = int(starts[_nz(head == 0)[0]].item())
    smpf, smpl = sa[starts], sa[ends]
    plcp = None
    if want_plcp:
        # PLCP[SA[i]] = PLCP[SA[i] - 1] - 1 where BWT[i] = BWT[i - 1] (the suffixes before the two are neighbours again):
        # only the run heads (irreducible positions) are compared, the run form breaks where PLCP + position changes
        q = sa[starts[1:]]
        v = _lcp_pairs(tt, q, sa[starts[1:] - 1])
        q = torch.cat([sa[:1], q])   # (SA[0] = n - 1, the '$': PLCP 0)
        v = torch.cat([torch.zeros(1, dtype=torch.int64, device=tt.device), v])
        q, order = torch.sort(q)
        sm = v[order] + q
        brk = torch.ones(q.numel(), dtype=torch.bool, device=tt.device)
        brk[1:] = sm[1:] != sm[:-1]
        plcp = (q[brk], sm[brk])
    host = lambda x: x.cpu().numpy().astype(np.uint64)
    rows = (host(head), host(starts), host(out), host(out_run), zero_pos)
    return rows, host(smpf), host(smpl), (None if plcp is None else (host(plcp[0]), host(plcp[1]))), sa


def build_move_resident(text, device: str | torch.device = "cuda", n_random_rows: int = 1 << 14, seed: int = 0) -> MoveArrays:
    """The parts of `build_move` (with the locate arrays) derived on `device`: the suffix arrays stay there, the host receives
    the O(r) arrays, the text and the PLCP in its run form (MoveArrays.plcp / sa / rev_sa are None).  `text`: ASCII bytes,
    uint8 array or uint8 tensor over ACGT with or without the final '$'.  Kept for checks: the suffix array at the top 2^16
    rows, at the rows around 2^31 and at `n_random_rows` random rows (sa_rows, sa_at_rows)."""
    dev = torch.device(device)
    if isinstance(text, torch.Tensor):
        tt = torch.from_numpy(CODE).to(text.device)[text.long()].to(dev)
    else:
        t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)
        tt = torch.from_numpy(CODE[t]).to(dev)
    if tt.numel() == 0 or int(tt[-1].item()) != 0:
        tt = torch.cat([tt, torch.zeros(1, dtype=torch.uint8, device=dev)])
    n = int(tt.numel())
    if bool((tt[:-1] == 0).any().item()) or bool((tt == 255).any().item()):
        raise ValueError("text must consist of A,C,G,T followed by one final '$'")
    if n & (n - 1) == 0:
        raise ValueError("a text size that is a power of two cannot be packed (moverepr.cpp:75-77: the terminating row's "
                         "start position does not fit ceil(log2(n)) bits)")
    cnt = torch.bincount(tt.long(), minlength=5).cpu().numpy()
    cum = [0] + np.cumsum(cnt)[:-1].tolist()
    rows, smpf, smpl, plcp, sa = _move_side(tt, cum, True)
    rng = np.random.default_rng(seed)
    keep = np.concatenate([np.arange(min(n, 1 << 16)), np.arange(max(0, (1 << 31) - (1 << 12)), min(n, (1 << 31) + (1 << 12))),
                           np.arange(max(0, n - (1 << 16)), n), rng.integers(0, n, n_random_rows)])
    keep = np.unique(keep).astype(np.int64)
    at = sa[torch.from_numpy(keep).to(dev)].cpu().numpy().astype(np.uint64)
    del sa
    rrows, rsmpf, rsmpl, _, rsa = _move_side(torch.flip(tt, dims=[0]), cum, False)
    del rsa

    def pred(samples):  # buildindex.cpp:990-1013, :1044-1066 (the keys are distinct)
        key = np.where(samples > 0, samples - np.uint64(1), np.uint64(n - 1))
        order = np.argsort(key, kind="stable")
        return key[order].astype(np.uint64), order.astype(np.uint64)

    pf, ftr = pred(smpf)
    pl, ltr = pred(smpl)
    t = (torch.from_numpy(np.frombuffer(b"$ACGT", np.uint8).copy()).to(dev)[tt.long()]).cpu().numpy()
    return MoveArrays(n=n, lfbp_fwd=_pack_rows(n, *rows), lfbp_rev=_pack_rows(n, *rrows), smpf=smpf, smpl=smpl, rev_smpf=rsmpf,
                      rev_smpl=rsmpl, pred_first=pf, first_to_run=ftr, pred_last=pl, last_to_run=ltr, plcp=None, sa=None, rev_sa=None,
                      text=t, plcp_pos=plcp[0], plcp_sum=plcp[1], sa_rows=keep.astype(np.uint64), sa_at_rows=at)


def plcp_from_runs(pos: np.ndarray, sm: np.ndarray, n: int) -> np.ndarray:
    """the PLCP values by text position from their run form (the inverse of columba_amd.plcp_runs)"""
    q = np.arange(n, dtype=np.int64)
    run = np.searchsorted(pos.astype(np.int64), q, side="right") - 1
    return (sm.astype(np.int64)[run] - q).astype(np.uint32)


def save_move(mv: MoveArrays, base: str) -> None:
    """Write the index parts as include/columba_amd_bmove.hpp (BMove) reads them: the two .LFBP files in the reference's
    format, everything the reference keeps in sdsl containers as plain little-endian 64-bit arrays."""
    mv.lfbp_fwd.tofile(base + ".LFBP")
    mv.lfbp_rev.tofile(base + ".rev.LFBP")
    pos, sm = mv.plcp_run_form()
    for ext, a in ((".smpf", mv.smpf), (".smpl", mv.smpl), (".rev.smpf", mv.rev_smpf), (".rev.smpl", mv.rev_smpl),
                   (".prdf", mv.pred_first), (".ftr", mv.first_to_run), (".prdl", mv.pred_last), (".ltr", mv.last_to_run),
                   (".plcp.pos", pos), (".plcp.sum", sm)):
        np.ascontiguousarray(a, dtype="<u8").tofile(base + ext + ".u64")


def plcp_gpu(mv: MoveArrays) -> np.ndarray:
    """PLCP values of a (repetitive) text on the GPU: PLCP[SA[i]] = LCP of the suffixes SA[i - 1] and SA[i], found by
    comparing one more character per round for the pairs still equal (the harness' stand-in for the reference's Kasai loop,
    bmove/plcp.h:56-80, which is what `build_move(with_locate=True)` runs on the CPU)."""
    n = mv.n
    t = torch.from_numpy(np.concatenate([mv.text, np.zeros(16, np.uint8)])).cuda()
    sa = torch.from_numpy(mv.sa.astype(np.int64)).cuda()
    cur, prv = sa[1:], sa[:-1]
    lcp = torch.zeros(n - 1, dtype=torch.int64, device="cuda")
    active = torch.arange(n - 1, device="cuda")
    while active.numel():
        a = (cur[active] + lcp[active]).clamp_(max=n)
        b = (prv[active] + lcp[active]).clamp_(max=n + 1)
        eq = t[a] == t[b]
        eq &= (a < n) & (b < n)
        idx = active[eq]
        lcp[idx] += 1
        active = idx
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    out[cur] = lcp
    return out.cpu().numpy().astype(np.uint32)


def pangenome(base_len: int, copies: int, snp: float, seed: int = 1) -> np.ndarray:
    """`copies` haplotypes of one random sequence of `base_len` characters, each with its own substitutions at rate `snp`
    (ASCII, no '$'): the repetitiveness (n / r of the BWT) of a collection of genomes of one species."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, base_len, dtype=np.uint8)
    parts = []
    for _ in range(copies):
        s = base.copy()
        m = rng.random(base_len) < snp
        s[m] = rng.integers(0, 4, int(m.sum()), dtype=np.uint8)
        parts.append(s)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[np.concatenate(parts)]
    if (text.shape[0] + 1) & text.shape[0] == 0:  # (a text size that is a power of two cannot be packed)
        text = text[:-1]
    return text
