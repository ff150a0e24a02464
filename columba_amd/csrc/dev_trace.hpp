// Stored rows of the in-text matrices and the walk back over them (traceBack / findCIGAR, bitparallelmatrix.h:460-586): the row
// formats the forward passes write, one reader per format, ONE walk from a cell to column 0 over either reader, the run-length CIGAR it
// can feed and the sequence assignment of an occurrence.  The kernels that use them (k_traceback, k_cigar) and the lock-step narrow walk
// of k_traceback<true, .>, a different algorithm over the narrow rows, are in kernels.hpp.
#pragma once
#include "dev_wave.hpp"
#include "host_util.hpp" // (AlnRec: the record k_cigar writes, shared with the units that read it)

namespace cmb {

// Row storage of the traceback pass, interleaved by slot so that the lanes of a wavefront (which
// walk rows in lock step) write whole 512-byte lines: element (row, slot) lives at [row * nSlots + slot].
// What the traceback reads of row i is bit (j - 32 b) + DIAG of HP and D0 with |i - j| inside the band, i.e.
// at most 18 (= 3 k) bits below and 6 above the row's diagonal bit: both 32-bit windows starting 18 bits below
// the diagonal are kept in ONE 64-bit word per row (low half HP, high half D0).
// Layout: `lines` 64-byte lines per lane (slot), line-major (traceLine); line g = the packed rows 8 g + 1 .. 8 g + 8.  The forward pass
// collects eight rows in registers and writes the line with four 16-byte stores; the traceback fetches a line
// (and the eight text codes of its rows) whenever it crosses into the next group of eight rows.
struct VPlanes {
    uint64_t* W;
    uint32_t nSlots, lines;
};
// line g of a lane's trace rows.  Line-major: the 64 lines a wavefront writes (or reads) for one group of rows are
// 4 KB of consecutive memory instead of 64 lines `lines` x 64 bytes apart.
__device__ __forceinline__ uint4* traceLine(const VPlanes& V, uint32_t slot, uint32_t line) {
    return reinterpret_cast<uint4*>(V.W) + ((size_t)line * V.nSlots + slot) * 4;
}
constexpr int TBW = 8, TBN = 16;   // rows per line: wide rows, narrow rows
constexpr uint32_t TB_BELOW = 18;  // narrow rows (32-bit matrix, maxED <= 4)
constexpr uint32_t TBW_BELOW = 21; // wide rows (64-bit / 16-row-block matrix, maxED <= 7: Wv = 3 maxED <= 21, Wh <= 7)
// low half: HP; high half: M | ~D0 — "the diagonal step is allowed" (bitparallelmatrix.h:559-562), folded in by the
// forward pass, which has the row's match word at hand: the trace then needs neither the text nor match words.
__device__ __forceinline__ uint64_t packTraceRow(uint32_t r, uint64_t HP, uint64_t diagOk) {
    const uint32_t sh = (r % MXW_BLOCK) + MXW_DIAG - TBW_BELOW;
    return (uint64_t)(uint32_t)(HP >> sh) | ((uint64_t)(uint32_t)(diagOk >> sh) << 32);
}
// NARROW rows (maxED <= 4): 16 + 16 bits per row, sixteen rows per 64-byte line — half the trace traffic.
// A trace only visits cells whose value is at most maxED, i.e. cells of the band j - i in [-3 maxED, maxED]
// (4 maxED + 1 <= 17 window bits, rel = j - i + TB_BELOW in [6, 22]); two of the 34 bits are never open:
//  * HP at the band's left edge (rel = 6): "horizontal" would come from a cell outside the band, whose value
//    exceeds maxED, so the bit is 0 wherever a trace reads it;
//  * "diagonal allowed" at the band's right edge (rel = 22): the alternative, a vertical step, would come from a
//    cell outside the band, so the bit is 1 wherever a trace (having read HP = 0) reads it.
// Kept: HP for rel 7..22 (low half), diagonal for rel 6..21 (high half).  The wide kernel CHECKS both rules on
// every step it takes (FLAG_CAPACITY if one is ever violated; CMB_TRACE_WIDE=1 selects it for any k).
constexpr uint32_t TBN_HP_LO = 7, TBN_DG_LO = 6, TBN_REL_LO = 6, TBN_REL_HI = 22, TBN_MAX_ED = 4;
// (HP and "diagonal allowed" of the 32-bit matrix: the diagonal of row r is bit r % 8 + MX32_DIAG)
__device__ __forceinline__ uint32_t packTraceRowNarrow(uint32_t r, uint32_t HP, uint32_t diagOk) {
    const uint32_t d = (r % MX32_BLOCK) + MX32_DIAG - TB_BELOW + 32u; // (+32: d itself would be negative)
    return ((HP >> (d + TBN_HP_LO - 32u)) & 0xFFFFu) | ((diagOk >> (d + TBN_DG_LO - 32u)) << 16);
}

// Row readers.  fetch(ti, tj, hp, dg): the HP bit and the "diagonal allowed" bit of cell (ti, tj); false: the cell lies outside what is
// stored (a path of cells <= maxED stays inside the band, so this is checked, not assumed).  The line readers stage the current line of a
// lane in the kernel's LDS window (one memory round trip per 8 or 16 rows) and know row 0, which the forward pass does not store.
struct WideLineRows { // wide rows: rel = tj + TBW_BELOW - ti in [0, 31]
    uint64_t (&w)[TBW][256];
    const VPlanes& V;
    uint32_t slot, tid;
    uint32_t curG = 0xFFFFFFFFu; // the line (rows 8 g + 1 .. 8 g + 8) held in w[.][tid]
    __device__ __forceinline__ bool fetch(uint32_t ti, uint32_t tj, bool& hp, bool& dg) {
        const uint32_t rel = tj + TBW_BELOW - ti;                        // bit of the row's windows
        uint64_t ww = packTraceRow(0, (~0ull) << MXW_LEFT, 0ull);        // row 0 (never steps diagonally: the walk asks ti > 0)
        if (ti > 0) {
            const uint32_t gq = (ti - 1) >> 3, jq = (ti - 1) & 7u;
            if (gq != curG) {
                curG = gq;
                const uint4* L = traceLine(V, slot, gq);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint4 v = L[h];
                    w[2 * h][tid] = (uint64_t)v.x | ((uint64_t)v.y << 32);
                    w[2 * h + 1][tid] = (uint64_t)v.z | ((uint64_t)v.w << 32);
                }
            }
            ww = w[jq][tid];
        }
        if (rel > 31u) return false;
        hp = ((uint32_t)ww >> rel) & 1u;
        dg = ((uint32_t)(ww >> 32) >> rel) & 1u;
        return true;
    }
};

struct NarrowLineRows { // narrow rows: rel = tj + TB_BELOW - ti in [TBN_REL_LO, TBN_REL_HI], the two implied bits filled in
    uint32_t (&w)[TBN][256];
    const VPlanes& V;
    uint32_t slot, tid;
    uint32_t curG = 0xFFFFFFFFu; // the line (rows 16 g + 1 .. 16 g + 16) held in w[.][tid]
    __device__ __forceinline__ bool fetch(uint32_t ti, uint32_t tj, bool& hp, bool& dg) {
        const uint32_t rel = tj + TB_BELOW - ti;
        uint32_t wn = packTraceRowNarrow(0, (~0u) << MX32_LEFT, 0u);
        if (ti > 0) {
            const uint32_t gq = (ti - 1) >> 4, jq = (ti - 1) & 15u;
            if (gq != curG) {
                curG = gq;
                const uint4* L = traceLine(V, slot, gq);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint4 v = L[h];
                    w[4 * h][tid] = v.x;
                    w[4 * h + 1][tid] = v.y;
                    w[4 * h + 2][tid] = v.z;
                    w[4 * h + 3][tid] = v.w;
                }
            }
            wn = w[jq][tid];
        }
        if (rel < TBN_REL_LO || rel > TBN_REL_HI) return false;
        hp = rel >= TBN_HP_LO && ((wn >> (rel - TBN_HP_LO)) & 1u);
        dg = rel == TBN_REL_HI || ((wn >> (16u + rel - TBN_DG_LO)) & 1u);
        return true;
    }
};

constexpr uint32_t CIG_M = 0, CIG_I = 1, CIG_D = 2; // the steps of a walk = the operations of a CIGAR
struct NoObserver {
    __device__ __forceinline__ void operator()(uint32_t, uint32_t, bool, bool) const {}
};
// From cell (ti, tj) to column 0: horizontal before diagonal before vertical, row 0 has horizontal steps only.  sink(op) takes every
// step (CIG_I / CIG_M / CIG_D); observe(ti, tj, hp, dg) sees every cell before its step.  FLAG_CAPACITY and the walk stops where it is if
// a cell is not stored or row 0 would step upwards.  (k_traceback<false, .> used to take the vertical arm without asking ti > 0: row 0's HP
// is all ones inside the stored window, so the arm was never reached from row 0 and the guarded form here computes the same.)
// k_verify_wide and k_cigar_wide keep written-out COPIES of this walk over their 16-byte slab rows (and k_cigar_wide of CigarRuns): on the
// shared pieces the first ran 3 % longer and the second lost a register tier.  A change here belongs there too.
template <class Rows, class Sink, class Observe = NoObserver>
__device__ __forceinline__ void walkToColumn0(Rows rows, uint32_t& ti, uint32_t& tj, uint32_t& flags, Sink sink, Observe observe = Observe()) {
    while (tj > 0) {
        bool hp, dg;
        if (!rows.fetch(ti, tj, hp, dg)) {
            flags |= FLAG_CAPACITY;
            break;
        }
        observe(ti, tj, hp, dg);
        if (hp) { // gap in horizontal direction: insertion (:488-494, :553)
            --tj;
            sink(CIG_I);
        } else if (ti > 0 && dg) { // diagonal (:496-506, :559): the characters match, or D0 is not set
            --ti;
            --tj;
            sink(CIG_M);
        } else if (ti > 0) { // gap in vertical direction: deletion (:508-514)
            --ti;
            sink(CIG_D);
        } else {
            flags |= FLAG_CAPACITY;
            break;
        }
    }
}

// The CIGAR of a walk, run-length encoded as the steps come (END to BEGIN): (length << 2 | op) at myOps[0 .. nOps), at most `stride` of them
struct CigarRuns {
    uint16_t* myOps;
    uint32_t stride, nOps = 0, state = 3u, run = 0;
    __device__ __forceinline__ void flush() {
        if (run) {
            if (nOps < stride) myOps[nOps] = (uint16_t)((run << 2) | state);
            nOps++;
        }
    }
    __device__ __forceinline__ void emit(uint32_t op) {
        if (op != state) {
            flush();
            state = op;
            run = 0;
        }
        run++;
    }
    __device__ __forceinline__ uint32_t finish(uint32_t& flags) { // the last run; the number of runs (FLAG_CAPACITY beyond `stride`)
        flush();
        if (nOps > stride) flags |= FLAG_CAPACITY;
        return nOps;
    }
};

// Sequence assignment of an occurrence [begin, end) (IndexInterface::findSeqName, indexinterface.cpp:799-832): the sequence `begin`
// lies in; seqStarts[0] == 0, seqStarts[nSeqs] = end of the last sequence
__device__ __forceinline__ void assignSequence(const uint32_t* __restrict__ seqStarts, uint32_t nSeqs, uint32_t begin, uint32_t end, AlnRec& a) {
    const uint32_t s = lastAtOrBelow(seqStarts, nSeqs, begin);
    a.seqId = s;
    a.seqBegin = begin - seqStarts[s];
    a.spans = end > seqStarts[s + 1] ? 1u : 0u;
}

} // namespace cmb
