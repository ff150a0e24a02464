// SAM text of a chunk of read PAIRS in ALL mode, paired and written on the device (cmb_pair_sam_device): byte for byte what cmb_pair_sam
// (pair_sam.hip) returns pair by pair, from what the two mates' runs left in HBM (dev_sam.hpp: one SamCtx per mate, every strand
// filtered by itself, so the lists of a read are [forward | reverse complement]).
//
// Mirrors (reference, src/), through pair_sam.hip:
//   SearchStrategy::pairSingleEndedMatchesAll    searchstrategy.cpp:1345-1399
//   processComb{FR,RF,FF}All / pairOccurrences   searchstrategy.h:753-861, searchstrategy.cpp:1281-1344
//   generateSAMPairedEnd                         searchstrategy.cpp:1904-1970, indexhelpers.cpp:114-166
//   getFlagsPE / getMapQPairedEnd                indexhelpers.h:340-371, :390-410
//   createUnmappedSAMOccurrencePE                indexhelpers.cpp:186-213
//
// The device handles the two classes that make up almost every chunk — both mates without an occurrence, and pairs with at least one
// concordant combination whose occurrences all lie inside one sequence — and leaves the rest to cmb_pair_sam on the host, whose text
// k_pair_write copies into place (SAM_HOST, as k_sam_write does for reads with a trimmed occurrence).  Of that rest, the classes the
// caller selects (cmb_pair_sam_device_classes) are formatted by k_pair_class_write into the same side buffer, behind the host's text:
// one mate unmapped, discordant pairs, unpaired records; a pair beyond the 10 000-combination rule is a pair without any occurrence.
// Only a pair with an occurrence over a sequence end or without a sequence always goes to the host.  The b-move filter leaves a
// per-strand group in the same (begin, distance, width) order (move_search.hpp: k_mvs_text_keys, k_mvs_filter), so
// cmb_move_pair_sam_device runs the same kernels on the lists its batches keep.
//
// Order.  pairOccurrences walks the up list in TextOcc order and, per up occurrence, the down list from the lower bound of its begin;
// the reference sorts both by (begin, distance, width).  A per-strand group leaves k_filter_write in exactly that order: the filter's
// radix key is group | begin | distance | width (kernels.hpp: k_pack_keys; the strand bit is 0 in per-strand keys), a group is
// read x strand, k_filter_mark ranks the survivors in key order and drops equal keys, and k_filter_write stores at offset + rank.  So
// the lists are read as they lie, nothing is sorted here.  A candidate is named by (combination, up index, down index), which is
// also its place in the reference's pair list.
//
//   k_pair_plan   a wavefront per pair, lane-strided over the up occurrences (lists and pair counts of any length, in rounds of 64):
//                 the class; for a concordant pair the number of pairs, the minimal summed distance, the first pair that has it (the
//                 primary, which changes places with the first pair), the number of pairs at that distance, and the exact byte
//                 length of the text; the number of records, and whether the pair counts as mapped
//   (rocPRIM)     exclusive 64-bit scans of the lengths, of the record counts and of the mapped flags (a sum each, no atomics)
//   k_pair_write  a wavefront per PAIR_PER_WAVE consecutive pairs, windows and 16-byte stores as in k_sam_write.  The primary pair's
//                 two lines by all lanes (identifier, names, SEQ, QUAL) and lane 0 (numbers, literals); every other pair by the lane
//                 that owns its up occurrence: the lanes' byte counts are scanned in 64 bits, and a lane walks its down occurrences
//                 with a cursor that only moves forward, so a pair with thousands of records costs each window only its own lines.
#pragma once
#include "dev_sam.hpp"
#include "dev_wave.hpp"

namespace cmb {

constexpr uint32_t PAIR_PER_WAVE = 8; // consecutive pairs per wavefront of k_pair_write

struct PairCtx {
    SamCtx m[2]; // read 1, read 2 of every pair (m[0].nReads pairs)
    uint32_t orientation, maxFrag, minFrag;
};

// one strand list of one mate
struct PairSide {
    uint64_t q0;
    uint32_t n, mate, strand;
};
// combination c of the orientation: pairOccurrences(up, down) of searchstrategy.h:790-803 (FR), :848-861 (RF), :819-832 (FF)
//   FR: (fw1, rc2), (fw2, rc1)     RF: (rc1, fw2), (rc2, fw1)     FF: (fw1, fw2), (rc2, rc1)
__device__ __forceinline__ void pairCombo(const PairCtx& pc, uint32_t r, uint32_t c, PairSide& U, PairSide& D) {
    U.mate = c, D.mate = 1u - c;
    U.strand = pc.orientation == 0u ? 0u : pc.orientation == 1u ? 1u : c;
    D.strand = pc.orientation == 0u ? 1u : pc.orientation == 1u ? 0u : c;
    const uint64_t* fu = pc.m[U.mate].foffs + 2ull * r + U.strand;
    const uint64_t* fd = pc.m[D.mate].foffs + 2ull * r + D.strand;
    U.q0 = fu[0], U.n = (uint32_t)(fu[1] - fu[0]);
    D.q0 = fd[0], D.n = (uint32_t)(fd[1] - fd[0]);
}
// first occurrence of the list whose begin is not below pos (std::lower_bound, searchstrategy.cpp:1296)
__device__ __forceinline__ uint32_t pairLowerBound(const uint4* __restrict__ occ, uint64_t q0, uint32_t n, uint32_t pos) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (occ[q0 + mid].x < pos) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
// the next down occurrence at or behind `it` that forms a pair with the up occurrence (begin uBegin, sequence uSeq), as the loop of
// pairOccurrences takes them (searchstrategy.cpp:1298-1340): false, and the walk is over, at the first fragment beyond maxFrag
__device__ __forceinline__ bool pairSeek(const PairCtx& pc, const SamCtx& cd, const PairSide& D, uint32_t uBegin, uint32_t uSeq, uint32_t& it) {
    for (; it < D.n; it++) {
        const uint32_t frag = cd.occ[D.q0 + it].y - uBegin;
        if (frag > pc.maxFrag) break;
        if (frag >= pc.minFrag && cd.aln[D.q0 + it].seqId == uSeq) return true;
    }
    it = D.n;
    return false;
}

// what a record needs of its read
struct PairRead {
    const uint8_t *id, *rd, *ql; // ql == nullptr: no qualities
    uint32_t idLen, readLen, qualLen;
};
__device__ __forceinline__ PairRead pairRead(const SamCtx& cx, uint32_t r, uint32_t idLen) {
    PairRead R;
    R.id = cx.ids + (cx.idOffs[r] - cx.idBase) + 1u;
    R.rd = cx.reads + cx.offs[r];
    R.readLen = (uint32_t)(cx.offs[r + 1] - cx.offs[r]);
    R.ql = cx.quals ? cx.quals + (cx.qualOffs[r] - cx.qualBase) : nullptr;
    R.qualLen = cx.quals ? (uint32_t)(cx.qualOffs[r + 1] - cx.qualOffs[r]) : 0u; // (empty: "*" on a mapped record, nothing on an unmapped one)
    R.idLen = idLen;
    return R;
}

// createUnmappedSAMOccurrencePE for a pair without any occurrence: "id \t FLAGS \t*\t0\t0\t*\t*\t0\t0\t SEQ \t QUAL \tPG:Z:Columba\n"
// (flags: 77 / 141 for such a pair; beside a mapped mate 1 | 4 | 32 x the mate's strand | 64 / 128)
__device__ __forceinline__ uint32_t pairUnmappedFlags(uint32_t mate) { return 1u | 4u | 8u | (mate ? 128u : 64u); }
__device__ __forceinline__ uint32_t pairUnmappedSeqAtF(const PairRead& R, uint32_t flags) { return R.idLen + 1u + decWidth(flags) + 15u; }
__device__ __forceinline__ uint64_t pairUnmappedLenF(const PairRead& R, uint32_t flags) {
    return (uint64_t)pairUnmappedSeqAtF(R, flags) + R.readLen + 1u + R.qualLen + 14u;
}
__device__ __forceinline__ uint32_t pairUnmappedSeqAt(const PairRead& R, uint32_t mate) { return pairUnmappedSeqAtF(R, pairUnmappedFlags(mate)); }
__device__ __forceinline__ uint64_t pairUnmappedLen(const PairRead& R, uint32_t mate) { return pairUnmappedLenF(R, pairUnmappedFlags(mate)); }

// a candidate pair and one of its two records (generateSAMPairedEnd, indexhelpers.cpp:114-166)
struct PairCand {
    SamHitDev u, d;
    uint32_t frag; // end of the down occurrence - begin of the up occurrence, inside their sequence
};
__device__ __forceinline__ PairCand pairLoad(const SamCtx& cu, uint64_t uq, const SamCtx& cd, uint64_t dq) {
    PairCand c;
    c.u = samLoadHit(cu, uq);
    c.d = samLoadHit(cd, dq);
    const uint4 od = cd.occ[dq];
    c.frag = c.d.pos1 + (od.y - od.x) - c.u.pos1;
    return c;
}
struct PairLine {
    SamHitDev h, m; // the record's occurrence and its mate's
    uint32_t flags, mapq, frag, neg;
};
__device__ __forceinline__ PairLine pairLine(const PairCand& c, bool down, uint32_t meMate, bool primary, uint32_t minDist, uint32_t nPairs,
                                             uint32_t proper = 2u /* 0: a discordant pair */) {
    PairLine L;
    L.h = down ? c.d : c.u;
    L.m = down ? c.u : c.d;
    L.flags = 1u | proper | (L.h.strand ? 16u : 0u) | (L.m.strand ? 32u : 0u) | (meMate ? 128u : 64u) | (primary ? 0u : 256u); // getFlagsPE
    L.mapq = c.u.dist + c.d.dist > minDist ? 0u : samMapQ(nPairs);                                                     // getMapQPairedEnd
    L.frag = c.frag;
    L.neg = L.h.pos1 > L.m.pos1 ? 1u : 0u; // TLEN is negative on the record that lies behind its mate
    return L;
}
__device__ __forceinline__ uint32_t pairMateNameAt(const PairLine& L, uint32_t idLen) {
    return idLen + 1u + decWidth(L.flags) + 1u + L.h.nameLen + 1u + decWidth(L.h.pos1) + 1u + decWidth(L.mapq) + 1u + L.h.cigLen + 1u;
}
__device__ __forceinline__ uint32_t pairSeqAt(const PairLine& L, uint32_t idLen) {
    return pairMateNameAt(L, idLen) + L.m.nameLen + 1u + decWidth(L.m.pos1) + 1u + L.neg + decWidth(L.frag) + 1u;
}
__device__ __forceinline__ uint32_t pairQualPrinted(const PairRead& R) { return R.qualLen ? R.qualLen : 1u; }
__device__ __forceinline__ uint32_t pairLineLen(const PairLine& L, const PairRead& R) {
    return pairSeqAt(L, R.idLen) + R.readLen + 1u + pairQualPrinted(R) + 6u + decWidth(L.h.dist) + 6u + decWidth(L.h.dist) + 14u;
}
// bytes of the two records of a candidate whose up occurrence belongs to read uMate
__device__ __forceinline__ uint64_t pairCandLen(const PairCand& c, uint32_t uMate, const PairRead* R, bool primary, uint32_t minDist, uint32_t nPairs) {
    return (uint64_t)pairLineLen(pairLine(c, false, uMate, primary, minDist, nPairs), R[uMate]) +
           pairLineLen(pairLine(c, true, 1u - uMate, primary, minDist, nPairs), R[1u - uMate]);
}

// generateSAMPairedEnd swaps the primary pair with the first one (searchstrategy.cpp:1925-1936).  The primary's records are written
// first; in the walk over the candidates the first pair's records then take the primary's place and its own place stays empty.
// -> which candidate's records stand at the place of candidate (c, u, d); false: none
__device__ __forceinline__ bool pairSlot(const PairPlan& pp, uint32_t c, uint32_t u, uint32_t d, uint32_t& sc, uint32_t& su, uint32_t& sd) {
    const bool isPrim = c == pp.primCombo && u == pp.primU && d == pp.primD;
    const bool isFirst = c == pp.firstCombo && u == pp.firstU && d == pp.firstD;
    sc = isPrim ? pp.firstCombo : c, su = isPrim ? pp.firstU : u, sd = isPrim ? pp.firstD : d;
    return !isFirst;
}
// bytes at the place of candidate (c, u, d) of pair r (both records, as secondary ones)
__device__ __forceinline__ uint64_t pairSlotLen(const PairCtx& pc, uint32_t r, const PairPlan& pp, const PairRead* R, uint32_t c, uint32_t u, uint32_t d) {
    uint32_t sc, su, sd;
    if (!pairSlot(pp, c, u, d, sc, su, sd)) return 0;
    PairSide U, D;
    pairCombo(pc, r, sc, U, D);
    const PairCand cand = pairLoad(pc.m[U.mate], U.q0 + su, pc.m[D.mate], D.q0 + sd);
    return pairCandLen(cand, U.mate, R, false, pp.minDist, pp.nPairs);
}

// ---- the pairs without a concordant combination, and those with one mate unmapped (cmb_pair_sam_device_classes; pair_sam.hip:238-278:
// pairDiscordantly -> addDiscPairs / addUnpairedMatches / addOneUnmapped).  Every occurrence they see is assigned and inside one sequence
// (the host condition comes first).  The class of a pair is also its place among the counters; class c >= 2 is selected by bit c - 2 of
// the caller's mask (CMB_PAIR_CLASS_*)
constexpr uint32_t PAIR_CLS_BOTH_UNMAPPED = 0, PAIR_CLS_CONCORDANT = 1, PAIR_CLS_ONE_UNMAPPED = 2, PAIR_CLS_DISCORDANT = 3, PAIR_CLS_UNPAIRED = 4,
                   PAIR_CLS_OVER_LIMIT = 5, PAIR_CLS_COUNTERS = 8;
constexpr unsigned long long PAIR_DISC_LIMIT = 10000; // combinations beyond which pairDiscordantly gives up (searchstrategy.cpp:1619)
__device__ const uint8_t PAIR_STAR[4] = {'*', 0, 0, 0};

// the first occurrence of minimal distance among the n at q0, that distance and how many have it.  A whole wavefront.
struct PairSolo {
    uint32_t primary, best, nBest;
};
__device__ __forceinline__ PairSolo pairSolo(const SamCtx& cx, uint64_t q0, uint32_t n, uint32_t lane) {
    unsigned long long key = ~0ull;
    for (uint32_t j = lane; j < n; j += 64u) {
        const unsigned long long k = ((unsigned long long)cx.occ[q0 + j].z << 32) | j;
        key = k < key ? k : key;
    }
    key = waveMin64(key);
    PairSolo S;
    S.primary = (uint32_t)key, S.best = (uint32_t)(key >> 32);
    uint32_t cnt = 0;
    for (uint32_t j = lane; j < n; j += 64u) cnt += cx.occ[q0 + j].z == S.best ? 1u : 0u;
    S.nBest = (uint32_t)waveSum64(cnt);
    return S;
}
// addOneUnmapped: the record of an occurrence whose mate has none (cmb_sam_pe without a mate: RNEXT "*", PNEXT 0, TLEN 0)
__device__ __forceinline__ PairLine pairHalfLine(const SamHitDev& h, uint32_t meMate, bool primary, uint32_t minDist, uint32_t nPairs) {
    PairLine L;
    L.h = h;
    L.m = SamHitDev{};
    L.m.name = PAIR_STAR, L.m.nameLen = 1u;
    L.flags = 1u | 8u | (h.strand ? 16u : 0u) | (meMate ? 128u : 64u) | (primary ? 0u : 256u);
    L.mapq = h.dist > minDist ? 0u : samMapQ(nPairs);
    L.frag = 0, L.neg = 0;
    return L;
}
// addDiscPairs: occurrence q1 of read 1 with occurrence q2 of read 2.  Up is the one that begins first inside its sequence, read 2's on
// a tie, whether or not the sequences are the same; the fragment size is 0 across sequences (pair_sam.hip:245-250).  uMate: whose is up
__device__ __forceinline__ PairCand pairDiscCand(const PairCtx& pc, uint64_t q1, uint64_t q2, uint32_t& uMate) {
    const SamCtx &c1 = pc.m[0], &c2 = pc.m[1];
    const SamHitDev a = samLoadHit(c1, q1), b = samLoadHit(c2, q2);
    const bool aUp = a.pos1 < b.pos1, sameRef = c1.aln[q1].seqId == c2.aln[q2].seqId;
    const uint4 od = aUp ? c2.occ[q2] : c1.occ[q1];
    PairCand c;
    c.u = aUp ? a : b;
    c.d = aUp ? b : a;
    c.frag = sameRef ? c.d.pos1 + (od.y - od.x) - c.u.pos1 : 0u;
    uMate = aUp ? 0u : 1u;
    return c;
}
__device__ __forceinline__ uint64_t pairDiscLen(const PairCtx& pc, uint64_t q1, uint64_t q2, const PairRead* R, bool primary, uint32_t minDist,
                                                uint32_t nPairs) {
    uint32_t uMate;
    const PairCand c = pairDiscCand(pc, q1, q2, uMate);
    return (uint64_t)pairLineLen(pairLine(c, false, uMate, primary, minDist, nPairs, 0u), R[uMate]) +
           pairLineLen(pairLine(c, true, 1u - uMate, primary, minDist, nPairs, 0u), R[1u - uMate]);
}
// bytes at the place of candidate (i1, i2) of a discordant pair whose lists begin at q10 and q20 (pairSlot with one combination)
__device__ __forceinline__ uint64_t pairDiscSlotLen(const PairCtx& pc, uint64_t q10, uint64_t q20, const PairPlan& pp, const PairRead* R, uint32_t i1,
                                                    uint32_t i2) {
    uint32_t sc, su, sd;
    if (!pairSlot(pp, 0u, i1, i2, sc, su, sd)) return 0;
    return pairDiscLen(pc, q10 + su, q20 + sd, R, false, pp.minDist, pp.nPairs);
}
// addUnpairedMatches: a record of cmb_sam_unpaired (no strand bit; SEQ and QUAL on the read's first record only)
__device__ __forceinline__ uint32_t pairSoloFlags(uint32_t mate, bool first) { return 1u | (mate ? 128u : 64u) | (first ? 0u : 256u); }
__device__ __forceinline__ uint32_t pairSoloMapQ(const SamHitDev& h, const PairSolo& S) { return h.dist == S.best ? samMapQ(S.nBest) : 0u; }
__device__ __forceinline__ uint32_t pairSoloLineLen(const PairRead& R, const SamHitDev& h, uint32_t mate, bool first, const PairSolo& S) {
    return samLineLen(R.idLen, h, pairSoloFlags(mate, first), pairSoloMapQ(h, S), first ? R.readLen : 1u, first ? pairQualPrinted(R) : 1u);
}

__global__ void __launch_bounds__(256)
k_pair_plan(PairCtx pc, uint32_t unmapped, SamPlan* __restrict__ plan, PairPlan* __restrict__ pplan, uint64_t* __restrict__ len,
            uint64_t* __restrict__ records /* SAM lines of the pair */, uint32_t* __restrict__ mapped /* 1: a concordant pair */,
            uint32_t* __restrict__ hostList /* [0]: how many */, uint32_t classes /* CMB_PAIR_CLASS_* the device formats */,
            uint32_t discordantAllowed, uint32_t* __restrict__ clsList /* [0]: how many */, uint64_t* __restrict__ clsLen,
            uint32_t* __restrict__ clsCount /* [PAIR_CLS_COUNTERS] */) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= pc.m[0].nReads) return; // (a whole wavefront)
    SamPlan pl{};
    uint32_t cls = PAIR_CLS_BOTH_UNMAPPED;
    bool side = false; // a pair of k_pair_class_write
    PairPlan pp{};
    PairRead R[2];
    uint32_t nOcc[2];
    for (uint32_t m = 0; m < 2u; m++) {
        R[m] = pairRead(pc.m[m], r, samIdLen(pc.m[m], r, lane));
        nOcc[m] = (uint32_t)(pc.m[m].foffs[2ull * r + 2u] - pc.m[m].foffs[2ull * r]);
    }
    pp.idLen[0] = R[0].idLen, pp.idLen[1] = R[1].idLen;
    uint64_t total = 0, nRecords = 0;
    uint32_t isMapped = 0;
    if (nOcc[0] == 0u && nOcc[1] == 0u) { // addBothUnmapped (searchstrategy.h:1236-1247)
        pl.kind = unmapped ? SAM_UNMAPPED : SAM_NOTHING;
        if (unmapped) total = pairUnmappedLen(R[0], 0u) + pairUnmappedLen(R[1], 1u), nRecords = 2;
    } else {
        const bool one = nOcc[0] == 0u || nOcc[1] == 0u; // addOneUnmapped
        bool host = one && !(classes & 1u);
        if (!host) { // findSeqName trims or drops: the lists the host pairs may differ from these
            uint32_t over = 0;
            for (uint32_t m = 0; m < 2u; m++) {
                const SamCtx& cx = pc.m[m];
                const uint64_t q0 = cx.foffs[2ull * r];
                for (uint32_t j = lane; j < nOcc[m]; j += 64u) {
                    const AlnRec a = cx.aln[q0 + j];
                    over |= a.spans != 0u || a.seqId >= cx.nSeqs ? 1u : 0u;
                }
            }
            host = __ballot(over != 0u) != 0ull;
        }
        unsigned long long nCand = 0;
        if (!host && one) cls = PAIR_CLS_ONE_UNMAPPED;
        if (!host && !one) {
            // every candidate once: their number, the first one, the first one of minimal summed distance and how many have it.  A key
            // orders the candidates of different up occurrences (distance | combination | up index); those of one up occurrence come in
            // order, so the lane keeps the first
            unsigned long long bestKey = ~0ull, firstKey = ~0ull;
            uint32_t bestD = 0, firstD = 0, laneMin = 0xFFFFFFFFu;
            unsigned long long laneCnt = 0;
            for (uint32_t c = 0; c < 2u; c++) {
                PairSide U, D;
                pairCombo(pc, r, c, U, D);
                if (!U.n || !D.n) continue; // (wave-uniform)
                const SamCtx &cu = pc.m[U.mate], &cd = pc.m[D.mate];
                for (uint32_t ub = 0; ub < U.n; ub += 64u) {
                    const uint32_t u = ub + lane;
                    if (u >= U.n) continue;
                    const uint4 uo = cu.occ[U.q0 + u];
                    const uint32_t uSeq = cu.aln[U.q0 + u].seqId;
                    const unsigned long long at = ((unsigned long long)c << 39) | u;
                    bool any = false;
                    for (uint32_t it = pairLowerBound(cd.occ, D.q0, D.n, uo.x); pairSeek(pc, cd, D, uo.x, uSeq, it); it++) {
                        const uint32_t sum = uo.z + cd.occ[D.q0 + it].z;
                        const unsigned long long key = ((unsigned long long)sum << 40) | at;
                        if (key < bestKey) bestKey = key, bestD = it;
                        if (sum < laneMin) laneMin = sum, laneCnt = 0;
                        laneCnt += sum == laneMin ? 1u : 0u;
                        if (!any && at < firstKey) firstKey = at, firstD = it;
                        any = true;
                        nCand++;
                    }
                }
            }
            nCand = waveSum64(nCand);
            if (nCand == 0) { // no concordant pair: pairDiscordantly (searchstrategy.cpp:1586-1646)
                cls = !discordantAllowed                                                               ? PAIR_CLS_UNPAIRED
                      : (unsigned long long)nOcc[0] * (unsigned long long)nOcc[1] > PAIR_DISC_LIMIT ? PAIR_CLS_OVER_LIMIT
                                                                                                       : PAIR_CLS_DISCORDANT;
            } else {
                cls = PAIR_CLS_CONCORDANT;
                const unsigned long long gBest = waveMin64(bestKey), gFirst = waveMin64(firstKey);
                pp.minDist = (uint32_t)(gBest >> 40);
                pp.primCombo = (uint32_t)(gBest >> 39) & 1u, pp.primU = (uint32_t)gBest;
                pp.primD = (uint32_t)waveSum64(bestKey == gBest ? bestD : 0u); // (one lane holds the key)
                pp.firstCombo = (uint32_t)(gFirst >> 39) & 1u, pp.firstU = (uint32_t)gFirst;
                pp.firstD = (uint32_t)waveSum64(firstKey == gFirst ? firstD : 0u);
                const unsigned long long atMin = waveSum64(laneMin == pp.minDist ? laneCnt : 0ull);
                pp.nPairs = atMin < 0xFFFFFFFFull ? (uint32_t)atMin : 0xFFFFFFFFu; // (MAPQ is 0 from ten pairs on)
            }
        }
        if (!host && cls >= PAIR_CLS_ONE_UNMAPPED && !((classes >> (cls - PAIR_CLS_ONE_UNMAPPED)) & 1u)) host = true; // (not selected)
        if (host) {
            pl.kind = SAM_HOST; // (its length comes from the host: k_sam_override)
            if (lane == 0) hostList[1u + atomicAdd(hostList, 1u)] = r;
        } else if (cls == PAIR_CLS_OVER_LIMIT) { // addUnpairedMatches twice, the second time on emptied lists: a pair without any occurrence
            pl.kind = unmapped ? SAM_UNMAPPED : SAM_NOTHING;
            if (unmapped) total = pairUnmappedLen(R[0], 0u) + pairUnmappedLen(R[1], 1u), nRecords = 2;
        } else if (cls == PAIR_CLS_ONE_UNMAPPED) {
            const uint32_t m = nOcc[0] ? 0u : 1u;
            const SamCtx& cx = pc.m[m];
            const uint64_t q0 = cx.foffs[2ull * r];
            const PairSolo S = pairSolo(cx, q0, nOcc[m], lane);
            pp.primU = S.primary, pp.minDist = S.best, pp.nPairs = S.nBest;
            unsigned long long sum = 0;
            for (uint32_t j = lane; j < nOcc[m]; j += 64u)
                sum += pairLineLen(pairHalfLine(samLoadHit(cx, q0 + j), m, j == S.primary, S.best, S.nBest), R[m]);
            const uint32_t mateFlags = 1u | 4u | (cx.occ[q0 + S.primary].w ? 32u : 0u) | (m ? 64u : 128u);
            total = waveSum64(sum) + pairUnmappedLenF(R[1u - m], mateFlags);
            nRecords = (uint64_t)nOcc[m] + 1u;
            side = true;
        } else if (cls == PAIR_CLS_DISCORDANT) {
            const uint64_t q10 = pc.m[0].foffs[2ull * r], q20 = pc.m[1].foffs[2ull * r];
            const PairSolo S1 = pairSolo(pc.m[0], q10, nOcc[0], lane), S2 = pairSolo(pc.m[1], q20, nOcc[1], lane);
            // the summed distance is minimal where both are, so the first such candidate in (i1, i2) order is (first, first)
            pp.primU = S1.primary, pp.primD = S2.primary, pp.minDist = S1.best + S2.best, pp.nPairs = S1.nBest * S2.nBest; // (<= 10 000)
            unsigned long long sum = 0;
            for (uint32_t i1 = lane; i1 < nOcc[0]; i1 += 64u)
                for (uint32_t i2 = 0; i2 < nOcc[1]; i2++)
                    sum += pairDiscLen(pc, q10 + i1, q20 + i2, R, i1 == pp.primU && i2 == pp.primD, pp.minDist, pp.nPairs);
            total = waveSum64(sum);
            nRecords = 2ull * nOcc[0] * nOcc[1];
            isMapped = 1u;
            side = true;
        } else if (cls == PAIR_CLS_UNPAIRED) {
            unsigned long long sum = 0;
            for (uint32_t m = 0; m < 2u; m++) {
                const SamCtx& cx = pc.m[m];
                const uint64_t q0 = cx.foffs[2ull * r];
                const PairSolo S = pairSolo(cx, q0, nOcc[m], lane);
                for (uint32_t j = lane; j < nOcc[m]; j += 64u) sum += pairSoloLineLen(R[m], samLoadHit(cx, q0 + j), m, j == S.primary, S);
            }
            total = waveSum64(sum);
            nRecords = (uint64_t)nOcc[0] + nOcc[1];
            side = true;
        } else {
            pl.kind = SAM_MAPPED;
            // the bytes: the primary's records, then every place of the walk
            unsigned long long sum = 0;
            for (uint32_t c = 0; c < 2u; c++) {
                PairSide U, D;
                pairCombo(pc, r, c, U, D);
                if (!U.n || !D.n) continue;
                const SamCtx &cu = pc.m[U.mate], &cd = pc.m[D.mate];
                for (uint32_t ub = 0; ub < U.n; ub += 64u) {
                    const uint32_t u = ub + lane;
                    if (u >= U.n) continue;
                    const uint4 uo = cu.occ[U.q0 + u];
                    const uint32_t uSeq = cu.aln[U.q0 + u].seqId;
                    for (uint32_t it = pairLowerBound(cd.occ, D.q0, D.n, uo.x); pairSeek(pc, cd, D, uo.x, uSeq, it); it++)
                        sum += pairSlotLen(pc, r, pp, R, c, u, it);
                }
            }
            PairSide U, D;
            pairCombo(pc, r, pp.primCombo, U, D);
            const PairCand prim = pairLoad(pc.m[U.mate], U.q0 + pp.primU, pc.m[D.mate], D.q0 + pp.primD);
            total = waveSum64(sum) + pairCandLen(prim, U.mate, R, true, pp.minDist, pp.nPairs);
            nRecords = 2ull * nCand;
            isMapped = 1u;
        }
    }
    if (side) pl.kind = SAM_HOST; // (k_pair_write copies it from the side buffer, where k_pair_class_write puts it)
    pl.cls = cls;
    if (lane == 0) {
        plan[r] = pl;
        pplan[r] = pp;
        len[r] = total;
        records[r] = nRecords;
        mapped[r] = isMapped;
        clsLen[r] = side ? total : 0ull;
        if (side) clsList[1u + atomicAdd(clsList, 1u)] = r;
        if (pl.kind != SAM_HOST || side) atomicAdd(clsCount + cls, 1u);
    }
}

// one record by one cursor.  COOP: identifier, names, SEQ and QUAL are left out (the wavefront copies them, pairCoopLine)
template <bool COOP> __device__ __forceinline__ void pairEmitLine(SamEm& e, const PairLine& L, const PairRead& R) {
    const uint32_t qualP = pairQualPrinted(R);
    if (COOP) e.skip(R.idLen);
    else e.bytes(R.id, R.idLen);
    e.ch('\t');
    e.dec(L.flags);
    e.ch('\t');
    if (COOP) e.skip(L.h.nameLen);
    else e.bytes(L.h.name, L.h.nameLen);
    e.ch('\t');
    e.dec(L.h.pos1);
    e.ch('\t');
    e.dec(L.mapq);
    e.ch('\t');
    e.cigar(L.h);
    e.ch('\t');
    if (COOP) e.skip(L.m.nameLen);
    else e.bytes(L.m.name, L.m.nameLen);
    e.ch('\t');
    e.dec(L.m.pos1);
    e.ch('\t');
    if (L.neg) e.ch('-');
    e.dec(L.frag);
    e.ch('\t');
    if (COOP) {
        e.skip(R.readLen);
        e.ch('\t');
        e.skip(qualP);
    } else {
        for (uint32_t i = 0; i < R.readLen; i++) e.ch(L.h.strand ? samComplement(samCleanBase(R.rd[R.readLen - 1u - i])) : samCleanBase(R.rd[i]));
        e.ch('\t');
        for (uint32_t i = 0; i < qualP; i++) e.ch(!R.qualLen ? (uint8_t)'*' : L.h.strand ? R.ql[R.qualLen - 1u - i] : R.ql[i]);
    }
    e.lit("\tAS:i:");
    e.dec(L.h.dist);
    e.lit("\tNM:i:");
    e.dec(L.h.dist);
    e.lit("\tPG:Z:Columba\n");
}
// all lanes: the record at `at`, whatever of it lies in the window
__device__ __forceinline__ void pairCoopLine(const SamWriter& w, uint64_t at, const PairLine& L, const PairRead& R, uint32_t lineLen) {
    const uint32_t idLen = R.idLen, readLen = R.readLen, qualLen = R.qualLen, qualP = pairQualPrinted(R), strand = L.h.strand;
    const uint8_t *id = R.id, *rd = R.rd, *ql = R.ql, *name = L.h.name, *mname = L.m.name;
    const uint32_t seqAt = pairSeqAt(L, idLen);
    w.coop(at, idLen, [&](uint64_t i) { return id[i]; });
    w.coop(at + idLen + 1u + decWidth(L.flags) + 1u, L.h.nameLen, [&](uint64_t i) { return name[i]; });
    w.coop(at + pairMateNameAt(L, idLen), L.m.nameLen, [&](uint64_t i) { return mname[i]; });
    w.coop(at + seqAt, readLen, [&](uint64_t i) { return strand ? samComplement(samCleanBase(rd[readLen - 1u - (uint32_t)i])) : samCleanBase(rd[i]); });
    w.coop(at + seqAt + readLen + 1u, qualP, [&](uint64_t i) { return !qualLen ? (uint8_t)'*' : strand ? ql[qualLen - 1u - (uint32_t)i] : ql[i]; });
    if ((threadIdx.x & 63u) == 0u && w.touches(at, lineLen)) {
        SamEm e = w.cursor(at);
        pairEmitLine<true>(e, L, R);
    }
}

__global__ void __launch_bounds__(64)
k_pair_write(PairCtx pc, const SamPlan* __restrict__ plan, const PairPlan* __restrict__ pplan, const uint64_t* __restrict__ outOffs,
             const uint8_t* __restrict__ side, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[SAM_WIN];
    const uint32_t lane = threadIdx.x;
    const uint32_t nPairsAll = pc.m[0].nReads;
    const uint64_t rr = (uint64_t)blockIdx.x * PAIR_PER_WAVE;
    if (rr >= nPairsAll) return;
    const uint32_t r0 = (uint32_t)rr, r1 = nPairsAll - r0 < PAIR_PER_WAVE ? nPairsAll : r0 + PAIR_PER_WAVE;
    SamWriter w{lds, out, 0, outOffs[r0], outOffs[r1]};
    if (w.G0 == w.G1) return;
    w.winLo = w.G0 / SAM_WIN * SAM_WIN;
    for (uint32_t r = r0; r < r1; r++) {
        const uint64_t start = outOffs[r], bytes = outOffs[r + 1] - start; // (the same in every lane)
        if (!bytes) continue;
        const SamPlan pl = plan[r];
        if (pl.kind == SAM_HOST) {
            const uint8_t* src = side + pl.sideOff;
            w.stream(start + bytes, [&]() { w.coop(start, bytes, [&](uint64_t i) { return src[i]; }); });
            continue;
        }
        const PairPlan pp = pplan[r];
        PairRead R[2];
        for (uint32_t m = 0; m < 2u; m++) R[m] = pairRead(pc.m[m], r, pp.idLen[m]);
        if (pl.kind == SAM_UNMAPPED) {
            uint64_t cur = start;
            for (uint32_t m = 0; m < 2u; m++) {
                const PairRead& Rm = R[m];
                const uint64_t recLen = pairUnmappedLen(Rm, m), seqAt = cur + pairUnmappedSeqAt(Rm, m);
                const uint8_t *id = Rm.id, *rd = Rm.rd, *ql = Rm.ql;
                w.stream(cur + recLen, [&]() {
                    w.coop(cur, Rm.idLen, [&](uint64_t i) { return id[i]; });
                    w.coop(seqAt, Rm.readLen, [&](uint64_t i) { return samCleanBase(rd[i]); });
                    w.coop(seqAt + Rm.readLen + 1u, Rm.qualLen, [&](uint64_t i) { return ql[i]; });
                    if (lane == 0 && w.touches(cur, recLen)) {
                        SamEm e = w.cursor(cur);
                        e.skip(Rm.idLen);
                        e.ch('\t');
                        e.dec(pairUnmappedFlags(m));
                        e.lit("\t*\t0\t0\t*\t*\t0\t0\t");
                        e.skip(Rm.readLen);
                        e.ch('\t');
                        e.skip(Rm.qualLen);
                        e.lit("\tPG:Z:Columba\n");
                    }
                });
                cur += recLen;
            }
            continue;
        }
        // SAM_MAPPED: the primary pair's records by all lanes ...
        uint64_t cur = start;
        {
            PairSide U, D;
            pairCombo(pc, r, pp.primCombo, U, D);
            const PairCand prim = pairLoad(pc.m[U.mate], U.q0 + pp.primU, pc.m[D.mate], D.q0 + pp.primD);
            for (uint32_t down = 0; down < 2u; down++) {
                const uint32_t me = down ? D.mate : U.mate;
                const PairLine L = pairLine(prim, down != 0u, me, true, pp.minDist, pp.nPairs);
                const uint32_t lineLen = pairLineLen(L, R[me]);
                w.stream(cur + lineLen, [&]() { pairCoopLine(w, cur, L, R[me], lineLen); });
                cur += lineLen;
            }
        }
        // ... the others by the lane of their up occurrence, 64 up occurrences at a time
        for (uint32_t c = 0; c < 2u; c++) {
            PairSide U, D;
            pairCombo(pc, r, c, U, D);
            if (!U.n || !D.n) continue; // (wave-uniform)
            const SamCtx &cu = pc.m[U.mate], &cd = pc.m[D.mate];
            for (uint32_t ub = 0; ub < U.n; ub += 64u) {
                const uint32_t u = ub + lane;
                uint32_t uBegin = 0, uSeq = 0, it = D.n;
                unsigned long long mine = 0;
                if (u < U.n) {
                    uBegin = cu.occ[U.q0 + u].x;
                    uSeq = cu.aln[U.q0 + u].seqId;
                    const uint32_t it0 = pairLowerBound(cd.occ, D.q0, D.n, uBegin);
                    for (it = it0; pairSeek(pc, cd, D, uBegin, uSeq, it); it++) mine += pairSlotLen(pc, r, pp, R, c, u, it);
                    it = it0;
                }
                unsigned long long total;
                uint64_t pos = cur + waveExclusiveScan64(mine, total); // this lane's next record, and the down occurrence it belongs to: `it`
                bool more = mine != 0ull;
                w.stream(cur + total, [&]() {
                    const uint64_t winHi = w.winLo + SAM_WIN;
                    while (more && pos < winHi) {
                        if (!pairSeek(pc, cd, D, uBegin, uSeq, it)) {
                            more = false;
                            break;
                        }
                        uint32_t sc, su, sd;
                        uint64_t pairLen = 0;
                        if (pairSlot(pp, c, u, it, sc, su, sd)) {
                            PairSide SU, SD;
                            pairCombo(pc, r, sc, SU, SD);
                            const PairCand cand = pairLoad(pc.m[SU.mate], SU.q0 + su, pc.m[SD.mate], SD.q0 + sd);
                            const PairLine up = pairLine(cand, false, SU.mate, false, pp.minDist, pp.nPairs);
                            const PairLine dn = pairLine(cand, true, SD.mate, false, pp.minDist, pp.nPairs);
                            const uint32_t upLen = pairLineLen(up, R[SU.mate]);
                            pairLen = (uint64_t)upLen + pairLineLen(dn, R[SD.mate]);
                            if (pos + pairLen > w.winLo) {
                                SamEm e = w.cursor(pos);
                                if (pos + upLen > w.winLo) pairEmitLine<false>(e, up, R[SU.mate]);
                                else e.skip(upLen);
                                pairEmitLine<false>(e, dn, R[SD.mate]);
                            }
                        }
                        if (pos + pairLen > winHi) break; // (goes on in the next window)
                        pos += pairLen;
                        it++;
                    }
                });
                cur += total;
            }
        }
    }
    if (w.G1 > w.winLo) {
        __syncthreads();
        w.flush();
    }
}

// one record of cmb_sam_unpaired by one cursor
__device__ __forceinline__ void pairEmitSolo(SamEm& e, const PairRead& R, const SamHitDev& h, uint32_t mate, bool first, const PairSolo& S) {
    e.bytes(R.id, R.idLen);
    e.ch('\t');
    e.dec(pairSoloFlags(mate, first));
    e.ch('\t');
    e.bytes(h.name, h.nameLen);
    e.ch('\t');
    e.dec(h.pos1);
    e.ch('\t');
    e.dec(pairSoloMapQ(h, S));
    e.ch('\t');
    e.cigar(h);
    e.lit("\t*\t0\t0\t");
    if (first) {
        for (uint32_t i = 0; i < R.readLen; i++) e.ch(h.strand ? samComplement(samCleanBase(R.rd[R.readLen - 1u - i])) : samCleanBase(R.rd[i]));
        e.ch('\t');
        const uint32_t qualP = pairQualPrinted(R);
        for (uint32_t i = 0; i < qualP; i++) e.ch(!R.qualLen ? (uint8_t)'*' : h.strand ? R.ql[R.qualLen - 1u - i] : R.ql[i]);
    } else {
        e.lit("*\t*");
    }
    e.lit("\tAS:i:");
    e.dec(h.dist);
    e.lit("\tNM:i:");
    e.dec(h.dist);
    e.lit("\tPG:Z:Columba\n");
}

// The pairs with one mate unmapped, the discordant and the unpaired ones (k_pair_plan listed them): a wavefront per pair writes the
// pair's text into the SIDE buffer, behind the bytes of the host's pairs, at base + offs[r], and notes the place in the pair's plan;
// k_pair_write copies it from there as it copies a host pair's.  So k_pair_write stays as it is, and no piece of the final text has two
// writers (SamWriter::flush stores whole windows of a piece).  Windows and cursors as in k_pair_write.
//   one mate unmapped  the mapped mate's records as k_sam_write orders a read's (the primary changes places with the first), a lane
//                      each 64 at a time; the unmapped mate's record follows the primary's
//   discordant         the primary candidate's two records by all lanes, then the full cross product in (i1, i2) order: a lane owns
//                      an occurrence of read 1 and walks read 2's list with a cursor that only moves forward
//   unpaired           read 1's records, then read 2's, each list STABLY sorted by distance: one pass over the list per distance that
//                      occurs, 64 occurrences at a time, a lane's record placed by a wave scan over those of that distance
__global__ void __launch_bounds__(64)
k_pair_class_write(PairCtx pc, SamPlan* __restrict__ plan, const PairPlan* __restrict__ pplan, const uint32_t* __restrict__ clsList,
                   const uint64_t* __restrict__ offs, uint64_t base, uint8_t* __restrict__ side) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[SAM_WIN];
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= clsList[0]) return;
    const uint32_t r = clsList[1u + blockIdx.x];
    const uint64_t start = base + offs[r], bytes = offs[r + 1] - offs[r];
    if (lane == 0) plan[r].sideOff = start;
    if (!bytes) return;
    SamWriter w{lds, side, start / SAM_WIN * SAM_WIN, start, start + bytes};
    const uint32_t cls = plan[r].cls;
    const PairPlan pp = pplan[r];
    PairRead R[2];
    uint64_t q0[2];
    uint32_t nOcc[2];
    for (uint32_t m = 0; m < 2u; m++) {
        R[m] = pairRead(pc.m[m], r, pp.idLen[m]);
        q0[m] = pc.m[m].foffs[2ull * r];
        nOcc[m] = (uint32_t)(pc.m[m].foffs[2ull * r + 2u] - q0[m]);
    }
    uint64_t cur = start;
    if (cls == PAIR_CLS_ONE_UNMAPPED) {
        const uint32_t m = nOcc[0] ? 0u : 1u, n = nOcc[m];
        const SamCtx& cx = pc.m[m];
        const PairRead &Rm = R[m], &Ro = R[1u - m];
        { // the primary's record, then the record of the mate
            const PairLine L = pairHalfLine(samLoadHit(cx, q0[m] + pp.primU), m, true, pp.minDist, pp.nPairs);
            const uint32_t lineLen = pairLineLen(L, Rm);
            w.stream(cur + lineLen, [&]() { pairCoopLine(w, cur, L, Rm, lineLen); });
            cur += lineLen;
            const uint32_t flags = 1u | 4u | (L.h.strand ? 32u : 0u) | (m ? 64u : 128u);
            const uint64_t recLen = pairUnmappedLenF(Ro, flags), seqAt = cur + pairUnmappedSeqAtF(Ro, flags);
            const uint8_t *id = Ro.id, *rd = Ro.rd, *ql = Ro.ql;
            w.stream(cur + recLen, [&]() {
                w.coop(cur, Ro.idLen, [&](uint64_t i) { return id[i]; });
                w.coop(seqAt, Ro.readLen, [&](uint64_t i) { return samCleanBase(rd[i]); });
                w.coop(seqAt + Ro.readLen + 1u, Ro.qualLen, [&](uint64_t i) { return ql[i]; });
                if (lane == 0 && w.touches(cur, recLen)) {
                    SamEm e = w.cursor(cur);
                    e.skip(Ro.idLen);
                    e.ch('\t');
                    e.dec(flags);
                    e.lit("\t*\t0\t0\t*\t*\t0\t0\t");
                    e.skip(Ro.readLen);
                    e.ch('\t');
                    e.skip(Ro.qualLen);
                    e.lit("\tPG:Z:Columba\n");
                }
            });
            cur += recLen;
        }
        for (uint32_t pb = 1u; pb < n; pb += 64u) {
            const uint32_t p = pb + lane;
            PairLine L{};
            unsigned long long mine = 0;
            if (p < n) {
                L = pairHalfLine(samLoadHit(cx, q0[m] + samOccAt(p, pp.primU)), m, false, pp.minDist, pp.nPairs);
                mine = pairLineLen(L, Rm);
            }
            unsigned long long total;
            const uint64_t at = cur + waveExclusiveScan64(mine, total);
            w.stream(cur + total, [&]() {
                if (!w.touches(at, mine)) return;
                SamEm e = w.cursor(at);
                pairEmitLine<false>(e, L, Rm);
            });
            cur += total;
        }
    } else if (cls == PAIR_CLS_DISCORDANT) {
        const uint32_t n1 = nOcc[0], n2 = nOcc[1];
        { // the primary pair's records by all lanes ...
            uint32_t uMate;
            const PairCand prim = pairDiscCand(pc, q0[0] + pp.primU, q0[1] + pp.primD, uMate);
            for (uint32_t down = 0; down < 2u; down++) {
                const uint32_t me = down ? 1u - uMate : uMate;
                const PairLine L = pairLine(prim, down != 0u, me, true, pp.minDist, pp.nPairs, 0u);
                const uint32_t lineLen = pairLineLen(L, R[me]);
                w.stream(cur + lineLen, [&]() { pairCoopLine(w, cur, L, R[me], lineLen); });
                cur += lineLen;
            }
        }
        // ... the others by the lane of their occurrence of read 1, 64 of those at a time
        for (uint32_t ub = 0; ub < n1; ub += 64u) {
            const uint32_t i1 = ub + lane;
            unsigned long long mine = 0;
            if (i1 < n1)
                for (uint32_t i2 = 0; i2 < n2; i2++) mine += pairDiscSlotLen(pc, q0[0], q0[1], pp, R, i1, i2);
            unsigned long long total;
            uint64_t pos = cur + waveExclusiveScan64(mine, total); // this lane's next candidate (i1, it) and where its records begin
            uint32_t it = 0;
            bool more = mine != 0ull;
            w.stream(cur + total, [&]() {
                const uint64_t winHi = w.winLo + SAM_WIN;
                while (more && pos < winHi) {
                    if (it >= n2) {
                        more = false;
                        break;
                    }
                    uint32_t sc, su, sd;
                    uint64_t pairLen = 0;
                    if (pairSlot(pp, 0u, i1, it, sc, su, sd)) {
                        uint32_t uMate;
                        const PairCand cand = pairDiscCand(pc, q0[0] + su, q0[1] + sd, uMate);
                        const PairLine up = pairLine(cand, false, uMate, false, pp.minDist, pp.nPairs, 0u);
                        const PairLine dn = pairLine(cand, true, 1u - uMate, false, pp.minDist, pp.nPairs, 0u);
                        const uint32_t upLen = pairLineLen(up, R[uMate]);
                        pairLen = (uint64_t)upLen + pairLineLen(dn, R[1u - uMate]);
                        if (pos + pairLen > w.winLo) {
                            SamEm e = w.cursor(pos);
                            if (pos + upLen > w.winLo) pairEmitLine<false>(e, up, R[uMate]);
                            else e.skip(upLen);
                            pairEmitLine<false>(e, dn, R[1u - uMate]);
                        }
                    }
                    if (pos + pairLen > winHi) break; // (goes on in the next window)
                    pos += pairLen;
                    it++;
                }
            });
            cur += total;
        }
    } else if (cls == PAIR_CLS_UNPAIRED) {
        for (uint32_t m = 0; m < 2u; m++) {
            const SamCtx& cx = pc.m[m];
            const uint32_t n = nOcc[m];
            const PairSolo S = pairSolo(cx, q0[m], n, lane);
            uint32_t bins = 0; // the distances that occur (<= 13: a bit each)
            for (uint32_t j = lane; j < n; j += 64u) bins |= 1u << (cx.occ[q0[m] + j].z & 31u);
            for (int d = 32; d >= 1; d >>= 1) bins |= __shfl_xor(bins, d);
            for (uint32_t dist = 0; dist < 32u; dist++) {
                if (!((bins >> dist) & 1u)) continue; // (wave-uniform)
                for (uint32_t jb = 0; jb < n; jb += 64u) {
                    const uint32_t j = jb + lane;
                    SamHitDev h{};
                    unsigned long long mine = 0;
                    const bool first = j == S.primary;
                    if (j < n && cx.occ[q0[m] + j].z == dist) {
                        h = samLoadHit(cx, q0[m] + j);
                        mine = pairSoloLineLen(R[m], h, m, first, S);
                    }
                    unsigned long long total;
                    const uint64_t at = cur + waveExclusiveScan64(mine, total);
                    if (!total) continue; // (wave-uniform)
                    w.stream(cur + total, [&]() {
                        if (!w.touches(at, mine)) return;
                        SamEm e = w.cursor(at);
                        pairEmitSolo(e, R[m], h, m, first, S);
                    });
                    cur += total;
                }
            }
        }
    }
    if (w.G1 > w.winLo) {
        __syncthreads();
        w.flush();
    }
}

} // namespace cmb
