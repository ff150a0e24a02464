// SAM text of a single-end chunk in ALL mode, written on the device (cmb_batch_sam_device): the lines host_sam.hpp and samOfRead
// (sam.hip) put together on the host, byte for byte, from what a run with alignments leaves in HBM — the read
// characters, the final occurrences of every read (k_filter_write), their CIGAR runs and sequence assignment (k_cigar) — plus
// the identifiers, qualities and sequence names of the chunk, packed.
//
// Mirrors (reference, src/), through host_sam.hpp:
//   Read::cleanUpRecord / ReadBundle            reads.h:43-58, :97-160
//   TextOcc::getFlagsSE / getMapQ / asXA         indexhelpers.h:321-331, :378-388, :416-421
//   TextOcc::generateSAMSingleEnd / ...XA        indexhelpers.cpp:56-120
//   TextOcc::createUnmappedSAMOccurrenceSE       indexhelpers.cpp:177-200
//   SearchStrategy::generateOutputSingleEnd      searchstrategy.cpp:1824-1902
//
//   shared by the two plan kernels: samIdLen (the cleaned identifier's length), samMappedLen (the bytes of a mapped read's records),
//   samUnmappedLen / samUnmappedSeqAt (the record of a read without an occurrence; the latter also places SEQ in k_sam_write)
//   k_sam_plan      a wavefront per read, lane-strided over its occurrences: the primary (first occurrence of minimal distance),
//                   minScore, nHits, whether an occurrence runs over the end of its sequence (that read is formatted on the host:
//                   findSeqName trims and verifies again, and may drop the occurrence), the exact byte length of the read's records
//   (rocPRIM)       exclusive 64-bit scan of the lengths: the position of every read in the text
//   k_sam_plan_best the same plan for the final lists of BEST mode: primary, minScore and nHits come from the strata bookkeeping,
//                   the host-formatted reads from a flag per read
//   k_sam_override  the lengths of the host-formatted reads, before the scan
//   k_sam_keep_*    the lists of a part without the occurrences its run dropped (cmb_batch_trim_on_device), before the plan
//   k_sam_write     a wavefront per SAM_READS_PER_WAVE consecutive reads, i.e. per contiguous piece of the text.  The piece is
//                   cut into windows of SAM_WIN bytes aligned in the TEXT; a window is assembled in LDS and stored with 16-byte
//                   words, single bytes only in the first and last word of the piece, which the wavefront shares with its
//                   neighbours.  SEQ, QUAL, identifier and name of a primary line are copied by all lanes; its numbers and
//                   literals by lane 0; secondary lines and XA entries by a lane each, 64 at a time, placed by a wave scan.  What
//                   does not fit the window is emitted again, clipped, after the window went out — so a line (an XA line of a
//                   repeat: tens of kilobytes) may be any number of windows long.
#pragma once
#include "host_util.hpp" // (SamPlan, SamDeviceBufs, AlnRec)

namespace cmb {

constexpr uint32_t SAM_WIN = 8192;           // bytes of text a wavefront assembles in LDS before it stores them
constexpr uint32_t SAM_READS_PER_WAVE = 16;  // consecutive reads per wavefront of k_sam_write
constexpr uint32_t SAM_NOTHING = 0, SAM_UNMAPPED = 1, SAM_MAPPED = 2, SAM_HOST = 3;

struct SamCtx {
    const uint8_t* reads; // raw read characters of the sub-batch
    const uint64_t* offs;
    const uint64_t* foffs; // first occurrence of every filter group
    uint32_t groupStride;  // groups per read (2: every strand filtered by itself)
    const uint4* occ;      // {begin, end, distance, strand}
    const AlnRec* aln;
    const uint16_t* ops; // CIGAR runs, stored end to begin
    uint32_t stride;
    const uint8_t* ids; // the sub-batch's slice of the packed inputs: byte idOffs[i] - idBase
    const uint64_t* idOffs;
    uint64_t idBase;
    const uint8_t* quals; // nullptr: every quality prints as "*"
    const uint64_t* qualOffs;
    uint64_t qualBase;
    const uint8_t* names;
    const uint64_t* nameOffs;
    uint32_t nSeqs, nReads, unmapped, xa;
};

// MAPQ = round(-10 log10(1 - 1 / nHits)) for an occurrence of minimal distance, 60 for a single one (indexhelpers.h:378-388):
// evaluated in double precision that is 3, 2, then 1 up to nine and 0 from ten occurrences on
__device__ __forceinline__ uint32_t samMapQ(uint32_t nHits) {
    constexpr uint8_t T[10] = {0, 60, 3, 2, 1, 1, 1, 1, 1, 1};
    return nHits < 10u ? T[nHits] : 0u;
}
__device__ __forceinline__ uint32_t decWidth(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
         : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ uint8_t samCleanBase(uint8_t c) { // reads.h:54-58
    if (c >= 'a' && c <= 'z') c -= 32;
    return c == 'A' || c == 'C' || c == 'G' || c == 'T' ? c : (uint8_t)'N';
}
__device__ __forceinline__ uint8_t samComplement(uint8_t c) { // nucleotide.h:250 (of a cleaned character)
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
}

// one occurrence as a SAM line sees it
struct SamHitDev {
    uint32_t pos1, dist, strand, nOps, nameLen, cigLen, spans;
    const uint16_t* ops;
    const uint8_t* name;
};
__device__ __forceinline__ SamHitDev samLoadHit(const SamCtx& cx, uint64_t q) {
    const uint4 o = cx.occ[q];
    const AlnRec a = cx.aln[q];
    SamHitDev h;
    h.pos1 = a.seqBegin + 1u; // SAM is 1-based
    h.dist = o.z;
    h.strand = o.w;
    h.spans = a.spans;
    h.nOps = a.nOps < cx.stride ? a.nOps : cx.stride;
    h.ops = cx.ops + q * cx.stride;
    h.cigLen = 0;
    for (uint32_t j = 0; j < h.nOps; j++) h.cigLen += decWidth((uint32_t)h.ops[j] >> 2) + 1u;
    h.nameLen = 0;
    h.name = cx.names;
    if (a.seqId < cx.nSeqs) {
        h.name = cx.names + cx.nameOffs[a.seqId];
        h.nameLen = (uint32_t)(cx.nameOffs[a.seqId + 1] - cx.nameOffs[a.seqId]);
    }
    return h;
}
// bytes of samLineSE (indexhelpers.cpp:56-91) up to the end of the CIGAR's trailing "\t*\t0\t0\t": where SEQ begins
__device__ __forceinline__ uint32_t samSeqOffset(uint32_t idLen, const SamHitDev& h, uint32_t flags, uint32_t mapq) {
    return idLen + 1u + decWidth(flags) + 1u + h.nameLen + 1u + decWidth(h.pos1) + 1u + decWidth(mapq) + 1u + h.cigLen + 7u;
}
__device__ __forceinline__ uint32_t samLineLen(uint32_t idLen, const SamHitDev& h, uint32_t flags, uint32_t mapq, uint32_t seqLen,
                                               uint32_t qualLen) {
    return samSeqOffset(idLen, h, flags, mapq) + seqLen + 1u + qualLen + 6u + decWidth(h.dist) + 6u + decWidth(h.dist) + 14u;
}
__device__ __forceinline__ uint32_t samXaEntryLen(const SamHitDev& h) { // "name,+pos,cigar,distance;" (indexhelpers.h:416-421)
    return h.nameLen + 2u + decWidth(h.pos1) + 1u + h.cigLen + 1u + decWidth(h.dist) + 1u;
}
// the occurrence printed at position p of a read's records: the primary swapped with the first one (searchstrategy.cpp:1883-1899)
__device__ __forceinline__ uint32_t samOccAt(uint32_t p, uint32_t primary) { return p == 0u ? primary : p == primary ? 0u : p; }

__device__ __forceinline__ uint32_t samQualLen(const SamCtx& cx, uint32_t r) {
    return cx.quals ? (uint32_t)(cx.qualOffs[r + 1] - cx.qualOffs[r]) : 1u;
}

// the record of a read without an occurrence (indexhelpers.cpp:177-200): "id \t4\t*\t0\t0\t*\t*\t0\t0\t SEQ \t QUAL \tPG:Z:Columba\n"
// (samUnmappedSeqAt: where SEQ begins in a record that begins at `start`)
__device__ __forceinline__ uint64_t samUnmappedSeqAt(uint64_t start, uint32_t idLen) { return start + idLen + 17u; }
__device__ __forceinline__ uint64_t samUnmappedLen(uint32_t idLen, uint32_t readLen, uint32_t qualLen) {
    return samUnmappedSeqAt(0, idLen) + readLen + 1u + qualLen + 14u;
}
// length of read r's cleaned identifier (reads.h:43-52): cut at the first space, without the first character.  A whole wavefront.
__device__ __forceinline__ uint32_t samIdLen(const SamCtx& cx, uint32_t r, uint32_t lane) {
    const uint8_t* id = cx.ids + (cx.idOffs[r] - cx.idBase);
    const uint32_t idRaw = (uint32_t)(cx.idOffs[r + 1] - cx.idOffs[r]);
    uint32_t sp = idRaw;
    for (uint32_t base = 0; base < idRaw; base += 64u) {
        const uint32_t i = base + lane;
        const unsigned long long m = __ballot(i < idRaw && id[i] == ' ');
        if (m) {
            sp = base + (uint32_t)__builtin_ctzll(m);
            break;
        }
    }
    return sp ? sp - 1u : 0u;
}
// bytes of the records of a mapped read whose plan (primary, minScore, nHits, idLen) is pl and whose n occurrences begin at q0: the
// primary's line with SEQ and QUAL, then a secondary line or an XA entry each.  A whole wavefront, lane-strided over the occurrences.
__device__ __forceinline__ uint64_t samMappedLen(const SamCtx& cx, const SamPlan& pl, uint64_t q0, uint32_t n, uint32_t readLen, uint32_t qualLen,
                                                 uint32_t lane) {
    const uint32_t mapq = samMapQ(pl.nHits);
    const bool star = !cx.quals || (cx.xa && qualLen == 0u); // (host_sam.hpp:96: an empty quality prints as "*" beside an XA tag)
    unsigned long long sum = 0;
    for (uint32_t p = lane; p < n; p += 64u) {
        const SamHitDev h = samLoadHit(cx, q0 + samOccAt(p, pl.primary));
        if (p == 0u) {
            sum += samLineLen(pl.idLen, h, h.strand ? 16u : 0u, mapq, readLen, star ? 1u : qualLen);
            if (cx.xa) sum += 6u + decWidth(pl.nHits - 1u) + 6u + decWidth(n - pl.nHits) + 6u; // X0, X1, XA:Z: (the newline moves to the end)
        } else if (cx.xa) {
            sum += samXaEntryLen(h);
        } else {
            sum += samLineLen(pl.idLen, h, h.strand ? 272u : 256u, h.dist == pl.minScore ? mapq : 0u, 1u, 1u);
        }
    }
    return waveSum64(sum);
}

__global__ void __launch_bounds__(256)
k_sam_plan(SamCtx cx, SamPlan* __restrict__ plan, uint64_t* __restrict__ len, uint32_t* __restrict__ hostList /* [0]: how many */) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= cx.nReads) return; // (a whole wavefront)
    SamPlan pl{};
    pl.idLen = samIdLen(cx, r, lane);
    const uint32_t readLen = (uint32_t)(cx.offs[r + 1] - cx.offs[r]);
    const uint32_t qualLen = samQualLen(cx, r);
    const uint64_t q0 = cx.foffs[(uint64_t)r * cx.groupStride], q1 = cx.foffs[(uint64_t)(r + 1) * cx.groupStride];
    const uint32_t n = (uint32_t)(q1 - q0);
    uint64_t total = 0;
    if (n == 0) {
        pl.kind = cx.unmapped ? SAM_UNMAPPED : SAM_NOTHING;
        if (cx.unmapped) total = samUnmappedLen(pl.idLen, readLen, qualLen);
    } else {
        unsigned long long best = ~0ull;
        uint32_t over = 0;
        for (uint32_t j = lane; j < n; j += 64u) {
            const unsigned long long key = ((unsigned long long)cx.occ[q0 + j].z << 32) | j;
            best = key < best ? key : best;
            over |= cx.aln[q0 + j].spans == 1u ? 1u : 0u;
        }
        best = waveMin64(best);
        pl.primary = (uint32_t)best;
        pl.minScore = (uint32_t)(best >> 32);
        if (__ballot(over != 0u)) {
            pl.kind = SAM_HOST; // (its length comes from the host: k_sam_override)
            if (lane == 0) hostList[1u + atomicAdd(hostList, 1u)] = r;
        } else {
            pl.kind = SAM_MAPPED;
            uint32_t cnt = 0;
            for (uint32_t j = lane; j < n; j += 64u) cnt += cx.occ[q0 + j].z == pl.minScore ? 1u : 0u;
            pl.nHits = (uint32_t)waveSum64(cnt);
            total = samMappedLen(cx, pl, q0, n, readLen, qualLen, lane);
        }
    }
    if (lane == 0) {
        plan[r] = pl;
        len[r] = total;
    }
}

// The plan of a chunk matched in BEST mode (cmb_best_sam_device; generateSE_SAM / generateSE_SAM_XATag as matchApproxBestPlusX calls
// them, searchstrategy.h:1612-1641): the lists are final and in the reference's order, so the primary is the first record and nothing
// is swapped; minScore is the read's best distance and nHits the number of occurrences at it BEFORE the deduplication (both from the
// strata bookkeeping, so X1 = n - nHits may wrap as it does on the host).  hostFlag: the reads the host formats (k_sam_override).
__global__ void __launch_bounds__(256)
k_sam_plan_best(SamCtx cx, const uint32_t* __restrict__ best, const uint32_t* __restrict__ hits, const uint8_t* __restrict__ hostFlag,
                SamPlan* __restrict__ plan, uint64_t* __restrict__ len) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= cx.nReads) return; // (a whole wavefront)
    SamPlan pl{};
    pl.idLen = samIdLen(cx, r, lane);
    const uint32_t readLen = (uint32_t)(cx.offs[r + 1] - cx.offs[r]);
    const uint32_t qualLen = samQualLen(cx, r);
    const uint64_t q0 = cx.foffs[(uint64_t)r * cx.groupStride], q1 = cx.foffs[(uint64_t)(r + 1) * cx.groupStride];
    const uint32_t n = (uint32_t)(q1 - q0);
    uint64_t total = 0;
    if (hostFlag[r]) {
        pl.kind = SAM_HOST; // (its length comes from the host: k_sam_override)
    } else if (n == 0) {
        pl.kind = cx.unmapped ? SAM_UNMAPPED : SAM_NOTHING;
        if (cx.unmapped) total = samUnmappedLen(pl.idLen, readLen, qualLen);
    } else {
        pl.kind = SAM_MAPPED;
        pl.primary = 0; // (samOccAt(p, 0) == p)
        pl.minScore = best[r];
        pl.nHits = hits[r];
        total = samMappedLen(cx, pl, q0, n, readLen, qualLen, lane);
    }
    if (lane == 0) {
        plan[r] = pl;
        len[r] = total;
    }
}

// Lists with occurrences the run dropped (AlnRec::spans == 4: over the end of their sequence and not found again on the trimmed window,
// cmb_batch_trim_on_device) are copied without those before the plan: no record is written for a dropped occurrence, it is no candidate
// for the primary and counts in no tag, so the plan and write kernels see the lists findSeqName leaves on the host.
//   k_sam_keep_flags  a lane per occurrence: 1 if it stays (one more element, 0, closes the scan)
//   (rocPRIM)         exclusive scan: the new index of every occurrence
//   k_sam_keep_copy   a lane per occurrence that stays: record, sequence assignment and CIGAR runs to their new index
//   k_sam_keep_offs   a lane per group boundary: the new first occurrence of every filter group
// All three are launched under the grid cap (host_grid.hpp) and loop.  The copy costs one more pass over the lists (32 bytes + the CIGAR
// runs per occurrence) and a second set of list buffers per part; only parts that dropped something pay it.
__global__ void k_sam_keep_flags(const AlnRec* __restrict__ aln, uint64_t n, uint32_t* __restrict__ keep) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += step) keep[i] = i < n && aln[i].spans != 4u ? 1u : 0u;
}
__global__ void k_sam_keep_copy(const uint4* __restrict__ occ, const AlnRec* __restrict__ aln, const uint16_t* __restrict__ ops, uint32_t stride,
                                uint64_t n, const uint64_t* __restrict__ pos, uint4* __restrict__ occOut, AlnRec* __restrict__ alnOut,
                                uint16_t* __restrict__ opsOut) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        if (pos[i + 1] == pos[i]) continue;
        const uint64_t d = pos[i];
        const AlnRec a = aln[i];
        occOut[d] = occ[i];
        alnOut[d] = a;
        const uint32_t m = a.nOps < stride ? a.nOps : stride;
        for (uint32_t j = 0; j < m; j++) opsOut[d * stride + j] = ops[i * stride + j];
    }
}
__global__ void k_sam_keep_offs(const uint64_t* __restrict__ goffs, uint64_t nGroups, const uint64_t* __restrict__ pos, uint64_t* __restrict__ out) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= nGroups; g += step) out[g] = pos[goffs[g]];
}

// the reads the host formatted (samOfRead): their lengths, and where their text lies in the side buffer
__global__ void k_sam_override(const uint32_t* __restrict__ reads, const uint64_t* __restrict__ sideOffs, uint32_t n, SamPlan* __restrict__ plan,
                               uint64_t* __restrict__ len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    plan[reads[i]].sideOff = sideOffs[i];
    len[reads[i]] = sideOffs[i + 1] - sideOffs[i];
}

// a lane's cursor into the window: bytes outside it are dropped (they were, or will be, emitted with another window)
struct SamEm {
    uint8_t* lds;
    int32_t rel; // position of the next byte relative to the window's first
    __device__ __forceinline__ void ch(uint8_t c) {
        if ((uint32_t)rel < SAM_WIN) lds[rel] = c;
        rel++;
    }
    __device__ __forceinline__ void skip(uint32_t n) { rel += (int32_t)n; }
    __device__ __forceinline__ void dec(uint32_t v) {
        const uint32_t w = decWidth(v);
        for (uint32_t i = w; i-- > 0u;) {
            const uint32_t at = (uint32_t)rel + i;
            if (at < SAM_WIN) lds[at] = (uint8_t)('0' + v % 10u);
            v /= 10u;
        }
        rel += (int32_t)w;
    }
    template <size_t N> __device__ __forceinline__ void lit(const char (&s)[N]) {
#pragma unroll
        for (size_t i = 0; i + 1 < N; i++) ch((uint8_t)s[i]);
    }
    __device__ __forceinline__ void bytes(const uint8_t* src, uint32_t n) {
        for (uint32_t i = 0; i < n; i++) ch(src[i]);
    }
    __device__ __forceinline__ void cigar(const SamHitDev& h) { // host_sam.hpp: cigarString (the runs are stored end to begin)
        for (uint32_t j = h.nOps; j-- > 0u;) {
            const uint32_t op = h.ops[j];
            dec(op >> 2);
            const uint32_t c = op & 3u;
            ch(c == 0u ? 'M' : c == 1u ? 'I' : c == 2u ? 'D' : '?');
        }
    }
};

// the wavefront's piece of the text, [G0, G1), and the window of it that is being assembled: text bytes [winLo, winLo + SAM_WIN),
// winLo a multiple of SAM_WIN.  All members are wave-uniform.
struct SamWriter {
    uint8_t* lds;
    uint8_t* out;
    uint64_t winLo, G0, G1;
    // is [start, start + len) in the window?  -> a cursor at its first byte (which may lie before the window)
    __device__ __forceinline__ bool touches(uint64_t start, uint64_t len) const { return len && start < winLo + SAM_WIN && start + len > winLo; }
    __device__ __forceinline__ SamEm cursor(uint64_t start) const { return SamEm{lds, (int32_t)(int64_t)(start - winLo)}; }
    // all lanes: bytes [start, start + len) = f(0 ...), the part inside the window
    template <class F> __device__ __forceinline__ void coop(uint64_t start, uint64_t len, F f) const {
        const uint64_t lo = start > winLo ? start : winLo;
        const uint64_t hi = start + len < winLo + SAM_WIN ? start + len : winLo + SAM_WIN;
        if (lo >= hi) return;
        const uint64_t i0 = lo - start;
        const uint32_t d0 = (uint32_t)(lo - winLo), n = (uint32_t)(hi - lo);
        for (uint32_t i = threadIdx.x & 63u; i < n; i += 64u) lds[d0 + i] = f(i0 + i);
    }
    // store the window's bytes of the piece: whole 16-byte words, single bytes where a word is shared with a neighbouring piece
    __device__ __forceinline__ void flush() const {
        const uint64_t lo = winLo > G0 ? winLo : G0, hi = winLo + SAM_WIN < G1 ? winLo + SAM_WIN : G1;
        if (lo >= hi) return;
        const uint32_t a = (uint32_t)(lo - winLo), b = (uint32_t)(hi - winLo), lane = threadIdx.x & 63u;
        const uint32_t wa = (a + 15u) & ~15u, wb = b & ~15u;
        uint8_t* dst = out + winLo;
        if (wa >= wb) { // (no whole word)
            for (uint32_t i = a + lane; i < b; i += 64u) dst[i] = lds[i];
            return;
        }
        for (uint32_t i = a + lane; i < wa; i += 64u) dst[i] = lds[i];
        for (uint32_t i = wa / 16u + lane; i < wb / 16u; i += 64u) ((uint4*)dst)[i] = ((const uint4*)lds)[i];
        for (uint32_t i = wb + lane; i < b; i += 64u) dst[i] = lds[i];
    }
    // emit() writes what it has of [.., end) into the window; windows that fill up on the way go out, and emit() runs again
    template <class F> __device__ __forceinline__ void stream(uint64_t end, F emit) {
        for (;;) {
            emit();
            if (end < winLo + SAM_WIN) break;
            __syncthreads(); // (a block is one wavefront: this orders its LDS traffic, nothing waits)
            flush();
            __syncthreads();
            winLo += SAM_WIN;
            if (end <= winLo) break;
        }
    }
};

// what k_sam_write needs of one read before it touches its bytes; loaded by a lane per read of the piece, so that the piece pays ONE
// chain of dependent loads (positions -> plan -> occurrence -> CIGAR runs and name) instead of one per read
struct SamRec {
    uint64_t start, bytes, idOff, rdOff, qlOff, q0, sideOff, nameOff;
    uint32_t kind, primary, minScore, nHits, idLen, readLen, qualLen, n;
    uint32_t pos1, dist, strand, nOps, nameLen, cigLen; // the primary occurrence
};
__device__ __forceinline__ uint32_t samUniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t samUniform(uint64_t v) {
    return ((uint64_t)samUniform((uint32_t)(v >> 32)) << 32) | samUniform((uint32_t)v);
}

__global__ void __launch_bounds__(64)
k_sam_write(SamCtx cx, const SamPlan* __restrict__ plan, const uint64_t* __restrict__ outOffs, const uint8_t* __restrict__ side,
            uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[SAM_WIN];
    __shared__ SamRec recs[SAM_READS_PER_WAVE];
    const uint32_t lane = threadIdx.x;
    const uint64_t rr = (uint64_t)blockIdx.x * SAM_READS_PER_WAVE;
    if (rr >= cx.nReads) return;
    const uint32_t r0 = (uint32_t)rr, r1 = cx.nReads - r0 < SAM_READS_PER_WAVE ? cx.nReads : r0 + SAM_READS_PER_WAVE;
    SamWriter w{lds, out, 0, outOffs[r0], outOffs[r1]};
    if (w.G0 == w.G1) return;
    w.winLo = w.G0 / SAM_WIN * SAM_WIN;
    if (lane < r1 - r0) {
        const uint32_t r = r0 + lane;
        SamRec c{};
        c.start = outOffs[r];
        c.bytes = outOffs[r + 1] - c.start;
        const SamPlan pl = plan[r];
        c.kind = pl.kind, c.primary = pl.primary, c.minScore = pl.minScore, c.nHits = pl.nHits, c.idLen = pl.idLen, c.sideOff = pl.sideOff;
        c.idOff = cx.idOffs[r] - cx.idBase + 1u;
        c.rdOff = cx.offs[r];
        c.readLen = (uint32_t)(cx.offs[r + 1] - c.rdOff);
        c.qlOff = cx.quals ? cx.qualOffs[r] - cx.qualBase : 0u;
        c.qualLen = samQualLen(cx, r);
        c.q0 = cx.foffs[(uint64_t)r * cx.groupStride];
        c.n = (uint32_t)(cx.foffs[(uint64_t)(r + 1) * cx.groupStride] - c.q0);
        if (c.kind == SAM_MAPPED && c.bytes) {
            const SamHitDev h = samLoadHit(cx, c.q0 + c.primary);
            c.pos1 = h.pos1, c.dist = h.dist, c.strand = h.strand, c.nOps = h.nOps, c.nameLen = h.nameLen, c.cigLen = h.cigLen;
            c.nameOff = (uint64_t)(h.name - cx.names);
        }
        recs[lane] = c;
    }
    __syncthreads();
    for (uint32_t r = r0; r < r1; r++) {
        const SamRec& rc = recs[r - r0];
        const uint64_t start = samUniform(rc.start), bytes = samUniform(rc.bytes);
        if (!bytes) continue;
        const uint32_t kind = samUniform(rc.kind);
        if (kind == SAM_HOST) {
            const uint8_t* src = side + samUniform(rc.sideOff);
            w.stream(start + bytes, [&]() { w.coop(start, bytes, [&](uint64_t i) { return src[i]; }); });
            continue;
        }
        const uint32_t idLen = samUniform(rc.idLen), readLen = samUniform(rc.readLen);
        const uint8_t* id = cx.ids + samUniform(rc.idOff);
        const uint8_t* rd = cx.reads + samUniform(rc.rdOff);
        const uint8_t* ql = cx.quals ? cx.quals + samUniform(rc.qlOff) : nullptr;
        uint32_t qualLen = samUniform(rc.qualLen);
        if (kind == SAM_UNMAPPED) {
            const uint64_t seqAt = samUnmappedSeqAt(start, idLen);
            w.stream(start + bytes, [&]() {
                w.coop(start, idLen, [&](uint64_t i) { return id[i]; });
                w.coop(seqAt, readLen, [&](uint64_t i) { return samCleanBase(rd[i]); });
                w.coop(seqAt + readLen + 1u, qualLen, [&](uint64_t i) { return ql ? ql[i] : (uint8_t)'*'; });
                if (lane == 0 && w.touches(start, bytes)) {
                    SamEm e = w.cursor(start);
                    e.skip(idLen);
                    e.lit("\t4\t*\t0\t0\t*\t*\t0\t0\t");
                    e.skip(readLen);
                    e.ch('\t');
                    e.skip(qualLen);
                    e.lit("\tPG:Z:Columba\n");
                }
            });
            continue;
        }
        // SAM_MAPPED: the primary's line by all lanes ...
        const uint64_t q0 = samUniform(rc.q0);
        const uint32_t n = samUniform(rc.n), primary = samUniform(rc.primary), minScore = samUniform(rc.minScore), nHits = samUniform(rc.nHits);
        const uint32_t mapq = samMapQ(nHits);
        const bool star = !ql || (cx.xa && qualLen == 0u);
        if (star) qualLen = 1u;
        uint64_t cur = start;
        {
            SamHitDev h;
            h.pos1 = samUniform(rc.pos1), h.dist = samUniform(rc.dist), h.strand = samUniform(rc.strand), h.nOps = samUniform(rc.nOps);
            h.nameLen = samUniform(rc.nameLen), h.cigLen = samUniform(rc.cigLen), h.spans = 0;
            h.name = cx.names + samUniform(rc.nameOff);
            h.ops = cx.ops + (q0 + primary) * cx.stride;
            const uint32_t flags = h.strand ? 16u : 0u;
            const uint32_t nameAt = idLen + 1u + decWidth(flags) + 1u, seqAt = samSeqOffset(idLen, h, flags, mapq);
            uint32_t lineLen = samLineLen(idLen, h, flags, mapq, readLen, qualLen);
            const uint32_t x0 = nHits - 1u, x1 = n - nHits;
            if (cx.xa) lineLen += 6u + decWidth(x0) + 6u + decWidth(x1) + 6u - (n > 1u ? 1u : 0u); // (the newline follows the last XA entry)
            w.stream(cur + lineLen, [&]() {
                w.coop(cur, idLen, [&](uint64_t i) { return id[i]; });
                w.coop(cur + nameAt, h.nameLen, [&](uint64_t i) { return h.name[i]; });
                w.coop(cur + seqAt, readLen, [&](uint64_t i) {
                    return h.strand ? samComplement(samCleanBase(rd[readLen - 1u - (uint32_t)i])) : samCleanBase(rd[i]);
                });
                w.coop(cur + seqAt + readLen + 1u, qualLen, [&](uint64_t i) {
                    return star ? (uint8_t)'*' : h.strand ? ql[qualLen - 1u - (uint32_t)i] : ql[i];
                });
                if (lane == 0 && w.touches(cur, lineLen)) {
                    SamEm e = w.cursor(cur);
                    e.skip(idLen);
                    e.ch('\t');
                    e.dec(flags);
                    e.ch('\t');
                    e.skip(h.nameLen);
                    e.ch('\t');
                    e.dec(h.pos1);
                    e.ch('\t');
                    e.dec(mapq);
                    e.ch('\t');
                    e.cigar(h);
                    e.lit("\t*\t0\t0\t");
                    e.skip(readLen);
                    e.ch('\t');
                    e.skip(qualLen);
                    e.lit("\tAS:i:");
                    e.dec(h.dist);
                    e.lit("\tNM:i:");
                    e.dec(h.dist);
                    e.lit("\tPG:Z:Columba");
                    if (cx.xa) {
                        e.lit("\tX0:i:");
                        e.dec(x0);
                        e.lit("\tX1:i:");
                        e.dec(x1);
                        e.lit("\tXA:Z:");
                    }
                    if (!cx.xa || n == 1u) e.ch('\n');
                }
            });
            cur += lineLen;
        }
        // ... the others a lane each, 64 at a time: secondary lines, or the entries of the XA tag
        for (uint32_t pb = 1u; pb < n; pb += 64u) {
            const uint32_t p = pb + lane;
            SamHitDev h{};
            uint32_t mine = 0, flags = 0, mq = 0;
            if (p < n) {
                h = samLoadHit(cx, q0 + samOccAt(p, primary));
                flags = h.strand ? 272u : 256u;
                mq = h.dist == minScore ? mapq : 0u;
                mine = cx.xa ? samXaEntryLen(h) + (p == n - 1u ? 1u : 0u) : samLineLen(idLen, h, flags, mq, 1u, 1u);
            }
            uint32_t total;
            const uint64_t at = cur + waveExclusiveScan(mine, total);
            w.stream(cur + total, [&]() {
                if (!w.touches(at, mine)) return;
                SamEm e = w.cursor(at);
                if (cx.xa) {
                    e.bytes(h.name, h.nameLen);
                    e.ch(',');
                    e.ch(h.strand ? '-' : '+');
                    e.dec(h.pos1);
                    e.ch(',');
                    e.cigar(h);
                    e.ch(',');
                    e.dec(h.dist);
                    e.ch(';');
                    if (p == n - 1u) e.ch('\n');
                } else {
                    e.bytes(id, idLen);
                    e.ch('\t');
                    e.dec(flags);
                    e.ch('\t');
                    e.bytes(h.name, h.nameLen);
                    e.ch('\t');
                    e.dec(h.pos1);
                    e.ch('\t');
                    e.dec(mq);
                    e.ch('\t');
                    e.cigar(h);
                    e.lit("\t*\t0\t0\t*\t*\tAS:i:");
                    e.dec(h.dist);
                    e.lit("\tNM:i:");
                    e.dec(h.dist);
                    e.lit("\tPG:Z:Columba\n");
                }
            });
            cur += total;
        }
    }
    if (w.G1 > w.winLo) {
        __syncthreads();
        w.flush();
    }
}

// test hook: the MAPQ k_sam_plan / k_sam_write print for 1 ... n occurrences of minimal distance
__global__ void k_sam_mapq(uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = samMapQ(i + 1u);
}

} // namespace cmb
