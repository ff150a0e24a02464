// BEST (+x strata) mode with the per-occurrence bookkeeping on the device (cmb_match_best_device): what matchBestWith (best.hip)
// does with host containers — processSeq's "keep what lies at or above the first distance not processed yet", the vectors per strand and
// distance, combineOccVectors' sort / unique / copy (reference src/searchstrategy.cpp:573-620, :791-812) — on the arrays a stratum batch
// leaves in HBM (foffs, two filter groups per read; fout; alnRec; alnOps at alnStride).
//
//   k_best_scan     after a stratum batch, a wavefront per read, lane-strided over its occurrences: which distances have an occurrence,
//                   which an occurrence inside one sequence (per strand, 14 bits each), whether a kept occurrence runs over a sequence
//                   end, and how many are kept
//   (rocPRIM)       exclusive scan of the exact counts: where every read's records go in the pool, which therefore never overflows
//   k_best_append   the kept records (occurrence, AlnRec, CIGAR runs at BEST_OPS_STRIDE, read) into the pool, in their order
//   k_best_collect  / k_best_gather: the pool records of the reads whose bookkeeping moved to the host (a spanning occurrence under edit
//                   distance is trimmed and verified again: it changes distance)
//   k_best_flag     at the end, a lane per pool record: is it one of its read's records at best ... min(best + x, cut-off)?  (+ nHits)
//   k_best_keys     the selected records as sort keys (read, distance, strand | sequence, begin | pool position); rocprim::merge_sort
//   k_best_uniq     a record that equals its predecessor in (read, distance, strand, sequence, begin) is dropped; records per read
//   k_best_emit     the final lists, every read's records at its offset
#pragma once
#include "host_util.hpp" // (AlnRec, BEST_OPS_STRIDE)

#include <rocprim/device/device_merge_sort.hpp>

namespace cmb {

// per read of a stratum (k_best_scan): bits 0-13 / 14-27 "an occurrence at distance d" of the forward / reverse strand, 28-41 / 42-55
// "an occurrence at distance d that lies inside one sequence", bit 56 "a kept occurrence runs over the end of its sequence"
constexpr uint32_t BEST_ANY0 = 0, BEST_ANY1 = 14, BEST_ASG0 = 28, BEST_ASG1 = 42, BEST_SPAN = 56;

struct BestPool {
    uint4* occ;
    AlnRec* aln;
    uint16_t* ops; // BEST_OPS_STRIDE per record, end to begin as k_cigar stores them
    uint32_t* read;
};

__device__ __forceinline__ unsigned long long waveOr64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d);
    return v;
}

// minD[r]: the first distance of read r that no stratum has processed yet (processSeq, searchstrategy.cpp:791-812)
__global__ void __launch_bounds__(256)
k_best_scan(const uint64_t* __restrict__ foffs, const uint4* __restrict__ fout, const AlnRec* __restrict__ aln, uint32_t nReads,
            const uint8_t* __restrict__ minD, unsigned long long* __restrict__ masks, uint64_t* __restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nReads) return; // (a whole wavefront)
    const uint64_t q0 = foffs[2ull * r], q1 = foffs[2ull * r + 2u];
    const uint32_t lo = minD[r];
    unsigned long long m = 0;
    uint32_t kept = 0;
    for (uint64_t q = q0 + lane; q < q1; q += 64u) {
        const uint4 o = fout[q];
        if (o.z < lo || o.z > 13u) continue;
        const uint32_t sp = aln[q].spans;
        kept++;
        m |= 1ull << ((o.w ? BEST_ANY1 : BEST_ANY0) + o.z);
        if (sp == 0u) m |= 1ull << ((o.w ? BEST_ASG1 : BEST_ASG0) + o.z);
        if (sp == 1u) m |= 1ull << BEST_SPAN;
    }
    m = waveOr64(m);
    const uint64_t n = waveSum64(kept);
    if (lane == 0) {
        masks[r] = m;
        cnt[r] = n;
    }
}

// ids[r]: the read's number in the chunk; poff[r]: its first record in the pool
__global__ void __launch_bounds__(256)
k_best_append(const uint64_t* __restrict__ foffs, const uint4* __restrict__ fout, const AlnRec* __restrict__ aln,
              const uint16_t* __restrict__ ops, uint32_t stride, uint32_t nReads, const uint8_t* __restrict__ minD,
              const uint32_t* __restrict__ ids, const uint64_t* __restrict__ poff, BestPool pool) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nReads) return;
    const uint64_t q0 = foffs[2ull * r], q1 = foffs[2ull * r + 2u];
    const uint32_t lo = minD[r], id = ids[r];
    const uint32_t nCopy = stride < BEST_OPS_STRIDE ? stride : BEST_OPS_STRIDE;
    uint64_t at = poff[r];
    for (uint64_t qb = q0; qb < q1; qb += 64u) {
        const uint64_t q = qb + lane;
        uint4 o{};
        bool keep = false;
        if (q < q1) {
            o = fout[q];
            keep = o.z >= lo && o.z <= 13u;
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const uint64_t dst = at + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
            pool.occ[dst] = o;
            pool.aln[dst] = aln[q];
            pool.read[dst] = id;
            const uint16_t* src = ops + q * stride;
            uint16_t* d = pool.ops + dst * BEST_OPS_STRIDE;
            for (uint32_t j = 0; j < nCopy; j++) d[j] = src[j];
        }
        at += (uint64_t)__popcll(bal);
    }
}

// the pool records the host takes over: all records of a read with mode 2 (it became a host read in this stratum), those from
// `base` on (this stratum's) of a read with mode 1 (it was one before)
__global__ void k_best_collect(const uint32_t* __restrict__ read, uint64_t from, uint64_t n, uint64_t base, const uint8_t* __restrict__ mode,
                               uint32_t* __restrict__ list /* [0]: how many */) {
    const uint64_t i = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = mode[read[i]];
    if (m == 2u || (m == 1u && i >= base)) list[1u + atomicAdd(list, 1u)] = (uint32_t)i;
}
__global__ void k_best_gather(const uint32_t* __restrict__ list, uint32_t n, BestPool pool, BestPool out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t q = list[i];
    out.occ[i] = pool.occ[q];
    out.aln[i] = pool.aln[q];
    out.read[i] = pool.read[q];
    for (uint32_t j = 0; j < BEST_OPS_STRIDE; j++) out.ops[(uint64_t)i * BEST_OPS_STRIDE + j] = pool.ops[q * BEST_OPS_STRIDE + j];
}

// what the end needs of a read: bits 0-7 best, 8-15 the last distance that is reported, 16 "its lists come from the pool" (a best
// distance was found and the bookkeeping stayed on the device), 32-45 / 46-59 the distances checkAlignments went through per strand
// (an occurrence over a sequence end does not survive that check: searchstrategy.cpp:536-571)
__device__ __forceinline__ bool bestSelected(unsigned long long st, const uint4& o, uint32_t spans) {
    if (!((st >> 16) & 1ull)) return false;
    const uint32_t best = (uint32_t)(st & 255u), hi = (uint32_t)((st >> 8) & 255u);
    if (o.z < best || o.z > hi) return false;
    const bool checked = (st >> ((o.w ? 46u : 32u) + o.z)) & 1ull;
    return spans == 0u || !checked;
}
__global__ void k_best_flag(BestPool pool, uint64_t n, const unsigned long long* __restrict__ state, uint32_t* __restrict__ flag,
                            uint32_t* __restrict__ nHits) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = pool.read[i];
    const unsigned long long st = state[r];
    const uint4 o = pool.occ[i];
    const bool sel = bestSelected(st, o, pool.aln[i].spans);
    flag[i] = sel ? 1u : 0u;
    if (sel && o.z == (uint32_t)(st & 255u)) atomicAdd(nHits + r, 1u); // (both strands at `best`, before the deduplication)
}

struct BestKey {
    unsigned long long hi; // read << 8 | distance << 1 | strand
    unsigned long long lo; // sequence << 32 | begin inside it
    unsigned long long idx; // position in the pool = the order in which the records were found
};
struct BestKeyLess {
    __device__ __host__ bool operator()(const BestKey& a, const BestKey& b) const {
        return a.hi != b.hi ? a.hi < b.hi : a.lo != b.lo ? a.lo < b.lo : a.idx < b.idx;
    }
};
__global__ void k_best_keys(BestPool pool, uint64_t n, const uint32_t* __restrict__ flag, const uint64_t* __restrict__ pos,
                            BestKey* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint4 o = pool.occ[i];
    const AlnRec a = pool.aln[i];
    keys[pos[i]] = BestKey{((unsigned long long)pool.read[i] << 8) | ((unsigned long long)o.z << 1) | (o.w ? 1ull : 0ull),
                           ((unsigned long long)a.seqId << 32) | a.seqBegin, i};
}
__global__ void k_best_uniq(const BestKey* __restrict__ keys, uint64_t n, uint64_t* __restrict__ uflag, uint32_t* __restrict__ perRead) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const BestKey k = keys[j];
    bool first = j == 0;
    if (!first) {
        const BestKey p = keys[j - 1];
        first = p.hi != k.hi || p.lo != k.lo;
    }
    uflag[j] = first ? 1u : 0u;
    if (first) atomicAdd(perRead + (uint32_t)(k.hi >> 8), 1u);
}
// upos: exclusive scan of uflag; devBase[r]: the records of the pool reads before r; offs[r]: the first record of read r in the final lists
__global__ void k_best_emit(const BestKey* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ uflag, const uint64_t* __restrict__ upos,
                            const uint64_t* __restrict__ devBase, const uint64_t* __restrict__ offs, BestPool pool, BestPool out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !uflag[j]) return;
    const BestKey k = keys[j];
    const uint32_t r = (uint32_t)(k.hi >> 8);
    const uint64_t dst = offs[r] + (upos[j] - devBase[r]), q = k.idx;
    out.occ[dst] = pool.occ[q];
    AlnRec a = pool.aln[q];
    a.nOps = a.nOps < BEST_OPS_STRIDE ? a.nOps : BEST_OPS_STRIDE;
    a.spans = 0; // (2, found with trimming, only comes from the host's bookkeeping)
    out.aln[dst] = a;
    for (uint32_t t = 0; t < BEST_OPS_STRIDE; t++) out.ops[dst * BEST_OPS_STRIDE + t] = pool.ops[q * BEST_OPS_STRIDE + t];
}

} // namespace cmb
