// Occurrences that run over the end of their sequence, trimmed on the device for a whole sub-batch (cmb_batch_trim_on_device): what
// IndexInterface::findSeqName does for one such occurrence (indexinterface.cpp:828-897; restated on the host in sam.hip: trimOccurrence),
// in a fixed number of launches after k_cigar, on what the run holds in HBM — the final occurrences with their sequence assignment, the
// sequence starts, the reads' bit-strings and match words of both strands, the text.
//
//   k_trim_plan     a lane per final occurrence: those with AlnRec::spans == 1 get their window [b, e) from the sequence starts — option 1,
//                   the begin lies within k of the end of its sequence: the next sequence from its start; option 2, the end lies within k
//                   of the start of the next sequence: cut there — and become a direct item {read x strand, b, e, meta} of the verification
//                   kernels (fixed start, nothing to locate: inTextVerificationOneString); itemOcc remembers the occurrence.  Every
//                   spanning occurrence is marked dropped here (spans = 4: no next sequence, an empty window, neither option, Hamming
//                   distance, or — until k_trim_commit says otherwise — nothing found in the window)
//   (kernels.hpp)   k_verify<false, true> + k_traceback<.., .., true> up to 7 errors, k_verify_wide<false, .., true> beyond: the BYITEM
//                   instances, whose text-occurrence records carry the ITEM where the production instances carry read x strand
//   k_trim_keys     a lane per record: (item, begin - b, distance, width) packed into 64 bits; holes sort last
//   (rocPRIM)       radix sort of the keys: the records of an item are adjacent, its minimum under TextOcc::operator< (begin, distance,
//                   width; indexhelpers.h:779-795) first — a segmented minimum without an atomic
//   k_trim_pick     a lane per sorted key: the head of every segment is its item's survivor, appended (one atomic per wavefront) to the
//                   compact list launchCigar works on
//   (kernels.hpp)   k_cigar / k_cigar_wide on the survivors, as for the batch's other occurrences
//   k_trim_commit   a lane per survivor: occurrence, sequence assignment (spans = 2) and CIGAR runs over the occurrence's own
#pragma once
#include "kernels.hpp"

namespace cmb {

constexpr uint32_t SPANS_OVER_END = 1u, SPANS_TRIMMED = 2u, SPANS_DROPPED = 4u; // AlnRec::spans (CMB_SPANS_*)
constexpr uint32_t TRIM_ITEM_BITS = 27; // an item's number rides above the 5 bits of meta of a traceback task (k_verify<false, true>)
// key of a verification record: item | begin - b (4 bits: at most k <= 13) | distance (4 bits) | width (24 bits)
constexpr uint32_t TRIM_KEY_ITEM = 32, TRIM_KEY_BEGIN = 28, TRIM_KEY_DIST = 24;

// stat: [0] spanning occurrences, [1] items
__global__ void __launch_bounds__(256)
k_trim_plan(const uint4* __restrict__ occ, const uint32_t* __restrict__ occRead, AlnRec* __restrict__ aln, uint64_t nOcc,
            const uint32_t* __restrict__ seqStarts, uint32_t nSeqs, uint32_t k, uint32_t hamming, uint4* __restrict__ items,
            uint32_t* __restrict__ itemOcc, uint32_t* __restrict__ stat) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t nSpanning = 0;
    for (uint64_t base = (blockIdx.x * blockDim.x + threadIdx.x) & ~63u; base < nOcc; base += stride) { // wave-uniform trip count
        const uint64_t i = base + (threadIdx.x & 63u);
        uint32_t b = 0, e = 0;
        uint4 o = make_uint4(0, 0, 0, 0);
        const bool spanning = i < nOcc && aln[i].spans == SPANS_OVER_END;
        if (spanning) {
            nSpanning++;
            o = occ[i];
            const uint32_t index = aln[i].seqId;
            // seqStarts has nSeqs + 1 elements: a next sequence exists if index + 1 < nSeqs, one behind it if index + 2 < nSeqs + 1
            if (!hamming && nSeqs >= 1u && index + 1u < nSeqs + 1u) {
                const uint32_t next = seqStarts[index + 1u];
                if (next - o.x <= k) { // option 1: begin is just before the end of the sequence
                    if (index + 2u < nSeqs + 1u) {
                        b = next;
                        e = min(o.y, seqStarts[index + 2u]);
                    }
                } else if (o.y - next <= k) { // option 2: end is just over the start of the next sequence
                    b = o.x;
                    e = next;
                }
            }
            aln[i].spans = SPANS_DROPPED;
        }
        const bool item = spanning && e > b;
        uint32_t total;
        const uint32_t at = waveAppend(&stat[1], item ? 1u : 0u, total);
        if (item) {
            items[at] = make_uint4(2u * occRead[i] + (o.w & 1u), b, e, (k << 12) | (1u << 20) | ((uint32_t)ITEM_EDIT << 21) | (1u << 23));
            itemOcc[at] = (uint32_t)i;
        }
    }
    const unsigned long long sum = waveSum64(nSpanning);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(&stat[0], (uint32_t)sum);
}

__global__ void __launch_bounds__(256)
k_trim_keys(const TextOccRec* __restrict__ text, uint32_t nText, const uint4* __restrict__ items, uint32_t nItems,
            unsigned long long* __restrict__ keys, uint32_t* __restrict__ flagWord) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t flags = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nText; i += stride) {
        const TextOccRec t = text[i];
        unsigned long long key = ~0ull;
        if (t.rsId != 0xFFFFFFFFu) { // (holes of the wavefronts' queue chunks)
            const uint32_t rel = t.rsId < nItems ? t.begin - items[t.rsId].y : ~0u, width = t.end - t.begin;
            if (rel > 15u || t.dist > 15u || t.end < t.begin || width >= (1u << TRIM_KEY_DIST)) flags |= FLAG_CAPACITY;
            else
                key = ((unsigned long long)t.rsId << TRIM_KEY_ITEM) | ((unsigned long long)rel << TRIM_KEY_BEGIN) |
                      ((unsigned long long)t.dist << TRIM_KEY_DIST) | width;
        }
        keys[i] = key;
    }
    if (flags) atomicOr(flagWord, flags);
}

// nPick: the survivors so far (at most one per item: the lists below hold nItems)
__global__ void __launch_bounds__(256)
k_trim_pick(const unsigned long long* __restrict__ keys, uint32_t nKeys, const uint4* __restrict__ items, const uint32_t* __restrict__ itemOcc,
            uint4* __restrict__ pickOcc, uint32_t* __restrict__ pickRead, uint32_t* __restrict__ pickDst, uint32_t* __restrict__ nPick) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t base = (blockIdx.x * blockDim.x + threadIdx.x) & ~63u; base < nKeys; base += stride) { // wave-uniform trip count
        const uint32_t i = base + (threadIdx.x & 63u);
        unsigned long long key = ~0ull;
        if (i < nKeys) key = keys[i];
        const uint32_t item = (uint32_t)(key >> TRIM_KEY_ITEM);
        const bool head = key != ~0ull && (i == 0u || (uint32_t)(keys[i - 1u] >> TRIM_KEY_ITEM) != item);
        uint32_t total;
        const uint32_t at = waveAppend(nPick, head ? 1u : 0u, total);
        if (head) {
            const uint4 it = items[item];
            const uint32_t begin = it.y + ((uint32_t)(key >> TRIM_KEY_BEGIN) & 15u);
            pickOcc[at] = make_uint4(begin, begin + ((uint32_t)key & ((1u << TRIM_KEY_DIST) - 1u)), (uint32_t)(key >> TRIM_KEY_DIST) & 15u, it.x & 1u);
            pickRead[at] = it.x >> 1;
            pickDst[at] = itemOcc[item];
        }
    }
}

__global__ void __launch_bounds__(256)
k_trim_commit(const uint4* __restrict__ pickOcc, const uint32_t* __restrict__ pickDst, const AlnRec* __restrict__ pickAln,
              const uint16_t* __restrict__ pickOps, uint32_t nPick, uint32_t stride, uint4* __restrict__ occ, AlnRec* __restrict__ aln,
              uint16_t* __restrict__ ops) {
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nPick; i += step) {
        const uint64_t dst = pickDst[i];
        AlnRec a = pickAln[i];
        a.spans = SPANS_TRIMMED;
        occ[dst] = pickOcc[i];
        aln[dst] = a;
        const uint32_t n = min(a.nOps, stride);
        for (uint32_t j = 0; j < n; j++) ops[dst * stride + j] = pickOps[(uint64_t)i * stride + j];
    }
}

} // namespace cmb
