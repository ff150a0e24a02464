// Kernels of the device index builder (build.hip): from the preprocessed text to the suffix arrays of the text and of the reversed
// text, and to every array include/columba_amd_build.hpp derives from them, in that header's layouts bit for bit (its functions
// bwtBitvectors, rankCounts, sparseSuffixArray and encodeBwt are the specification).
//
// Suffix array: a radix sort on the first 20 symbols (3 bits each, 0 = beyond the end, so a suffix that is a proper prefix of another
// sorts first), then prefix doubling in the Larsson-Sadakane manner on group-head ranks: rank[p] = the row of the first suffix of the
// group p lies in.  A round looks only at the rows of groups that are still open (more than one suffix): it sorts them by
// (rank[p], rank[p + h] + 1 or 0 beyond the end) — the rows of a group stay in the group's slots, because the group's rank is the
// major key and the list of open rows is in row order —, writes them back, and derives heads, ranks and the next list of open rows.
// The same kernels sort the reversed text: sym() reads the text from its end.
//
// Every kernel that loops over rows or positions is launched through host_grid.hpp's cap (one lane per row and trip, 256 lanes per
// block); the kernels that take one lane per output word or per 512-bit block do not loop and are not capped.
// Lengths: n < 2^32 - 1, so rows, positions and ranks are 32-bit and a doubling key fits 64 bits; loop counters are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cmb {

constexpr uint32_t BLD_BLOCK = 256;
constexpr uint32_t BLD_KEY_SYMBOLS = 20; // 3 bits each: the initial sort's key has 60 bits

__device__ __forceinline__ uint32_t bldCode(uint8_t ch) { // codeOf (columba_amd_build.hpp): $ A C G T -> 0 .. 4
    return ch == '$' ? 0u : ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 3u : 4u;
}
// symbol p of the string that is sorted: the text, or the text read from its end
__device__ __forceinline__ uint32_t bldSym(const uint8_t* __restrict__ text, uint64_t n, bool rev, uint64_t p) {
    return bldCode(text[rev ? n - 1 - p : p]);
}
__device__ __forceinline__ uint64_t bldGid() { return (uint64_t)blockIdx.x * BLD_BLOCK + threadIdx.x; }
__device__ __forceinline__ uint64_t bldStride() { return (uint64_t)gridDim.x * BLD_BLOCK; }

// The text as preprocessFastaFiles leaves it: A, C, G, T and one '$', the last byte.  bad[0] counts every other byte; hist[c] counts
// the symbols of code c.
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_check(const uint8_t* __restrict__ text, uint64_t n, uint32_t* __restrict__ bad,
                                                          unsigned long long* __restrict__ hist) {
    __shared__ uint32_t sh[6];
    if (threadIdx.x < 6) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t cnt[5] = {0, 0, 0, 0, 0}, wrong = 0;
    for (uint64_t i = bldGid(); i < n; i += bldStride()) {
        const uint8_t ch = text[i];
        const bool ok = i + 1 == n ? ch == '$' : (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
        wrong += !ok;
        const uint32_t c = bldCode(ch);
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) cnt[k] += ok && c == k; // (no indexing by c: the counters stay in registers)
    }
    for (int c = 0; c < 5; c++)
        if (cnt[c]) atomicAdd(&sh[c], cnt[c]);
    if (wrong) atomicAdd(&sh[5], wrong);
    __syncthreads();
    if (threadIdx.x < 5 && sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
    if (threadIdx.x == 5 && sh[5]) atomicAdd(bad, sh[5]);
}

// key[p] = the first 20 symbols of suffix p, each as code + 1, 0 beyond the end; val[p] = p
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_key20(const uint8_t* __restrict__ text, uint64_t n, bool rev, uint64_t* __restrict__ key,
                                                          uint32_t* __restrict__ val) {
    for (uint64_t p = bldGid(); p < n; p += bldStride()) {
        uint64_t k = 0;
        for (uint32_t j = 0; j < BLD_KEY_SYMBOLS; j++) k = k << 3 | (p + j < n ? bldSym(text, n, rev, p + j) + 1u : 0u);
        key[p] = k;
        val[p] = (uint32_t)p;
    }
}

// After a sort of m list entries (rows == nullptr: the list is every row, entry j is row j): head[j] = the row of entry j where a
// group begins there, else 0 — an inclusive maximum scan turns it into the group-head row of every entry.
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_heads(const uint64_t* __restrict__ key, const uint32_t* __restrict__ rows, uint64_t m,
                                                          uint32_t* __restrict__ head) {
    for (uint64_t j = bldGid(); j < m; j += bldStride()) {
        const bool first = j == 0 || key[j] != key[j - 1];
        head[j] = first ? (rows ? rows[j] : (uint32_t)j) : 0u;
    }
}
// ... then: the suffixes go back to their rows, every one takes the head row of its group as its rank, and open[j] says whether the
// group of entry j still holds more than one suffix
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_ranks(const uint32_t* __restrict__ val, const uint32_t* __restrict__ head,
                                                          const uint32_t* __restrict__ rows, uint64_t m, uint32_t* __restrict__ sa,
                                                          uint32_t* __restrict__ rank, uint8_t* __restrict__ open) {
    for (uint64_t j = bldGid(); j < m; j += bldStride()) {
        const uint32_t row = rows ? rows[j] : (uint32_t)j, p = val[j], h = head[j];
        if (rows) sa[row] = p; // (the first sort's values are the suffix array itself)
        rank[p] = h;
        const bool single = h == row && (j + 1 == m || head[j + 1] == (rows ? rows[j + 1] : (uint32_t)(j + 1)));
        open[j] = !single;
    }
}
// the keys of a doubling round over the open rows: (rank of the suffix) << 32 | (rank h positions on + 1, 0 beyond the end)
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_round_keys(const uint32_t* __restrict__ rows, uint64_t m, const uint32_t* __restrict__ sa,
                                                               const uint32_t* __restrict__ rank, uint64_t n, uint64_t h,
                                                               uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    for (uint64_t j = bldGid(); j < m; j += bldStride()) {
        const uint32_t p = sa[rows[j]];
        const uint64_t q = (uint64_t)p + h;
        key[j] = (uint64_t)rank[p] << 32 | (q < n ? (uint64_t)rank[q] + 1u : 0u);
        val[j] = p;
    }
}

// bwt[i] = code of the character before suffix SA[i] (the text's last for SA[i] == 0); for the reversed text the character
// T[n - revSA[i]] (T[0] for revSA[i] == 0), as buildIndex reads it from the text itself.  The row of the '$' goes to dollarPos.
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_bwt(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ sa, bool rev,
                                                        uint8_t* __restrict__ bwt, unsigned long long* __restrict__ dollarPos) {
    for (uint64_t i = bldGid(); i < n; i += bldStride()) {
        const uint64_t j = sa[i];
        const uint8_t ch = rev ? (j > 0 ? text[n - j] : text[0]) : (j > 0 ? text[j - 1] : text[n - 1]);
        const uint32_t c = bldCode(ch);
        bwt[i] = (uint8_t)c;
        if (c == 0) *dollarPos = i;
    }
}

// BWTRepresentation<5>: word w of bitvector k (symbols 1 .. k) at bv[4 w + k - 1].  One wavefront's ballot over 64 rows is that word.
// nWords = ceil((n + 1) / 64): the rows from n on hold no symbol.
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_bitvectors(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t nWords,
                                                               uint64_t* __restrict__ bv) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = bldGid(); (i >> 6) < nWords; i += bldStride()) { // (the condition is the same for a whole wavefront)
        const uint32_t c = i < n ? bwt[i] : 0u;
        uint64_t mine = 0;
        for (uint32_t k = 1; k <= 4; k++) {
            const uint64_t word = __ballot(c != 0 && c <= k);
            if (lane == k - 1) mine = word;
        }
        if (lane < 4) bv[(i >> 6) * 4 + lane] = mine;
    }
}
// the sampled rows of the sparse suffix array: bit i of the bitvector = SA[i] % sparseness == 0
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_sa_mark(const uint32_t* __restrict__ sa, uint64_t n, uint32_t mask, uint64_t nWords,
                                                            uint64_t* __restrict__ bv) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = bldGid(); (i >> 6) < nWords; i += bldStride()) {
        const uint64_t word = __ballot(i < n && (sa[i] & mask) == 0);
        if (lane == 0) bv[i >> 6] = word;
    }
}

// rankCounts for K interleaved bitvectors (word w of vector k at words[w K + k]), one lane per (block, vector): the seven 9-bit
// partial sums of the block go to counts[2 (b K + k) + 1] (where that lies below cw), the block's total to tot[k nBlocks + b] for the
// exclusive scan that gives the absolute counts.  Partial sums of words past the end stay 0.
template <uint32_t K>
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_block_counts(const uint64_t* __restrict__ words, uint64_t nWords, uint64_t nBlocks,
                                                                 uint64_t cw, uint64_t* __restrict__ counts, uint64_t* __restrict__ tot) {
    const uint64_t id = bldGid();
    if (id >= nBlocks * K) return;
    const uint64_t b = id / K, k = id % K;
    uint64_t within = 0, l2 = 0;
    for (uint32_t j = 0; j < 8; j++) {
        const uint64_t w = b * 8 + j;
        if (w >= nWords) break;
        if (j > 0) l2 |= within << (9 * (j - 1));
        within += (uint64_t)__popcll(words[w * K + k]);
    }
    if (2 * id + 1 < cw) counts[2 * id + 1] = l2;
    tot[k * nBlocks + b] = within;
}
template <uint32_t K>
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_block_starts(const uint64_t* __restrict__ before, uint64_t nBlocks, uint64_t cw,
                                                                 uint64_t* __restrict__ counts) {
    const uint64_t id = bldGid();
    if (id >= nBlocks * K) return;
    if (2 * id < cw) counts[2 * id] = before[(id % K) * nBlocks + id / K];
}

// encodeBwt: 3 bits per symbol, most significant bit first, one continuous stream; one lane per 64-bit word
__global__ void __launch_bounds__(BLD_BLOCK) k_bld_pack3(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t nWords, uint64_t* __restrict__ out) {
    const uint64_t w = bldGid();
    if (w >= nWords) return;
    const uint64_t bit0 = w * 64;
    uint64_t word = 0;
    for (uint64_t i = bit0 / 3; i < n && 3 * i < bit0 + 64; i++) {
        const uint64_t c = bwt[i];
        const int64_t shift = (int64_t)(bit0 + 61) - (int64_t)(3 * i); // where the symbol's lowest bit lands in this word
        if (shift >= 0) word |= c << shift;
        else word |= c >> (-shift);
    }
    out[w] = word;
}

} // namespace cmb
