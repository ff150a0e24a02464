// Kernels of the device builder of the run-length compressed (b-move) index (build.hip: cmb_build_move_*): from the text and the two
// suffix arrays a cmb_build handle holds in HBM to the move tables, the samples at run boundaries, the phi predecessors and the PLCP in
// its run form — what include/columba_amd_build.hpp (buildMoveIndex) and columba_amd/movebuild.py compute on the host, value for value
// and, for the .LFBP images, byte for byte.
//
// Per direction (the text, the reversed text), over the BWT bytes k_bld_bwt recomputes from the text and the suffix array:
//   k_mvb_flags     flag[i] = a run starts in row i; a selection over the row numbers compacts them into starts[r]
//   k_mvb_heads     head and start row of every run into the run table (four 64-bit words per run: head, start row, LF of the start row,
//                   the run that holds it), the suffix array at the run's first and last row (the samples)
//   k_mvb_lens, k_mvb_lf   LF of a run start = C[head] + the lengths of the earlier runs of that head (below)
//   k_mvb_out_run   the run that holds the LF image: a binary search over starts, one lane per run
//   k_mvb_rows      the run table as the 16-byte rows of the resident index (move_row.hpp), with the terminating row
//   k_mvb_pack      the run table as the bit-packed rows of a .LFBP file (moverepr.cpp:170-181), with the terminating row
// and for the text alone
//   k_mvb_pred_keys the keys of the predecessor structures: (sample - 1 cyclically, run), sorted by a radix sort on the bits of n
//   k_mvb_lcp_prefix, k_mvb_lcp_wave   the PLCP at the irreducible positions (below)
//   k_mvb_plcp_keep after a sort by position: the positions where PLCP + position changes start a run of the PLCP's run form
//
// LF BY RUN LENGTHS, NOT BY RANK.  The handle's cumulative bitvectors with their rank9 counts would answer "how many c before row i" too,
// but a rank is two dependent loads from arrays of n / 2 and n / 8 bytes at a random row, and the count of one character is the
// difference of two such ranks.  The run lengths are already here, in order: four exclusive sums over r values (one per character, a
// run counts its length where its head is that character) stream r words each and touch nothing of size n.
//
// PLCP.  PLCP[SA[i]] = PLCP[SA[i] - 1] - 1 wherever BWT[i] == BWT[i - 1], so only the run starts (the irreducible positions) need a
// comparison of the suffixes SA[i] and SA[i - 1].  The sum of the irreducible LCP values is at most 2 n log2 n (Kärkkäinen, Manzini,
// Puglisi: Permuted Longest-Common-Prefix Array, CPM 2009), which bounds the characters both passes compare together; one pair
// alone may have an LCP near n (a homopolymer, a tandem repeat).  So k_mvb_lcp_prefix takes a lane per pair over the first
// MVB_PREFIX characters only and lists the pairs that are still equal there; k_mvb_lcp_wave gives each of those a whole wavefront,
// which compares 64 x 8 bytes per step and finds the first mismatch with a ballot.  The '$' is unique, so two different suffixes differ
// at or before the end of the shorter one: bytes beyond the text count as a mismatch and are never read.
//
// Every kernel here loops over runs, rows or pairs and is launched through rowLaunch (build.hip): 256 lanes per block, the test cap
// applies.  Lengths: n < 2^32 - 1 from the handle; the run table and k_mvb_pack take 64-bit values (cmb_build_pack_lfbp packs rows of
// texts up to 2^40 - 1 characters).
#pragma once
#include "dev_build.hpp"
#include "move_row.hpp"

namespace cmb {

constexpr uint32_t MVB_PREFIX = 32; // characters the lane-per-pair pass compares (a multiple of 8)

// count[0] += the number of run starts (a ballot per wavefront and trip, one atomic per wavefront)
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_flags(const uint8_t* __restrict__ bwt, uint64_t n, uint8_t* __restrict__ flag,
                                                          unsigned long long* __restrict__ count) {
    unsigned long long mine = 0;
    for (uint64_t i = bldGid(); (i & ~63ull) < n; i += bldStride()) { // (the condition is the same for a whole wavefront)
        const bool f = i < n && (i == 0 || bwt[i] != bwt[i - 1]);
        if (i < n) flag[i] = f;
        mine += (unsigned long long)__popcll(__ballot(f));
    }
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(count, mine);
}

__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_heads(const uint8_t* __restrict__ bwt, const uint32_t* __restrict__ sa,
                                                          const uint64_t* __restrict__ starts, uint64_t r, uint64_t n, uint64_t* __restrict__ run,
                                                          uint64_t* __restrict__ smpF, uint64_t* __restrict__ smpL) {
    for (uint64_t j = bldGid(); j < r; j += bldStride()) {
        const uint64_t s = starts[j], e = j + 1 < r ? starts[j + 1] : n;
        run[4 * j] = bwt[s], run[4 * j + 1] = s, run[4 * j + 2] = 0; // (LF of the '$' run: row 0)
        smpF[j] = sa[s], smpL[j] = sa[e - 1];
    }
}

// len[j] = the length of run j where its head is c, else 0 (a character occurs fewer than 2^32 times: 32-bit sums)
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_lens(const uint64_t* __restrict__ run, const uint64_t* __restrict__ starts, uint64_t r, uint64_t n,
                                                         uint32_t c, uint32_t* __restrict__ len) {
    for (uint64_t j = bldGid(); j < r; j += bldStride())
        len[j] = run[4 * j] == c ? (uint32_t)((j + 1 < r ? starts[j + 1] : n) - starts[j]) : 0u;
}
// ... and with their exclusive sums: LF of the first row of every run of c
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_lf(const uint32_t* __restrict__ before, uint64_t r, uint32_t c, uint64_t cumC,
                                                       uint64_t* __restrict__ run) {
    for (uint64_t j = bldGid(); j < r; j += bldStride())
        if (run[4 * j] == c) run[4 * j + 2] = cumC + before[j];
}

__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_out_run(const uint64_t* __restrict__ starts, uint64_t r, uint64_t* __restrict__ run) {
    for (uint64_t j = bldGid(); j < r; j += bldStride()) {
        const uint64_t x = run[4 * j + 2];
        uint64_t lo = 0, hi = r; // the first run that starts beyond x
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (starts[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        run[4 * j + 3] = lo - 1; // (starts[0] == 0 <= x)
    }
}

// rows 0 .. r of a table from the run table; row r is the terminating row (0, n, n, r)
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_rows(const uint64_t* __restrict__ run, uint64_t r, uint64_t n, uint4* __restrict__ rows) {
    for (uint64_t j = bldGid(); j <= r; j += bldStride())
        rows[j] = j < r ? packMoveRow((uint32_t)run[4 * j], run[4 * j + 1], run[4 * j + 2], run[4 * j + 3]) : packMoveRow(0, n, n, r);
}
// the same rows as a .LFBP file holds them: rowBytes = ceil((3 + 2 bitsN + bitsR) / 8) bytes each, the fields at bits 0, 3, 3 + bitsN and
// 3 + 2 bitsN, every value cut to its field (bitsN <= 40, bitsR <= bitsN: at most 123 bits)
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_pack(const uint64_t* __restrict__ run, uint64_t r, uint64_t n, uint32_t bitsN, uint32_t bitsR,
                                                         uint32_t rowBytes, uint8_t* __restrict__ out) {
    const uint64_t maskN = (1ull << bitsN) - 1, maskR = (1ull << bitsR) - 1;
    for (uint64_t j = bldGid(); j <= r; j += bldStride()) {
        uint64_t lo = 0, hi = 0;
        auto place = [&](uint64_t v, uint32_t off) {
            if (off < 64) {
                lo |= v << off;
                if (off > 0) hi |= v >> (64 - off);
            } else
                hi |= v << (off - 64);
        };
        place(j < r ? run[4 * j] & 7u : 0u, 0);
        place((j < r ? run[4 * j + 1] : n) & maskN, 3);
        place((j < r ? run[4 * j + 2] : n) & maskN, 3 + bitsN);
        place((j < r ? run[4 * j + 3] : r) & maskR, 3 + 2 * bitsN);
        uint8_t* p = out + j * rowBytes;
        for (uint32_t b = 0; b < rowBytes; b++) p[b] = (uint8_t)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xFFu);
    }
}

__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_pred_keys(const uint64_t* __restrict__ smp, uint64_t r, uint64_t n, uint64_t* __restrict__ key,
                                                              uint64_t* __restrict__ val) {
    for (uint64_t j = bldGid(); j < r; j += bldStride()) {
        const uint64_t s = smp[j];
        key[j] = s > 0 ? s - 1 : n - 1;
        val[j] = j;
    }
}

// how many of the 8 bytes at pa and pb are equal before the first that differs (8: all); a byte beyond the text differs
__device__ __forceinline__ uint32_t mvbEqual8(const uint8_t* __restrict__ text, uint64_t n, uint64_t pa, uint64_t pb) {
    if (pa + 8 <= n && pb + 8 <= n) {
        uint64_t x, y;
        __builtin_memcpy(&x, text + pa, 8);
        __builtin_memcpy(&y, text + pb, 8);
        const uint64_t d = x ^ y;
        return d ? (uint32_t)(__ffsll((unsigned long long)d) - 1) >> 3 : 8u;
    }
    for (uint32_t k = 0; k < 8; k++)
        if (pa + k >= n || pb + k >= n || text[pa + k] != text[pb + k]) return k;
    return 8u;
}
// sum[j] = PLCP + position at the first row of run j (run 0: SA[0] = n - 1, PLCP 0), for the pairs that differ within MVB_PREFIX
// characters; the others go to the list `open` (count[0] of them, in no particular order)
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_lcp_prefix(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ sa,
                                                               const uint64_t* __restrict__ starts, uint64_t r, uint64_t* __restrict__ sum,
                                                               uint32_t* __restrict__ open, uint32_t* __restrict__ count) {
    for (uint64_t j = bldGid(); j < r; j += bldStride()) {
        const uint64_t i = starts[j], a = sa[i];
        if (j == 0) {
            sum[0] = a;
            continue;
        }
        const uint64_t b = sa[i - 1];
        uint32_t l = 0, d = 8;
        while (l < MVB_PREFIX && d == 8) d = mvbEqual8(text, n, a + l, b + l), l += d;
        if (d == 8) open[atomicAdd(count, 1u)] = (uint32_t)j;
        else sum[j] = a + l;
    }
}
// one wavefront per listed pair, from character MVB_PREFIX on: lane k compares bytes 8 k .. 8 k + 7 of a step of 512
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_lcp_wave(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ sa,
                                                             const uint64_t* __restrict__ starts, const uint32_t* __restrict__ open, uint64_t m,
                                                             uint64_t* __restrict__ sum) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = bldGid(); (i >> 6) < m; i += bldStride()) { // (the condition is the same for a whole wavefront)
        const uint32_t j = open[i >> 6];
        const uint64_t row = starts[j], a = sa[row], b = sa[row - 1];
        uint64_t l = MVB_PREFIX;
        for (;;) { // ends: a lane whose bytes lie beyond the text reports a mismatch
            const uint32_t d = mvbEqual8(text, n, a + l + 8u * lane, b + l + 8u * lane);
            const uint64_t hit = __ballot(d < 8);
            if (hit) {
                const int first = __ffsll((unsigned long long)hit) - 1;
                l += 8u * (uint32_t)first + (uint32_t)__shfl((int)d, first);
                break;
            }
            l += 512;
        }
        if (lane == 0) sum[j] = a + l;
    }
}
// after the sort by position: keep[j] = PLCP + position differs from the entry before (entry 0, position 0, is always kept)
__global__ void __launch_bounds__(BLD_BLOCK) k_mvb_plcp_keep(const uint64_t* __restrict__ sum, uint64_t r, uint8_t* __restrict__ keep) {
    for (uint64_t j = bldGid(); j < r; j += bldStride()) keep[j] = j == 0 || sum[j] != sum[j - 1];
}

} // namespace cmb
