// Kernels of the device FASTQ parser (reads.hip): from a window of raw file bytes to the packed arrays every batch and SAM entry point
// takes (seqs + offs, ids + id_offs, quals + qual_offs).  The specification is Reader of include/columba_amd_io.hpp, byte for byte.
//
// THE LARGEST WINDOW is READS_MAX_WINDOW = 2^30 bytes (1 GiB): byte positions and line numbers are 32-bit below it.
//
// Bytes -> lines.  A tile is READS_TILE = 4096 bytes: 256 lanes with one 16-byte load each.  k_rd_count counts the newlines of every
// tile, a scan of the counts gives every tile the number of its first line, k_rd_place reads the tile again, ranks its newlines (a
// wavefront scan by __shfl_up, the four wavefront totals through LDS) and writes lineEnd[line] = the position of the line's '\n'.  A
// tile without a newline (a 70 000-character read spans 17 of them) has count 0 and writes nothing.  Line i is the bytes
// [lineEnd[i - 1] + 1, lineEnd[i]); the last line of a final window may lack its newline and ends at the end of the window.
//
// Lines -> records.  Which field of which record a line is depends on every line before it: Reader skips a line that is empty or begins
// with '\r' only where a record would begin, and takes the next four lines as they are.  That is a machine with four states (0: a
// record may begin, 1 .. 3: the read, the separator, the quality follow), and a line is a function from state to state: in state 0
// a blank-like line stays and any other goes to 1; from 1 .. 3 every line advances, 3 back to 0.  Such a function is four 2-bit
// values, one byte (READS_FN_*).  Composition is associative, so an exclusive scan of the lines' functions under composition
// (RdCompose; rocPRIM's device scan carries it across wavefronts, blocks and launches) gives every line the function of everything
// before it, whose value at 0 is the state the line is read in.  A line read in state 0 that is not blank-like begins a record;
// the selection of those lines is recLine[record], and the record's fields are the lines recLine, + 1 and + 3 where they exist.
//
// Records -> packed arrays.  k_rd_fields chomps the three fields of a record (trailing '\r'; a line holds no '\n'), notes the first record
// without '@' and the first with an empty read, the three lengths are scanned into 64-bit offsets, and k_rd_gather copies: 16 lanes
// per field, whole destination words from two aligned source words (the fields of a 150 bp record are 38 words: byte stores would be
// four times the store instructions, as k_prep found for its rows), single bytes only in front of the first and behind the last word
// boundary of a field, where the neighbouring field owns the rest of the word.
//
// Every kernel loops over the items beyond its launch (host_grid.hpp's cap); loop counters are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cmb {

constexpr uint32_t READS_BLOCK = 256;
constexpr uint32_t READS_TILE = READS_BLOCK * 16;  // bytes per block and trip of the byte pass
constexpr uint64_t READS_MAX_WINDOW = 1ull << 30;  // the largest window cmb_reads_parse_fastq takes
constexpr uint32_t READS_GATHER_LANES = 16;        // lanes that copy one field
constexpr uint32_t READS_NONE = 0xFFFFFFFFu;       // no record without '@' / with an empty read
// a line as a function of the state: f(s) in bits [2 s, 2 s + 2)
constexpr uint8_t READS_FN_LINE = 1u | 2u << 2 | 3u << 4 | 0u << 6;
constexpr uint8_t READS_FN_BLANK = 0u | 2u << 2 | 3u << 4 | 0u << 6;
constexpr uint8_t READS_FN_IDENTITY = 0u | 1u << 2 | 2u << 4 | 3u << 6;

struct RdCompose { // first a, then b
    __host__ __device__ uint8_t operator()(const uint8_t& a, const uint8_t& b) const {
        uint32_t g = 0;
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) g |= ((b >> (2u * ((a >> (2u * s)) & 3u))) & 3u) << (2u * s);
        return (uint8_t)g;
    }
};

__device__ __forceinline__ uint64_t rdGid() { return (uint64_t)blockIdx.x * READS_BLOCK + threadIdx.x; }
__device__ __forceinline__ uint64_t rdStride() { return (uint64_t)gridDim.x * READS_BLOCK; }
// 0x80 in every byte of w that is '\n' (exact per byte: no carry leaves a byte)
__device__ __forceinline__ uint32_t rdNewlines(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t rdCount(const uint4& v) {
    return __popc(rdNewlines(v.x)) + __popc(rdNewlines(v.y)) + __popc(rdNewlines(v.z)) + __popc(rdNewlines(v.w));
}

// count[t] = the newlines of tile t (the window is padded with zero bytes to whole 16-byte vectors)
__global__ void __launch_bounds__(READS_BLOCK) k_rd_count(const uint4* __restrict__ bytes, uint64_t nVec, uint64_t nTiles, uint32_t* __restrict__ count) {
    __shared__ uint32_t sh[READS_BLOCK / 64];
    for (uint64_t t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const uint64_t v = t * READS_BLOCK + threadIdx.x;
        uint32_t c = v < nVec ? rdCount(bytes[v]) : 0u;
#pragma unroll
        for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) count[t] = sh[0] + sh[1] + sh[2] + sh[3];
        __syncthreads();
    }
}
// lineEnd[base[t] + j] = the position of newline j of tile t
__global__ void __launch_bounds__(READS_BLOCK) k_rd_place(const uint4* __restrict__ bytes, uint64_t nVec, uint64_t nTiles, const uint32_t* __restrict__ base,
                                                           uint32_t* __restrict__ lineEnd) {
    __shared__ uint32_t sh[READS_BLOCK / 64];
    for (uint64_t t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const uint64_t v = t * READS_BLOCK + threadIdx.x;
        uint4 d = make_uint4(0, 0, 0, 0);
        if (v < nVec) d = bytes[v];
        const uint32_t c = rdCount(d);
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if ((int)(threadIdx.x & 63) >= o) incl += up;
        }
        if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t line = base[t] + incl - c;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) line += sh[w];
        const uint32_t words[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            uint32_t m = rdNewlines(words[k]);
            while (m) {
                const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
                lineEnd[line++] = (uint32_t)(v * 16u + k * 4u + (bit >> 3));
                m &= m - 1u;
            }
        }
        __syncthreads();
    }
}

// where line i ends (the position of its '\n', or the end of the window for a last line without one) and begins
__device__ __forceinline__ uint32_t rdLineEnd(const uint32_t* __restrict__ lineEnd, uint32_t nNewlines, uint32_t nBytes, uint64_t i) {
    return i < nNewlines ? lineEnd[i] : nBytes;
}
__device__ __forceinline__ uint32_t rdLineBegin(const uint32_t* __restrict__ lineEnd, uint64_t i) { return i ? lineEnd[i - 1] + 1u : 0u; }

// fn[i] = line i as a function of the state
__global__ void __launch_bounds__(READS_BLOCK) k_rd_classify(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ lineEnd, uint32_t nNewlines,
                                                              uint32_t nBytes, uint64_t nLines, uint8_t* __restrict__ fn) {
    for (uint64_t i = rdGid(); i < nLines; i += rdStride()) {
        const uint32_t s = rdLineBegin(lineEnd, i), e = rdLineEnd(lineEnd, nNewlines, nBytes, i);
        fn[i] = (e == s || bytes[s] == '\r') ? READS_FN_BLANK : READS_FN_LINE;
    }
}
// start[i] = line i begins a record: it is read in state 0 (before[i]: the composed function of the lines in front of it) and is not blank-like
__global__ void __launch_bounds__(READS_BLOCK) k_rd_starts(const uint8_t* __restrict__ fn, const uint8_t* __restrict__ before, uint64_t nLines,
                                                            uint8_t* __restrict__ start) {
    for (uint64_t i = rdGid(); i < nLines; i += rdStride()) start[i] = (before[i] & 3u) == 0u && fn[i] == READS_FN_LINE;
}
// The fields of the records [0, nRec): field f of record r (0: identifier, 1: read, 2: quality) begins at fBegin[f * stride + r] and has
// fLen[f * stride + r] bytes after chomp; a line the window does not hold is an empty field.  first[0] = the first record whose
// identifier line does not begin with '@', first[1] = the first whose read is empty (READS_NONE before the launch).
__global__ void __launch_bounds__(READS_BLOCK) k_rd_fields(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ lineEnd, uint32_t nNewlines,
                                                            uint32_t nBytes, uint64_t nLines, const uint32_t* __restrict__ recLine, uint64_t nRec,
                                                            uint64_t stride, uint32_t* __restrict__ fBegin, uint32_t* __restrict__ fLen,
                                                            uint32_t* __restrict__ first) {
    for (uint64_t r = rdGid(); r < nRec; r += rdStride()) {
        const uint64_t line0 = recLine[r];
#pragma unroll
        for (uint32_t f = 0; f < 3; f++) {
            const uint64_t line = line0 + (f == 2 ? 3u : f);
            uint32_t s = 0, e = 0;
            if (line < nLines) {
                s = rdLineBegin(lineEnd, line), e = rdLineEnd(lineEnd, nNewlines, nBytes, line);
                while (e > s && bytes[e - 1] == '\r') e--;
            }
            fBegin[f * stride + r] = s;
            fLen[f * stride + r] = e - s;
            if (f == 0 && bytes[s] != '@') atomicMin(&first[0], (uint32_t)r); // (a line that begins a record is not empty)
            if (f == 1 && e == s) atomicMin(&first[1], (uint32_t)r);
        }
    }
}

// out[f][offs[f][r] ...) = field f of record r, for the records [0, nRec): READS_GATHER_LANES lanes per field.  `words` is the window
// as 32-bit words (padded: the word behind the last byte may be read).
__global__ void __launch_bounds__(READS_BLOCK) k_rd_gather(const uint32_t* __restrict__ words, const uint32_t* __restrict__ fBegin,
                                                            const uint32_t* __restrict__ fLen, uint64_t stride, const uint64_t* __restrict__ offs,
                                                            uint64_t offStride, uint8_t* out0, uint8_t* out1, uint8_t* out2, uint64_t nRec) {
    const uint8_t* __restrict__ bytes = reinterpret_cast<const uint8_t*>(words);
    const uint32_t lane = threadIdx.x % READS_GATHER_LANES;
    for (uint64_t item = rdGid() / READS_GATHER_LANES; item < 3 * nRec; item += rdStride() / READS_GATHER_LANES) {
        const uint64_t r = item / 3;
        const uint32_t f = (uint32_t)(item % 3);
        uint8_t* out = f == 0 ? out0 : f == 1 ? out1 : out2;
        const uint32_t src = fBegin[f * stride + r], len = fLen[f * stride + r];
        const uint64_t d0 = offs[f * offStride + r], d1 = d0 + len;
        const uint64_t a0 = (d0 + 3u) & ~3ull, a1 = d1 & ~3ull; // the whole words of the field are [a0, a1)
        if (a0 >= a1) {
            for (uint32_t j = lane; j < len; j += READS_GATHER_LANES) out[d0 + j] = bytes[src + j];
            continue;
        }
        if (lane < a0 - d0) out[d0 + lane] = bytes[src + lane];
        if (lane < d1 - a1) out[a1 + lane] = bytes[src + (uint32_t)(a1 - d0) + lane];
        uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
        for (uint64_t w = a0 / 4 + lane; w < a1 / 4; w += READS_GATHER_LANES) {
            const uint32_t p = src + (uint32_t)(w * 4 - d0); // the source of the word's first byte
            const uint32_t lo = words[p >> 2], hi = words[(p >> 2) + 1];
            out32[w] = __funnelshift_r(lo, hi, (p & 3u) * 8u);
        }
    }
}

} // namespace cmb
