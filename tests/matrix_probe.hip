// Device probe of the bit-parallel matrices and trace rows (tests/test_gpu_matrix_probe.py; the formats are those of
// tests/matrixtruth.py).  TEST INFRASTRUCTURE: a stand-alone program that calls the product's own __device__ functions of
// dev_matrix.hpp and dev_trace.hpp, one lane per case, and writes down what they compute — cells, verdicts, rightmost active
// columns, match words, walks — for comparison with plain dynamic programming (oracle/groundtruth.c).
//
//   matrix_probe <case file> <result file>
//
// Every HIP call is checked; the first error ends the program with a non-zero status and nothing is launched after it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dev_trace.hpp" // (and through it dev_matrix.hpp and the in-index geometries of dev_bfs_edit.hpp)

using namespace cmb;

#define HIP_OK(call)                                                                                         \
    do {                                                                                                     \
        const hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                              \
            fprintf(stderr, "matrix_probe: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(1);                                                                                         \
        }                                                                                                    \
    } while (0)

// ---- formats (little endian; mirrored in tests/matrixtruth.py) ----
constexpr uint32_t N_GEO = 7, MC_WORDS = 16, WQ_WORDS = 8, TC_WORDS = 8, ROW_BYTES = 64, ROW_CELLS = 56;
constexpr uint32_t WALK_WORDS = 32, MAX_WALKS = 32, WALK_STRIDE = WALK_WORDS - 4;
struct Header {          // 32 x u64
    uint64_t magic;      // 'CMBPROBE'
    uint64_t nSrc, poolBytes, nMat, matRows, yBytes, nRaw, nWordQ, nTrace[2], traceLines[2];
    uint64_t geoBegin[N_GEO + 1];
    uint64_t pad[32 - 12 - (N_GEO + 1)];
};
static_assert(sizeof(Header) == 256, "header");
// a source string: {offset into the pool, length}; its four bit-strings are laid out as k_prep lays out a read's (gWords words each,
// zero padded), built by the host below
// matrix case:  0 src, 1 xOff, 2 xLen, 3 yOff, 4 yLen, 5 maxED, 6 nZeros (in-text), 7 nInit, 8 rawOff, 9 increase, 10 first row of
//               its results, 11 rows
// word query:   0 kind, 1 src, 2 xOff, 3 xLen, 4 nucleotide, 5 block or row
// trace case:   0 src, 1 xLen, 2 yOff, 3 yLen, 4 maxED, 5 nZeros
struct MatRow {
    uint8_t verdict, ovgl;
    uint16_t score, rac, nCells;
    uint8_t cells[ROW_CELLS];
};
static_assert(sizeof(MatRow) == ROW_BYTES, "row");

struct Strings { // the bit-strings of every source
    const uint32_t* G;
    const uint64_t* gOff; // first word of a source's four strings
    const uint32_t* gw;   // words per string
    __device__ __forceinline__ const uint32_t* of(uint32_t src, uint32_t ch) const { return G + gOff[src] + (size_t)ch * gw[src]; }
};

// ---- the seven geometries: start state, match word of a row (taken the way production takes it), row, cell, predicate ----
// in-index: the product's own geometry structs (dev_bfs_edit.hpp); the match word of a row comes from its context block's word
template <class Mx>
struct InIndex {
    typedef typename Mx::W W;
    static constexpr bool IN_TEXT = false;
    static constexpr uint32_t BLOCK = Mx::BLOCK, LEFT = Mx::LEFT, DIAG = Mx::DIAG;
    static __device__ __forceinline__ W mword(const uint32_t* Gc, uint32_t xOff, uint32_t xLen, uint32_t i) {
        return Mx::mword(matchWord<Mx::CTX_LEFT, Mx::CTX_BLOCK>(Gc, xOff, xLen, i / Mx::CTX_BLOCK), i);
    }
    static __device__ __forceinline__ bool row(const MatGeom& g, uint32_t i, W M, W& HP, W& HN, W& D0, W& RAC, uint32_t& sc) {
        return Mx::row(g, i, M, HP, HN, D0, RAC, sc);
    }
    static __device__ __forceinline__ uint32_t cell(uint32_t i, uint32_t j, W HP, W HN, uint32_t sc) { return Mx::cell(i, j, HP, HN, sc); }
    static __device__ __forceinline__ bool ovgl(const MatGeom& g, uint32_t i, W HN) { return Mx::ovgl(g, i, HN); }
};
// in-text, k <= 7: the two matrices of forwardPass, match words from the 32-row block words of the full read
template <bool W32>
struct InTextBlockWords {
    typedef InTextMx<W32> Mx;
    typedef typename Mx::W W;
    static constexpr bool IN_TEXT = true;
    static constexpr uint32_t BLOCK = Mx::BLOCK, LEFT = Mx::LEFT, DIAG = Mx::DIAG;
    static __device__ __forceinline__ W mword(const uint32_t* Gc, uint32_t, uint32_t xLen, uint32_t i) {
        return Mx::matchWordOf(matchWord<MXF_LEFT>(Gc, 0u, xLen, i / MX_BLOCK), i);
    }
    static __device__ __forceinline__ bool row(const MatGeom& g, uint32_t i, W M, W& HP, W& HN, W& D0, W& RAC, uint32_t& sc) {
        return Mx::row(g, i, M, HP, HN, D0, RAC, sc);
    }
    static __device__ __forceinline__ uint32_t cell(uint32_t i, uint32_t j, W HP, W HN, uint32_t sc) { return Mx::cell(i, j, HP, HN, sc); }
    static __device__ __forceinline__ bool ovgl(const MatGeom&, uint32_t, W) { return false; }
};
// in-text, k 8 .. 13: the wide left margin, match words straight from the bit-strings
template <uint32_t BLOCK_, uint32_t DIAG_, uint32_t LEFT_>
struct InTextWide {
    typedef uint64_t W;
    static constexpr bool IN_TEXT = true;
    static constexpr uint32_t BLOCK = BLOCK_, LEFT = LEFT_, DIAG = DIAG_;
    static __device__ __forceinline__ W mword(const uint32_t* Gc, uint32_t, uint32_t xLen, uint32_t i) {
        return matchWord<LEFT, BLOCK>(Gc, 0u, xLen, i / BLOCK);
    }
    static __device__ __forceinline__ bool row(const MatGeom& g, uint32_t i, W M, W& HP, W& HN, W& D0, W& RAC, uint32_t& sc) {
        return computeRowWide<BLOCK, DIAG>(g, i, M, HP, HN, D0, RAC, sc);
    }
    static __device__ __forceinline__ uint32_t cell(uint32_t i, uint32_t j, W HP, W HN, uint32_t sc) { return cellAt<BLOCK, DIAG>(i, j, HP, HN, sc); }
    static __device__ __forceinline__ bool ovgl(const MatGeom&, uint32_t, W) { return false; }
};

// the geometry and start state of an in-text matrix (forwardPass: a first column of nZeros zeros)
template <class P>
__device__ __forceinline__ void inTextStart(MatGeom& g, uint32_t xLen, uint32_t maxED, uint32_t nZeros, typename P::W& HP, typename P::W& HN,
                                            typename P::W& RAC, uint32_t& score) {
    typedef typename P::W W;
    g.n = xLen + 1;
    g.maxED = maxED;
    g.Wv = nZeros - 1 + maxED;
    g.Wh = maxED;
    g.m = max(g.Wv + g.n, g.Wv + g.Wh + 1u);
    HP = (W)(~(W)0) << P::LEFT;
    HN = ((W)1 << (P::LEFT + 1u - nZeros)) - (W)1;
    RAC = racInit((W)0, P::DIAG + g.Wh);
    score = 0;
}

template <class P>
__global__ void __launch_bounds__(256)
k_matrix(Strings S, const uint32_t* __restrict__ cases, uint32_t caseBegin, uint32_t caseEnd, const uint8_t* __restrict__ yPool,
         const uint16_t* __restrict__ rawPool, MatRow* __restrict__ rows, uint32_t* __restrict__ rowsDone) {
    typedef typename P::W W;
    const uint32_t ci = caseBegin + blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= caseEnd) return;
    const uint32_t* c = cases + (size_t)ci * MC_WORDS;
    const uint32_t src = c[0], xOff = c[1], xLen = c[2], yLen = c[4], maxED = c[5], nZeros = c[6], nInit = c[7], increase = c[9];
    const uint8_t* Y = yPool + c[3];
    const uint16_t* raw = rawPool + c[8];
    MatRow* out = rows + c[10];
    MatGeom g;
    W HP, HN, RAC, D0 = 0;
    uint32_t score;
    if (P::IN_TEXT) inTextStart<P>(g, xLen, maxED, nZeros, HP, HN, RAC, score);
    else
        initMatrix<P::LEFT, P::DIAG, W>(g, xLen, maxED, raw[0] + increase, raw[nInit - 1] + increase, raw, increase, nInit, HP, HN, RAC, score);
    const uint32_t nRows = min(min(yLen, g.m - 1u), c[11]);
    uint32_t done = 0;
    for (uint32_t i = 1; i <= nRows; i++) {
        const uint32_t code = Y[i - 1];
        const W M = code < 4u ? P::mword(S.of(src, code), xOff, xLen, i) : (W)0;
        const bool valid = P::row(g, i, M, HP, HN, D0, RAC, score);
        MatRow r;
        r.verdict = valid;
        r.ovgl = P::IN_TEXT ? 0 : P::ovgl(g, i, HN);
        r.score = (uint16_t)score;
        r.rac = (uint16_t)racIndex(RAC);
        const uint32_t fc = g.firstColumn(i), lc = min(g.n - 1u, i + g.Wh);
        uint32_t nc = 0;
        for (uint32_t t = 0; t < ROW_CELLS; t++) {
            uint32_t v = 0;
            if (fc + t <= lc) {
                v = min(P::cell(i, fc + t, HP, HN, score), 255u);
                nc = t + 1;
            }
            r.cells[t] = (uint8_t)v;
        }
        r.nCells = (uint16_t)nc;
        out[i - 1] = r;
        done = i;
        if (!valid) break;
    }
    rowsDone[ci] = done;
}

__global__ void __launch_bounds__(256)
k_words(Strings S, const uint32_t* __restrict__ queries, uint32_t nQ, uint64_t* __restrict__ res) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nQ) return;
    const uint32_t* q = queries + (size_t)qi * WQ_WORDS;
    const uint32_t kind = q[0], xOff = q[2], xLen = q[3], a = q[5];
    const uint32_t* Gc = S.of(q[1], q[4]);
    uint64_t w = 0;
    switch (kind) {
    case 0: w = matchWord<MX_LEFT, MX_BLOCK>(Gc, xOff, xLen, a); break;
    case 1: w = matchWord<MXF_LEFT>(Gc, xOff, xLen, a); break;
    case 2: w = matchWord<MXN_LEFT, MXN_BLOCK>(Gc, xOff, xLen, a); break;
    case 3: w = matchWord<MXY_LEFT, MXY_BLOCK>(Gc, xOff, xLen, a); break;
    case 4: w = matchWordW(matchWord<MXF_LEFT>(Gc, xOff, xLen, a / MX_BLOCK), a); break;
    case 5: w = matchWord32(matchWord<MXF_LEFT>(Gc, xOff, xLen, a / MX_BLOCK), a); break;
    case 6: w = matchWordSmall(matchWord<MX_LEFT, MX_BLOCK>(Gc, xOff, xLen, a / MX_BLOCK), a); break;
    default: w = ~0ull;
    }
    res[qi] = w;
}

// forward pass as forwardPass<STORE = true> runs it (the row of InTextMx<NARROW>, packed with M | ~D0, stored through traceLine), then
// walkToColumn0 from every final-column row whose cell is at most maxED, with the readers and LDS windows k_cigar gives it
template <bool NARROW>
__global__ void __launch_bounds__(256)
k_trace(Strings S, const uint32_t* __restrict__ cases, uint32_t nCases, const uint8_t* __restrict__ yPool, VPlanes V,
        uint16_t* __restrict__ walks, uint32_t* __restrict__ nWalksOut, uint32_t* __restrict__ validOut) {
    __shared__ uint64_t wW[NARROW ? 1 : TBW][256];
    __shared__ uint32_t wN[NARROW ? TBN : 1][256];
    typedef InTextBlockWords<NARROW> P;
    typedef typename P::W W;
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x, tid = threadIdx.x;
    if (slot >= nCases) return; // (no barrier below: every lane works on its own column of the LDS windows)
    const uint32_t* c = cases + (size_t)slot * TC_WORDS;
    const uint32_t src = c[0], xLen = c[1], yLen = c[3], maxED = c[4], nZeros = c[5];
    const uint8_t* Y = yPool + c[2];
    MatGeom g;
    W HP, HN, RAC, D0 = 0;
    uint32_t score;
    inTextStart<P>(g, xLen, maxED, nZeros, HP, HN, RAC, score);
    constexpr uint32_t GROUP = NARROW ? TBN : TBW;
    const uint32_t size = min(min(yLen, g.m - 1u), V.lines * GROUP), firstFinal = g.m - g.sfc(), col = g.n - 1;
    uint64_t startMask = 0; // final-column rows firstFinal + t whose cell is at most maxED
    if (firstFinal == 0 && P::cell(0, col, HP, HN, score) <= maxED) startMask |= 1ull;
    uint32_t valid = 0;
    for (uint32_t r = 1; r <= size; r++) {
        const uint32_t code = Y[r - 1];
        const W M = code < 4u ? P::mword(S.of(src, code), 0u, xLen, r) : (W)0;
        const bool ok = P::row(g, r, M, HP, HN, D0, RAC, score);
        uint4* L = traceLine(V, slot, (r - 1) / GROUP);
        if (NARROW) reinterpret_cast<uint32_t*>(L)[(r - 1) % GROUP] = packTraceRowNarrow(r, (uint32_t)HP, (uint32_t)(M | ~D0));
        else reinterpret_cast<uint64_t*>(L)[(r - 1) % GROUP] = packTraceRow(r, (uint64_t)HP, (uint64_t)(M | ~D0));
        if (!ok) break;
        valid = r;
        if (r >= firstFinal && r - firstFinal < 64u && P::cell(r, col, HP, HN, score) <= maxED) startMask |= 1ull << (r - firstFinal);
    }
    validOut[slot] = valid;
    uint32_t nW = 0;
    for (uint32_t t = 0; t < 64u && nW < MAX_WALKS; t++) {
        if (!((startMask >> t) & 1ull)) continue;
        uint16_t* rec = walks + ((size_t)slot * MAX_WALKS + nW) * WALK_WORDS;
        uint32_t ti = firstFinal + t, tj = col, flags = 0;
        CigarRuns runs{rec + 4, WALK_STRIDE};
        auto sink = [&](uint32_t op) { runs.emit(op); };
        if constexpr (NARROW) walkToColumn0(NarrowLineRows{wN, V, slot, tid}, ti, tj, flags, sink);
        else walkToColumn0(WideLineRows{wW, V, slot, tid}, ti, tj, flags, sink);
        const uint32_t nOps = runs.finish(flags);
        rec[0] = (uint16_t)(firstFinal + t);
        rec[1] = (uint16_t)ti;
        rec[2] = (uint16_t)nOps;
        rec[3] = (uint16_t)flags;
        nW++;
    }
    nWalksOut[slot] = nW;
}

// ---- host ----
template <typename T>
static std::vector<T> readArray(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "matrix_probe: case file too short\n");
        exit(2);
    }
    return v;
}
template <typename T>
static T* toDevice(const std::vector<T>& v, size_t extra = 0) { // (never an empty allocation; `extra` zeroed elements of padding)
    T* d = nullptr;
    const size_t bytes = (v.size() + extra + 1) * sizeof(T);
    HIP_OK(hipMalloc(&d, bytes));
    HIP_OK(hipMemset(d, 0, bytes));
    if (!v.empty()) HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T>
static T* zeroed(size_t n) {
    T* d = nullptr;
    HIP_OK(hipMalloc(&d, (n + 1) * sizeof(T)));
    HIP_OK(hipMemset(d, 0, (n + 1) * sizeof(T)));
    return d;
}
template <typename T>
static void writeBack(FILE* f, const T* d, size_t n) {
    std::vector<T> v(n);
    if (n) HIP_OK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    if (n && fwrite(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "matrix_probe: cannot write the result file\n");
        exit(2);
    }
}
static void launched(const char* what) { // a launch error or a fault ends the program here
    const hipError_t e1 = hipGetLastError();
    const hipError_t e2 = e1 == hipSuccess ? hipDeviceSynchronize() : e1;
    if (e2 != hipSuccess) {
        fprintf(stderr, "matrix_probe: %s: %s\n", what, hipGetErrorString(e2));
        exit(1);
    }
}
template <class P>
static void runMatrix(const Header& h, uint32_t geo, Strings S, const uint32_t* dCases, const uint8_t* dY, const uint16_t* dRaw, MatRow* dRows,
                      uint32_t* dDone) {
    const uint32_t b = (uint32_t)h.geoBegin[geo], e = (uint32_t)h.geoBegin[geo + 1];
    if (e <= b) return;
    hipLaunchKernelGGL(k_matrix<P>, dim3((e - b + 255) / 256), dim3(256), 0, 0, S, dCases, b, e, dY, dRaw, dRows, dDone);
    launched("k_matrix");
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: matrix_probe <case file> <result file>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "matrix_probe: cannot open %s\n", argv[1]);
        return 2;
    }
    const Header h = readArray<Header>(f, 1)[0];
    if (h.magic != 0x45424f5250424d43ull) {
        fprintf(stderr, "matrix_probe: not a case file\n");
        return 2;
    }
    const auto srcs = readArray<uint32_t>(f, 2 * h.nSrc);
    const auto pool = readArray<uint8_t>(f, h.poolBytes);
    const auto mcases = readArray<uint32_t>(f, (size_t)MC_WORDS * h.nMat);
    const auto ypool = readArray<uint8_t>(f, h.yBytes);
    const auto raws = readArray<uint16_t>(f, h.nRaw);
    const auto wq = readArray<uint32_t>(f, (size_t)WQ_WORDS * h.nWordQ);
    const auto tcN = readArray<uint32_t>(f, (size_t)TC_WORDS * h.nTrace[0]);
    const auto tcW = readArray<uint32_t>(f, (size_t)TC_WORDS * h.nTrace[1]);
    fclose(f);

    // bounds of everything a kernel indexes with a value from the file: checked here, once
    auto bad = [](const char* what) {
        fprintf(stderr, "matrix_probe: case file inconsistent: %s\n", what);
        exit(2);
    };
    for (uint64_t s = 0; s < h.nSrc; s++)
        if ((uint64_t)srcs[2 * s] + srcs[2 * s + 1] > h.poolBytes) bad("source");
    if (h.geoBegin[0] != 0 || h.geoBegin[N_GEO] != h.nMat) bad("geometry ranges");
    for (uint32_t g = 0; g < N_GEO; g++)
        if (h.geoBegin[g] > h.geoBegin[g + 1]) bad("geometry ranges");
    for (uint64_t i = 0; i < h.nMat; i++) {
        const uint32_t* c = &mcases[i * MC_WORDS];
        if (c[0] >= h.nSrc || (uint64_t)c[1] + c[2] > srcs[2 * c[0] + 1] || (uint64_t)c[3] + c[4] > h.yBytes || c[7] < 1 ||
            (uint64_t)c[8] + c[7] > std::max<uint64_t>(h.nRaw, 1) || (uint64_t)c[10] + c[11] > h.matRows || c[6] < 1 || c[6] > 2 * c[5] + 1)
            bad("matrix case");
        static const uint32_t geoMaxED[N_GEO] = {MX_MAX_ED, MX32_MAX_ED, MXW_MAX_ED, 10, MXN_MAX_ED, MXN_MAX_ED, MXS_MAX_ED};
        uint32_t g = 0;
        while (i >= h.geoBegin[g + 1]) g++;
        if (c[5] > geoMaxED[g] || c[7] > 64) bad("matrix case: maxED of its geometry");
    }
    for (uint64_t i = 0; i < h.nWordQ; i++) {
        const uint32_t* q = &wq[i * WQ_WORDS];
        if (q[1] >= h.nSrc || (uint64_t)q[2] + q[3] > srcs[2 * q[1] + 1] || q[4] > 3 || q[5] > 4096) bad("word query");
    }
    for (int w = 0; w < 2; w++) {
        const auto& tc = w ? tcW : tcN;
        for (uint64_t i = 0; i < h.nTrace[w]; i++) {
            const uint32_t* c = &tc[i * TC_WORDS];
            if (c[0] >= h.nSrc || c[1] != srcs[2 * c[0] + 1] || (uint64_t)c[2] + c[3] > h.yBytes || c[4] < 1 || c[4] > (w ? 7u : 4u) || c[5] < 1 ||
                c[5] > 2 * c[4] + 1 || c[1] + 4 * c[4] + 2 > 0xFFFFu)
                bad("trace case");
        }
    }

    // the bit-strings of every source, as k_prep writes a read's: bit j of string ch <=> character j is nucleotide ch; gWords words, zero padded
    std::vector<uint64_t> gOff(h.nSrc);
    std::vector<uint32_t> gw(h.nSrc);
    uint64_t total = 0;
    for (uint64_t s = 0; s < h.nSrc; s++) {
        gw[s] = gWords(srcs[2 * s + 1]);
        gOff[s] = total;
        total += 4ull * gw[s];
    }
    std::vector<uint32_t> G(total, 0u);
    for (uint64_t s = 0; s < h.nSrc; s++)
        for (uint32_t j = 0; j < srcs[2 * s + 1]; j++) {
            const uint8_t ch = pool[srcs[2 * s] + j];
            if (ch < 4) G[gOff[s] + (size_t)ch * gw[s] + j / 32] |= 1u << (j % 32);
        }
    Strings S{toDevice(G, 8), toDevice(gOff), toDevice(gw)};
    const uint8_t* dY = toDevice(ypool);
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "matrix_probe: cannot open %s\n", argv[2]);
        return 2;
    }

    { // stage `matrix`
        const uint32_t* dCases = toDevice(mcases);
        const uint16_t* dRaw = toDevice(raws);
        MatRow* dRows = zeroed<MatRow>(h.matRows);
        uint32_t* dDone = zeroed<uint32_t>(h.nMat);
        runMatrix<InIndex<MxRef64>>(h, 0, S, dCases, dY, dRaw, dRows, dDone);
        runMatrix<InTextBlockWords<true>>(h, 1, S, dCases, dY, dRaw, dRows, dDone);
        runMatrix<InTextBlockWords<false>>(h, 2, S, dCases, dY, dRaw, dRows, dDone);
        runMatrix<InTextWide<MXX_BLOCK, MXX_DIAG, MXX_LEFT>>(h, 3, S, dCases, dY, dRaw, dRows, dDone);
        runMatrix<InTextWide<MXY_BLOCK, MXY_DIAG, MXY_LEFT>>(h, 4, S, dCases, dY, dRaw, dRows, dDone);
        runMatrix<InIndex<MxNarrow>>(h, 5, S, dCases, dY, dRaw, dRows, dDone);
        runMatrix<InIndex<MxSmall32>>(h, 6, S, dCases, dY, dRaw, dRows, dDone);
        writeBack(out, dDone, h.nMat);
        writeBack(out, dRows, h.matRows);
    }
    { // stage `words`
        const uint32_t* dQ = toDevice(wq);
        uint64_t* dRes = zeroed<uint64_t>(h.nWordQ);
        if (h.nWordQ) {
            hipLaunchKernelGGL(k_words, dim3((uint32_t)((h.nWordQ + 255) / 256)), dim3(256), 0, 0, S, dQ, (uint32_t)h.nWordQ, dRes);
            launched("k_words");
        }
        writeBack(out, dRes, h.nWordQ);
    }
    for (int w = 0; w < 2; w++) { // stage `trace`: narrow rows, wide rows
        const auto& tc = w ? tcW : tcN;
        const uint32_t n = (uint32_t)h.nTrace[w], nSlots = (n + 255u) / 256u * 256u;
        const uint32_t* dC = toDevice(tc);
        VPlanes V{zeroed<uint64_t>((size_t)h.traceLines[w] * nSlots * 8), nSlots, (uint32_t)h.traceLines[w]};
        uint16_t* dWalks = zeroed<uint16_t>((size_t)n * MAX_WALKS * WALK_WORDS);
        uint32_t* dN = zeroed<uint32_t>(n);
        uint32_t* dValid = zeroed<uint32_t>(n);
        if (n) {
            if (w) hipLaunchKernelGGL(k_trace<false>, dim3(nSlots / 256), dim3(256), 0, 0, S, dC, n, dY, V, dWalks, dN, dValid);
            else hipLaunchKernelGGL(k_trace<true>, dim3(nSlots / 256), dim3(256), 0, 0, S, dC, n, dY, V, dWalks, dN, dValid);
            launched("k_trace");
        }
        writeBack(out, dN, n);
        writeBack(out, dValid, n);
        writeBack(out, dWalks, (size_t)n * MAX_WALKS * WALK_WORDS);
    }
    if (fclose(out) != 0) return 2;
    return 0;
}
