// The device index builder behind cmb_build_* (include/columba_amd.h): from the preprocessed text to a suffix array of the text and of
// the reversed text, to the Vanilla index arrays in the reference's layouts, and — without a round trip through host arrays — to a
// resident cmb_index (indexFromDeviceArrays, columba_amd.hip).  The kernels and the algorithm: dev_build.hpp.
//
// MEMORY.  While a suffix array is sorted the build holds, per text character: the text (1 byte), two 64-bit key buffers (16), two
// 32-bit value buffers, one of which becomes the suffix array (8), the ranks (4), two lists of open rows (8) and the open flags (1):
// 38 bytes.  The second pass (the reversed text) runs after the first has released all but its suffix array (4) and its derived arrays
// (bitvectors 1/2, counts 1/8, 3-bit BWT 3/8: 1 byte), so the peak is 43 bytes per character plus rocPRIM's scratch (histograms and
// look-back states: a few MB).  cmb_build_create checks that against hipMemGetInfo before it allocates anything.
// LENGTH.  n < 2^32 - 1 as everywhere on the FM-index path.  rocPRIM's radix sort, scans and selections take a size_t length: the
// radix sort (device_radix_sort.hpp, radix_sort_onesweep_iteration) works through batches of 2^30 items with 64-bit offsets, the scan
// and the selection through chunks of their size_limit, so lengths of 2^31 and beyond need no split here.  That was verified by
// reading the headers of rocPRIM 7.2; tools/build_bench.py compares a build at 3.0 * 10^9 characters with the harness builder.
//
// THE B-MOVE INDEX (cmb_build_move_*; kernels and algorithm: dev_move_build.hpp).  The first call derives, one direction after the other,
// the run table, the samples and, for the text, the predecessors and the PLCP's run form, and keeps them in the handle: 56 bytes per
// run (88 for the text's direction) and 16 per PLCP run.  While it works it holds 2 bytes per character (the BWT bytes and the
// run-start flags, gone once the runs are known) and at most 256 bytes per run (starts, run lengths and their sums, sort keys and values
// in and out, the open pairs, rocPRIM's scratch); both needs are compared with hipMemGetInfo before the allocation, and so are the packed
// rows of a download (at most 16 bytes per run, allocated per call).  Host
// synchronisations per direction: the number of runs, and for the text the number of pairs the wavefront pass takes and the number of
// PLCP runs.
#include "dev_move_build.hpp"
#include "units.hpp"

#include <chrono>
#include <memory>
#include <utility>

#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

using namespace cmb;

static int fail(int code, const std::string& msg) { return failWith(code, msg); }

struct cmb_build {
    int device = 0;
    uint64_t n = 0;
    DevBuf<uint8_t> text;      // ASCII, as given
    DevBuf<uint32_t> saF, saR; // suffix arrays of the text and of the reversed text
    DevBuf<uint64_t> bvF, cntF, bvR, cntR, bwt3;
    uint64_t dollarF = 0, dollarR = 0;
    uint64_t hist[5] = {0, 0, 0, 0, 0}; // how often every code occurs
    DevBuf<uint8_t> tmp;                // rocPRIM's scratch
    std::vector<std::pair<std::string, double>> times;
    // cmb_build_move_*: the O(runs) arrays of the b-move index, derived on first use
    struct MoveSide {
        uint64_t runs = 0, zeroPos = 0;
        DevBuf<uint64_t> run; // {head, start row, LF of the start row, the run that holds it} per run
        DevBuf<uint64_t> smpF, smpL;
    } mv[2]; // the text, the reversed text
    DevBuf<uint64_t> predFirst, firstToRun, predLast, lastToRun, plcpPos, plcpSum;
    bool moveDone = false;
};

namespace {
constexpr uint64_t BLD_BYTES_PER_CHAR = 43; // (above)
struct Sampled {                            // the rows a sparse suffix array keeps
    uint32_t mask;
    __host__ __device__ bool operator()(const uint32_t& v) const { return (v & mask) == 0; }
};
struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() { // (every phase ends in a synchronise)
        HIPCHK(hipDeviceSynchronize());
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};
constexpr uint32_t BLD_GRID = 1u << 16;
// one lane per row and trip under the test cap
template <typename... KA, typename... A> void rowLaunch(void (*kern)(KA...), const char* name, uint64_t items, A... args) {
    if (!items) return;
    const uint32_t grid = capBlocks((uint32_t)std::min<uint64_t>((items + BLD_BLOCK - 1) / BLD_BLOCK, BLD_GRID));
    gridLine(getenv("CMB_VERBOSE") != nullptr, name, items, (uint64_t)grid * BLD_BLOCK);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(BLD_BLOCK), 0, 0, args...);
    HIPCHK(hipGetLastError());
}
// one lane per item, no loop
template <typename... KA, typename... A> void itemLaunch(void (*kern)(KA...), uint64_t items, A... args) {
    if (!items) return;
    hipLaunchKernelGGL(kern, dim3((unsigned)((items + BLD_BLOCK - 1) / BLD_BLOCK)), dim3(BLD_BLOCK), 0, 0, args...);
    HIPCHK(hipGetLastError());
}
template <typename T> void moveBuf(DevBuf<T>& from, DevBuf<T>& to) {
    to.release();
    std::swap(from.p, to.p);
    std::swap(from.n, to.n);
}
uint32_t bitsOf(uint64_t v) { // how many bits hold the values 0 .. v
    uint32_t b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}
uint64_t readWord(const uint64_t* d) {
    uint64_t v = 0;
    HIPCHK(hipMemcpy(&v, d, sizeof(v), hipMemcpyDeviceToHost));
    return v;
}

// the suffix array of the text (rev: of the reversed text) into `sa`
void suffixArrayOnDevice(cmb_build* b, bool rev, DevBuf<uint32_t>& sa) {
    const uint64_t n = b->n;
    const std::string tag = rev ? "rev: " : "fwd: ";
    const hipStream_t s0 = nullptr;
    Clock clk;
    DevBuf<uint64_t> keyA, keyB, count;
    DevBuf<uint32_t> valA, valB, rank, rowsA, rowsB;
    DevBuf<uint8_t> open;
    keyA.alloc(n), keyB.alloc(n), valA.alloc(n), valB.alloc(n), rank.alloc(n), rowsA.alloc(n), rowsB.alloc(n), open.alloc(n), count.alloc(1);
    rowLaunch(k_bld_key20, "k_bld_key20", n, (const uint8_t*)b->text.p, n, rev, keyA.p, valA.p);
    rocprim::double_buffer<uint64_t> keys(keyA.p, keyB.p);
    rocprim::double_buffer<uint32_t> vals(valA.p, valB.p);
    withScratch(b->tmp, [&](void* p, size_t& bytes) { return rocprim::radix_sort_pairs(p, bytes, keys, vals, (size_t)n, 0u, 3u * BLD_KEY_SYMBOLS, s0); });
    if (vals.current() != valA.p) std::swap(valA.p, valB.p); // valA: the suffix array from here on; valB: values of the rounds' sorts
    uint32_t* const saP = valA.p;
    uint32_t* rows = nullptr; // the open rows that were sorted last, in row order; nullptr: every row
    uint32_t* rowsNext = rowsA.p;
    uint64_t m = n, h = BLD_KEY_SYMBOLS;
    // heads, ranks and the next list of open rows from the m entries keys.current() / vals.current() hold after a sort (the group heads
    // lie in the key buffer the sort has left free)
    auto settle = [&]() {
        uint32_t* head = (uint32_t*)keys.alternate();
        rowLaunch(k_bld_heads, "k_bld_heads", m, (const uint64_t*)keys.current(), (const uint32_t*)rows, m, head);
        withScratch(b->tmp, [&](void* p, size_t& bytes) { return rocprim::inclusive_scan(p, bytes, head, head, (size_t)m, rocprim::maximum<uint32_t>(), s0); });
        rowLaunch(k_bld_ranks, "k_bld_ranks", m, (const uint32_t*)vals.current(), (const uint32_t*)head, (const uint32_t*)rows, m, saP, rank.p, open.p);
        if (rows)
            withScratch(b->tmp, [&](void* p, size_t& bytes) { return rocprim::select(p, bytes, rows, open.p, rowsNext, count.p, (size_t)m, s0); });
        else
            withScratch(b->tmp, [&](void* p, size_t& bytes) {
                return rocprim::select(p, bytes, rocprim::counting_iterator<uint32_t>(0), open.p, rowsNext, count.p, (size_t)m, s0);
            });
        m = readWord(count.p);
        rows = rowsNext;
        rowsNext = rows == rowsA.p ? rowsB.p : rowsA.p;
    };
    settle();
    b->times.push_back({tag + "sort of 20 symbols, " + std::to_string(m) + " rows stay open", clk.lap()});
    const uint32_t keyBits = 32u + bitsOf(n);
    while (m) {
        // the open rows by (rank, rank h positions on); their values are sorted between valB and the list of open rows that is not in use
        // (the selection writes it only after k_bld_ranks has read the values)
        keys = rocprim::double_buffer<uint64_t>(keyA.p, keyB.p);
        vals = rocprim::double_buffer<uint32_t>(valB.p, rowsNext);
        const uint64_t sorted = m;
        rowLaunch(k_bld_round_keys, "k_bld_round_keys", m, (const uint32_t*)rows, m, (const uint32_t*)saP, (const uint32_t*)rank.p, n, h, keys.current(),
                  vals.current());
        withScratch(b->tmp, [&](void* p, size_t& bytes) { return rocprim::radix_sort_pairs(p, bytes, keys, vals, (size_t)m, 0u, keyBits, s0); });
        settle();
        b->times.push_back({tag + "round h=" + std::to_string(h) + ", " + std::to_string(sorted) + " rows sorted, " + std::to_string(m) + " stay open", clk.lap()});
        h *= 2;
    }
    moveBuf(valA, sa);
}

// K interleaved bitvectors of nWords words each -> their rank9 counts (cw words, zero where rankCounts leaves none)
template <uint32_t K> void rankCountsOnDevice(cmb_build* b, const uint64_t* words, uint64_t nWords, uint64_t nBlocks, uint64_t cw, uint64_t* counts) {
    HIPCHK(hipMemset(counts, 0, std::max<uint64_t>(cw, 1) * sizeof(uint64_t)));
    if (!nBlocks) return;
    DevBuf<uint64_t> tot;
    tot.alloc(nBlocks * K);
    itemLaunch(k_bld_block_counts<K>, nBlocks * K, words, nWords, nBlocks, cw, counts, tot.p);
    for (uint32_t k = 0; k < K; k++) scanExclusive(b->tmp, tot.p + k * nBlocks, tot.p + k * nBlocks, (size_t)nBlocks, nullptr);
    itemLaunch(k_bld_block_starts<K>, nBlocks * K, (const uint64_t*)tot.p, nBlocks, cw, counts);
}

// BWT, bitvectors and counts of one direction; the 3-bit BWT of the forward one
void deriveBwtArrays(cmb_build* b, bool rev) {
    const uint64_t n = b->n, N = n + 1, nw = (N + 63) / 64, nblk = (N + 511) / 512;
    DevBuf<uint8_t> bwt;
    DevBuf<uint64_t> dollar;
    bwt.alloc(n), dollar.alloc(1);
    HIPCHK(hipMemcpy(dollar.p, &n, sizeof(uint64_t), hipMemcpyHostToDevice)); // (bwtBitvectors: n where there is none)
    rowLaunch(k_bld_bwt, "k_bld_bwt", n, (const uint8_t*)b->text.p, n, (const uint32_t*)(rev ? b->saR.p : b->saF.p), rev, bwt.p,
              (unsigned long long*)dollar.p);
    (rev ? b->dollarR : b->dollarF) = readWord(dollar.p);
    DevBuf<uint64_t>& bv = rev ? b->bvR : b->bvF;
    DevBuf<uint64_t>& cnt = rev ? b->cntR : b->cntF;
    bv.alloc(nw * 4), cnt.alloc(nblk * 8);
    rowLaunch(k_bld_bitvectors, "k_bld_bitvectors", nw * 64, (const uint8_t*)bwt.p, n, nw, bv.p);
    rankCountsOnDevice<4>(b, bv.p, nw, nblk, nblk * 8, cnt.p);
    if (!rev) {
        const uint64_t w3 = n * 3 / 64 + 1;
        b->bwt3.alloc(w3);
        itemLaunch(k_bld_pack3, w3, (const uint8_t*)bwt.p, n, w3, b->bwt3.p);
    }
    HIPCHK(hipDeviceSynchronize());
}

struct SparseSizes {
    uint64_t bvWords, cntWords, nSamples;
};
SparseSizes sparseSizes(uint64_t n, uint32_t s) {
    const uint64_t nw = (n + 63) / 64;
    return {nw, (nw + 7) / 4, (n + s - 1) / s};
}
// sparseSuffixArray on the device: the sampled-row bitvector, its counts and the samples in row order (a stable selection)
void sparseOnDevice(cmb_build* b, uint32_t s, DevBuf<uint64_t>& bv, DevBuf<uint64_t>& cnt, DevBuf<uint32_t>& samples) {
    const uint64_t n = b->n;
    const SparseSizes z = sparseSizes(n, s);
    bv.alloc(z.bvWords), cnt.alloc(z.cntWords), samples.alloc(z.nSamples);
    rowLaunch(k_bld_sa_mark, "k_bld_sa_mark", z.bvWords * 64, (const uint32_t*)b->saF.p, n, s - 1u, z.bvWords, bv.p);
    rankCountsOnDevice<1>(b, bv.p, z.bvWords, (z.bvWords + 7) / 8, z.cntWords, cnt.p);
    DevBuf<uint64_t> count;
    count.alloc(1);
    withScratch(b->tmp, [&](void* p, size_t& bytes) {
        return rocprim::select(p, bytes, b->saF.p, samples.p, count.p, (size_t)n, Sampled{s - 1u}, (hipStream_t) nullptr);
    });
    if (readWord(count.p) != z.nSamples) throw std::runtime_error("the suffix array is no permutation of the text positions");
}
bool powerOfTwo(uint32_t s) { return s != 0 && (s & (s - 1)) == 0; }
int noDevice() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(CMB_ERR_DEVICE, "no HIP device available (the product path has no CPU fallback)");
    return CMB_OK;
}
template <typename T> void download(T* host, const DevBuf<T>& d, uint64_t count) {
    if (count) HIPCHK(hipMemcpy(host, d.p, count * sizeof(T), hipMemcpyDeviceToHost));
}

// ---- the b-move index
uint32_t ceilLog2(uint64_t v) { // moverepr.h:44-46 (build::bitsFor)
    uint32_t b = 0;
    while (b < 64 && (1ull << b) < v) b++;
    return b;
}
bool isPowerOfTwo(uint64_t n) { return (n & (n - 1)) == 0; }
const char* const MOVE_POWER_OF_TWO =
    "a text size that is a power of two cannot be packed into a move table (the terminating row's start position n does not fit "
    "ceil(log2 n) bits, moverepr.cpp:75-77)";
void needFree(uint64_t need, const std::string& what) {
    size_t freeB = 0, totalB = 0;
    HIPCHK(hipMemGetInfo(&freeB, &totalB));
    if (freeB < need)
        throw std::runtime_error("the move tables on the device need " + std::to_string(need) + " bytes for " + what + ", " + std::to_string(freeB) +
                                 " are free");
}
template <typename T> void copyBuf(const DevBuf<T>& from, DevBuf<T>& to, uint64_t count) {
    to.alloc(count);
    if (count) HIPCHK(hipMemcpy(to.p, from.p, count * sizeof(T), hipMemcpyDeviceToDevice));
}
constexpr uint64_t MVB_BYTES_PER_CHAR = 2, MVB_BYTES_PER_RUN = 256; // (above)

// the O(runs) arrays of one direction into the handle
void deriveMoveSide(cmb_build* b, bool rev) {
    const uint64_t n = b->n;
    const std::string tag = rev ? "move rev: " : "move fwd: ";
    const hipStream_t s0 = nullptr;
    cmb_build::MoveSide& m = b->mv[rev ? 1 : 0];
    const uint32_t* sa = rev ? b->saR.p : b->saF.p;
    Clock clk;
    needFree(n * MVB_BYTES_PER_CHAR + (64ull << 20), std::to_string(n) + " characters (" + std::to_string(MVB_BYTES_PER_CHAR) + " per character)");
    DevBuf<uint8_t> bwt, flag;
    DevBuf<uint64_t> word, starts;
    bwt.alloc(n), flag.alloc(n), word.alloc(2);
    HIPCHK(hipMemset(word.p, 0, 2 * sizeof(uint64_t)));
    rowLaunch(k_bld_bwt, "k_bld_bwt", n, (const uint8_t*)b->text.p, n, sa, rev, bwt.p, (unsigned long long*)(word.p + 1));
    rowLaunch(k_mvb_flags, "k_mvb_flags", n, (const uint8_t*)bwt.p, n, flag.p, (unsigned long long*)word.p);
    const uint64_t r = readWord(word.p);
    needFree(r * MVB_BYTES_PER_RUN + (64ull << 20), std::to_string(r) + " runs (" + std::to_string(MVB_BYTES_PER_RUN) + " per run)");
    starts.alloc(r), m.run.alloc(4 * r), m.smpF.alloc(r), m.smpL.alloc(r);
    withScratch(b->tmp, [&](void* p, size_t& bytes) {
        return rocprim::select(p, bytes, rocprim::counting_iterator<uint64_t>(0), flag.p, starts.p, word.p + 1, (size_t)n, s0);
    });
    rowLaunch(k_mvb_heads, "k_mvb_heads", r, (const uint8_t*)bwt.p, sa, (const uint64_t*)starts.p, r, n, m.run.p, m.smpF.p, m.smpL.p);
    HIPCHK(hipDeviceSynchronize());
    bwt.release(), flag.release();
    b->times.push_back({tag + "run starts, heads and samples of " + std::to_string(r) + " runs", clk.lap()});
    {
        DevBuf<uint32_t> len, before;
        len.alloc(r), before.alloc(r);
        uint64_t cum = b->hist[0];
        for (uint32_t c = 1; c <= 4; c++) {
            rowLaunch(k_mvb_lens, "k_mvb_lens", r, (const uint64_t*)m.run.p, (const uint64_t*)starts.p, r, n, c, len.p);
            scanExclusive(b->tmp, (const uint32_t*)len.p, before.p, (size_t)r, s0);
            rowLaunch(k_mvb_lf, "k_mvb_lf", r, (const uint32_t*)before.p, r, c, cum, m.run.p);
            cum += b->hist[c];
        }
        rowLaunch(k_mvb_out_run, "k_mvb_out_run", r, (const uint64_t*)starts.p, r, m.run.p);
        HIPCHK(hipDeviceSynchronize());
    }
    m.runs = r, m.zeroPos = rev ? b->dollarR : b->dollarF;
    b->times.push_back({tag + "LF of the run starts and their runs", clk.lap()});
    if (rev) return;
    const uint32_t keyBits = bitsOf(n - 1);
    auto predecessors = [&](const DevBuf<uint64_t>& smp, DevBuf<uint64_t>& marked, DevBuf<uint64_t>& toRun) {
        DevBuf<uint64_t> key, val;
        key.alloc(r), val.alloc(r), marked.alloc(r), toRun.alloc(r);
        rowLaunch(k_mvb_pred_keys, "k_mvb_pred_keys", r, (const uint64_t*)smp.p, r, n, key.p, val.p);
        withScratch(b->tmp, [&](void* p, size_t& bytes) {
            return rocprim::radix_sort_pairs(p, bytes, key.p, marked.p, val.p, toRun.p, (size_t)r, 0u, keyBits, s0);
        });
        HIPCHK(hipDeviceSynchronize());
    };
    predecessors(m.smpF, b->predFirst, b->firstToRun);
    predecessors(m.smpL, b->predLast, b->lastToRun);
    b->times.push_back({tag + "predecessors", clk.lap()});
    DevBuf<uint64_t> sum, posSorted, sumSorted;
    DevBuf<uint32_t> open, nOpen;
    sum.alloc(r), open.alloc(r), nOpen.alloc(1);
    HIPCHK(hipMemset(nOpen.p, 0, sizeof(uint32_t)));
    rowLaunch(k_mvb_lcp_prefix, "k_mvb_lcp_prefix", r, (const uint8_t*)b->text.p, n, sa, (const uint64_t*)starts.p, r, sum.p, open.p, nOpen.p);
    uint32_t mOpen = 0;
    HIPCHK(hipMemcpy(&mOpen, nOpen.p, sizeof(mOpen), hipMemcpyDeviceToHost));
    rowLaunch(k_mvb_lcp_wave, "k_mvb_lcp_wave", (uint64_t)mOpen * 64, (const uint8_t*)b->text.p, n, sa, (const uint64_t*)starts.p,
              (const uint32_t*)open.p, (uint64_t)mOpen, sum.p);
    b->times.push_back({tag + "PLCP at " + std::to_string(r) + " run starts, " + std::to_string(mOpen) + " by a wavefront each", clk.lap()});
    open.release();
    posSorted.alloc(r), sumSorted.alloc(r);
    withScratch(b->tmp, [&](void* p, size_t& bytes) {
        return rocprim::radix_sort_pairs(p, bytes, m.smpF.p, posSorted.p, sum.p, sumSorted.p, (size_t)r, 0u, keyBits, s0);
    });
    DevBuf<uint8_t> keep;
    keep.alloc(r);
    rowLaunch(k_mvb_plcp_keep, "k_mvb_plcp_keep", r, (const uint64_t*)sumSorted.p, r, keep.p);
    withScratch(b->tmp, [&](void* p, size_t& bytes) { return rocprim::select(p, bytes, posSorted.p, keep.p, sum.p, word.p, (size_t)r, s0); });
    const uint64_t nPlcp = readWord(word.p);
    copyBuf(sum, b->plcpPos, nPlcp);
    withScratch(b->tmp, [&](void* p, size_t& bytes) { return rocprim::select(p, bytes, sumSorted.p, keep.p, sum.p, word.p, (size_t)r, s0); });
    HIPCHK(hipDeviceSynchronize());
    copyBuf(sum, b->plcpSum, nPlcp);
    b->times.push_back({tag + "PLCP run form, " + std::to_string(nPlcp) + " runs", clk.lap()});
}
// selects the handle's device (every cmb_build_move_* call works on it, the later ones too) and derives on first use
void deriveMove(cmb_build* b) {
    HIPCHK(hipSetDevice(b->device));
    if (b->moveDone) return;
    const size_t phases = b->times.size();
    try {
        deriveMoveSide(b, false);
        deriveMoveSide(b, true);
    } catch (...) { // a later call derives again: its phases must not stand beside those of the attempt that failed
        b->times.resize(phases);
        throw;
    }
    b->tmp.release();
    b->moveDone = true;
}
uint64_t lfbpBytes(uint64_t n, uint64_t r, uint32_t lengthBits) {
    return 3 * (uint64_t)(lengthBits / 8) + (uint64_t)((3 + 2 * ceilLog2(n) + ceilLog2(r) + 7) / 8) * (r + 1);
}
// the image of a .LFBP file from a run table in HBM: the header from the host, the rows packed by k_mvb_pack
void packLfbp(const uint64_t* run, uint64_t n, uint64_t r, uint64_t zeroPos, uint32_t lengthBits, uint8_t* out) {
    const uint32_t bitsN = ceilLog2(n), bitsR = ceilLog2(r), rowBytes = (3 + 2 * bitsN + bitsR + 7) / 8;
    const size_t W = lengthBits / 8;
    needFree((uint64_t)rowBytes * (r + 1) + (64ull << 20), std::to_string(r + 1) + " packed rows (" + std::to_string(rowBytes) + " bytes each)");
    DevBuf<uint8_t> body;
    body.alloc((size_t)rowBytes * (r + 1));
    rowLaunch(k_mvb_pack, "k_mvb_pack", r + 1, run, r, n, bitsN, bitsR, rowBytes, body.p);
    const uint64_t hdr[3] = {n, r, zeroPos};
    for (int i = 0; i < 3; i++) memcpy(out + i * W, &hdr[i], W); // (little-endian, as MoveLFReprBP::write leaves them)
    HIPCHK(hipMemcpy(out + 3 * W, body.p, (size_t)rowBytes * (r + 1), hipMemcpyDeviceToHost));
}
void moveSizes(const cmb_build* b, uint32_t lengthBits, cmb_build_move_sizes* z) {
    z->text_length = b->n, z->runs = b->mv[0].runs, z->rev_runs = b->mv[1].runs;
    z->lfbp_bytes = lfbpBytes(b->n, z->runs, lengthBits), z->rev_lfbp_bytes = lfbpBytes(b->n, z->rev_runs, lengthBits);
    z->n_plcp = b->plcpPos.n;
}
} // namespace

extern "C" int cmb_build_create(const char* text, uint64_t n, int device, cmb_build** out) {
    if (!text || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (n == 0) return fail(CMB_ERR_INVALID, "the text is empty: it ends in '$'");
    if (n >= 0xFFFFFFFFull) return fail(CMB_ERR_UNSUPPORTED, "text length must fit a 32-bit length_t");
    if (int rc = noDevice()) return rc;
    try {
        HIPCHK(hipSetDevice(device));
        size_t freeB = 0, totalB = 0;
        HIPCHK(hipMemGetInfo(&freeB, &totalB));
        const uint64_t need = n * BLD_BYTES_PER_CHAR + (64ull << 20);
        if (freeB < need)
            return fail(CMB_ERR_DEVICE, "building the index of " + std::to_string(n) + " characters on the device needs " + std::to_string(need) +
                                            " bytes (" + std::to_string(BLD_BYTES_PER_CHAR) + " per character), " + std::to_string(freeB) + " are free");
        std::unique_ptr<cmb_build> b(new cmb_build());
        b->device = device, b->n = n;
        Clock clk;
        b->text.upload((const uint8_t*)text, n);
        { // what preprocessFastaFiles leaves: A, C, G, T and a final '$'
            DevBuf<uint32_t> bad;
            DevBuf<uint64_t> hist;
            bad.alloc(1), hist.alloc(5);
            HIPCHK(hipMemset(bad.p, 0, sizeof(uint32_t)));
            HIPCHK(hipMemset(hist.p, 0, 5 * sizeof(uint64_t)));
            rowLaunch(k_bld_check, "k_bld_check", n, (const uint8_t*)b->text.p, n, bad.p, (unsigned long long*)hist.p);
            uint32_t hb = 0;
            HIPCHK(hipMemcpy(&hb, bad.p, sizeof(hb), hipMemcpyDeviceToHost));
            if (hb)
                return fail(CMB_ERR_INVALID, std::to_string(hb) + " characters of the text are not upper-case A, C, G, T followed by one final '$'");
            HIPCHK(hipMemcpy(b->hist, hist.p, sizeof(b->hist), hipMemcpyDeviceToHost));
        }
        b->times.push_back({"upload and check", clk.lap()});
        for (int rev = 0; rev < 2; rev++) { // one pass after the other: the sort buffers of the first are gone before the second
            suffixArrayOnDevice(b.get(), rev != 0, rev ? b->saR : b->saF);
            clk.lap();
            deriveBwtArrays(b.get(), rev != 0);
            b->times.push_back({rev ? "rev: BWT, bitvectors, counts" : "fwd: BWT, bitvectors, counts, 3-bit BWT", clk.lap()});
        }
        *out = b.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" void cmb_build_destroy(cmb_build* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;
}
extern "C" int cmb_build_sizes_of(const cmb_build* b, cmb_build_sizes* out) {
    if (!b || !out) return fail(CMB_ERR_INVALID, "null argument");
    const uint64_t N = b->n + 1;
    out->text_length = b->n;
    out->bv_words = 4 * ((N + 63) / 64);
    out->cnt_words = 8 * ((N + 511) / 512);
    out->bwt_words = b->n * 3 / 64 + 1;
    return CMB_OK;
}
extern "C" int cmb_build_bwt_arrays(cmb_build* b, cmb_build_arrays* io, uint64_t* needed) {
    if (!b || !io || !io->bv_fwd || !io->cnt_fwd || !io->bv_rev || !io->cnt_rev || !io->bwt_words) return fail(CMB_ERR_INVALID, "null argument");
    cmb_build_sizes z;
    cmb_build_sizes_of(b, &z);
    if (io->bv_cap < z.bv_words || io->cnt_cap < z.cnt_words || io->bwt_cap < z.bwt_words) {
        if (needed) needed[0] = z.bv_words, needed[1] = z.cnt_words, needed[2] = z.bwt_words;
        return fail(CMB_ERR_OVERFLOW, "output buffers too small: " + std::to_string(z.bv_words) + " bitvector words, " + std::to_string(z.cnt_words) +
                                          " count words and " + std::to_string(z.bwt_words) + " words of 3-bit BWT are needed");
    }
    try {
        HIPCHK(hipSetDevice(b->device));
        download(io->bv_fwd, b->bvF, z.bv_words), download(io->cnt_fwd, b->cntF, z.cnt_words);
        download(io->bv_rev, b->bvR, z.bv_words), download(io->cnt_rev, b->cntR, z.cnt_words);
        download(io->bwt_words, b->bwt3, z.bwt_words);
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
    io->dollar_pos_fwd = b->dollarF, io->dollar_pos_rev = b->dollarR;
    uint64_t sum = 0;
    for (int c = 0; c < 5; c++) io->counts[c] = sum, sum += b->hist[c];
    for (int i = 0; i < 256; i++) io->char_counts[i] = 0;
    for (int c = 0; c < 5; c++) io->char_counts[(unsigned char)"$ACGT"[c]] = (uint32_t)b->hist[c];
    return CMB_OK;
}
extern "C" int cmb_build_sparse_sa_sizes(const cmb_build* b, uint32_t sparseness, uint64_t* bv_words, uint64_t* count_words, uint64_t* n_samples) {
    if (!b || !bv_words || !count_words || !n_samples) return fail(CMB_ERR_INVALID, "null argument");
    if (!powerOfTwo(sparseness)) return fail(CMB_ERR_INVALID, "suffix array sparseness must be a power of two");
    const SparseSizes z = sparseSizes(b->n, sparseness);
    *bv_words = z.bvWords, *count_words = z.cntWords, *n_samples = z.nSamples;
    return CMB_OK;
}
extern "C" int cmb_build_sparse_sa(cmb_build* b, uint32_t sparseness, uint64_t* bv, uint64_t bv_cap, uint64_t* counts, uint64_t count_cap,
                                   uint32_t* samples, uint64_t sample_cap, uint64_t* n_samples) {
    if (!b || !bv || !counts || !samples || !n_samples) return fail(CMB_ERR_INVALID, "null argument");
    if (!powerOfTwo(sparseness)) return fail(CMB_ERR_INVALID, "suffix array sparseness must be a power of two");
    const SparseSizes z = sparseSizes(b->n, sparseness);
    *n_samples = z.nSamples;
    if (bv_cap < z.bvWords || count_cap < z.cntWords || sample_cap < z.nSamples)
        return fail(CMB_ERR_OVERFLOW, "output buffers too small: " + std::to_string(z.bvWords) + " bitvector words, " + std::to_string(z.cntWords) +
                                          " count words and " + std::to_string(z.nSamples) + " samples are needed");
    try {
        HIPCHK(hipSetDevice(b->device));
        DevBuf<uint64_t> dBv, dCnt;
        DevBuf<uint32_t> dSamples;
        sparseOnDevice(b, sparseness, dBv, dCnt, dSamples);
        download(bv, dBv, z.bvWords), download(counts, dCnt, z.cntWords), download(samples, dSamples, z.nSamples);
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_build_suffix_array(cmb_build* b, int reverse, uint32_t* out, uint64_t cap) {
    if (!b || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (cap < b->n) return fail(CMB_ERR_OVERFLOW, "output buffer too small: " + std::to_string(b->n) + " entries are needed");
    try {
        HIPCHK(hipSetDevice(b->device));
        download(out, reverse ? b->saR : b->saF, b->n);
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_build_index(cmb_build* b, uint32_t sparseness, uint32_t kmer_size, uint32_t in_text_switch, const uint32_t* seq_starts,
                               uint32_t n_seqs, cmb_index** out) {
    if (!b || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (!powerOfTwo(sparseness)) return fail(CMB_ERR_INVALID, "suffix array sparseness must be a power of two");
    if (kmer_size > 15) return fail(CMB_ERR_INVALID, "k-mer size > 15 (the reference's -K option takes 0 ... 15, alignparameters.cpp:449)");
    try {
        HIPCHK(hipSetDevice(b->device));
        DevBuf<uint64_t> saBv, saCnt;
        DevBuf<uint32_t> samples;
        sparseOnDevice(b, sparseness, saBv, saCnt, samples);
        IndexDeviceArrays a{};
        a.n = b->n, a.text = b->text.p;
        uint64_t sum = 0;
        for (int c = 0; c < 5; c++) a.counts[c] = sum, sum += b->hist[c];
        a.dollarFwd = b->dollarF, a.dollarRev = b->dollarR;
        a.bvFwd = b->bvF.p, a.cntFwd = b->cntF.p, a.bvRev = b->bvR.p, a.cntRev = b->cntR.p;
        a.saBv = saBv.p, a.saBvCounts = saCnt.p, a.saSamples = samples.p, a.nSamples = samples.n;
        a.saSparseness = sparseness, a.seqStarts = seq_starts, a.nSeqs = seq_starts ? n_seqs : 0;
        a.kmerSize = kmer_size, a.inTextSwitch = in_text_switch;
        return indexFromDeviceArrays(a, b->device, out);
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_build_timings(const cmb_build* b, const char** names, float* ms, uint32_t cap) {
    if (!b) return 0;
    uint32_t n = 0;
    for (const auto& t : b->times) {
        if (n >= cap) break;
        if (names) names[n] = t.first.c_str();
        if (ms) ms[n] = (float)t.second;
        n++;
    }
    return (int)n;
}

extern "C" int cmb_build_move_sizes_of(cmb_build* b, uint32_t length_bits, cmb_build_move_sizes* out) {
    if (!b || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (length_bits != 64 && length_bits != 32) return fail(CMB_ERR_INVALID, "length_bits must be 64 or 32");
    if (isPowerOfTwo(b->n)) return fail(CMB_ERR_UNSUPPORTED, MOVE_POWER_OF_TWO);
    try {
        deriveMove(b);
        moveSizes(b, length_bits, out);
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_build_move_arrays(cmb_build* b, cmb_build_move_arrays_io* io, uint64_t* needed) {
    if (!b || !io || !io->lfbp || !io->rev_lfbp || !io->samples_first || !io->samples_last || !io->pred_first || !io->first_to_run ||
        !io->pred_last || !io->last_to_run || !io->rev_samples_first || !io->rev_samples_last || !io->plcp_pos || !io->plcp_sum)
        return fail(CMB_ERR_INVALID, "null argument");
    if (io->length_bits != 64 && io->length_bits != 32) return fail(CMB_ERR_INVALID, "length_bits must be 64 or 32");
    if (isPowerOfTwo(b->n)) return fail(CMB_ERR_UNSUPPORTED, MOVE_POWER_OF_TWO);
    try {
        deriveMove(b);
        cmb_build_move_sizes z;
        moveSizes(b, io->length_bits, &z);
        if (io->lfbp_cap < z.lfbp_bytes || io->rev_lfbp_cap < z.rev_lfbp_bytes || io->runs_cap < z.runs || io->rev_runs_cap < z.rev_runs ||
            io->plcp_cap < z.n_plcp) {
            if (needed) needed[0] = z.lfbp_bytes, needed[1] = z.rev_lfbp_bytes, needed[2] = z.runs, needed[3] = z.rev_runs, needed[4] = z.n_plcp;
            return fail(CMB_ERR_OVERFLOW, "output buffers too small: " + std::to_string(z.lfbp_bytes) + " and " + std::to_string(z.rev_lfbp_bytes) +
                                              " bytes of move tables, " + std::to_string(z.runs) + " and " + std::to_string(z.rev_runs) +
                                              " values per run and " + std::to_string(z.n_plcp) + " PLCP runs are needed");
        }
        packLfbp(b->mv[0].run.p, b->n, z.runs, b->mv[0].zeroPos, io->length_bits, io->lfbp);
        packLfbp(b->mv[1].run.p, b->n, z.rev_runs, b->mv[1].zeroPos, io->length_bits, io->rev_lfbp);
        download(io->samples_first, b->mv[0].smpF, z.runs), download(io->samples_last, b->mv[0].smpL, z.runs);
        download(io->rev_samples_first, b->mv[1].smpF, z.rev_runs), download(io->rev_samples_last, b->mv[1].smpL, z.rev_runs);
        download(io->pred_first, b->predFirst, z.runs), download(io->first_to_run, b->firstToRun, z.runs);
        download(io->pred_last, b->predLast, z.runs), download(io->last_to_run, b->lastToRun, z.runs);
        download(io->plcp_pos, b->plcpPos, z.n_plcp), download(io->plcp_sum, b->plcpSum, z.n_plcp);
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_build_move_index(cmb_build* b, int with_locate, int attach_text, const uint32_t* seq_starts, uint32_t n_seqs,
                                    cmb_move_index** out) {
    if (!b || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (isPowerOfTwo(b->n)) return fail(CMB_ERR_UNSUPPORTED, MOVE_POWER_OF_TWO);
    if (attach_text && b->n >= 0xFFFFFF00ull)
        return fail(CMB_ERR_UNSUPPORTED, "alignments on texts of 2^32 characters and more are not implemented");
    *out = nullptr;
    try {
        deriveMove(b);
        MoveDeviceArrays a;
        a.n = b->n;
        for (int s = 0; s < 2; s++) { // the rows go straight into the buffer the index keeps; the O(runs) arrays of the handle are copied
            const cmb_build::MoveSide& m = b->mv[s];
            a.side[s].runs = m.runs, a.side[s].zeroCharPos = m.zeroPos;
            a.side[s].rows.alloc(m.runs + 2);
            rowLaunch(k_mvb_rows, "k_mvb_rows", m.runs + 1, (const uint64_t*)m.run.p, m.runs, b->n, a.side[s].rows.p);
            copyBuf(m.smpF, a.side[s].smpF, m.runs), copyBuf(m.smpL, a.side[s].smpL, m.runs);
        }
        if (with_locate) {
            const uint64_t r = b->mv[0].runs;
            copyBuf(b->predFirst, a.predFirst, r), copyBuf(b->firstToRun, a.firstToRun, r);
            copyBuf(b->predLast, a.predLast, r), copyBuf(b->lastToRun, a.lastToRun, r);
            copyBuf(b->plcpPos, a.plcpPos, b->plcpPos.n), copyBuf(b->plcpSum, a.plcpSum, b->plcpSum.n);
            a.hasLocate = true;
        }
        if (int rc = moveIndexFromDeviceArrays(a, b->device, out)) return rc;
        if (attach_text) { // through a host copy: cmb_move_attach_text takes the text from the host
            std::vector<char> text(b->n);
            HIPCHK(hipMemcpy(text.data(), b->text.p, b->n, hipMemcpyDeviceToHost));
            if (int rc = cmb_move_attach_text(*out, text.data(), b->n, seq_starts, seq_starts ? n_seqs : 0)) {
                cmb_move_destroy(*out);
                *out = nullptr;
                return rc;
            }
        }
        return CMB_OK;
    } catch (const std::exception& e) {
        if (*out) cmb_move_destroy(*out);
        *out = nullptr;
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_build_pack_lfbp(uint64_t n, uint64_t r, uint64_t zero_pos, const uint64_t* rows, uint32_t length_bits, uint8_t* out,
                                   uint64_t cap, uint64_t* bytes) {
    if (!rows || !out || !bytes) return fail(CMB_ERR_INVALID, "null argument");
    if (length_bits != 64 && length_bits != 32) return fail(CMB_ERR_INVALID, "length_bits must be 64 or 32");
    if (n < 3 || r < 2 || r > n || zero_pos >= n) return fail(CMB_ERR_INVALID, "implausible text size, number of runs or position of the sentinel");
    if (length_bits == 32 && n > 0xFFFFFFFFull) return fail(CMB_ERR_INVALID, "the text size does not fit a 32-bit length_t");
    if (isPowerOfTwo(n)) return fail(CMB_ERR_UNSUPPORTED, MOVE_POWER_OF_TWO);
    if (ceilLog2(n) > 40) return fail(CMB_ERR_UNSUPPORTED, "texts of 2^40 characters and more are not supported");
    *bytes = lfbpBytes(n, r, length_bits);
    if (cap < *bytes) return fail(CMB_ERR_OVERFLOW, "output buffer too small: " + std::to_string(*bytes) + " bytes are needed");
    if (int rc = noDevice()) return rc;
    try {
        HIPCHK(hipSetDevice(0));
        DevBuf<uint64_t> run;
        run.upload(rows, 4 * r);
        packLfbp(run.p, n, r, zero_pos, length_bits, out);
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
