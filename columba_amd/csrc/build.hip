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
#include "dev_build.hpp"
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
