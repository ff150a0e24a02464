// The device FASTQ parser behind cmb_reads_* (include/columba_amd.h): a window of raw file bytes is uploaded once, split into lines,
// records and fields on the device (kernels and algorithm: dev_reads.hpp) and comes back as the packed arrays cmb_batch_create,
// cmb_match_best_device and cmb_sam_inputs take, in page-locked buffers of the handle; the same arrays stay in HBM.
//
// Host synchronisations per window: the number of newlines, the number of records that begin in the window, the first record without
// '@' / with an empty read, and the download (whose offsets give the sizes of the three byte arrays).
#include "dev_reads.hpp"
#include "units.hpp"

#include <chrono>
#include <memory>

#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

using namespace cmb;

static int fail(int code, const std::string& msg) { return failWith(code, msg); }

struct cmb_reads {
    int device = 0;
    // the window (padded with zero bytes to whole 16-byte vectors and one more) and what the passes derive from it
    DevBuf<uint8_t> window, fn, before, start, tmp;
    DevBuf<uint32_t> tileCount, tileBase, lineEnd, recLine, fBegin, fLen, first;
    DevBuf<uint64_t> count;
    // the packed arrays of the last parse: offs = {offs, id_offs, qual_offs}, nRecords + 1 each; bytes = {ids, seqs, quals} in field order
    DevBuf<uint64_t> offs;
    DevBuf<uint8_t> bytes[3];
    PinnedBuf<uint64_t> hOffs;
    PinnedBuf<char> hBytes[3];
    uint32_t nRecords = 0;
    uint64_t nBytesOf[3] = {0, 0, 0};
};

namespace {
static_assert(READS_MAX_WINDOW == CMB_READS_MAX_WINDOW, "the header states the largest window");
constexpr uint32_t READS_GRID = 2048; // blocks of a capped launch
enum { F_ID = 0, F_SEQ = 1, F_QUAL = 2 };

int noDevice() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(CMB_ERR_DEVICE, "no HIP device available (the product path has no CPU fallback)");
    return CMB_OK;
}
uint32_t gridFor(uint64_t blocks) { return capBlocks((uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks, 1), READS_GRID)); }
// one lane per item and trip (perItem lanes for the gather)
template <typename... KA, typename... A> void laneLaunch(void (*kern)(KA...), const char* name, uint64_t items, uint32_t perItem, A... args) {
    if (!items) return;
    const uint32_t grid = gridFor((items * perItem + READS_BLOCK - 1) / READS_BLOCK);
    gridLine(getenv("CMB_VERBOSE") != nullptr, name, items * perItem, (uint64_t)grid * READS_BLOCK);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(READS_BLOCK), 0, 0, args...);
    HIPCHK(hipGetLastError());
}
// one block per tile and trip
template <typename... KA, typename... A> void tileLaunch(void (*kern)(KA...), const char* name, uint64_t nVec, uint64_t nTiles, A... args) {
    const uint32_t grid = gridFor(nTiles);
    gridLine(getenv("CMB_VERBOSE") != nullptr, name, nVec, (uint64_t)grid * READS_BLOCK);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(READS_BLOCK), 0, 0, args...);
    HIPCHK(hipGetLastError());
}
template <typename T> T readValue(const T* d) {
    T v{};
    HIPCHK(hipMemcpy(&v, d, sizeof(T), hipMemcpyDeviceToHost));
    return v;
}
struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() {
        HIPCHK(hipDeviceSynchronize());
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};
// the first character of the first line that is neither empty nor begins with '\r' (0: there is none)
char firstRecordCharacter(const char* bytes, uint64_t n) {
    uint64_t p = 0;
    while (p < n && (bytes[p] == '\n' || bytes[p] == '\r')) {
        const void* nl = memchr(bytes + p, '\n', n - p);
        if (!nl) return 0;
        p = (uint64_t)((const char*)nl - bytes) + 1;
    }
    return p < n ? bytes[p] : 0;
}
void nothingParsed(cmb_reads* r) {
    r->nRecords = 0;
    r->nBytesOf[0] = r->nBytesOf[1] = r->nBytesOf[2] = 0;
    growTo(r->offs, 3);
    HIPCHK(hipMemset(r->offs.p, 0, 3 * sizeof(uint64_t)));
    r->hOffs.resize(3);
    r->hOffs.p[0] = r->hOffs.p[1] = r->hOffs.p[2] = 0;
    for (int f = 0; f < 3; f++) {
        growTo(r->bytes[f], 1);
        r->hBytes[f].resize(1);
    }
}

int parseWindow(cmb_reads* r, const char* bytes, uint64_t n, uint32_t maxRecords, bool final, cmb_reads_info* info) {
    const bool verbose = getenv("CMB_VERBOSE") != nullptr;
    const hipStream_t s0 = nullptr;
    info->n_records = 0, info->stop = CMB_READS_STOP_WINDOW, info->consumed = 0;
    nothingParsed(r);
    if (!n) return CMB_OK;
    Clock clk;
    // ---- bytes -> lines
    const uint64_t nVec = (n + 15) / 16, nTiles = (nVec + READS_BLOCK - 1) / READS_BLOCK;
    growTo(r->window, nVec * 16 + 16);
    HIPCHK(hipMemcpy(r->window.p, bytes, n, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(r->window.p + n, 0, nVec * 16 + 16 - n));
    const double msUpload = clk.lap();
    growTo(r->tileCount, nTiles + 1), growTo(r->tileBase, nTiles + 1);
    HIPCHK(hipMemset(r->tileCount.p + nTiles, 0, sizeof(uint32_t)));
    tileLaunch(k_rd_count, "k_rd_count", nVec, nTiles, (const uint4*)r->window.p, nVec, nTiles, r->tileCount.p);
    scanExclusive(r->tmp, r->tileCount.p, r->tileBase.p, (size_t)nTiles + 1, s0);
    const uint32_t nNewlines = readValue(r->tileBase.p + nTiles);
    const uint64_t nLines = (uint64_t)nNewlines + (final && bytes[n - 1] != '\n' ? 1 : 0);
    double msKernels = 0;
    uint64_t nStarts = 0;
    if (nLines) {
        growTo(r->lineEnd, nNewlines);
        tileLaunch(k_rd_place, "k_rd_place", nVec, nTiles, (const uint4*)r->window.p, nVec, nTiles, (const uint32_t*)r->tileBase.p, r->lineEnd.p);
        // ---- lines -> records
        growTo(r->fn, nLines), growTo(r->before, nLines), growTo(r->start, nLines), growTo(r->recLine, nLines), growTo(r->count, 1);
        laneLaunch(k_rd_classify, "k_rd_classify", nLines, 1, (const uint8_t*)r->window.p, (const uint32_t*)r->lineEnd.p, nNewlines, (uint32_t)n, nLines,
                   r->fn.p);
        withScratch(r->tmp, [&](void* p, size_t& b) {
            return rocprim::exclusive_scan(p, b, r->fn.p, r->before.p, READS_FN_IDENTITY, (size_t)nLines, RdCompose(), s0);
        });
        laneLaunch(k_rd_starts, "k_rd_starts", nLines, 1, (const uint8_t*)r->fn.p, (const uint8_t*)r->before.p, nLines, r->start.p);
        withScratch(r->tmp, [&](void* p, size_t& b) {
            return rocprim::select(p, b, rocprim::counting_iterator<uint32_t>(0), r->start.p, r->recLine.p, r->count.p, (size_t)nLines, s0);
        });
        nStarts = readValue(r->count.p);
    }
    // a record counts if the window ends the file or holds the newline of its fourth line (only the last one can lack it)
    uint64_t nAvailable = nStarts;
    if (nStarts && !final && (uint64_t)readValue(r->recLine.p + (nStarts - 1)) + 3 >= nLines) nAvailable--;
    const uint64_t nLook = std::min<uint64_t>(nAvailable, maxRecords);
    if (!nLook) {
        msKernels = clk.lap();
        if (verbose) fprintf(stderr, "[reads] %llu bytes, 0 records: upload %.3f ms, kernels %.3f ms, download 0.000 ms\n", (unsigned long long)n, msUpload, msKernels);
        return CMB_OK;
    }
    // ---- records -> fields
    const uint64_t stride = nLook + 1;
    growTo(r->fBegin, 3 * stride), growTo(r->fLen, 3 * stride), growTo(r->first, 2);
    HIPCHK(hipMemset(r->first.p, 0xFF, 2 * sizeof(uint32_t)));
    HIPCHK(hipMemset(r->fLen.p, 0, 3 * stride * sizeof(uint32_t)));
    laneLaunch(k_rd_fields, "k_rd_fields", nLook, 1, (const uint8_t*)r->window.p, (const uint32_t*)r->lineEnd.p, nNewlines, (uint32_t)n, nLines,
               (const uint32_t*)r->recLine.p, nLook, stride, r->fBegin.p, r->fLen.p, r->first.p);
    uint32_t first[2];
    HIPCHK(hipMemcpy(first, r->first.p, sizeof(first), hipMemcpyDeviceToHost));
    // the chunk: the records in front of the first empty read (Reader::next returns false there, having consumed the record's lines)
    const bool stoppedByEmpty = first[1] != READS_NONE;
    const uint64_t nTake = stoppedByEmpty ? first[1] : nLook;
    const uint64_t nReached = nTake + (stoppedByEmpty ? 1 : 0); // the records Reader would have looked at
    if (first[0] != READS_NONE && first[0] < nReached)
        return fail(CMB_ERR_INVALID, "record " + std::to_string(first[0]) + " of the window does not begin with '@': the data does not appear to be in FastQ format");
    info->n_records = (uint32_t)nTake;
    info->stop = stoppedByEmpty ? CMB_READS_STOP_EMPTY_READ : nTake == maxRecords ? CMB_READS_STOP_MAX_RECORDS : CMB_READS_STOP_WINDOW;
    {
        const uint64_t lastLine = std::min<uint64_t>((uint64_t)readValue(r->recLine.p + (nReached - 1)) + 3, nLines - 1);
        info->consumed = lastLine < nNewlines ? (uint64_t)readValue(r->lineEnd.p + lastLine) + 1 : n;
    }
    // ---- fields -> packed arrays
    const uint64_t offStride = nTake + 1;
    growTo(r->offs, 3 * offStride);
    // (field order in the handle's arrays: identifiers, reads, qualities; the scan reads one length behind the records: a 0 or a real one)
    for (int f = 0; f < 3; f++) scanExclusive(r->tmp, r->fLen.p + f * stride, r->offs.p + f * offStride, (size_t)offStride, s0);
    r->hOffs.resize(3 * offStride);
    HIPCHK(hipMemcpy(r->hOffs.p, r->offs.p, 3 * offStride * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int f = 0; f < 3; f++) {
        r->nBytesOf[f] = r->hOffs.p[f * offStride + nTake];
        growTo(r->bytes[f], (r->nBytesOf[f] + 3) / 4 * 4 + 4);
    }
    laneLaunch(k_rd_gather, "k_rd_gather", 3 * nTake, READS_GATHER_LANES, (const uint32_t*)r->window.p, (const uint32_t*)r->fBegin.p, (const uint32_t*)r->fLen.p,
               stride, (const uint64_t*)r->offs.p, offStride, r->bytes[0].p, r->bytes[1].p, r->bytes[2].p, nTake);
    msKernels = clk.lap();
    for (int f = 0; f < 3; f++) {
        r->hBytes[f].resize(r->nBytesOf[f] + 1);
        if (r->nBytesOf[f]) HIPCHK(hipMemcpyAsync(r->hBytes[f].p, r->bytes[f].p, r->nBytesOf[f], hipMemcpyDeviceToHost, s0));
    }
    const double msDownload = clk.lap();
    r->nRecords = (uint32_t)nTake;
    if (verbose)
        fprintf(stderr, "[reads] %llu bytes, %llu records: upload %.3f ms, kernels %.3f ms, download %.3f ms\n", (unsigned long long)n,
                (unsigned long long)nTake, msUpload, msKernels, msDownload);
    return CMB_OK;
}
} // namespace

extern "C" int cmb_reads_create(int device, cmb_reads** out) {
    if (!out) return fail(CMB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = noDevice()) return rc;
    try {
        HIPCHK(hipSetDevice(device));
        std::unique_ptr<cmb_reads> r(new cmb_reads);
        r->device = device;
        nothingParsed(r.get());
        *out = r.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" void cmb_reads_destroy(cmb_reads* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}
extern "C" int cmb_reads_parse_fastq(cmb_reads* r, const char* bytes, uint64_t n_bytes, uint32_t max_records, int final, cmb_reads_info* info) {
    if (!r || !info || (n_bytes && !bytes)) return fail(CMB_ERR_INVALID, "null argument");
    if (!max_records) return fail(CMB_ERR_INVALID, "max_records must be at least 1");
    if (n_bytes > READS_MAX_WINDOW)
        return fail(CMB_ERR_UNSUPPORTED, "a window of " + std::to_string(n_bytes) + " bytes: the parser takes at most " + std::to_string(READS_MAX_WINDOW));
    if (firstRecordCharacter(bytes, n_bytes) == '>')
        return fail(CMB_ERR_UNSUPPORTED, "the window begins a FASTA record ('>'): FASTA read files are read on the host");
    try {
        HIPCHK(hipSetDevice(r->device));
        return parseWindow(r, bytes, n_bytes, max_records, final != 0, info);
    } catch (const std::exception& e) {
        r->nRecords = 0;
        r->nBytesOf[0] = r->nBytesOf[1] = r->nBytesOf[2] = 0;
        if (r->hOffs.cap >= 3) r->hOffs.p[0] = r->hOffs.p[1] = r->hOffs.p[2] = 0; // (the three offset arrays of an empty chunk)
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_reads_arrays(const cmb_reads* r, cmb_reads_view* out) {
    if (!r || !out) return fail(CMB_ERR_INVALID, "null argument");
    const uint64_t offStride = (uint64_t)r->nRecords + 1;
    out->seqs = r->hBytes[F_SEQ].p, out->offs = r->hOffs.p + F_SEQ * offStride;
    out->ids = r->hBytes[F_ID].p, out->id_offs = r->hOffs.p + F_ID * offStride;
    out->quals = r->hBytes[F_QUAL].p, out->qual_offs = r->hOffs.p + F_QUAL * offStride;
    out->n_records = r->nRecords;
    return CMB_OK;
}
extern "C" int cmb_reads_device_arrays(const cmb_reads* r, void** ptrs, uint64_t* bytes) {
    if (!r || !ptrs || !bytes) return fail(CMB_ERR_INVALID, "null argument");
    const uint64_t offStride = (uint64_t)r->nRecords + 1;
    const int field[3] = {F_SEQ, F_ID, F_QUAL};
    for (int i = 0; i < 3; i++) {
        ptrs[2 * i] = r->bytes[field[i]].p, bytes[2 * i] = r->nBytesOf[field[i]];
        ptrs[2 * i + 1] = r->offs.p + field[i] * offStride, bytes[2 * i + 1] = offStride * sizeof(uint64_t);
    }
    return CMB_OK;
}
