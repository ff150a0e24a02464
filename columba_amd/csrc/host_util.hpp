// Host-side HIP plumbing shared by the library's translation units that use the device: the error check, owning device
// and page-locked buffers, the device primitives (sorts, scan, run-length encode: rocPRIM), which geometry and tables a batch runs on,
// what both backends do when a batch is created, and the event timer behind cmb_batch_timings / cmb_move_batch_timings.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp> // (after <cstring>: its headers call memset unqualified)
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include "dev_bfs_edit.hpp"  // the record geometries of the frontier (GeoX, GeoW, GeoN32, GeoN)
#include "host_dispatch.hpp" // runtime values to template arguments, the geometry rule (no HIP: a CPU program tests it)
#include "host_grid.hpp"     // CMB_TEST_GRID_CAP and the clamps of the geometry knobs (no HIP: a CPU program tests it)
#include "host_schemes.hpp"

struct cmb_index;

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace cmb {

// a capacity as the kernels take it: 32 bits, saturating below the values they keep for flags
inline uint32_t cap32(size_t x) { return (uint32_t)std::min<size_t>(x, 0xFFFFFFF0u); }

// An owning device array.  n is the number of elements that was asked for (0 after alloc(0)); the allocation itself holds at least
// one element, so p is a valid pointer once alloc() has run.
template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count) {
        release();
        HIPCHK(hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)));
        n = count;
    }
    void upload(const T* h, size_t count) {
        alloc(count);
        if (count) HIPCHK(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
    }
    void uploadPadded(const T* h, size_t count, size_t pad) { // `pad` zeroed elements behind the data (k_prep reads 16-byte chunks)
        alloc(count + pad);
        if (count) HIPCHK(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(p + count, 0, pad * sizeof(T)));
    }
    size_t bytes() const { return n * sizeof(T); }
};
// room for `count` elements, with some to spare; contents are not kept
template <typename T> void growTo(DevBuf<T>& d, size_t count) {
    if (d.n < count || !d.p) d.alloc(count + count / 8 + 256);
}

// page-locked host memory (results are copied at PCIe speed, asynchronously)
template <typename T> struct PinnedBuf {
    T* p = nullptr;
    size_t cap = 0, n = 0;
    PinnedBuf() {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    void resize(size_t count) { // contents are not kept
        if (count > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
            const size_t want = count + count / 4 + 64;
            HIPCHK(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
            cap = want;
        }
        n = count;
    }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T* data() { return p; }
    const T* data() const { return p; }
};

// rocPRIM's two-call idiom — a size query, the scratch, the run — in one place: call(scratch, bytes) is the primitive; tmp is its scratch
// and grows as needed (a quarter to spare: the slices of a b-move chunk differ in size)
template <typename Call> void withScratch(DevBuf<uint8_t>& tmp, Call&& call) {
    size_t bytes = 0;
    HIPCHK(call((void*)nullptr, bytes));
    if (tmp.n < bytes || !tmp.p) tmp.alloc(bytes + bytes / 4 + 256);
    HIPCHK(call((void*)tmp.p, bytes));
}
// out[i] = in[0] + ... + in[i - 1] in the width of `out` (64 bits; 32 for the keep -> slot scan of the b-move backend), on stream s
template <typename T, typename O> void scanExclusive(DevBuf<uint8_t>& tmp, const T* in, O* out, size_t n, hipStream_t s) {
    withScratch(tmp, [&](void* p, size_t& bytes) { return rocprim::exclusive_scan(p, bytes, in, out, (O)0, n, rocprim::plus<O>(), s); });
}
// radix sorts on the key bits [bit0, bit1), keys alone or with a value each (fewer than 2^31 of them: the callers refuse more before;
// the input stays as it is — plain pointers, so that rocPRIM instantiates what it did for the direct calls)
template <typename K> void sortKeys(DevBuf<uint8_t>& tmp, K* in, K* out, uint32_t n, uint32_t bit0, uint32_t bit1, hipStream_t s) {
    withScratch(tmp, [&](void* p, size_t& bytes) { return rocprim::radix_sort_keys(p, bytes, in, out, n, bit0, bit1, s); });
}
template <typename K, typename V>
void sortPairs(DevBuf<uint8_t>& tmp, K* kIn, K* kOut, V* vIn, V* vOut, uint32_t n, uint32_t bit0, uint32_t bit1, hipStream_t s) {
    withScratch(tmp, [&](void* p, size_t& bytes) { return rocprim::radix_sort_pairs(p, bytes, kIn, kOut, vIn, vOut, n, bit0, bit1, s); });
}
// the distinct keys of a sorted list, how often each occurs, and (nRuns[0]) how many there are
template <typename K> void runLengthEncode(DevBuf<uint8_t>& tmp, K* in, uint32_t n, K* uniq, uint32_t* counts, uint32_t* nRuns, hipStream_t s) {
    withScratch(tmp, [&](void* p, size_t& bytes) { return rocprim::run_length_encode(p, bytes, in, n, uniq, counts, nRuns, s); });
}

// ---- which instance a batch runs (both batch structs use the same member names)
// the geometry of a batch's frontier (host_dispatch.hpp: frontierGeo); read per attempt: noSmallMatrix changes between two
template <typename Batch> FrontierGeo frontierGeoOf(const Batch* b) {
    return frontierGeo(b->wide, b->k, b->noSmallMatrix, getenv("CMB_MATRIX64") != nullptr, MX_MAX_ED, MXS_MAX_ED);
}
template <typename T> struct TypeTag {
    using type = T;
};
// f(TypeTag<Geo>{}): the geometry as a type
template <typename F> decltype(auto) withGeo(FrontierGeo g, F&& f) {
    switch (g) {
    case FrontierGeo::X: return f(TypeTag<GeoX>{});
    case FrontierGeo::W: return f(TypeTag<GeoW>{});
    case FrontierGeo::N32: return f(TypeTag<GeoN32>{});
    default: return f(TypeTag<GeoN>{});
    }
}
// f(std::integral_constant<int, MP>{}): the table size of the batch's width, for the kernels that depend on nothing else
template <typename Batch, typename F> decltype(auto) withTables(const Batch* b, F&& f) {
    return b->wide ? f(std::integral_constant<int, MAXP_WIDE>{}) : f(std::integral_constant<int, MAXP>{});
}
// ... and the tables of that size (Geo::MP of a geometry)
template <int MP, typename Batch> auto stratOf(Batch* b) {
    if constexpr (MP == MAXP) return b->strat.p;
    else return b->stratW.p;
}
template <int MP, typename Batch> auto partsOf(Batch* b) {
    if constexpr (MP == MAXP) return b->parts.p;
    else return b->partsW.p;
}

// ---- what both backends do when a batch is created
// the strategy flattened at k errors into the narrow or the wide table of the batch, and what the run needs to know of either
template <typename Batch> void adoptStrategy(Batch* b, const cmb_strategy* st, uint32_t k) {
    auto summary = [&](const auto& t) {
        b->sNumParts = t.numParts, b->sPartition = t.partition, b->sNSchemes = t.nSchemes;
        for (int i = 0; i < t.nSchemes; i++) b->sMaxSearches = std::max<uint32_t>(b->sMaxSearches, t.sch[i].nSearches);
    };
    if (b->wide) summary(b->hostStratW = st->template flatten<MAXP_WIDE>(k));
    else summary(b->hostStrat = st->template flatten<MAXP>(k));
}
// the shortest and the longest of n reads given by their offsets (maxLen at least 1; minLen ~0 without reads); false: offsets decrease
inline bool readLengths(const uint64_t* offs, uint32_t n, uint32_t& minLen, uint32_t& maxLen) {
    maxLen = 1, minLen = ~0u;
    for (uint32_t i = 0; i < n; i++) {
        if (offs[i + 1] < offs[i]) return false;
        maxLen = std::max<uint32_t>(maxLen, (uint32_t)(offs[i + 1] - offs[i]));
        minLen = std::min<uint32_t>(minLen, (uint32_t)(offs[i + 1] - offs[i]));
    }
    return true;
}
// rows of per-read arrays are padded to a multiple of 16 bytes (16-byte stores in k_prep); the number of 32-character words per read
// does not change
inline uint32_t paddedLen(uint32_t maxLen) { return (maxLen + 15u) & ~15u; }

// device time per kernel group of a run: end(name) waits for the stream and adds the time since begin() to the record of that name
struct KernelTime {
    const char* name;
    float ms;
};
struct Timer {
    hipStream_t s;
    hipEvent_t a, b;
    std::vector<KernelTime>& out;
    Timer(hipStream_t st, std::vector<KernelTime>& o) : s(st), out(o) {
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
    }
    ~Timer() {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
    }
    void begin() { (void)hipEventRecord(a, s); }
    void end(const char* name) {
        (void)hipEventRecord(b, s);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        for (auto& t : out)
            if (!strcmp(t.name, name)) {
                t.ms += ms;
                return;
            }
        out.push_back({name, ms});
    }
};

// a composite batch's counters and busy time per kernel group: those of its parts summed (the parts overlap on the device)
template <typename Batch> void foldSubBatches(Batch* b) {
    memset(b->cnts, 0, sizeof(b->cnts));
    b->times.clear();
    for (const Batch* c : b->subs) {
        for (size_t i = 0; i < sizeof(b->cnts) / sizeof(b->cnts[0]); i++) b->cnts[i] += c->cnts[i];
        for (const KernelTime& t : c->times) {
            auto u = std::find_if(b->times.begin(), b->times.end(), [&](const KernelTime& x) { return !strcmp(x.name, t.name); });
            if (u == b->times.end()) b->times.push_back(t);
            else u->ms += t.ms;
        }
    }
}

// CIGAR and sequence assignment of one occurrence (kernels.hpp: k_cigar): nOps runs of (length << 2 | op) stored END to BEGIN;
// seqId = the sequence `begin` lies in (IndexInterface::findSeqName, indexinterface.cpp:799-832); spans = the occurrence runs over its
// end (the host trims or drops those, :833-899)
struct AlnRec {
    uint32_t seqId, seqBegin, nOps, spans;
};
static_assert(sizeof(AlnRec) == 16, "AlnRec is copied between the device and the host as it stands");
constexpr uint32_t BEST_OPS_STRIDE = 2u * 13u + 3u; // CIGAR runs of an occurrence with up to 13 errors (k_cigar: 2 k + 3)
struct SamPlan { // per read (32 bytes; dev_sam.hpp)
    uint32_t kind;    // SAM_*
    uint32_t primary; // index of the primary among the read's occurrences
    uint32_t minScore, nHits;
    uint32_t idLen; // cleaned identifier: raw[1, idLen + 1)
    uint32_t cls;   // read pairs: the pair's PAIR_CLS_* (dev_pair.hpp; k_pair_class_write reads it); 0 for single reads
    uint64_t sideOff; // SAM_HOST: where the read's text lies in the side buffer
};
// per read pair with a concordant combination (dev_pair.hpp).  A candidate pair is (combination of the orientation, index in the up
// list, index in the down list): the primary — the first pair of minimal summed distance — and the first pair, which changes places with it.
// A discordant pair has one combination, (read 1's list, read 2's list); a pair with one mate unmapped has primU (the primary among the
// mapped mate's occurrences), minDist and nPairs alone
struct PairPlan {
    uint32_t primCombo, primU, primD;
    uint32_t firstCombo, firstU, firstD;
    uint32_t minDist, nPairs; // the minimal summed distance and how many pairs have it
    uint32_t idLen[2];        // cleaned identifiers of read 1 and read 2
};
// What the device SAM driver (sam.hip: samUpload, samSplice, samScan, samWrite) keeps in HBM for one (sub-)batch or one BEST result:
// the chunk's packed identifiers, qualities and sequence names with their offsets, the plan, length and position of every read in the
// text, the text of the reads the host formatted with its offsets and read numbers, the text itself (the scan's scratch is the owner's)
struct SamDeviceBufs {
    DevBuf<uint8_t> ids, quals, names, side, text;
    DevBuf<uint64_t> idOffs, qualOffs, nameOffs, len, offs, sideOffs;
    DevBuf<SamPlan> plan;
    DevBuf<uint32_t> sideReads;
};
// ... and what a (sub-)batch of either backend owns for the SAM and pair drivers: the driver's buffers; the reads (pairs) the plan kernel
// leaves to the host ([0]: how many); in the first part, the finished text of the whole batch; in a part with read 1 of every pair, the
// plan of the concordant pairs, per pair the SAM lines the device writes and whether it counts as mapped, and the 64-bit scan of either;
// for the pairs k_pair_class_write formats into the side buffer (cmb_pair_sam_device_classes): their list ([0]: how many), their byte
// lengths (0 for every other pair) with the scan of those, and the number of pairs per device class
struct SamBufs {
    SamDeviceBufs sam;
    DevBuf<uint32_t> hostList;
    PinnedBuf<char> samOut;
    DevBuf<PairPlan> pairPlan;
    DevBuf<uint64_t> pairRecords, pairSums;
    DevBuf<uint32_t> pairMapped;
    DevBuf<uint32_t> clsList, clsCount;
    DevBuf<uint64_t> clsLen, clsOffs;
    // the lists of a part without its dropped occurrences (AlnRec::spans == 4; dev_sam.hpp: k_sam_keep_*), for the plan and write kernels
    DevBuf<uint32_t> keepFlag;
    DevBuf<uint64_t> keepPos, keepOffs;
    DevBuf<uint4> keepOcc;
    DevBuf<AlnRec> keepAln;
    DevBuf<uint16_t> keepOps;
};
// The final lists a (sub-)batch of either backend holds in HBM for its whole chunk, as the SAM driver and the strata bookkeeping read
// them (dev_sam.hpp: SamCtx; dev_best.hpp: k_best_scan / k_best_append), beside the host copies the host-formatted reads are taken
// from.  One view per part, in read order (columba_amd.hip: batchListViews; move_backend.hip: moveBatchListViews).
struct ListView {
    uint32_t nReads = 0, k = 0;
    int metric = 1;
    cmb_index* textIndex = nullptr; // whose text and sequence starts the lists refer to (nullptr: a b-move index without its text)
    const uint8_t* reads = nullptr; // device: raw read characters of the part, and their offsets
    const uint64_t* offs = nullptr;
    const uint64_t* goffs = nullptr; // device: first record of every filter group, groupStride groups per read
    uint32_t groupStride = 1;
    const uint4* occ = nullptr;    // device: {begin, end, distance, strand}
    const AlnRec* aln = nullptr;
    const uint16_t* ops = nullptr; //         CIGAR runs at `stride`, stored end to begin
    uint32_t stride = 0;
    hipStream_t stream = nullptr;
    // host: read offsets of the part (from 0); occurrences as records of hOccBytes (cmb_occ: 16, or cmb_move_occ with 64-bit begin and
    // end: 24) with their offsets per filter group or per read; AlnRec and CIGAR runs as on the device
    const uint64_t* hostOffs = nullptr;
    const void* hOcc = nullptr;
    uint32_t hOccBytes = 0;
    const uint64_t* hOccOffs = nullptr;
    bool hOffsPerGroup = false;
    const AlnRec* hAln = nullptr;
    const uint16_t* hOps = nullptr;
    const uint64_t* cnts = nullptr; // counters and kernel times of the part's run
    const std::vector<KernelTime>* times = nullptr;
    SamBufs* bufs = nullptr;
    DevBuf<uint8_t>* scanTmp = nullptr; // the part's scratch for the drivers' scans
    // the run trimmed the occurrences over the end of their sequence itself (cmb_batch_trim_on_device): AlnRec::spans is 0, 2 (trimmed:
    // an ordinary occurrence) or 4 (dropped: no record is written for it), never 1; how many of the part's occurrences are dropped
    bool trimOnDevice = false;
    uint64_t trimDropped = 0;
};

} // namespace cmb
