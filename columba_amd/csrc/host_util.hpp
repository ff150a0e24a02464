// Host-side HIP plumbing shared by the library's translation units (columba_amd.hip, move_backend.hip): the error check, owning device
// and page-locked buffers, the 64-bit exclusive scan and the event timer behind cmb_batch_timings / cmb_move_batch_timings.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <rocprim/device/device_scan.hpp> // (after <cstring>: its headers call memset unqualified)

#include "host_grid.hpp" // CMB_TEST_GRID_CAP and the clamps of the geometry knobs (no HIP: a CPU program tests it)

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

// out[i] = in[0] + ... + in[i - 1] in 64 bits, on stream s; tmp is rocPRIM's scratch and grows as needed
template <typename T> void scanExclusive(DevBuf<uint8_t>& tmp, const T* in, uint64_t* out, size_t n, hipStream_t s) {
    size_t bytes = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), s));
    if (tmp.n < bytes || !tmp.p) tmp.alloc(bytes + 256);
    HIPCHK(rocprim::exclusive_scan(tmp.p, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), s));
}

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

struct SamPlan { // per read (32 bytes; dev_sam.hpp)
    uint32_t kind;    // SAM_*
    uint32_t primary; // index of the primary among the read's occurrences
    uint32_t minScore, nHits;
    uint32_t idLen; // cleaned identifier: raw[1, idLen + 1)
    uint32_t pad;
    uint64_t sideOff; // SAM_HOST: where the read's text lies in the side buffer
};
// per read pair with a concordant combination (dev_pair.hpp).  A candidate pair is (combination of the orientation, index in the up
// list, index in the down list): the primary — the first pair of minimal summed distance — and the first pair, which changes places with it
struct PairPlan {
    uint32_t primCombo, primU, primD;
    uint32_t firstCombo, firstU, firstD;
    uint32_t minDist, nPairs; // the minimal summed distance and how many pairs have it
    uint32_t idLen[2];        // cleaned identifiers of read 1 and read 2
};
// What the device SAM driver (columba_amd.hip: samUpload, samSplice, samScan, samWrite) keeps in HBM for one (sub-)batch or one BEST result:
// the chunk's packed identifiers, qualities and sequence names with their offsets, the plan, length and position of every read in the
// text, the text of the reads the host formatted with its offsets and read numbers, the text itself (the scan's scratch is the owner's)
struct SamDeviceBufs {
    DevBuf<uint8_t> ids, quals, names, side, text;
    DevBuf<uint64_t> idOffs, qualOffs, nameOffs, len, offs, sideOffs;
    DevBuf<SamPlan> plan;
    DevBuf<uint32_t> sideReads;
};
// ... and what a b-move (sub-)batch owns for that driver (cmb_move_batch_sam_device): its buffers, the list of host-formatted reads, the
// scan's scratch, and — in the first part — the finished text of the whole batch in page-locked memory
struct MoveSamBufs {
    SamDeviceBufs sam;
    DevBuf<uint32_t> hostList;
    DevBuf<uint8_t> scanTmp;
    PinnedBuf<char> samOut;
};
// The final lists a b-move (sub-)batch keeps in HBM for its whole chunk (cmb_move_batch_keep_device_lists), as columba_amd.hip's SAM
// driver and strata bookkeeping read them (dev_sam.hpp: SamCtx; dev_best.hpp: k_best_scan / k_best_append), beside the host copies the
// host-formatted reads are taken from.  One view per part, in read order (move_backend.hip: moveBatchListViews).
struct MoveListView {
    uint32_t nReads = 0, k = 0;
    int metric = 1;
    const uint8_t* reads = nullptr; // device: raw read characters of the part, and their offsets
    const uint64_t* offs = nullptr;
    const uint64_t* goffs = nullptr; // device: first record of every filter group, groupStride groups per read
    uint32_t groupStride = 1;
    const uint4* occ = nullptr; // device: {begin, end, distance, strand}
    const uint4* aln = nullptr; //         AlnRec {seqId, seqBegin, nOps, spans}
    const uint16_t* ops = nullptr; //      CIGAR runs at `stride`, stored end to begin
    uint32_t stride = 0;
    uint64_t nOcc = 0;
    hipStream_t stream = nullptr;
    // host: read offsets of the part (from 0), occurrences as {begin, end (64 bits), distance, strand} of 24 bytes with their offsets per
    // read, AlnRec and CIGAR runs as on the device
    const uint64_t* hostOffs = nullptr;
    const void* hOcc = nullptr;
    const uint64_t* hOccOffs = nullptr;
    const uint4* hAln = nullptr;
    const uint16_t* hOps = nullptr;
    const uint64_t* cnts = nullptr; // counters and kernel times of the part's run
    const std::vector<KernelTime>* times = nullptr;
    MoveSamBufs* samBufs = nullptr;
};

} // namespace cmb
