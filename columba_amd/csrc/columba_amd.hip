// C-ABI implementation (include/columba_amd.h) on top of the HIP kernels.  gfx950 only.
#include "../../include/columba_amd.h"
#include "host_schemes.hpp"
#include "host_util.hpp"
#include "kernels.hpp"
#include "dev_trim.hpp"
#include "units.hpp"

#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

using namespace cmb;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
namespace cmb {
int failWith(int code, const std::string& msg) { return fail(code, msg); } // for the library's other translation units (host_error.hpp)
}
// ------------------------------------------------------------------------------------ index
struct cmb_index {
    int device = 0;
    uint32_t saSparseness = 0;
    DevIndex d{};
    DevBuf<uint4> blkF, blkR; // 32-byte rank blocks
    DevBuf<uint32_t> saSamples;
    DevBuf<uint32_t> saDense; // derived at creation / validation (buildDenseSA), not replicated; empty: the sparse walk
    DevBuf<uint8_t> text;
    DevBuf<uint32_t> text2;
    DevBuf<uint4> kmer;
    std::vector<uint32_t> seqStarts;
    DevBuf<uint32_t> seqStartsDev; // the same on the device (k_cigar: sequence assignment); [0, n - 1] if none were given
    uint32_t nSeqsDev = 0;
    uint64_t bytes = 0;
    bool textOnly = false; // cmb_index_create_text_only: no BWT, no suffix array — alignments and SAM records only
    void uploadSeqStarts() {
        std::vector<uint32_t> v = seqStarts;
        if (v.size() < 2) v = {0u, d.n ? d.n - 1u : 0u};
        seqStartsDev.upload(v.data(), v.size());
        nSeqsDev = (uint32_t)v.size() - 1u;
    }
};

#ifdef CMB_BFS_STATS
extern "C" int cmb_debug_bfs_stats(unsigned long long* out, int reset) { // diagnostic build only
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(cmb::g_bfsStats), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(cmb::g_bfsStats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef CMB_BOUNDS
extern "C" int cmb_debug_oob(unsigned long long* out) { // diagnostic build only (tools/bounds_check.sh)
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(cmb::g_oob), 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef CMB_STAGE_STATS
extern "C" int cmb_debug_stage_stats(unsigned long long* out, int reset) { // diagnostic build only
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(cmb::g_stageStats), 24 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[24] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(cmb::g_stageStats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
extern "C" const char* cmb_last_error(void) { return g_err.c_str(); }
extern "C" const char* cmb_version(void) { return "columba_amd 0.1 (gfx950)"; }

static void useDevice(int device) { HIPCHK(hipSetDevice(device)); }

// k_check_index on the arrays of an index (at creation, and after its arrays were filled by a collective)
static int probeIndex(cmb_index* ix) {
    DevBuf<uint32_t> bad;
    bad.alloc(1);
    HIPCHK(hipMemset(bad.p, 0, sizeof(uint32_t)));
    const uint32_t nProbe = std::min<uint32_t>(ix->d.n, 1u << 20);
    if (!nProbe) return CMB_OK;
    hipLaunchKernelGGL(k_check_index, dim3((nProbe + 255) / 256), dim3(256), 0, 0, ix->d, ix->saSparseness, nProbe, (uint32_t)std::min<size_t>(ix->saSamples.n, 0xFFFFFFFFu), bad.p);
    HIPCHK(hipGetLastError());
    uint32_t hb = 0;
    HIPCHK(hipMemcpy(&hb, bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (hb)
        return fail(CMB_ERR_INVALID, "the index arrays do not belong together: " + std::to_string(hb) + " of " + std::to_string(nProbe) +
                                         " probed suffix-array rows do not reach a sampled row within " + std::to_string(ix->saSparseness) +
                                         " LF steps (wrong sparseness, or bit vectors / samples / BWT of different texts)");
    return CMB_OK;
}
// The dense suffix array (DevIndex::saDense): every locate becomes one 4-byte load instead of the sparse walk's ~(s + 3) / 2 rank
// blocks and a sample.  It is a speed-up, so it must not take the memory read batches need: it is built only if at least
// min(128 GiB, half the device) stays free after it — a batch of the headline's 10^7 reads holds ~10 KB per read (~93 GiB), and two
// ranks sharing one device hold half as many reads each (CMB_TEST_SA_MIN_FREE_GB overrides the 128 GiB for tests).  CMB_SA_SPARSE=1
// keeps the walk.  An index whose walks do not all take SA[row] % sparseness steps (the LF counter of locateRow relies on it) keeps
// the walk too.  The index's DevIndex must be bound to its arrays; ix->bytes follows the array.
static void buildDenseSA(cmb_index* ix) {
    ix->bytes -= ix->saDense.bytes();
    ix->saDense.release();
    ix->d.saDense = nullptr;
    const uint64_t n = ix->d.n;
    if (getenv("CMB_SA_SPARSE") || n == 0 || ix->saSparseness == 0 || !ix->saSamples.p || !ix->d.fwd.blk) return;
    size_t freeB = 0, totalB = 0;
    HIPCHK(hipMemGetInfo(&freeB, &totalB));
    uint64_t minFree = std::min<uint64_t>(128ull << 30, totalB / 2);
    if (const char* e = getenv("CMB_TEST_SA_MIN_FREE_GB")) minFree = (uint64_t)(atof(e) * (double)(1ull << 30));
    if (freeB < n * sizeof(uint32_t) || freeB - n * sizeof(uint32_t) < minFree) return;
    ix->saDense.alloc(n);
    DevBuf<uint32_t> bad;
    bad.alloc(1);
    HIPCHK(hipMemset(bad.p, 0, sizeof(uint32_t)));
    const uint32_t nSamples = (uint32_t)std::min<size_t>(ix->saSamples.n, 0xFFFFFFFFu);
    hipLaunchKernelGGL(k_dense_sa, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 16)), dim3(256), 0, 0, ix->d, nSamples,
                       ix->saDense.p, bad.p);
    HIPCHK(hipGetLastError());
    uint32_t hb = 0;
    HIPCHK(hipMemcpy(&hb, bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (hb) {
        ix->saDense.release();
        return;
    }
    ix->d.saDense = ix->saDense.p;
    ix->bytes += ix->saDense.bytes();
}
extern "C" int cmb_index_validate(cmb_index* idx) {
    if (!idx) return fail(CMB_ERR_INVALID, "null argument");
    try {
        useDevice(idx->device);
        if (int rc = probeIndex(idx)) return rc;
        buildDenseSA(idx); // (each replica derives its own: the array is not one of the broadcast ones)
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

extern "C" int cmb_index_create(const cmb_index_desc* desc, int device, cmb_index** out) {
    if (!desc || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (desc->text_length == 0 || desc->text_length >= 0xFFFFFFFFull)
        return fail(CMB_ERR_UNSUPPORTED, "text length must fit a 32-bit length_t");
    if (desc->kmer_size > 15) return fail(CMB_ERR_INVALID, "k-mer size > 15 (the reference's -K option takes 0 ... 15, alignparameters.cpp:449)");
    if (desc->sa_sparseness == 0 || (desc->sa_sparseness & (desc->sa_sparseness - 1)))
        return fail(CMB_ERR_INVALID, "suffix array sparseness must be a power of two");
    try {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            return fail(CMB_ERR_DEVICE, "no HIP device available (the product path has no CPU fallback)");
        useDevice(device);
        // the upload boundary: the description's host arrays into HBM as they are, the rest is indexFromDeviceArrays
        const uint64_t n = desc->text_length, N = n + 1, saW = (n + 63) / 64;
        DevBuf<uint64_t> bvF, cntF, bvR, cntR, saBv, saCnt;
        DevBuf<uint32_t> samples;
        DevBuf<uint8_t> text;
        bvF.upload(desc->bv_fwd, 4 * ((N + 63) / 64)), cntF.upload(desc->cnt_fwd, 8 * ((N + 511) / 512));
        bvR.upload(desc->bv_rev, 4 * ((N + 63) / 64)), cntR.upload(desc->cnt_rev, 8 * ((N + 511) / 512));
        saBv.upload(desc->sa_bv, saW), saCnt.upload(desc->sa_bv_counts, (saW + 7) / 4);
        samples.upload(desc->sa_samples, desc->n_samples);
        text.upload(desc->text, n);
        IndexDeviceArrays a{};
        a.n = n, a.text = text.p;
        for (int i = 0; i < 5; i++) a.counts[i] = desc->counts[i];
        a.dollarFwd = desc->dollar_pos_fwd, a.dollarRev = desc->dollar_pos_rev;
        a.bvFwd = bvF.p, a.cntFwd = cntF.p, a.bvRev = bvR.p, a.cntRev = cntR.p;
        a.saBv = saBv.p, a.saBvCounts = saCnt.p, a.saSamples = samples.p, a.nSamples = desc->n_samples;
        a.saSparseness = desc->sa_sparseness, a.seqStarts = desc->seq_starts, a.nSeqs = desc->seq_starts ? desc->n_seqs : 0;
        a.kmerSize = desc->kmer_size, a.inTextSwitch = desc->in_text_switch;
        return indexFromDeviceArrays(a, device, out);
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
int cmb::indexFromDeviceArrays(const IndexDeviceArrays& a, int device, cmb_index** out) {
    try {
        useDevice(device);
        std::unique_ptr<cmb_index> ix(new cmb_index());
        ix->device = device;
        ix->saSparseness = a.saSparseness;
        const uint64_t n = a.n, N = n + 1;
        const uint64_t nBlocks = N / RANK_BLOCK + 1; // rank(N) must be answerable
        for (int dir = 0; dir < 2; dir++) {        // re-pack the reference arrays, one direction at a time
            DevBuf<uint4>& blk = dir ? ix->blkR : ix->blkF;
            blk.alloc(nBlocks * 2);
            hipLaunchKernelGGL(k_relayout, dim3((unsigned)((nBlocks + 255) / 256)), dim3(256), 0, 0, dir ? a.bvRev : a.bvFwd,
                               dir ? a.cntRev : a.cntFwd, N, nBlocks, blk.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
        }
        const uint64_t saW = (n + 63) / 64;
        { // the sparse suffix array's bitvector + rank9 counts ride in slot 3 of the forward blocks (k_relayout_sa)
            hipLaunchKernelGGL(k_relayout_sa, dim3((unsigned)((nBlocks + 255) / 256)), dim3(256), 0, 0, a.saBv, a.saBvCounts, saW,
                               nBlocks, ix->blkF.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
        }
        // (a description without samples has always left ONE element here: saSamples.n is the sample count of the probe and of
        // cmb_index_layout_of, and counts into cmb_index_device_bytes)
        ix->saSamples.alloc(std::max<size_t>(a.nSamples, 1));
        if (a.nSamples) HIPCHK(hipMemcpy(ix->saSamples.p, a.saSamples, a.nSamples * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        // padded: the verification kernels read (unaligned) 16-byte chunks up to two chunks ahead, and lanes whose
        // candidate has ended keep prefetching while their wavefront runs (at most MAX_READ + 3 k rows + 48 bytes)
        constexpr uint64_t TEXT_PAD = 640;
        static_assert(TEXT_PAD >= (uint64_t)VROWS + 64, "text padding must cover the longest verification window");
        // ... and the CIGAR kernels' reads of text[begin, end) for an occurrence that ends beyond the text: begin < n,
        // end - begin <= MAX_READ + 13 (MAX_K), and forwardPass prefetches up to 64 bytes past the longest window of its wavefront
        static_assert(TEXT_PAD >= (uint64_t)MAX_READ + 13 + 64, "text padding must cover an occurrence that begins on the last character");
        ix->text.alloc(n + TEXT_PAD);
        HIPCHK(hipMemset(ix->text.p, 0, n + TEXT_PAD));
        HIPCHK(hipMemcpy(ix->text.p, a.text, n, hipMemcpyDeviceToDevice));
        hipLaunchKernelGGL(k_encode_text, dim3(4096), dim3(256), 0, 0, ix->text.p, n, n + TEXT_PAD); // ASCII -> codes 0..4
        HIPCHK(hipGetLastError());
        bool packedOk = false;
        { // 2-bit copy for the matrix kernels (k_pack_text); the words past the text's padding are never used
            const uint64_t nWords = (n + TEXT_PAD) / 16;
            ix->text2.alloc(nWords + 16);
            HIPCHK(hipMemset(ix->text2.p, 0, (nWords + 16) * sizeof(uint32_t)));
            DevBuf<uint32_t> bad;
            bad.alloc(1);
            HIPCHK(hipMemset(bad.p, 0, sizeof(uint32_t)));
            hipLaunchKernelGGL(k_pack_text, dim3(4096), dim3(256), 0, 0, ix->text.p, n, nWords, ix->text2.p, bad.p);
            HIPCHK(hipGetLastError());
            uint32_t hb = 0;
            HIPCHK(hipMemcpy(&hb, bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
            packedOk = hb == 0 && !getenv("CMB_TEXT_BYTES");
            if (!packedOk) ix->text2.release();
        }
        ix->kmer.alloc(1ull << (2 * a.kmerSize));
        if (a.seqStarts) ix->seqStarts.assign(a.seqStarts, a.seqStarts + a.nSeqs);
        DevIndex& d = ix->d;
        d.n = (uint32_t)n;
        for (int i = 0; i < 5; i++) d.counts[i] = (uint32_t)a.counts[i];
        d.fwd = DevBWT{ix->blkF.p, (uint32_t)a.dollarFwd};
        d.rev = DevBWT{ix->blkR.p, (uint32_t)a.dollarRev};
        d.saSamples = ix->saSamples.p;
        d.saSparseness = ix->saSparseness;
        d.text = ix->text.p;
        d.text2 = packedOk ? ix->text2.p : nullptr;
        d.kmer = ix->kmer.p;
        d.kmerSize = a.kmerSize;
        d.switchPoint = a.inTextSwitch;
        const uint32_t total = 1u << (2 * a.kmerSize);
        hipLaunchKernelGGL(k_kmer_table, dim3((total + 255) / 256), dim3(256), 0, 0, d, ix->kmer.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        if (int rc = probeIndex(ix.get())) return rc; // the arrays must belong together, or findSA would never end
        ix->bytes = ix->blkF.bytes() + ix->blkR.bytes() + ix->saSamples.bytes() + ix->text.bytes() + ix->text2.bytes() + ix->kmer.bytes();
        buildDenseSA(ix.get());
        ix->uploadSeqStarts();
        *out = ix.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
// ---- replication: layout description, empty twin, raw device arrays (include/columba_amd.h)
namespace {
struct ArrayRef {
    void** p;
    size_t* n;
    size_t elem;
};
// the seven device arrays of an index in the order of cmb_index_layout::bytes
inline void indexArrays(cmb_index* ix, ArrayRef out[CMB_DEV_ARRAYS]) {
    out[0] = {(void**)&ix->blkF.p, &ix->blkF.n, sizeof(uint4)};
    out[1] = {(void**)&ix->blkR.p, &ix->blkR.n, sizeof(uint4)};
    out[2] = {(void**)&ix->saSamples.p, &ix->saSamples.n, sizeof(uint32_t)};
    out[3] = {(void**)&ix->text.p, &ix->text.n, sizeof(uint8_t)};
    out[4] = {(void**)&ix->text2.p, &ix->text2.n, sizeof(uint32_t)};
    out[5] = {(void**)&ix->kmer.p, &ix->kmer.n, sizeof(uint4)};
}
inline void bindDevIndex(cmb_index* ix) { // DevIndex pointers from the owning buffers
    DevIndex& d = ix->d;
    d.fwd.blk = ix->blkF.p;
    d.rev.blk = ix->blkR.p;
    d.saSamples = ix->saSamples.p;
    d.saDense = ix->saDense.n ? ix->saDense.p : nullptr;
    d.saSparseness = ix->saSparseness;
    d.text = ix->text.p;
    d.text2 = ix->text2.n ? ix->text2.p : nullptr;
    d.kmer = ix->kmer.p;
}
} // namespace

extern "C" int cmb_index_layout_of(const cmb_index* idx, cmb_index_layout* out) {
    if (!idx || !out) return fail(CMB_ERR_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    out->text_length = idx->d.n;
    for (int i = 0; i < 5; i++) out->counts[i] = idx->d.counts[i];
    out->dollar_pos_fwd = idx->d.fwd.dollarPos;
    out->dollar_pos_rev = idx->d.rev.dollarPos;
    out->n_samples = idx->saSamples.n;
    out->sa_sparseness = idx->saSparseness;
    out->kmer_size = idx->d.kmerSize;
    out->in_text_switch = idx->d.switchPoint;
    out->n_seqs = (uint32_t)idx->seqStarts.size();
    ArrayRef a[CMB_DEV_ARRAYS];
    indexArrays(const_cast<cmb_index*>(idx), a);
    for (int i = 0; i < CMB_DEV_ARRAYS; i++) out->bytes[i] = *a[i].p ? (uint64_t)(*a[i].n * a[i].elem) : 0;
    return CMB_OK;
}
extern "C" int cmb_index_seq_starts(const cmb_index* idx, uint32_t* out) {
    if (!idx || (!out && !idx->seqStarts.empty())) return fail(CMB_ERR_INVALID, "null argument");
    if (!idx->seqStarts.empty()) memcpy(out, idx->seqStarts.data(), idx->seqStarts.size() * sizeof(uint32_t));
    return CMB_OK;
}
// An index that holds ONLY the text (codes + 2-bit copy) and the sequence starts: what alignments, trimming at sequence ends and SAM
// records need of an index — for the b-move flavour, whose own index has no text (cmb_move_attach_text).  No batch can be created on it.
extern "C" int cmb_index_create_text_only(const char* text, uint64_t n, const uint32_t* seq_starts, uint32_t n_seqs, int device,
                                          cmb_index** out) {
    if (!text || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (n == 0 || n >= 0xFFFFFF00ull) return fail(CMB_ERR_UNSUPPORTED, "text length must fit a 32-bit length_t");
    try {
        useDevice(device);
        std::unique_ptr<cmb_index> ix(new cmb_index());
        ix->device = device;
        ix->textOnly = true;
        constexpr uint64_t TEXT_PAD = 640; // (as in cmb_index_create: the windows of k_cigar / k_cigar_wide, also of occurrences that end beyond the text)
        static_assert(TEXT_PAD >= (uint64_t)VROWS + 64 && TEXT_PAD >= (uint64_t)MAX_READ + 13 + 64, "text padding must cover the longest window");
        ix->text.alloc(n + TEXT_PAD);
        HIPCHK(hipMemset(ix->text.p, 0, n + TEXT_PAD));
        HIPCHK(hipMemcpy(ix->text.p, text, n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_encode_text, dim3(4096), dim3(256), 0, 0, ix->text.p, n, n + TEXT_PAD);
        const uint64_t nWords = (n + TEXT_PAD) / 16;
        ix->text2.alloc(nWords + 16);
        HIPCHK(hipMemset(ix->text2.p, 0, (nWords + 16) * sizeof(uint32_t)));
        DevBuf<uint32_t> bad;
        bad.alloc(1);
        HIPCHK(hipMemset(bad.p, 0, sizeof(uint32_t)));
        hipLaunchKernelGGL(k_pack_text, dim3(4096), dim3(256), 0, 0, ix->text.p, n, nWords, ix->text2.p, bad.p);
        HIPCHK(hipGetLastError());
        uint32_t hb = 0;
        HIPCHK(hipMemcpy(&hb, bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (hb) ix->text2.release();
        if (seq_starts && n_seqs) ix->seqStarts.assign(seq_starts, seq_starts + n_seqs); // (entries: the starts and the final n - 1, as cmb_index_desc)
        ix->d.n = (uint32_t)n;
        ix->d.text = ix->text.p;
        ix->d.text2 = hb ? nullptr : ix->text2.p;
        ix->uploadSeqStarts();
        ix->bytes = ix->text.bytes() + ix->text2.bytes();
        *out = ix.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

extern "C" int cmb_index_create_empty(const cmb_index_layout* L, const uint32_t* seq_starts, int device, cmb_index** out) {
    if (!L || !out) return fail(CMB_ERR_INVALID, "null argument");
    if (L->text_length == 0 || L->text_length >= 0xFFFFFFFFull || L->kmer_size > 15)
        return fail(CMB_ERR_INVALID, "index layout out of range");
    try {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            return fail(CMB_ERR_DEVICE, "no HIP device available (the product path has no CPU fallback)");
        useDevice(device);
        std::unique_ptr<cmb_index> ix(new cmb_index());
        ix->device = device;
        ix->saSparseness = L->sa_sparseness;
        ArrayRef a[CMB_DEV_ARRAYS];
        indexArrays(ix.get(), a);
        {   // the sizes must be those cmb_index_create gives an index of this text length (a kernel indexes them by position)
            const uint64_t n = L->text_length, rankBytes = ((n + 1) / RANK_BLOCK + 1) * 2 * sizeof(uint4);
            if (L->sa_sparseness == 0 || (L->sa_sparseness & (L->sa_sparseness - 1)))
                return fail(CMB_ERR_INVALID, "index layout: suffix array sparseness must be a power of two");
            if (L->bytes[0] != rankBytes || L->bytes[1] != rankBytes)
                return fail(CMB_ERR_INVALID, "index layout: rank blocks do not have the size of this text length");
            if (L->bytes[2] < ((n + L->sa_sparseness - 1) / L->sa_sparseness) * sizeof(uint32_t))
                return fail(CMB_ERR_INVALID, "index layout: fewer suffix array samples than text length / sparseness");
            if (L->bytes[3] < n) return fail(CMB_ERR_INVALID, "index layout: text shorter than the text length");
            if (L->bytes[4] != 0 && L->bytes[4] < (n + 15) / 16 * sizeof(uint32_t))
                return fail(CMB_ERR_INVALID, "index layout: 2-bit text shorter than the text length");
            if (L->bytes[5] != (sizeof(uint4) << (2 * L->kmer_size)))
                return fail(CMB_ERR_INVALID, "index layout: k-mer table does not have 4^k entries");
        }
        uint64_t total = 0;
        for (int i = 0; i < CMB_DEV_ARRAYS; i++) {
            if (L->bytes[i] % a[i].elem) return fail(CMB_ERR_INVALID, "index layout: array size is not a whole number of elements");
            if (L->bytes[i] == 0) continue; // absent (2-bit text)
            HIPCHK(hipMalloc(a[i].p, L->bytes[i]));
            *a[i].n = L->bytes[i] / a[i].elem;
            total += L->bytes[i];
        }
        if (!ix->blkF.p || !ix->blkR.p || !ix->text.p || !ix->kmer.p)
            return fail(CMB_ERR_INVALID, "index layout: a required array is missing");
        DevIndex& d = ix->d;
        d.n = (uint32_t)L->text_length;
        for (int i = 0; i < 5; i++) d.counts[i] = (uint32_t)L->counts[i];
        d.fwd.dollarPos = (uint32_t)L->dollar_pos_fwd;
        d.rev.dollarPos = (uint32_t)L->dollar_pos_rev;
        d.kmerSize = L->kmer_size;
        d.switchPoint = L->in_text_switch;
        bindDevIndex(ix.get());
        if (seq_starts && L->n_seqs) ix->seqStarts.assign(seq_starts, seq_starts + L->n_seqs);
        ix->uploadSeqStarts();
        ix->bytes = total;
        *out = ix.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_index_device_arrays(cmb_index* idx, void** ptrs, uint64_t* bytes) {
    if (!idx || !ptrs || !bytes) return fail(CMB_ERR_INVALID, "null argument");
    ArrayRef a[CMB_DEV_ARRAYS];
    indexArrays(idx, a);
    for (int i = 0; i < CMB_DEV_ARRAYS; i++) {
        ptrs[i] = *a[i].p;
        bytes[i] = *a[i].p ? (uint64_t)(*a[i].n * a[i].elem) : 0;
    }
    return CMB_OK;
}

extern "C" void cmb_index_destroy(cmb_index* idx) {
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    delete idx;
}
extern "C" uint64_t cmb_index_device_bytes(const cmb_index* idx) { return idx ? idx->bytes : 0; }
extern "C" int cmb_index_kmer_table(const cmb_index* idx, uint32_t* out) {
    if (!idx || !out) return fail(CMB_ERR_INVALID, "null argument");
    try {
        useDevice(idx->device);
        HIPCHK(hipMemcpy(out, idx->kmer.p, idx->kmer.bytes(), hipMemcpyDeviceToHost));
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

// --------------------------------------------------------------------------------- strategy
extern "C" int cmb_strategy_create(int metric, int partition, uint32_t kmer_cutoff, cmb_strategy** out) {
    if (!out || metric < 0 || metric > 1 || partition < 0 || partition > 2)
        return fail(CMB_ERR_INVALID, "bad metric / partition strategy");
    cmb_strategy* s = new cmb_strategy();
    s->metric = metric;
    s->partition = partition;
    s->kmerCutOff = kmer_cutoff;
    *out = s;
    return CMB_OK;
}
extern "C" int cmb_strategy_create_named(const char* name, int metric, int partition, cmb_strategy** out) {
    cmb_strategy* s = nullptr;
    int rc = cmb_strategy_create(metric, partition, 20, &s);
    if (rc) return rc;
    try {
        fillNamed(*s, name ? name : "");
    } catch (const std::exception& e) {
        delete s;
        return fail(CMB_ERR_INVALID, e.what());
    }
    *out = s;
    return CMB_OK;
}
extern "C" int cmb_strategy_create_from_dir(const char* dir, int mode, int metric, int partition,
                                            cmb_strategy** out) {
    if (mode < CMB_DIR_CUSTOM || mode > CMB_DIR_CUSTOM_DYNAMIC) return fail(CMB_ERR_INVALID, "bad scheme directory mode");
    cmb_strategy* s = nullptr;
    int rc = cmb_strategy_create(metric, partition, 20, &s);
    if (rc) return rc;
    try {
        if (mode == CMB_DIR_MULTIPLE) fillFromMultipleDir(*s, dir ? dir : "");
        else fillFromCustomDir(*s, dir ? dir : "", mode == CMB_DIR_CUSTOM_DYNAMIC);
    } catch (const std::exception& e) {
        delete s;
        return fail(CMB_ERR_INVALID, e.what());
    }
    *out = s;
    return CMB_OK;
}
extern "C" int cmb_strategy_add_scheme(cmb_strategy* s, uint32_t k, uint32_t n_searches, uint32_t n_parts,
                                       const uint32_t* pi, const uint32_t* L, const uint32_t* U) {
    if (!s || !pi || !L || !U) return fail(CMB_ERR_INVALID, "null argument");
    try {
        HostScheme sch;
        sch.k = k;
        for (uint32_t i = 0; i < n_searches; i++) {
            HostSearch h;
            h.pi.assign(pi + i * n_parts, pi + (i + 1) * n_parts);
            h.L.assign(L + i * n_parts, L + (i + 1) * n_parts);
            h.U.assign(U + i * n_parts, U + (i + 1) * n_parts);
            h.sIdx = i;
            sch.searches.push_back(h);
        }
        sch.finalize();
        for (const auto& h : sch.searches) (void)toDevSearch(h);
        s->schemes[k].push_back(sch);
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_INVALID, e.what());
    }
}
extern "C" int cmb_strategy_set_partition_params(cmb_strategy* s, uint32_t k, const double* seeding,
                                                 uint32_t n_seeding, const uint64_t* weights, uint32_t n_weights,
                                                 const double* begins, uint32_t n_begins) {
    if (!s) return fail(CMB_ERR_INVALID, "null argument");
    PartitionParams pp;
    if (n_seeding) pp.seeding.assign(seeding, seeding + n_seeding);
    if (n_weights) pp.weights.assign(weights, weights + n_weights);
    if (n_begins) pp.begins.assign(begins, begins + n_begins);
    s->params[k] = pp;
    return CMB_OK;
}
extern "C" void cmb_strategy_destroy(cmb_strategy* s) { delete s; }
extern "C" int cmb_strategy_describe(const cmb_strategy* s, uint32_t k, uint32_t* n_schemes, uint32_t* n_parts,
                                     uint32_t* critical_parts, uint32_t cap) {
    if (!s) return fail(CMB_ERR_INVALID, "null argument");
    auto it = s->schemes.find(k);
    if (it == s->schemes.end() || it->second.empty())
        return fail(CMB_ERR_INVALID, "the search strategy does not support distance " + std::to_string(k));
    if (n_schemes) *n_schemes = (uint32_t)it->second.size();
    if (n_parts) *n_parts = it->second.front().numParts();
    for (uint32_t i = 0; critical_parts && i < cap && i < it->second.size(); i++)
        critical_parts[i] = it->second[i].critical;
    return CMB_OK;
}
extern "C" int cmb_strategy_export_scheme(const cmb_strategy* s, uint32_t k, uint32_t scheme, uint32_t* pi, uint32_t* L,
                                          uint32_t* U, uint32_t cap, uint32_t* n_searches, uint32_t* n_parts) {
    if (!s) return fail(CMB_ERR_INVALID, "null argument");
    auto it = s->schemes.find(k);
    if (it == s->schemes.end() || scheme >= it->second.size())
        return fail(CMB_ERR_INVALID, "the search strategy has no such scheme for distance " + std::to_string(k));
    const HostScheme& h = it->second[scheme];
    const uint32_t ns = (uint32_t)h.searches.size(), np = h.numParts();
    if (n_searches) *n_searches = ns;
    if (n_parts) *n_parts = np;
    if ((uint64_t)ns * np > cap) return fail(CMB_ERR_OVERFLOW, "output arrays too small");
    for (uint32_t i = 0; i < ns; i++)
        for (uint32_t j = 0; j < np; j++) {
            if (pi) pi[i * np + j] = h.searches[i].pi[j];
            if (L) L[i * np + j] = h.searches[i].L[j];
            if (U) U[i * np + j] = h.searches[i].U[j];
        }
    return CMB_OK;
}
extern "C" int cmb_strategy_export_partition(const cmb_strategy* s, uint32_t k, double* seeding, uint64_t* weights,
                                             double* begins, uint32_t cap, uint32_t* kmer_cutoff) {
    if (!s) return fail(CMB_ERR_INVALID, "null argument");
    try {
        const PartitionParams d = s->partitionFor(k);
        const uint32_t P = (uint32_t)d.weights.size();
        if (P > cap) return fail(CMB_ERR_OVERFLOW, "output arrays too small");
        for (uint32_t i = 0; i + 2 < P && seeding; i++) seeding[i] = d.seeding[i];
        for (uint32_t i = 0; i < P && weights; i++) weights[i] = d.weights[i];
        for (uint32_t i = 0; i + 1 < P && begins; i++) begins[i] = d.begins[i];
        if (kmer_cutoff) *kmer_cutoff = s->kmerCutOff;
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_INVALID, e.what());
    }
}

// ------------------------------------------------------------------------------------ batch
struct cmb_batch {
    cmb_index* ix = nullptr;
    uint32_t k = 0, nReads = 0, maxLen = 0, gw = 0;
    uint32_t minLen = 0; // shortest read of the batch and of every chunk staged since (picks the verification stages
                         // that carry final-column code)
    int metric = 1;
    DevStrategyK hostStrat{};
    // schemes with more than MAXP parts (the greedy schemes for 8 ... 13 errors): tables of MAXP_WIDE parts, run by the wide instances
    // of k_parts / k_exact / k_hbfs (Hamming distance; the edit-distance matcher stops at 7 errors)
    bool wide = false;
    bool wideEdit = false; // edit distance 8 ... 13: wide records AND the wide layout of the filter keys
    bool noSmallMatrix = false; // a phase of an earlier run did not fit the 32-bit in-index matrix (GeoN32): this batch stays on GeoN
    DevStrategyKT<MAXP_WIDE> hostStratW{};
    DevBuf<DevStrategyKT<MAXP_WIDE>> stratW;
    DevBuf<PartOutT<MAXP_WIDE>> partsW;
    uint32_t sNumParts = 0, sPartition = 0, sNSchemes = 0, sMaxSearches = 0; // of whichever table the batch runs on
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> reads, seq;
    DevBuf<uint32_t> rec; // read records for k_parts / k_exact (k_prep)
    DevBuf<ExactTask> exq; // searches with further exact phases (k_parts -> k_exact)
    DevBuf<uint8_t> psel; // selected scheme per read x strand (bit 7: nothing to search)
    uint32_t recW = 0;
    DevBuf<uint64_t> offs;
    DevBuf<uint32_t> G;
    DevBuf<uint4> mfull; // match words of the full reads per 32-row block (k_prep)
    DevBuf<DevStrategyK> strat;
    // frontier search (dev_bfs_edit.hpp): node / event double buffers, F records, contexts, list arena
    DevBuf<uint4> bfsQ[2], bfsEv[2], bfsF, bfsC, bfsA;
    DevBuf<uint32_t> bfsCnt;               // nq[passes], ne[passes], pool[4]
    DevBuf<unsigned long long> bfsBlockCnt; // [BFS_GRID_CNT][4]
    size_t bfsQCap = 0, bfsEvCap = 0, bfsFCap = 0, bfsCCap = 0, bfsACap = 0;
    // naive backtracking (dev_bfs_naive.hpp): node double buffer, nodes per pass
    DevBuf<uint4> nvQ[2];
    DevBuf<uint32_t> nvCnt;
    size_t nvQCap = 0;
    bool hasNaive = false; // reads of the running chunk take that path (k_parts marked them in psel)
    DevBuf<PartOut> parts;
    DevBuf<DfsTask> dfs;
    DevBuf<uint64_t> vW; // packed trace rows [row][slot]
    DevBuf<uint4> tbq;
    DevBuf<uint8_t> dpSlab; // k_verify_wide: the band rows of one candidate per slot
    DevBuf<uint32_t> dpList, dpWork; // k_wide_filter: the keys that go on to k_verify_wide; [0] next key, [1] number of those
    DevBuf<uint4> items;
    DevBuf<FMOccRec> fm, fmUniq;
    DevBuf<TextOccRec> text;
    DevBuf<uint4> fout;
    DevBuf<unsigned long long> keysA, keysB;
    DevBuf<uint32_t> fcounts, fsegB, fsegE, frank;
    DevBuf<uint64_t> foffs;
    DevBuf<unsigned long long> fmKeysA, fmKeysB;
    DevBuf<uint32_t> fmIdxA, fmIdxB, fmN;
    DevBuf<uint8_t> sortTmp, scanTmp;
    DevBuf<unsigned long long> vkeysA, vkeysB; // verification keys (k_verify) / sorted, then distinct
    DevBuf<uint32_t> vcounts, vruns;           // multiplicities of the distinct keys / number of runs
    DevBuf<uint4> vsA[2], vsB[2];              // staged verification: survivor lists (ping-pong)
    DevBuf<uint32_t> vsC[2], vsN;
    DevBuf<uint32_t> cnt;
    DevBuf<unsigned long long> counters;
    uint32_t nSlots = 0;
    std::vector<uint64_t> hostOffs;
    bool perStrand = false; // every strand filtered by itself (BEST mode: mapRead, searchstrategy.h:490-523)
    // alignments of the final occurrences (cmb_batch_want_alignments): CIGAR runs + sequence assignment
    bool wantAln = false;
    DevBuf<uint32_t> foutRead;
    DevBuf<uint16_t> alnOps;
    DevBuf<AlnRec> alnRec;
    uint32_t alnStride = 0;
    PinnedBuf<uint16_t> hAlnOps;
    PinnedBuf<AlnRec> hAlnRec;
    // occurrences over the end of their sequence trimmed on the device (cmb_batch_trim_on_device; dev_trim.hpp): the direct items with their
    // occurrences, the verification's records, counters and flags — its own, the search counters of the batch stay as the search left
    // them —, the keys of the records, the survivors with their alignments
    bool trimOn = false;
    uint64_t trimStats[3] = {0, 0, 0}; // spanning, trimmed, dropped occurrences of the last run
    DevBuf<uint4> trimItems, trimPickOcc;
    DevBuf<uint32_t> trimItemOcc, trimPickRead, trimPickDst, trimCnt; // trimCnt: [0, 8) as Queues::cnt, [8] spanning, [9] items, [10] survivors
    DevBuf<TextOccRec> trimText;
    DevBuf<unsigned long long> trimKeysA, trimKeysB, trimCounters;
    DevBuf<AlnRec> trimAln;
    DevBuf<uint16_t> trimOps;
    SamBufs samBufs; // (what the SAM and pair drivers keep with this part: cmb_batch_sam_device, cmb_pair_sam_device, sam.hip)
    // cmb_verify_batch_staged: candidates given by the caller take the place of the search's in-text items, and the
    // raw text occurrences (before the filter) are what is handed back
    std::vector<uint4> presetItems;
    std::vector<TextOccRec> presetOut;
    // A large batch is a COMPOSITE of sub-batches that run concurrently, one host thread + HIP stream each: the
    // stages of different sub-batches drift apart, so VALU-bound matrix kernels of one overlap memory-bound
    // extension kernels of another (starting them one after the other on purpose was measured slower: the
    // device idles at both ends).
    std::vector<cmb_batch*> subs;
    std::vector<uint32_t> subBound; // composite: first read of every sub-batch (+ total)
    // the NEXT chunk of reads, uploaded on a stream of its own while this one is being matched (cmb_batch_stage_reads);
    // cmb_batch_run swaps it in
    DevBuf<uint8_t> readsStage;
    DevBuf<uint64_t> offsStage;
    std::vector<uint64_t> hostOffsStage, hostOffsActive;
    // the offsets of a registered chunk once more in PAGE-LOCKED memory, two buffers taking turns: the upload a run starts must not stall
    // the host (from pageable memory hipMemcpyAsync copies through bounce buffers before it returns — milliseconds in which the run has
    // not launched a kernel yet), and the next registration must not overwrite offsets the copy engine is still reading
    PinnedBuf<uint64_t> offsPin[2];
    int pinNext = 0, pinStaged = 0;
    hipStream_t copyStream = nullptr;
    hipEvent_t copyDone = nullptr;
    bool staged = false;                 // readsStage / offsStage hold an uploaded chunk (or its upload is in flight)
    const char* pendingSeqs = nullptr;   // a registered chunk whose upload the next run starts
    bool pending = false;
    cmb_batch* parent = nullptr;
    uint32_t subIndex = 0;
    // results
    PinnedBuf<cmb_occ> occs;
    PinnedBuf<uint64_t> occOffs;
    uint64_t cnts[CMB_CNT_MAX];
    std::vector<KernelTime> times;
    bool done = false;
    ~cmb_batch() {
        for (cmb_batch* c : subs) delete c;
        if (copyDone) (void)hipEventDestroy(copyDone);
        if (copyStream) (void)hipStreamDestroy(copyStream);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

static int batchCreateOne(cmb_index* idx, const cmb_strategy* st, uint32_t max_distance, const char* seqs,
                          const uint64_t* offs, uint32_t n_reads, cmb_batch** out);
constexpr uint32_t MAX_SUB_READS = 1u << 23; // reads per sub-batch (keys: kernels.hpp k_pack_keys, packVerifyKey)
// bits of the group (the read, or read x strand when every strand is filtered by itself) in the filter keys of a
// sub-batch: 24 in layouts 0 and 1, 22 in the wide layout 2 (dev_search.hpp: keyBits)
static uint32_t keyLayoutOf(const cmb_batch* b) { return b->metric == CMB_METRIC_HAMMING ? 1u : b->wideEdit ? 2u : 0u; }
static uint32_t groupBits(const cmb_batch* b) { return 64u - keyBits(keyLayoutOf(b)).group; }

extern "C" int cmb_batch_create(cmb_index* idx, const cmb_strategy* st, uint32_t max_distance, const char* seqs,
                                const uint64_t* offs, uint32_t n_reads, cmb_batch** out) {
    if (!idx || !st || !offs || !out || (!seqs && n_reads)) return fail(CMB_ERR_INVALID, "null argument");
    if (idx->textOnly) return fail(CMB_ERR_INVALID, "this index holds only the text (cmb_index_create_text_only): nothing can be matched on it");
    if (n_reads >= 0x7FFFFFFFu) return fail(CMB_ERR_INVALID, "too many reads in one batch");
    // sub-batches: 3 from 8 M reads, 2 from 2 M (below that the fixed cost per frontier level dominates; measured
    // on 10 M reads: 1 -> 26.4, 2 -> 30.4, 3 -> 30.6, 4 -> 29.5 M reads/s); CMB_SUBBATCHES overrides
    uint32_t S = n_reads >= 8000000u ? 3u : n_reads >= 2000000u ? 2u : 1u;
    if (getenv("CMB_SUBBATCHES")) S = (uint32_t)std::max(1, atoi(getenv("CMB_SUBBATCHES")));
    // a sub-batch holds fewer than 2^24 reads (24-bit read number of the filter key, 25 bits of read x strand in the
    // verification key): larger batches are cut into more sub-batches up front, never refused after the work is done
    // (a sub-batch made larger than its keys hold by CMB_SUBBATCH_SPLIT is refused here, or by cmb_batch_filter_per_strand
    // when read x strand would not fit: both before any work)
    // (22 group bits in the wide filter keys; from 11 errors on the frontier of a read can hold millions of nodes on a large reference —
    // 20 000 reads at 12 errors on 3 Gbp overflowed pools of 2^32 slots —, so those sub-batches are small and run three at a time)
    const uint32_t maxSub = st->metric != CMB_METRIC_EDIT || max_distance <= 7 ? MAX_SUB_READS : max_distance <= MX_MAX_ED ? (1u << 20) : (1u << 11);
    S = std::max<uint32_t>(S, (uint32_t)(((uint64_t)n_reads + maxSub - 1) / maxSub));
    S = std::min<uint32_t>(S, std::max<uint32_t>(n_reads, 1u));
    if (S <= 1) return batchCreateOne(idx, st, max_distance, seqs, offs, n_reads, out);
    std::unique_ptr<cmb_batch> parent(new cmb_batch());
    parent->ix = idx;
    parent->k = max_distance;
    parent->nReads = n_reads;
    parent->metric = st->metric;
    // slice bounds: equal shares, or CMB_SUBBATCH_SPLIT="w0,w1,..." (relative weights; unequal sub-batches reach
    // their stages at different times)
    std::vector<double> wts(S, 1.0);
    if (const char* sp = getenv("CMB_SUBBATCH_SPLIT")) {
        std::vector<double> w;
        for (const char* q = sp; *q;) {
            char* e = nullptr;
            const double v = strtod(q, &e);
            if (e == q) break;
            if (v > 0) w.push_back(v);
            q = *e == ',' ? e + 1 : e;
        }
        if (w.size() == S) wts = w;
    }
    double wsum = 0;
    for (double v : wts) wsum += v;
    std::vector<uint32_t> bound(S + 1, 0);
    {
        double acc = 0;
        for (uint32_t j = 0; j < S; j++) {
            acc += wts[j];
            bound[j + 1] = j + 1 == S ? n_reads : (uint32_t)((double)n_reads * (acc / wsum));
        }
    }
    for (uint32_t j = 0; j < S; j++) {
        const uint32_t lo = bound[j], hi = std::max(bound[j + 1], bound[j]);
        std::vector<uint64_t> o(hi - lo + 1);
        for (uint32_t i = lo; i <= hi; i++) {
            if (i > lo && offs[i] < offs[i - 1]) return fail(CMB_ERR_INVALID, "read offsets must be non-decreasing");
            o[i - lo] = offs[i] - offs[lo];
        }
        cmb_batch* c = nullptr;
        const int rc = batchCreateOne(idx, st, max_distance, seqs + offs[lo], o.data(), hi - lo, &c);
        if (rc != CMB_OK) return rc;
        c->parent = parent.get();
        c->subIndex = j;
        parent->subs.push_back(c);
    }
    parent->subBound = bound;
    *out = parent.release();
    return CMB_OK;
}

static int batchCreateOne(cmb_index* idx, const cmb_strategy* st, uint32_t max_distance, const char* seqs,
                          const uint64_t* offs, uint32_t n_reads, cmb_batch** out) {
    try {
        useDevice(idx->device);
        std::unique_ptr<cmb_batch> b(new cmb_batch());
        b->ix = idx;
        b->k = max_distance;
        b->nReads = n_reads;
        b->metric = st->metric;
        if (n_reads >= (1u << 24)) // (only reachable through CMB_SUBBATCH_SPLIT weights: checked before any work)
            return fail(CMB_ERR_UNSUPPORTED, "more than 2^24 reads in one sub-batch");
        if (max_distance > 0) {
            // in-text verification: nZeros + maxED = 3k+1 must fit the first column of the in-text matrix (the reference
            // switches to its 128-bit matrix at k = 7, fmindex.h:240-246; here: 64-bit words / 16-row blocks, LEFT = 22)
            // edit distance beyond 7 errors: the wide record geometry of the frontier (GeoW up to 10 errors, the reach of the reference's
            // 64-bit in-index matrix; GeoX with its 16-row blocks beyond); the staged in-text matrices stop at 7, candidates are verified by
            // k_wide_filter + k_verify_wide
            b->wideEdit = st->metric == CMB_METRIC_EDIT && 3 * max_distance + 1 > MXW_LEFT;
            try {
                b->wide = st->numPartsFor(max_distance) > (uint32_t)MAXP || b->wideEdit;
                if (max_distance > 13) return fail(CMB_ERR_UNSUPPORTED, "more than 13 errors (MAX_K, definitions.h:50)");
                adoptStrategy(b.get(), st, max_distance);
            } catch (const std::exception& e) {
                return fail(CMB_ERR_INVALID, e.what());
            }
        }
        if ((uint64_t)n_reads >= (1ull << groupBits(b.get()))) // (wide keys: 22 group bits)
            return fail(CMB_ERR_UNSUPPORTED, "more than 2^" + std::to_string(groupBits(b.get())) + " reads in one sub-batch at this distance");
        uint32_t maxLen, minLen;
        if (!readLengths(offs, n_reads, minLen, maxLen)) return fail(CMB_ERR_INVALID, "read offsets must be non-decreasing");
        b->minLen = n_reads ? minLen : 0u;
        if (maxLen > (uint32_t)MAX_READ)
            return fail(CMB_ERR_UNSUPPORTED, "reads longer than " + std::to_string(MAX_READ) + " are not supported");
        maxLen = paddedLen(maxLen);
        b->maxLen = maxLen;
        b->gw = gWords(maxLen);
        b->hostOffs.assign(offs, offs + n_reads + 1);
        HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        b->reads.uploadPadded((const uint8_t*)seqs, offs[n_reads], 64);
        b->offs.upload(offs, n_reads + 1);
        b->seq.alloc((size_t)2 * n_reads * maxLen);
        b->G.alloc((size_t)n_reads * 8 * b->gw); // eight bit-strings per read (both strands use them: gString)
        b->recW = ((1 + 2 * ((maxLen + 31) / 32)) + 3) / 4 * 4;
        b->rec.alloc((size_t)2 * n_reads * b->recW);
        if (b->wide) {
            b->stratW.upload(&b->hostStratW, 1);
            b->partsW.alloc((size_t)2 * n_reads);
        } else {
            b->strat.upload(&b->hostStrat, 1);
            b->parts.alloc((size_t)2 * n_reads);
        }
        // first guesses; a queue that turns out too small grows and the search runs again (CMB_TEST_SMALL_POOLS starts the queues of
        // the prologue from almost nothing so that tests exercise that path)
        const bool smallPools = getenv("CMB_TEST_SMALL_POOLS") != nullptr;
        b->dfs.alloc(smallPools ? 64 : (size_t)n_reads * 2 + 4096);
        b->items.alloc(smallPools ? 64 : (size_t)n_reads * 64 + 4096);
        b->exq.alloc(smallPools ? 16 : 65536);
        b->fm.alloc((size_t)n_reads * 8 + 4096);
        b->text.alloc((size_t)n_reads * 48 + 4096);
        b->cnt.alloc(8);
        b->counters.alloc(CMB_CNT_MAX);
        *out = b.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

namespace {

struct HostOcc {
    uint32_t begin, end, dist, strand;
};

// ordering of TextOcc (indexhelpers.h:779-795) with the strand as final, deterministic tie-break
inline bool occLess(const HostOcc& a, const HostOcc& b) {
    if (a.begin != b.begin) return a.begin < b.begin;
    if (a.dist != b.dist) return a.dist < b.dist;
    const uint32_t wa = a.end > a.begin ? a.end - a.begin : 0, wb = b.end > b.begin ? b.end - b.begin : 0;
    if (wa != wb) return wa < wb;
    return a.strand < b.strand;
}

} // namespace

static int batchRunOne(cmb_batch* b);

extern "C" int cmb_batch_run(cmb_batch* b) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    if (b->subs.empty()) return batchRunOne(b);
    b->done = false;
    std::vector<int> rc(b->subs.size(), CMB_OK);
    std::vector<std::string> err(b->subs.size());
    // CMB_SERIAL_SUBBATCHES: one sub-batch after the other — every kernel has the device to itself, which is what
    // per-kernel timings and counters want (bench.py times its throughput steps concurrently and takes the
    // kernel table from one extra serial step)
    const bool serial = getenv("CMB_SERIAL_SUBBATCHES") != nullptr;
    // workers take the sub-batches in order, three at a time (the number that pays, cmb_batch_create); CMB_MAX_CONCURRENT=m: at most m
    const char* mcEnv = getenv("CMB_MAX_CONCURRENT");
    size_t nWorkers = serial ? 1 : std::min<size_t>(b->subs.size(), 3);
    if (mcEnv && !serial) nWorkers = std::min<size_t>(b->subs.size(), std::max(1, atoi(mcEnv)));
    // (beyond 7 errors, where the sub-batches are many and their pools large, a finished sub-batch gives its pools back: the next one allocates what it needs)
    const bool manySubs = b->subs.size() > 3 && b->k > 7;
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (size_t w = 0; w < nWorkers; w++)
        th.emplace_back([&] {
            for (;;) {
                const size_t j = next.fetch_add(1);
                if (j >= b->subs.size()) break;
                cmb_batch* c = b->subs[j];
                rc[j] = batchRunOne(c);
                if (rc[j] != CMB_OK) err[j] = cmb_last_error(); // (the message lives in the worker's thread-local storage)
                if (manySubs) { // (results, alignments and counters are on the host; a second run allocates again)
                    for (int q2 = 0; q2 < 2; q2++) c->bfsQ[q2].release(), c->bfsEv[q2].release();
                    c->bfsF.release(), c->bfsC.release(), c->bfsA.release(), c->dpSlab.release(), c->dpList.release(), c->vW.release();
                    c->sortTmp.release(), c->scanTmp.release(), c->vkeysA.release(), c->vkeysB.release();
                }
            }
        });
    for (auto& t : th) t.join();
    for (size_t j = 0; j < rc.size(); j++)
        if (rc[j] != CMB_OK) return fail(rc[j], err[j]);
    foldSubBatches(b);
    b->done = true;
    return CMB_OK;
}

// Streaming: the reads of the NEXT chunk (same number of reads, none longer than the batch was created for) are copied
// to the device on a stream of their own while the current chunk is matched; the next cmb_batch_run takes them.  The
// host memory must stay valid until that run has started (page-locked memory makes the copy asynchronous and fast).
extern "C" int cmb_batch_stage_reads(cmb_batch* b, const char* seqs, const uint64_t* offs, uint32_t n_reads) {
    if (!b || !offs || (!seqs && n_reads)) return fail(CMB_ERR_INVALID, "null argument");
    if (n_reads != b->nReads) return fail(CMB_ERR_INVALID, "a staged chunk must hold as many reads as the batch was created with");
    if (!b->subs.empty()) {
        for (size_t j = 0; j < b->subs.size(); j++) {
            const uint32_t lo = b->subBound[j], hi = b->subBound[j + 1];
            std::vector<uint64_t> o(hi - lo + 1);
            for (uint32_t i = lo; i <= hi; i++) o[i - lo] = offs[i] - offs[lo];
            const int rc = cmb_batch_stage_reads(b->subs[j], seqs + offs[lo], o.data(), hi - lo);
            if (rc != CMB_OK) return rc;
        }
        return CMB_OK;
    }
    uint32_t maxLen, minLen;
    if (!readLengths(offs, n_reads, minLen, maxLen)) return fail(CMB_ERR_INVALID, "read offsets must be non-decreasing");
    b->minLen = std::min(b->minLen, n_reads ? minLen : 0u);
    if (maxLen > b->maxLen) return fail(CMB_ERR_INVALID, "a staged read is longer than the batch was created for");
    if (b->pending) return fail(CMB_ERR_INVALID, "a chunk is already registered for the next run");
    b->hostOffsStage.assign(offs, offs + n_reads + 1);
    b->offsPin[b->pinNext].resize((size_t)n_reads + 1);
    memcpy(b->offsPin[b->pinNext].p, offs, ((size_t)n_reads + 1) * sizeof(uint64_t));
    b->pinStaged = b->pinNext;
    b->pinNext ^= 1;
    b->pendingSeqs = seqs;
    b->pending = true;
    return CMB_OK;
}
// start the upload of the registered chunk on the copy stream (called by a run, right after its own reads are in place)
static void startStagedUpload(cmb_batch* b) {
    if (!b->copyStream) {
        HIPCHK(hipStreamCreateWithFlags(&b->copyStream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&b->copyDone, hipEventDisableTiming));
    }
    const uint32_t n = b->nReads;
    const size_t nChars = b->hostOffsStage[n];
    if (b->readsStage.n < nChars) b->readsStage.alloc(nChars + nChars / 16 + 256);
    if (b->offsStage.n < (size_t)n + 1) b->offsStage.alloc((size_t)n + 1);
    if (nChars) HIPCHK(hipMemcpyAsync(b->readsStage.p, b->pendingSeqs, nChars, hipMemcpyHostToDevice, b->copyStream));
    HIPCHK(hipMemcpyAsync(b->offsStage.p, b->offsPin[b->pinStaged].p, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice,
                          b->copyStream));
    HIPCHK(hipEventRecord(b->copyDone, b->copyStream));
    b->pending = false;
    b->staged = true;
}

// ---- launches that more than one function makes ---------------------------------------------------------------------------------
// 64-byte lines of the trace rows of one slot: 16 narrow (k <= TBN_MAX_ED) or 8 wide rows to a line (a group is written whole)
static uint32_t traceLines(bool narrow, uint32_t rows) { return narrow ? (rows + 15u) / 16u + 2u : (rows + 7u) / 8u + 2u; }

// k_traceback over the nTb tasks of tbq (runTraceback, verifyDirect): the instance of the trace rows and of the text — packed or bytes;
// the wide rows read either text through one instance
static void launchTraceback(hipStream_t s, const DevIndex& d, bool narrow, const uint64_t* offs, MFull mf, const uint4* tbq, uint32_t nTb, VPlanes vp,
                            Queues q, uint32_t rowMin, bool byItem = false /* the tasks of k_verify<false, true> (trimSpanning) */) {
    auto kTrace = withBools([](auto nrw, auto packed, auto item) { return k_traceback<nrw(), nrw() && packed(), item()>; }, narrow,
                            d.text2 != nullptr, byItem);
    hipLaunchKernelGGL(kTrace, dim3(vp.nSlots / 256), dim3(256), 0, s, d, offs, mf, tbq, nTb, vp, q, rowMin);
}

// The CIGAR step of a run (runCigar), cmb::moveCigarsOnText and cmb_cigar_windows: CIGAR and sequence assignment of nOcc occurrences
// {begin, end, distance, strand} of the reads occRead (device pointers throughout).  wide: k_cigar_wide, the matrix with the wide left margin
// (k_cigar's match words reach 9 columns right of the diagonal: beyond CIGAR_BLOCK_WORDS_MAX_ED errors), at most 64 k slots of `slab`;
// otherwise the k_cigar instance of the trace rows (narrow or wide, for `rows` matrix rows per slot of vW) and of the text.  The caller says
// which, owns the scratch — it grows to what the launch needs — and counts the slots
struct CigarJob {
    const uint64_t* offs;
    const uint32_t* G;
    uint32_t gw, maxLen;
    MFull mf;
    const uint4* occs;
    const uint32_t* occRead;
    uint64_t nOcc;
    uint16_t* ops;
    uint32_t stride;
    AlnRec* aln;
    uint32_t* flagWord;
    uint32_t gapless;
};
static void launchCigar(cmb_index* ix, hipStream_t s, const CigarJob& j, bool wide, bool narrow, uint32_t rows, uint32_t slots, DevBuf<uint64_t>& vW,
                        DevBuf<uint8_t>& slab, bool verbose) {
    if (wide) {
        const uint32_t wSlots = std::min<uint32_t>(slots, 256u * 256u);
        const uint32_t slotBytes = (vwRows(j.maxLen) + 1u) * VW_ROW_BYTES;
        gridLine(verbose, "k_cigar_wide", j.nOcc, wSlots);
        if (slab.n < (size_t)slotBytes * wSlots) slab.alloc((size_t)slotBytes * wSlots);
        hipLaunchKernelGGL(k_cigar_wide, dim3(wSlots / 256), dim3(256), 0, s, ix->d, j.offs, j.G, j.gw, j.occs, j.occRead, j.nOcc, slab.p, slotBytes,
                           ix->seqStartsDev.p, ix->nSeqsDev, j.ops, j.stride, j.aln, j.flagWord, 0u);
        return;
    }
    const uint32_t tLines = traceLines(narrow, rows);
    if (vW.n < (size_t)tLines * 8 * slots) vW.alloc((size_t)tLines * 8 * slots);
    VPlanes vp{vW.p, slots, tLines};
    auto kc = withBools([](auto nrw, auto packed) { return k_cigar<nrw(), packed()>; }, narrow, ix->d.text2 != nullptr);
    gridLine(verbose, "k_cigar", j.nOcc, slots);
    hipLaunchKernelGGL(kc, dim3(slots / 256), dim3(256), 0, s, ix->d, j.offs, j.mf, j.occs, j.occRead, j.nOcc, vp, ix->seqStartsDev.p, ix->nSeqsDev, j.ops,
                       j.stride, j.aln, j.flagWord, j.gapless);
}

// k_prep over nReads reads (runPrep, verifyDirect, cmb_cigar_windows): the codes, the bit-strings, the read records (rec, or null) and the
// match words of the full reads (mfull with nBlk blocks per read x strand, or null) in one launch that leaves no word of them unwritten.
// A block takes as many reads per pass as give it a (read, chunk) pair per thread; at most 64 k blocks loop over the passes
static void launchPrep(hipStream_t s, const uint8_t* reads, const uint64_t* offs, uint32_t nReads, uint32_t maxLen, uint32_t gw, uint8_t* seq, uint32_t* G,
                       uint32_t* rec, uint32_t recW, uint4* mfull, uint32_t nBlk, bool verbose) {
    const uint32_t chunks = (maxLen + 31) / 32;
    const uint32_t perPass = std::max(1u, 256u / chunks);
    const uint32_t passes = (nReads + perPass - 1) / perPass;
    const uint32_t blocks = capBlocks(std::min<uint32_t>(passes, 65536u));
    gridLine(verbose, "k_prep", passes, (uint64_t)blocks * 256);
    if (!blocks) return;
    hipLaunchKernelGGL(k_prep, dim3(blocks), dim3(256), prepLdsWords(perPass, gw) * sizeof(uint32_t), s, reads, offs, nReads, maxLen, gw, chunks, perPass, seq,
                       G, rec, recW, mfull, nBlk);
}

// one level of the frontier search, as the pass loop of runFrontierEdit launches it
template <class Geo> static void launchBfsPass(cmb_batch* b, const BfsBufs& B, uint32_t pass, const Queues& q) {
    hipLaunchKernelGGL(k_bfs_pass<Geo>, dim3(B.gridX + B.gridEv), dim3(256), 0, b->stream, b->ix->d, stratOf<Geo::MP>(b), B, pass, b->offs.p, b->gw, b->G.p,
                       partsOf<Geo::MP>(b), q);
}

// ---- one run of a batch: batchRunOne below calls these stages in the order of DESIGN.md §1 ----------------------------------------
namespace {
// What the stages of a run share (values only); whatever a single stage needs is a local of that stage
struct RunCtx {
    cmb_batch* b;
    hipStream_t s;
    Timer& tm;
    Queues q{};
    MFull mf{nullptr, 0}; // the match words of the full reads (runPrep)
    // the last read-back of b->cnt (readCounts): [0] items, [1] in-index occurrences, [2] text occurrences, [3] the FLAG_* bits,
    // [4] searches with further exact phases, [5] search tasks, [7] traceback tasks
    uint32_t hcnt[8] = {};
    // (the environment is read per run, not per process: tests set it between runs)
    const char* verboseEnv = nullptr;
    bool verbose = false, smallPools = false;
    // 11 ... 13 errors: the in-index matrix with 16-row blocks (GeoX, beyond the reference's 64-bit in-index matrix: dev_matrix.hpp, MXN_*),
    // the in-text matrix with 8-row blocks
    bool geoX = false;
    bool preset = false; // no search: the candidates come from the caller (cmb_verify_batch_staged)
    uint32_t nItems = 0, nFm = 0, nFmUniq = 0, nText = 0;
    uint64_t naiveSurvivors = 0;
    std::chrono::steady_clock::time_point t0; // where the last line of lap() ended
};
// How a stage of the search ends when it does not fail: the search goes on, or the attempt runs again — the stage has grown what was too
// small, or changed the geometry; the loop of batchRunOne counts the attempts and holds their limits
enum class Step { GoOn, AgainNaiveQueue, AgainPools, AgainGeometry };
} // namespace

static void lap(RunCtx& c, const char* what) {
    if (!c.verbose) return;
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[host] %-28s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - c.t0).count());
    c.t0 = t1;
}
// the queue sizes and flags of the device, once everything on the stream has run
static void readCounts(RunCtx& c) {
    HIPCHK(hipMemcpyAsync(c.hcnt, c.b->cnt.p, sizeof(c.hcnt), hipMemcpyDeviceToHost, c.s));
    HIPCHK(hipStreamSynchronize(c.s));
}
// the counters of the run so far as the batch reports them (blocking)
static void downloadCounters(cmb_batch* b) {
    unsigned long long hc[CMB_CNT_MAX];
    HIPCHK(hipMemcpy(hc, b->counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    for (int i = 0; i < CMB_CNT_MAX; i++) b->cnts[i] = hc[i];
}
static uint32_t stratBytesOf(const cmb_batch* b) {
    return (uint32_t)(((b->wide ? sizeof(DevStrategyKT<MAXP_WIDE>) : sizeof(DevStrategyK)) + 15) / 16 * 16);
}
// slots of k_exact: k = 0 one lane per read x strand; otherwise a small grid that loops over the ExactTasks k_parts left
static uint32_t exactSlots(const cmb_batch* b) {
    return capSlots(b->k ? 256u * 256u : (uint32_t)std::min<uint64_t>((2ull * b->nReads + 255) / 256 * 256, 256ull * 4096ull));
}

static int adoptStagedChunk(RunCtx& c) {
    cmb_batch* b = c.b;
    if (b->staged) { // the chunk uploaded during the previous run becomes the batch's reads
        HIPCHK(hipEventSynchronize(b->copyDone));
        std::swap(b->reads.p, b->readsStage.p);
        std::swap(b->reads.n, b->readsStage.n);
        std::swap(b->offs.p, b->offsStage.p);
        std::swap(b->offs.n, b->offsStage.n);
        b->hostOffs.swap(b->hostOffsActive);
        b->staged = false;
    }
    if (b->pending) { // the chunk registered since travels to the device while this run's kernels execute
        startStagedUpload(b);
        b->hostOffsActive.swap(b->hostOffsStage); // (offsets of the chunk in flight: the batch's from the next run on; the next registration refills hostOffsStage)
    }
    return CMB_OK;
}

static int runPrep(RunCtx& c) {
    cmb_batch* b = c.b;
    HIPCHK(hipMemsetAsync(b->counters.p, 0, CMB_CNT_MAX * sizeof(unsigned long long), c.s));
    c.tm.begin();
    if (b->metric == CMB_METRIC_EDIT && b->k > 0) { // (the match words of the full reads: k_prep writes them along with the rest)
        c.mf.nBlk = mfullBlocks(b->maxLen);
        const uint64_t nW = 2ull * b->nReads * c.mf.nBlk;
        if (b->mfull.n < 2 * nW) b->mfull.alloc(2 * nW);
        c.mf.p = b->mfull.p;
    }
    launchPrep(c.s, b->reads.p, b->offs.p, b->nReads, b->maxLen, b->gw, b->seq.p, b->G.p, b->rec.p, b->recW, const_cast<uint4*>(c.mf.p), c.mf.nBlk,
               c.verbose);
    c.tm.end("k_prep");
    return CMB_OK;
}

// the caller's candidates in the place of the search's in-text items
static int adoptPreset(RunCtx& c) {
    cmb_batch* b = c.b;
    if (b->items.n < b->presetItems.size()) b->items.alloc(b->presetItems.size() + 1024);
    HIPCHK(hipMemsetAsync(b->cnt.p, 0, 8 * sizeof(uint32_t), c.s));
    HIPCHK(hipMemcpyAsync(b->items.p, b->presetItems.data(), b->presetItems.size() * sizeof(uint4), hipMemcpyHostToDevice, c.s));
    HIPCHK(hipStreamSynchronize(c.s));
    memset(c.hcnt, 0, sizeof(c.hcnt));
    c.hcnt[0] = (uint32_t)b->presetItems.size();
    c.q.items = b->items.p;
    c.q.itemCap = cap32(b->items.n);
    return CMB_OK;
}

// k_parts + k_exact into the queues at their present sizes, and the first look at what they left
static int runPrologue(RunCtx& c, int attempt) {
    cmb_batch* b = c.b;
    cmb_index* ix = b->ix;
    hipStream_t s = c.s;
    Queues& q = c.q;
    const uint32_t nReads = b->nReads, tasks = 2 * nReads;
    HIPCHK(hipMemsetAsync(b->cnt.p, 0, 8 * sizeof(uint32_t), s));
    if (attempt) {
        HIPCHK(hipMemsetAsync(b->counters.p, 0, CMB_CNT_MAX * sizeof(unsigned long long), s));
    }
    q.items = b->items.p;
    q.itemCap = cap32(b->items.n);
    q.fm = b->fm.p;
    q.fmCap = cap32(b->fm.n);
    q.text = b->text.p;
    q.textCap = cap32(b->text.n);
    const uint32_t dfsCap = cap32(b->dfs.n);
    c.tm.begin();
    const uint32_t pParts = b->k ? b->sNumParts : 1;
    const uint32_t stratBytes = stratBytesOf(b);
    const uint32_t rdWords = 2 * ((b->maxLen + 31) / 32);
    const bool longReads = b->maxLen > 256;
    const uint32_t exCap = cap32(b->exq.n);
    if (b->k) {
        const uint32_t pCap = capSlots(envSlots("CMB_P_SLOTS", 256u * 32768u)); // (one lane per read x strand
        // up to 8 M: k_parts 65.7 ms with 512 k lanes looping over the tasks, 65.0 / 62.1 / 62.5 ms with 1 M / 4 M / 8 M)
        const uint32_t pSlots = std::min<uint32_t>(((tasks + 255) / 256) * 256, pCap);
        if (b->psel.n < tasks) b->psel.alloc(tasks);
        const size_t pLds = stratBytes + (5 * pParts + rdWords) * 256 * sizeof(uint32_t);
        gridLine(c.verbose, "k_parts", tasks, pSlots);
        withTables(b, [&](auto mp) {
            withInt<3>((int)b->sPartition, [&](auto part) {
                withBools(
                    [&](auto lng) {
                        constexpr int MP = decltype(mp)::value;
                        auto kp = k_parts<decltype(part)::value, decltype(lng)::value, MP>;
                        if (MP != MAXP && pLds > 64 * 1024)
                            HIPCHK(hipFuncSetAttribute((const void*)kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pLds));
                        hipLaunchKernelGGL(kp, dim3(pSlots / 256), dim3(256), pLds, s, ix->d, stratOf<MP>(b), nReads, b->k, b->maxLen, b->seq.p,
                                           (const uint4*)b->rec.p, b->recW / 4, partsOf<MP>(b), b->psel.p, b->dfs.p, dfsCap, b->exq.p, exCap, q);
                    },
                    longReads);
            });
        });
    }
    // k_exact: k = 0 one lane per read x strand; otherwise the ExactTasks k_parts left — their number is on the device, a small
    // grid loops over them (none in the common case: every search of the multiple_opt schemes has one exact phase)
    const uint32_t eSlots = exactSlots(b);
    if (!b->k) gridLine(c.verbose, "k_exact", tasks, eSlots); // (k > 0: the number of its tasks is on the device until the prologue is read back)
    const size_t eLds = stratBytes + (pParts + rdWords) * 256 * sizeof(uint32_t);
    withTables(b, [&](auto mp) {
        constexpr int MP = decltype(mp)::value;
        auto ke = withBools([](auto lng) { return k_exact<lng(), MP>; }, longReads);
        hipLaunchKernelGGL(ke, dim3(eSlots / 256), dim3(256), eLds, s, ix->d, stratOf<MP>(b), nReads, b->k, b->maxLen, b->seq.p,
                           (const uint4*)b->rec.p, b->recW / 4, partsOf<MP>(b), b->exq.p, exCap, b->dfs.p, dfsCap, q);
    });
    c.tm.end("k_partition");
    HIPCHK(hipGetLastError());
    readCounts(c);
    return CMB_OK;
}

// ---- reads not longer than the number of parts (and every read of a one-part strategy): naive backtracking
// (searchstrategy.cpp:148-152, :442-459 -> dev_bfs_naive.hpp); k_parts marked them in psel
static int runNaiveSearch(RunCtx& c, Step& step) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    const uint32_t tasks = 2 * b->nReads;
    c.tm.begin();
    const uint32_t maxPassN = b->maxLen + 2 * b->k + 4; // (rows of the matrix: len + 2 k + 1 at most)
    if (!b->nvQCap) b->nvQCap = c.smallPools ? 64 : 16384;
    for (int j = 0; j < 2; j++)
        if (b->nvQ[j].n < 3 * b->nvQCap) b->nvQ[j].alloc(3 * b->nvQCap);
    const size_t cntWords = (size_t)maxPassN + 2;
    if (b->nvCnt.n < cntWords) b->nvCnt.alloc(cntWords);
    HIPCHK(hipMemsetAsync(b->nvCnt.p, 0, cntWords * sizeof(uint32_t), s));
    NaiveBufs N{};
    N.Q[0] = b->nvQ[0].p;
    N.Q[1] = b->nvQ[1].p;
    N.qCap = cap32(b->nvQ[0].n / 3);
    N.nq = b->nvCnt.p;
    const bool edit = b->metric == CMB_METRIC_EDIT;
    hipLaunchKernelGGL(k_naive_start, dim3((tasks + 255) / 256), dim3(256), 0, s, b->ix->d, b->psel.p, b->offs.p, tasks, b->k, edit ? 0u : 1u, N, c.q,
                       c.geoX ? 1u : 0u);
    std::vector<uint32_t> hc(cntWords);
    uint32_t pass = 0, peakQ = 0;
    bool drained = false;
    // (the matrix of 11 ... 13 errors is the edit distance's alone)
    auto kNaive = withBools([](auto e, auto x) { return k_naive_pass<e(), e() && x()>; }, edit, c.geoX);
    const uint32_t nvGrid = capBlocks(BFS_GRID); // (k_naive_start above takes one lane per read x strand and does not loop: no cap)
    while (!drained && pass < maxPassN) {
        const uint32_t upTo = std::min(pass + 16u, maxPassN);
        for (; pass < upTo; pass++)
            hipLaunchKernelGGL(kNaive, dim3(nvGrid), dim3(256), 0, s, b->ix->d, N, pass, b->offs.p, b->gw, b->G.p, b->seq.p, b->maxLen, b->k, c.q);
        HIPCHK(hipMemcpyAsync(hc.data(), b->nvCnt.p, cntWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        readCounts(c);
        if (c.hcnt[3] & (FLAG_NAIVE_Q | FLAG_ITEM_OVERFLOW | FLAG_FMOCC_OVERFLOW)) break;
        drained = hc[pass] == 0;
    }
    for (uint32_t p2 = 0; p2 <= pass && p2 < cntWords; p2++) peakQ = std::max(peakQ, hc[p2]);
    if (c.verbose) fprintf(stderr, "[naive] %u roots, %u passes, peak frontier %u\n", hc[0], pass, peakQ);
    gridLine(c.verbose, "k_naive_pass", peakQ, 256ull * nvGrid); // (the largest frontier of a pass)
    c.tm.end("k_naive");
    HIPCHK(hipGetLastError());
    if (c.hcnt[3] & FLAG_NAIVE_Q) {
        b->nvQCap = std::max<size_t>(4 * b->nvQCap, (size_t)peakQ + peakQ / 4);
        step = Step::AgainNaiveQueue;
        return CMB_OK;
    }
    if (!drained && !(c.hcnt[3] & (FLAG_ITEM_OVERFLOW | FLAG_FMOCC_OVERFLOW)))
        return fail(CMB_ERR_INTERNAL, "the naive search did not finish within its pass bound");
    return CMB_OK;
}

// The pools of the edit-distance frontier as the kernels take them (dev_bfs_edit.hpp): grown to the capacities the batch asks for,
// their cntWords counters (nodes and events per level, four pool sizes) zeroed on the stream, for a search of at most maxPass levels
static BfsBufs frontierBufs(RunCtx& c, uint32_t maxPass, size_t cntWords) {
    cmb_batch* b = c.b;
    // node planes / uint4 per event of the record geometry (dev_bfs_edit.hpp: GeoN, GeoW)
    const size_t qPlanes = 3 + (b->wide ? GeoW::PK_U4 : GeoN::PK_U4), evU4 = 1 + (b->wide ? GeoW::PK_U4 : GeoN::PK_U4);
    // (GeoX: blocks of 16 rows — up to 32 of them for 480 + 26 rows, two uint4 of match words each)
    const uint32_t ctxU4 = c.geoX ? CTX_U4_X : ctxU4For(b->maxLen);
    BfsBufs B{};
    for (int j = 0; j < 2; j++) {
        if (b->bfsQ[j].n < qPlanes * b->bfsQCap) b->bfsQ[j].alloc(qPlanes * b->bfsQCap);
        if (b->bfsEv[j].n < evU4 * b->bfsEvCap) b->bfsEv[j].alloc(evU4 * b->bfsEvCap);
        B.Q[j] = b->bfsQ[j].p;
        B.Ev[j] = b->bfsEv[j].p;
    }
    if (b->bfsF.n < F_U4 * b->bfsFCap) b->bfsF.alloc(F_U4 * b->bfsFCap);
    if (b->bfsC.n < (size_t)ctxU4 * b->bfsCCap) b->bfsC.alloc((size_t)ctxU4 * b->bfsCCap);
    if (b->bfsA.n < b->bfsACap) b->bfsA.alloc(b->bfsACap);
    if (b->bfsCnt.n < cntWords) b->bfsCnt.alloc(cntWords);
    if (b->bfsBlockCnt.n < (size_t)BFS_GRID_CNT * 4) b->bfsBlockCnt.alloc((size_t)BFS_GRID_CNT * 4);
    HIPCHK(hipMemsetAsync(b->bfsCnt.p, 0, cntWords * sizeof(uint32_t), c.s));
    HIPCHK(hipMemsetAsync(b->bfsBlockCnt.p, 0, (size_t)BFS_GRID_CNT * 4 * sizeof(unsigned long long), c.s));
    B.F = b->bfsF.p;
    B.C = b->bfsC.p;
    B.A = b->bfsA.p;
    B.qCap = cap32(b->bfsQ[0].n / qPlanes);
    B.evCap = cap32(b->bfsEv[0].n / evU4);
    B.fCap = cap32(b->bfsF.n / F_U4);
    B.cCap = cap32(b->bfsC.n / ctxU4);
    B.ctxU4 = ctxU4;
    B.ctxMblk = c.geoX ? CTX_MBLK_X : ctxMblkFor(b->maxLen);
    B.aCap = cap32(b->bfsA.n);
    B.chain = getenv("CMB_BFS_CHAIN") ? (uint32_t)std::max(1, atoi(getenv("CMB_BFS_CHAIN"))) : BFS_CHAIN;
    B.gridX = capBlocks(std::min<uint32_t>(BFS_GRID_CNT, envBlocks("CMB_BFS_GRID", BFS_GRID_X)));
    B.gridEv = capBlocks(envBlocks("CMB_BFS_GRID_EV", BFS_GRID_EV));
    // (CMB_TEST_NARROW_WV: tests lower the bound so that the re-run on the 64-bit geometry is exercised)
    B.narrowWv = getenv("CMB_TEST_NARROW_WV") ? (uint32_t)std::max(0, atoi(getenv("CMB_TEST_NARROW_WV"))) : 0xFFFFu;
    B.nq = b->bfsCnt.p;
    B.ne = b->bfsCnt.p + (maxPass + 2);
    B.pool = b->bfsCnt.p + 2 * (maxPass + 2);
    B.blockCnt = b->bfsBlockCnt.p;
    return B;
}

// ---- frontier search: start pass, then (expand, events) per level until both queues drain
static int runFrontierEdit(RunCtx& c, Step& step) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    const uint32_t nReads = b->nReads, nDfs = c.hcnt[5];
    c.tm.begin();
    const uint32_t maxPass = 2 * b->maxLen + 8 * (b->wide ? MAXP_WIDE : MAXP) + 64;
    if (!b->bfsQCap) {
        // first guess; every pool grows (and the search re-runs) when it turns out too small.
        // CMB_TEST_SMALL_POOLS starts from almost nothing so that tests exercise that path.
        const size_t slack = c.smallPools ? 64 : 65536;
        const size_t per = c.smallPools ? 0 : 1;
        b->bfsQCap = per * (size_t)nReads * 2 + slack;
        b->bfsEvCap = per * (size_t)nReads / 2 + slack;
        b->bfsFCap = per * (size_t)nReads * 16 + slack;
        b->bfsCCap = per * (size_t)nReads * 2 + slack;
        b->bfsACap = per * (size_t)nReads * 8 + slack;
    }
    b->bfsQCap = std::max<size_t>(b->bfsQCap, (size_t)nDfs + 1024);
    const size_t cntWords = 2 * ((size_t)maxPass + 2) + 4;
    const BfsBufs B = frontierBufs(c, maxPass, cntWords);
    // up to 6 errors the frontier carries the in-index matrix on 32-bit words (GeoN32, dev_matrix.hpp: MXS_*); CMB_MATRIX64=1
    // keeps the reference's 64-bit words (GeoN), as does a batch one of whose phases did not fit the small matrix
    const FrontierGeo geo = frontierGeoOf(b);
    const uint32_t startGrid = capBlocks(std::min<uint32_t>((nDfs + 255) / 256, BFS_GRID));
    gridLine(c.verbose, "k_bfs_start", nDfs, 256ull * startGrid);
    withGeo(geo, [&](auto g) {
        using Geo = typename decltype(g)::type;
        hipLaunchKernelGGL(k_bfs_start<Geo>, dim3(startGrid), dim3(256), 0, s, b->ix->d, stratOf<Geo::MP>(b), B, b->dfs.p, nDfs, b->offs.p, b->gw, b->G.p,
                           partsOf<Geo::MP>(b), c.q);
    });
    // (the instance of a pass is chosen here, once per attempt: the loop below calls through a pointer)
    const auto bfsPass = withGeo(geo, [](auto g) { return &launchBfsPass<typename decltype(g)::type>; });
    std::vector<uint32_t> hc(cntWords);
    // passes between two looks at the queue sizes (a pass on a drained frontier costs the device ~4 us, a look costs the host a round trip)
    const uint32_t CHECK = getenv("CMB_BFS_CHECK") ? (uint32_t)std::max(1, atoi(getenv("CMB_BFS_CHECK"))) : 16;
    uint32_t pass = 0, peakQ = 0, peakEv = 0;
    bool drained = false;
    while (!drained && pass < maxPass) {
        const uint32_t upTo = std::min(pass + CHECK, maxPass);
        for (; pass < upTo; pass++) bfsPass(b, B, pass, c.q);
        HIPCHK(hipMemcpyAsync(hc.data(), b->bfsCnt.p, cntWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        readCounts(c);
        if (c.hcnt[3] & BFS_STOP) break;
        drained = hc[pass] == 0 && hc[maxPass + 2 + pass] == 0;
    }
    for (uint32_t p2 = 0; p2 <= pass && p2 < maxPass + 2; p2++) {
        peakQ = std::max(peakQ, hc[p2]);
        peakEv = std::max(peakEv, hc[maxPass + 2 + p2]);
    }
    const uint32_t* pool = hc.data() + 2 * (maxPass + 2);
    if (c.verbose)
        fprintf(stderr, "[bfs] %u tasks, %u passes, peak frontier %u, peak events %u, F %u, contexts %u, arena %u\n", nDfs, pass, peakQ, peakEv, pool[0],
                pool[1], pool[2]);
    gridLine(c.verbose, "k_bfs_pass", peakQ, 256ull * B.gridX); // (the largest frontier and the most events of a pass)
    gridLine(c.verbose, "k_bfs_pass_events", peakEv, 256ull * B.gridEv);
    if (c.verbose && atoi(c.verboseEnv) > 1)
        for (uint32_t p2 = 0; p2 <= pass; p2++) fprintf(stderr, "  pass %u: %u nodes, %u events\n", p2, hc[p2], hc[maxPass + 2 + p2]);
    hipLaunchKernelGGL(k_bfs_finish, dim3(1), dim3(256), 0, s, B, c.q);
    int rc = CMB_OK;
    if (c.hcnt[3] & FLAG_NARROW_MATRIX) { // (a first column wider than the small matrix holds: once more on the reference's words)
        if (c.verbose) fprintf(stderr, "[bfs] a phase did not fit the 32-bit in-index matrix: re-running on 64-bit words\n");
        b->noSmallMatrix = true;
        step = Step::AgainGeometry;
    } else if (c.hcnt[3] & (FLAG_BFS_Q | FLAG_BFS_EV | FLAG_BFS_F | FLAG_BFS_CTX | FLAG_BFS_ARENA)) {
        // a pool was too small: grow what was asked for (at least x2) and run the search again
        // (an attempt only shows the demand up to the pass that overflowed: beyond 7 errors, where the first guesses are far
        // off — 64 reads at 12 errors on 3 Gbp took eleven attempts at x 2 —, the pools grow x 4)
        const size_t gf = b->k > 7 ? 4 : 2;
        const struct {
            uint32_t flag;
            size_t* cap;
            uint32_t demand;
        } pools[] = {{FLAG_BFS_Q, &b->bfsQCap, peakQ},
                     {FLAG_BFS_EV, &b->bfsEvCap, peakEv},
                     {FLAG_BFS_F, &b->bfsFCap, pool[0]},
                     {FLAG_BFS_CTX, &b->bfsCCap, pool[1]},
                     {FLAG_BFS_ARENA, &b->bfsACap, pool[2]}};
        for (const auto& p : pools)
            if (c.hcnt[3] & p.flag) *p.cap = std::max<size_t>(gf * *p.cap, (size_t)p.demand + p.demand / 4);
        step = Step::AgainPools;
    } else if (!drained && !(c.hcnt[3] & BFS_STOP)) {
        rc = fail(CMB_ERR_INTERNAL, "frontier search did not finish within its pass bound");
    }
    if (step != Step::GoOn) HIPCHK(hipStreamSynchronize(s));
    c.tm.end("k_dfs");
    return rc;
}

// ---- Hamming distance: the same frontier idea without a matrix (dev_bfs_hamming.hpp)
static int runFrontierHamming(RunCtx& c, Step& step) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    const uint32_t nDfs = c.hcnt[5];
    c.tm.begin();
    const uint32_t maxPass = b->maxLen + 2 * (b->wide ? MAXP_WIDE : MAXP) + 16;
    if (!b->bfsQCap) b->bfsQCap = (c.smallPools ? 0 : (size_t)b->nReads * 4) + 1024;
    b->bfsQCap = std::max<size_t>(b->bfsQCap, (size_t)nDfs + 1024);
    for (int j = 0; j < 2; j++)
        if (b->bfsQ[j].n < 2 * b->bfsQCap) b->bfsQ[j].alloc(2 * b->bfsQCap);
    const size_t cntWords = (size_t)maxPass + 2;
    if (b->bfsCnt.n < cntWords) b->bfsCnt.alloc(cntWords);
    if (b->bfsBlockCnt.n < (size_t)BFS_GRID_CNT * 4) b->bfsBlockCnt.alloc((size_t)BFS_GRID_CNT * 4);
    HIPCHK(hipMemsetAsync(b->bfsCnt.p, 0, cntWords * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(b->bfsBlockCnt.p, 0, (size_t)BFS_GRID_CNT * 4 * sizeof(unsigned long long), s));
    HbfsBufs H{};
    H.Q[0] = b->bfsQ[0].p;
    H.Q[1] = b->bfsQ[1].p;
    H.qCap = cap32(b->bfsQ[0].n / 2);
    H.nq = b->bfsCnt.p;
    H.blockCnt = b->bfsBlockCnt.p;
    const uint32_t hLds = stratBytesOf(b);
    const uint32_t startGrid = capBlocks(std::min<uint32_t>((nDfs + 255) / 256, BFS_GRID)), passGrid = capBlocks(BFS_GRID);
    gridLine(c.verbose, "k_hbfs_start", nDfs, 256ull * startGrid);
    withTables(b, [&](auto mp) {
        constexpr int MP = decltype(mp)::value;
        hipLaunchKernelGGL((k_hbfs<true, MP>), dim3(startGrid), dim3(256), hLds, s, b->ix->d, stratOf<MP>(b), H, 0u, b->dfs.p, nDfs, b->maxLen, b->seq.p,
                           partsOf<MP>(b), c.q);
    });
    std::vector<uint32_t> hc(cntWords);
    uint32_t pass = 0, peakQ = 0;
    bool drained = false;
    while (!drained && pass < maxPass) {
        const uint32_t upTo = std::min(pass + 16u, maxPass);
        for (; pass < upTo; pass++)
            withTables(b, [&](auto mp) {
                constexpr int MP = decltype(mp)::value;
                hipLaunchKernelGGL((k_hbfs<false, MP>), dim3(passGrid), dim3(256), hLds, s, b->ix->d, stratOf<MP>(b), H, pass, (const DfsTask*)nullptr, 0u,
                                   b->maxLen, b->seq.p, partsOf<MP>(b), c.q);
            });
        HIPCHK(hipMemcpyAsync(hc.data(), b->bfsCnt.p, cntWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        readCounts(c);
        if (c.hcnt[3] & BFS_STOP) break;
        drained = hc[pass] == 0;
    }
    for (uint32_t p2 = 0; p2 <= pass && p2 < cntWords; p2++) peakQ = std::max(peakQ, hc[p2]);
    if (c.verbose) fprintf(stderr, "[hbfs] %u tasks, %u passes, peak frontier %u\n", nDfs, pass, peakQ);
    gridLine(c.verbose, "k_hbfs_pass", peakQ, 256ull * passGrid); // (the largest frontier of a pass)
    BfsBufs Bf{};
    Bf.blockCnt = b->bfsBlockCnt.p;
    hipLaunchKernelGGL(k_bfs_finish, dim3(1), dim3(256), 0, s, Bf, c.q);
    int rc = CMB_OK;
    if (c.hcnt[3] & FLAG_BFS_Q) {
        b->bfsQCap = std::max<size_t>(2 * b->bfsQCap, (size_t)peakQ + peakQ / 4);
        HIPCHK(hipStreamSynchronize(s));
        step = Step::AgainPools;
    } else if (!drained && !(c.hcnt[3] & BFS_STOP)) {
        rc = fail(CMB_ERR_INTERNAL, "frontier search did not finish within its pass bound");
    }
    c.tm.end("k_dfs");
    return rc;
}

// One attempt of the search with the queues and pools at their present sizes: prologue, naive backtracking, frontier.  Step::GoOn: the
// attempt ran to its end, and c.hcnt holds what it left — overflowed work queues included, which the caller grows
static int searchAttempt(RunCtx& c, int attempt, Step& step) {
    cmb_batch* b = c.b;
    int rc = runPrologue(c, attempt);
    if (rc != CMB_OK) return rc;
    b->hasNaive = (c.hcnt[3] & FLAG_UNSUPPORTED_READ) != 0;
    if (b->hasNaive && ((rc = runNaiveSearch(c, step)) != CMB_OK || step != Step::GoOn)) return rc;
    if (c.hcnt[3] & FLAG_SEED_OVERLAP)
        return fail(CMB_ERR_INVALID,
                    "dynamic partitioning: the seeds of a read overlap — the k-mer size of the index is too large "
                    "for the seeding positions of this search strategy at this read length (the reference caps "
                    "the k-mer size, e.g. at 4 for kuch2 and 01*0: alignparameters.cpp:1070-1114, :1275-1278)");
    if (c.verbose && b->k) fprintf(stderr, "[prologue] %u items, %u search tasks, %u searches with further exact phases\n", c.hcnt[0], c.hcnt[5], c.hcnt[4]);
    if (b->k) gridLine(c.verbose, "k_exact", c.hcnt[4], exactSlots(b));
    if ((c.hcnt[3] & (FLAG_ITEM_OVERFLOW | FLAG_DFS_OVERFLOW | FLAG_EXACT_OVERFLOW)) || !c.hcnt[5]) return CMB_OK;
    rc = b->metric == CMB_METRIC_EDIT ? runFrontierEdit(c, step) : runFrontierHamming(c, step);
    if (rc != CMB_OK || step != Step::GoOn) return rc;
    HIPCHK(hipGetLastError());
    readCounts(c);
    return CMB_OK;
}

// ---- de-duplicate the in-index occurrences (Occurrences::eraseDoublesFM, indexhelpers.h:2135-2146); their number arrives in c.nFmUniq
// with the next wait for the stream
static int dedupFmOccurrences(RunCtx& c) {
    cmb_batch* b = c.b;
    const uint32_t nFm = c.nFm;
    if (!nFm) return CMB_OK;
    if (b->fmKeysA.n < nFm) {
        b->fmKeysA.alloc((size_t)nFm + nFm / 4 + 256);
        b->fmKeysB.alloc(b->fmKeysA.n);
        b->fmIdxA.alloc(b->fmKeysA.n);
        b->fmIdxB.alloc(b->fmKeysA.n);
        b->fmUniq.alloc(b->fmKeysA.n);
    }
    if (b->fmN.n < 1) b->fmN.alloc(1);
    HIPCHK(hipMemsetAsync(b->fmN.p, 0, sizeof(uint32_t), c.s));
    hipLaunchKernelGGL(k_fm_keys, dim3((nFm + 255) / 256), dim3(256), 0, c.s, b->fm.p, nFm, b->fmKeysA.p, b->fmIdxA.p);
    sortPairs(b->sortTmp, b->fmKeysA.p, b->fmKeysB.p, b->fmIdxA.p, b->fmIdxB.p, nFm, 0, 64, c.s);
    hipLaunchKernelGGL(k_fm_unique, dim3((nFm + 255) / 256), dim3(256), 0, c.s, b->fm.p, b->fmKeysB.p, b->fmIdxB.p, nFm, b->fmUniq.p, b->fmN.p, c.q);
    HIPCHK(hipMemcpyAsync(&c.nFmUniq, b->fmN.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
    return CMB_OK;
}

// k_verify over the items, then — edit distance — the key sort and the matrix kernels over the distinct keys; c.hcnt[7] traceback tasks
static int verifyCandidates(RunCtx& c) {
    cmb_batch* b = c.b;
    cmb_index* ix = b->ix;
    hipStream_t s = c.s;
    const Queues& q = c.q;
    const MFull mf = c.mf;
    const uint32_t nReads = b->nReads, nItems = c.nItems;
    const bool verbose = c.verbose;
    // (lanes of k_verify: 128 k / 256 k / 512 k -> 34.8 / 32.0 / 35.9 ms of the locate group on the headline workload, round 4)
    const uint32_t vCap = capSlots(envSlots("CMB_V_SLOTS", 256u * 1024u, 256u * 2048u));
    const uint32_t vSlots = std::min<uint32_t>(((nItems + 255) / 256) * 256, vCap);
    gridLine(verbose, "k_verify", nItems, vSlots);
    // Edit distance: identical verifications (same read x strand, text window and bounds — the parts of
    // one read seeding the same alignment) are performed once: k_verify only locates and emits a key per
    // candidate, the keys are sorted and run-length encoded, k_verify_edit verifies the distinct ones and
    // scales the counters by the multiplicities.
    // (25 key bits for read x strand; 23 in the key layout of batches at 8 ... 13 errors — 64 - VKW_RS — whose sub-batches
    // hold at most 2^20 reads: the sorted bits below end at VKW_RS + rsBits <= 64)
    const bool dedup = b->metric == CMB_METRIC_EDIT && b->k > 0 && 2ull * nReads < (b->wideEdit ? (1ull << (64u - VKW_RS)) : (1ull << 25));
    if (b->wideEdit && !dedup) return fail(CMB_ERR_INTERNAL, "a sub-batch beyond 7 errors holds more reads than its verification keys number");
    const uint32_t tbCap = cap32(b->tbq.n);
    c.tm.begin();
    if (dedup) growTo(b->vkeysA, nItems), growTo(b->vkeysB, nItems), growTo(b->vcounts, nItems), growTo(b->vruns, 4);
    auto kv = withBools([](auto keys) { return k_verify<keys()>; }, dedup);
    hipLaunchKernelGGL(kv, dim3(vSlots / 256), dim3(256), 0, s, ix->d, b->offs.p, b->maxLen, b->gw, b->seq.p, mf, b->items.p, nItems, b->tbq.p, tbCap,
                       dedup ? b->vkeysA.p : (unsigned long long*)nullptr, q, b->wideEdit ? 1u : 0u); // (1: the wide key layout)
    if (!dedup) {
        c.tm.end("k_verify");
        readCounts(c);
        return CMB_OK;
    }
    uint32_t nRuns = 0;
    // sorted bits: low VK_LOW bits of the start, the bounds, read x strand (2 nReads < 2^rsBits, so
    // that the all-ones key of the other items sorts behind every real key) — see packVerifyKey
    uint32_t rsBits = 1;
    while ((1ull << rsBits) <= 2ull * nReads) rsBits++;
    const uint32_t bit0 = 32u - VK_LOW, bit1 = (b->wideEdit ? VKW_RS : 39u) + rsBits;
    sortKeys(b->sortTmp, b->vkeysA.p, b->vkeysB.p, nItems, bit0, bit1, s);
    runLengthEncode(b->scanTmp, b->vkeysB.p, nItems, b->vkeysA.p, b->vcounts.p, b->vruns.p, s);
    HIPCHK(hipMemcpyAsync(&nRuns, b->vruns.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c.tm.end("k_verify"); // locate + key sort + run-length encode; the matrix stages are timed apart
    c.tm.begin();
    if (verbose) fprintf(stderr, "[verify] %u items, %u distinct keys\n", nItems, nRuns);
    if (nRuns && b->wideEdit) {
        // 8 ... 13 errors: the band (up to 53 columns) needs the wide left margins of the 64-bit in-text matrix (dev_matrix.hpp:
        // MXX_*, MXY_*): k_wide_filter sorts out the candidates that never reach their final column, k_verify_wide<true> verifies the rest
        const uint32_t fGrid = capBlocks(std::min<uint32_t>((nRuns + 255) / 256, 2048u));
        gridLine(verbose, "k_wide_filter", nRuns, 256ull * fGrid);
        // (every key, the slots a wavefront leaves unused when it retires a chunk — fewer than 64 of 256 —, a chunk per wavefront)
        const size_t listNeed = (size_t)nRuns + nRuns / 3 + (size_t)fGrid * 4 * 256 + 512;
        if (b->dpList.n < listNeed) b->dpList.alloc(listNeed + listNeed / 8);
        if (b->dpWork.n < 4) b->dpWork.alloc(4);
        HIPCHK(hipMemsetAsync(b->dpWork.p, 0, 4 * sizeof(uint32_t), s));
        auto kFilter = k_wide_filter<WxTen>;
        auto kWide = k_verify_wide<true, WxTen>;
        if (c.geoX) kFilter = k_wide_filter<WxThirteen>, kWide = k_verify_wide<true, WxThirteen>;
        hipLaunchKernelGGL(kFilter, dim3(fGrid), dim3(256), 0, s, ix->d, b->offs.p, b->G.p, b->gw, b->vkeysA.p, b->vcounts.p, nRuns, b->dpWork.p,
                           b->dpList.p, cap32(b->dpList.n), q);
        const uint32_t slotBytes = (vwRows(b->maxLen) + 1u) * VW_ROW_BYTES;
        // (six wavefronts per SIMD: 1024 SIMDs x 6 x 64 lanes — forward pass and traceback wait for memory; a slot is 3 - 8 KB)
        const uint32_t dSlots = std::min<uint32_t>(((nRuns + 255) / 256) * 256, capSlots(envSlots("CMB_VW_SLOTS", 256u * 1536u)));
        if (b->dpSlab.n < (size_t)slotBytes * dSlots) b->dpSlab.alloc((size_t)slotBytes * dSlots);
        hipLaunchKernelGGL(kWide, dim3(dSlots / 256), dim3(256), 0, s, ix->d, b->offs.p, b->maxLen, b->seq.p, b->G.p, b->gw, (const uint4*)nullptr,
                           cap32(b->dpList.n), b->vkeysA.p, b->vcounts.p, b->dpList.p, b->dpWork.p + 1, b->dpSlab.p, slotBytes, q);
        if (verbose) {
            uint32_t hw[2];
            HIPCHK(hipMemcpyAsync(hw, b->dpWork.p, sizeof(hw), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            fprintf(stderr, "[verify] %u list slots (survivors and holes) for %u distinct candidates\n", hw[1], nRuns);
            gridLine(verbose, "k_verify_wide", hw[1], dSlots); // (it loops over the list the filter left)
        }
    } else if (nRuns) {
        // staged verification (kernels.hpp: k_verify_stage): one launch per nb 32-row matrix blocks,
        // survivor lists ping-pong, list sizes stay on the device
        // nb 32-row blocks per stage: fewer stages re-fetch fewer text lines and move fewer survivor
        // records, more blocks leave more lanes idle behind candidates that ended (CMB_STAGE_BLOCKS)
        const char* nbEnv = getenv("CMB_STAGE_BLOCKS");
        // (round 4, 150 bp reads at 4 errors: 1 / 2 / 3 / 4 / 6 blocks per stage -> 53.1 / 31.4 / 29.4 / 32.0 / 38.0 ms of k_verify_edit)
        const uint32_t nb = nbEnv ? std::min(8u, std::max(1u, (uint32_t)atoi(nbEnv))) : 3u;
        const uint32_t nStages = (vRows(b->maxLen) + 32u * nb - 1u) / (32u * nb) + 1u;
        for (int j = 0; j < 2; j++)
            if (b->vsC[j].n < nRuns) {
                b->vsA[j].alloc((size_t)nRuns + nRuns / 8 + 256);
                b->vsB[j].alloc(b->vsA[j].n);
                b->vsC[j].alloc(b->vsA[j].n);
            }
        if (b->vsN.n < nStages + 2) b->vsN.alloc(nStages + 2);
        HIPCHK(hipMemsetAsync(b->vsN.p, 0, (nStages + 2) * sizeof(uint32_t), s));
        const uint32_t listCap = cap32(b->vsC[0].n);
        const uint32_t gridCap = capBlocks(envBlocks("CMB_STAGE_GRID", 8192u));
        const uint32_t grid = std::min<uint32_t>((nRuns + 255) / 256, gridCap);
        gridLine(verbose, "k_verify_stage", nRuns, 256ull * grid); // (the first stage: the later ones take its survivors)
        VStageList L0{b->vsA[0].p, b->vsB[0].p, b->vsC[0].p}, L1{b->vsA[1].p, b->vsB[1].p, b->vsC[1].p};
        // k <= 4: the matrix on 32-bit words (dev_matrix.hpp); CMB_MATRIX_WIDE=1 keeps the 64-bit words
        const bool w32 = b->k <= MX32_MAX_ED && !getenv("CMB_MATRIX_WIDE");
        const bool packed = ix->d.text2 != nullptr; // 2-bit text (cmb_index_create)
        // stages no read of the batch can reach its final-column rows in (row >= len - maxED - 1,
        // maxED <= 7) run the instance without final-column code
        auto needsFinal = [&](uint32_t st) { return 32u * nb * (st + 1u) - 1u + 8u >= b->minLen; };
        auto stageKernel = [&](bool first, bool fin) {
            return withBools([](auto f, auto w, auto p, auto c2) { return k_verify_stage<f(), w(), p(), c2()>; }, first, w32, packed, fin);
        };
        hipLaunchKernelGGL(stageKernel(true, needsFinal(0)), dim3(grid), dim3(256), 0, s, ix->d, b->offs.p, mf, b->vkeysA.p, b->vcounts.p, nRuns, L0, L1,
                           b->vsN.p, listCap, 0u, nb, b->tbq.p, tbCap, q);
        for (uint32_t st = 1; st < nStages; st++)
            hipLaunchKernelGGL(stageKernel(false, needsFinal(st)), dim3(grid), dim3(256), 0, s, ix->d, b->offs.p, mf, (const unsigned long long*)nullptr,
                               (const uint32_t*)nullptr, 0u, (st & 1u) ? L1 : L0, (st & 1u) ? L0 : L1, b->vsN.p, listCap, st, nb, b->tbq.p, tbCap, q);
        if (verbose) {
            std::vector<uint32_t> hn(nStages + 2);
            HIPCHK(hipMemcpyAsync(hn.data(), b->vsN.p, hn.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            fprintf(stderr, "[verify] survivors per stage:");
            for (uint32_t st = 1; st <= nStages; st++) fprintf(stderr, " %u", hn[st]);
            fprintf(stderr, "\n");
        }
    }
    c.tm.end("k_verify_edit");
    readCounts(c);
    return CMB_OK;
}

// k_traceback over the c.hcnt[7] tasks the verification left
static int runTraceback(RunCtx& c) {
    cmb_batch* b = c.b;
    const uint32_t nTb = c.hcnt[7];
    if (!nTb) return CMB_OK;
    const uint32_t slotCap = capSlots(envSlots("CMB_TB_SLOTS", 512u * 1024u)); // (measured 64 k … 2 M slots: 84 / 49 / 34.4 / 32.8 / 31 / 29 ms alone; 512 k best beside other sub-batches)
    const uint32_t tSlots = std::min<uint32_t>(((nTb + 255) / 256) * 256, slotCap);
    gridLine(c.verbose, "k_traceback", nTb, tSlots);
    // 64-byte lines of 16 narrow (k <= 4) or 8 wide trace rows (a group is written whole)
    const bool narrow = b->k <= TBN_MAX_ED && !getenv("CMB_TRACE_WIDE");
    const uint32_t tLines = traceLines(narrow, vRows(b->maxLen));
    if (b->vW.n < (size_t)tLines * 8 * tSlots) b->vW.alloc((size_t)tLines * 8 * tSlots);
    VPlanes vp{b->vW.p, tSlots, tLines};
    c.tm.begin();
    // no final-column row (> len - maxED - 1, maxED <= 7) at or before this row, for any read of the batch
    const uint32_t rowMin = b->minLen > 8u ? b->minLen - 8u : 0u;
    launchTraceback(c.s, b->ix->d, narrow, b->offs.p, c.mf, b->tbq.p, nTb, vp, c.q, rowMin);
    c.tm.end("k_traceback");
    return CMB_OK;
}

// ---- locate + verify: the items and the distinct in-index occurrences become text occurrences (c.nText of them).  The text queue is
// retried on overflow: a retry starts from the counters as the search left them, with the overflow flag cleared
static int locateAndVerify(RunCtx& c) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    // traceback task queue: at most one task per item + the chunk slack of every k_verify wavefront
    // (a chunk of 256 is retired when the wavefront's next group does not fit: at most 63 holes per chunk)
    const size_t tbNeed = (size_t)c.nItems + (size_t)c.nItems / 2 + (size_t)(256u * 2048u / 64u + 1) * 256u;
    if (b->tbq.n < tbNeed) b->tbq.alloc(tbNeed + c.nItems / 8);
    for (int attempt = 0;; attempt++) {
        c.q.text = b->text.p;
        c.q.textCap = cap32(b->text.n);
        uint32_t zero[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(b->cnt.p + 2, zero, sizeof(zero), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b->cnt.p + 7, zero, sizeof(uint32_t), hipMemcpyHostToDevice, s));
        unsigned long long keep[CMB_CNT_MAX];
        HIPCHK(hipMemcpyAsync(keep, b->counters.p, sizeof(keep), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (c.nItems) {
            int rc = verifyCandidates(c);
            if (rc == CMB_OK) rc = runTraceback(c);
            if (rc != CMB_OK) return rc;
        }
        readCounts(c);
        if (c.nFmUniq) {
            c.tm.begin();
            const uint32_t nb = (uint32_t)std::min<size_t>(((size_t)c.nFmUniq + 255) / 256, 4096);
            hipLaunchKernelGGL(k_fmocc, dim3(nb), dim3(256), 0, s, b->ix->d, b->fmUniq.p, c.nFmUniq, c.q);
            c.tm.end("k_fmocc");
        }
        HIPCHK(hipGetLastError());
        readCounts(c);
        if (!(c.hcnt[3] & FLAG_TEXT_OVERFLOW)) break;
        if (attempt >= 3) return fail(CMB_ERR_INTERNAL, "text occurrence queue keeps overflowing");
        b->text.alloc((size_t)c.hcnt[2] + c.hcnt[2] / 8 + 1024);
        HIPCHK(hipMemcpy(b->counters.p, keep, sizeof(keep), hipMemcpyHostToDevice));
        uint32_t fl = c.hcnt[3] & ~(uint32_t)FLAG_TEXT_OVERFLOW; // clear the overflow flag for the retry
        HIPCHK(hipMemcpy(b->cnt.p + 3, &fl, sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    c.nText = c.hcnt[2];
    return CMB_OK;
}

// candidates given by the caller: the raw text occurrences and the counters are the result
static int finishPreset(RunCtx& c) {
    cmb_batch* b = c.b;
    if (c.hcnt[3] & (FLAG_CAPACITY | FLAG_TRACE_RULE)) return fail(CMB_ERR_INTERNAL, "a traceback left the band");
    b->presetOut.resize(c.nText);
    if (c.nText) HIPCHK(hipMemcpy(b->presetOut.data(), b->text.p, (size_t)c.nText * sizeof(TextOccRec), hipMemcpyDeviceToHost));
    downloadCounters(b);
    b->done = true;
    return CMB_OK;
}

// The filter of getUniqueTextOccurrences / getTextOccHamming (indexinterface.cpp:1331-1491) up to the ranks: the nText text occurrences
// packed into keys (k_pack_keys: per read, or per read x strand; psel: only those of the reads it marks) -> one 64-bit radix sort ->
// per-group scan.  Leaves the sorted keys in keysB, the rank of every survivor within its group in frank, the survivors per group in
// fcounts and their exclusive scan in foffs, whose last element (foffs[nGroups], the total) the caller reads
static void rankSurvivors(RunCtx& c, uint32_t nText, uint32_t nGroups, uint32_t perStrandKeys, const uint8_t* psel, int mode, uint32_t keyLayout) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    growTo(b->keysA, nText), growTo(b->keysB, nText), growTo(b->frank, nText);
    if (b->fcounts.n < (size_t)nGroups + 1) {
        b->fcounts.alloc((size_t)nGroups + 1);
        b->foffs.alloc((size_t)nGroups + 1);
        b->fsegB.alloc((size_t)nGroups + 1);
        b->fsegE.alloc((size_t)nGroups + 1);
    }
    if (nText) {
        hipLaunchKernelGGL(k_pack_keys, dim3((nText + 255) / 256), dim3(256), 0, s, b->text.p, nText, b->offs.p, b->k, b->keysA.p, b->cnt.p, perStrandKeys,
                           psel, keyLayout);
        sortKeys(b->sortTmp, b->keysA.p, b->keysB.p, nText, 0, 64, s);
    }
    HIPCHK(hipMemsetAsync(b->fcounts.p, 0, ((size_t)nGroups + 1) * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(b->fsegB.p, 0xFF, ((size_t)nGroups + 1) * sizeof(uint32_t), s));
    if (nText) {
        HIPCHK(hipMemsetAsync(b->frank.p, 0xFF, (size_t)nText * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_filter_segments, dim3((nText + 255) / 256), dim3(256), 0, s, b->keysB.p, nText, b->fsegB.p, b->fsegE.p, keyBits(keyLayout).group);
    }
    hipLaunchKernelGGL(k_filter_mark, dim3((nGroups + 255) / 256), dim3(256), 0, s, b->keysB.p, nGroups, b->k, mode, b->fcounts.p, b->frank.p, b->fsegB.p,
                       b->fsegE.p, keyLayout);
    scanExclusive(b->scanTmp, b->fcounts.p, b->foffs.p, (size_t)nGroups + 1, s);
}

// ---- naive backtracking: the filter pass of approxMatchesNaive[Hamming] itself, per read x strand (dev_bfs_naive.hpp): the occurrences
// of the naive reads are dropped from the text queue and their survivors appended to it
static int filterNaive(RunCtx& c) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    const uint32_t nText = c.nText;
    if (!b->hasNaive || !nText) return CMB_OK;
    const uint32_t keyLayout = keyLayoutOf(b);
    const uint32_t nG = 2u * b->nReads;
    if (nG >= (1u << groupBits(b))) return fail(CMB_ERR_UNSUPPORTED, "more than 2^23 reads in a sub-batch with reads matched by naive backtracking");
    c.tm.begin();
    rankSurvivors(c, nText, nG, 1u, (const uint8_t*)b->psel.p, b->metric == CMB_METRIC_HAMMING ? 1 : 2, keyLayout);
    HIPCHK(hipMemcpyAsync(&c.naiveSurvivors, b->foffs.p + nG, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    readCounts(c);
    int rc = CMB_OK;
    if (c.hcnt[3] & FLAG_CAPACITY) {
        rc = fail(CMB_ERR_INTERNAL, "occurrence does not fit the filter key (width / distance range) or a traceback left the band");
    } else if ((uint64_t)nText + c.naiveSurvivors >= 0xFFFFFFF0ull) {
        rc = fail(CMB_ERR_UNSUPPORTED, "too many occurrences in one sub-batch");
    } else {
        if (b->text.n < (size_t)nText + c.naiveSurvivors) { // grow, keeping the records
            DevBuf<TextOccRec> bigger;
            bigger.alloc((size_t)nText + c.naiveSurvivors + 1024);
            HIPCHK(hipMemcpyAsync(bigger.p, b->text.p, (size_t)nText * sizeof(TextOccRec), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
            std::swap(bigger.p, b->text.p);
            std::swap(bigger.n, b->text.n);
        }
        hipLaunchKernelGGL(k_naive_drop, dim3((nText + 255) / 256), dim3(256), 0, s, b->text.p, nText, (const uint8_t*)b->psel.p);
        if (c.naiveSurvivors)
            hipLaunchKernelGGL(k_naive_keep, dim3((nText + 255) / 256), dim3(256), 0, s, b->keysB.p, nText, b->offs.p, b->k, b->frank.p, b->foffs.p,
                               b->text.p + nText, keyLayout);
        HIPCHK(hipGetLastError());
        c.nText += (uint32_t)c.naiveSurvivors;
    }
    c.tm.end("k_naive_filter");
    return rc;
}

// groups of the final filter: reads, or read x strand when every strand is filtered by itself
static uint32_t filterGroups(const cmb_batch* b) { return b->perStrand ? 2u * b->nReads : b->nReads; }

// ---- sort + filter on the device (getUniqueTextOccurrences / getTextOccHamming, indexinterface.cpp:1331-1491): the `total` final
// occurrences in fout, group by group (foffs)
static int filterFinal(RunCtx& c, uint64_t& total) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    const uint32_t nText = c.nText, nGroups = filterGroups(b), keyLayout = keyLayoutOf(b);
    // (group numbers 0 ... nGroups - 1: 2^24 groups fit the 24 bits of layouts 0 and 1 — a BEST sub-batch of 2^23 reads)
    if (nGroups > (1u << groupBits(b))) return fail(CMB_ERR_UNSUPPORTED, "more filter groups in one sub-batch than the keys number");
    c.tm.begin();
    rankSurvivors(c, nText, nGroups, b->perStrand ? 1u : 0u, (const uint8_t*)nullptr, b->k == 0 ? 0 : (b->metric == CMB_METRIC_HAMMING ? 1 : 2), keyLayout);
    HIPCHK(hipMemcpyAsync(&total, b->foffs.p + nGroups, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    readCounts(c);
    int rc = CMB_OK;
    if (c.hcnt[3] & FLAG_TRACE_RULE) {
        rc = fail(CMB_ERR_INTERNAL, "a traceback read a band-edge bit the narrow trace rows take as implied");
    } else if (c.hcnt[3] & FLAG_CAPACITY) {
        rc = fail(CMB_ERR_INTERNAL, "occurrence does not fit the filter key (width / distance range) or a traceback left the band");
    } else {
        growTo(b->fout, total);
        if (b->wantAln) growTo(b->foutRead, total);
        if (total)
            hipLaunchKernelGGL(k_filter_write, dim3((nText + 255) / 256), dim3(256), 0, s, b->keysB.p, nText, b->offs.p, b->k, b->frank.p, b->foffs.p,
                               b->fout.p, b->wantAln ? b->foutRead.p : (uint32_t*)nullptr, b->perStrand ? 1u : 0u, keyLayout);
        HIPCHK(hipGetLastError());
    }
    c.tm.end("k_filter");
    return rc;
}

// CIGAR + sequence of every final occurrence (k_cigar), on request
static int runCigar(RunCtx& c, uint64_t total) {
    cmb_batch* b = c.b;
    if (!b->wantAln) return CMB_OK;
    c.tm.begin();
    b->alnStride = 2u * b->k + 3u;
    if (b->alnRec.n < total) {
        b->alnRec.alloc((size_t)total + total / 8 + 256);
        b->alnOps.alloc(b->alnRec.n * std::max<size_t>(b->alnStride, 2u * 7u + 3u));
    }
    if (total) {
        const uint32_t cSlots = capSlots((uint32_t)std::min<uint64_t>(((total + 255) / 256) * 256, 512u * 1024u));
        MFull mfc = c.mf;
        if (!mfc.p) mfc.nBlk = 0; // (Hamming / exact batches have no match words: every CIGAR is len x M, nothing is traced)
        const CigarJob job{b->offs.p, b->G.p, b->gw, b->maxLen, mfc, b->fout.p, b->foutRead.p, (uint64_t)total, b->alnOps.p, b->alnStride,
                           b->alnRec.p, b->cnt.p + 3, (b->metric != CMB_METRIC_EDIT || b->k == 0) ? 1u : 0u};
        launchCigar(b->ix, c.s, job, b->metric == CMB_METRIC_EDIT && b->k > CIGAR_BLOCK_WORDS_MAX_ED, b->k <= TBN_MAX_ED && !getenv("CMB_TRACE_WIDE"),
                    vRows(b->maxLen), cSlots, b->vW, b->dpSlab, c.verbose);
    }
    c.tm.end("k_cigar");
    HIPCHK(hipGetLastError());
    return CMB_OK;
}

// ---- on request (cmb_batch_trim_on_device): the final occurrences that run over the end of their sequence are trimmed to the sequence
// they belong to, verified on the trimmed window and replaced by the minimal occurrence found there, or marked dropped — findSeqName
// (indexinterface.cpp:828-897) for the whole sub-batch, dev_trim.hpp.  The verification writes into queues, counters and flags of its own
static int trimSpanning(RunCtx& c, uint64_t total) {
    cmb_batch* b = c.b;
    memset(b->trimStats, 0, sizeof(b->trimStats));
    if (!b->trimOn) return CMB_OK;
    if (!b->wantAln) return fail(CMB_ERR_INVALID, "trimming on the device needs the alignments (cmb_batch_want_alignments)");
    if (!total) return CMB_OK;
    if (total >= 0xFFFFFFF0ull) return fail(CMB_ERR_UNSUPPORTED, "too many occurrences in one sub-batch");
    cmb_index* ix = b->ix;
    hipStream_t s = c.s;
    const bool verbose = c.verbose;
    // ---- plan: one item per spanning occurrence with a window (never more than occurrences)
    c.tm.begin();
    growTo(b->trimItems, total), growTo(b->trimItemOcc, total);
    if (b->trimCnt.n < 16) b->trimCnt.alloc(16);
    if (b->trimCounters.n < CMB_CNT_MAX) b->trimCounters.alloc(CMB_CNT_MAX);
    HIPCHK(hipMemsetAsync(b->trimCnt.p, 0, 16 * sizeof(uint32_t), s));
    const uint32_t pBlocks = capBlocks((uint32_t)std::min<uint64_t>((total + 255) / 256, 4096));
    gridLine(verbose, "k_trim_plan", total, 256ull * pBlocks);
    const uint32_t nSeqs = ix->seqStarts.size() >= 2 ? (uint32_t)ix->seqStarts.size() - 1u : 0u; // (none given: nothing can be trimmed)
    hipLaunchKernelGGL(k_trim_plan, dim3(pBlocks), dim3(256), 0, s, b->fout.p, b->foutRead.p, b->alnRec.p, total, ix->seqStartsDev.p, nSeqs, b->k,
                       b->metric == CMB_METRIC_HAMMING ? 1u : 0u, b->trimItems.p, b->trimItemOcc.p, b->trimCnt.p + 8);
    HIPCHK(hipGetLastError());
    uint32_t planned[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(planned, b->trimCnt.p + 8, sizeof(planned), hipMemcpyDeviceToHost, s));
    c.tm.end("k_trim_plan"); // (waits for the stream)
    const uint32_t nItems = planned[1];
    b->trimStats[0] = planned[0], b->trimStats[2] = planned[0];
    if (verbose) fprintf(stderr, "[trim] %llu occurrences, %u over the end of their sequence, %u windows to verify\n", (unsigned long long)total, planned[0], nItems);
    if (!nItems) return CMB_OK;
    if (nItems >= (1u << TRIM_ITEM_BITS)) return fail(CMB_ERR_UNSUPPORTED, "more trimmed windows in one sub-batch than the verification records number");
    // ---- verification of the windows, as the hooks run it (verifyDirect): k_verify + k_traceback up to 7 errors, k_verify_wide beyond.
    // The record queue is retried on overflow with the size the kernels asked for
    c.tm.begin();
    const bool dp = 3 * b->k + 1 > MXW_LEFT;
    const uint32_t vSlots = std::min<uint32_t>(((nItems + 255) / 256) * 256, capSlots(256u * 1024u));
    const uint32_t tSlots = std::min<uint32_t>(((nItems + 255) / 256) * 256, capSlots(512u * 1024u));
    const uint32_t dSlots = std::min<uint32_t>(((nItems + 255) / 256) * 256, capSlots(envSlots("CMB_VW_SLOTS", 256u * 1536u)));
    // (a record or two per window; every wavefront may leave a partly used chunk of 256 records, and up to 63 holes in a chunk it retires)
    const size_t textNeed = c.smallPools ? 64 : (size_t)nItems * 3 + (size_t)((dp ? dSlots : vSlots + tSlots) / 64u + 2u) * 256u;
    if (b->trimText.n < textNeed) b->trimText.alloc(textNeed);
    const size_t tbNeed = (size_t)nItems + nItems / 2 + (size_t)(vSlots / 64u + 1u) * 256u;
    if (!dp && b->tbq.n < tbNeed) b->tbq.alloc(tbNeed);
    uint32_t hc[8] = {};
    for (int attempt = 0;; attempt++) {
        HIPCHK(hipMemsetAsync(b->trimCnt.p, 0, 8 * sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(b->trimCounters.p, 0, CMB_CNT_MAX * sizeof(unsigned long long), s));
        Queues q{};
        q.text = b->trimText.p, q.textCap = cap32(b->trimText.n), q.cnt = b->trimCnt.p, q.counters = b->trimCounters.p;
        if (dp) {
            const uint32_t slotBytes = (vwRows(b->maxLen) + 1u) * VW_ROW_BYTES;
            if (b->dpSlab.n < (size_t)slotBytes * dSlots) b->dpSlab.alloc((size_t)slotBytes * dSlots);
            gridLine(verbose, "k_verify_wide (trim)", nItems, dSlots);
            auto kWide = k_verify_wide<false, WxTen, true>;
            if (b->k > MX_MAX_ED) kWide = k_verify_wide<false, WxThirteen, true>;
            hipLaunchKernelGGL(kWide, dim3(dSlots / 256), dim3(256), 0, s, ix->d, b->offs.p, b->maxLen, b->seq.p, b->G.p, b->gw, b->trimItems.p, nItems,
                               (const unsigned long long*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, b->dpSlab.p,
                               slotBytes, q);
        } else {
            gridLine(verbose, "k_verify (trim)", nItems, vSlots);
            hipLaunchKernelGGL((k_verify<false, true>), dim3(vSlots / 256), dim3(256), 0, s, ix->d, b->offs.p, b->maxLen, b->gw, b->seq.p, c.mf, b->trimItems.p,
                               nItems, b->tbq.p, cap32(b->tbq.n), (unsigned long long*)nullptr, q, 0u);
            HIPCHK(hipMemcpyAsync(hc, b->trimCnt.p, sizeof(hc), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (hc[7] && !(hc[3] & FLAG_CAPACITY)) {
                const bool narrow = b->k <= TBN_MAX_ED && !getenv("CMB_TRACE_WIDE");
                const uint32_t slots = std::min<uint32_t>(((hc[7] + 255) / 256) * 256, tSlots);
                const uint32_t tLines = traceLines(narrow, vRows(b->maxLen));
                if (b->vW.n < (size_t)tLines * 8 * slots) b->vW.alloc((size_t)tLines * 8 * slots);
                gridLine(verbose, "k_traceback (trim)", hc[7], slots);
                launchTraceback(s, ix->d, narrow, b->offs.p, c.mf, b->tbq.p, hc[7], VPlanes{b->vW.p, slots, tLines}, q, 0u, true);
            }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hc, b->trimCnt.p, sizeof(hc), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!(hc[3] & FLAG_TEXT_OVERFLOW)) break;
        if (attempt >= 3) return fail(CMB_ERR_INTERNAL, "the record queue of the trimmed windows keeps overflowing");
        if (verbose) fprintf(stderr, "[retry] trim: %u verification records do not fit %zu\n", hc[2], b->trimText.n);
        b->trimText.alloc((size_t)hc[2] + hc[2] / 8 + 1024);
    }
    c.tm.end("k_trim_verify");
    if (hc[3] & (FLAG_CAPACITY | FLAG_TRACE_RULE)) return fail(CMB_ERR_INTERNAL, "the verification of a trimmed window left the band");
    const uint32_t nText = hc[2];
    if (!nText) return CMB_OK;
    // ---- pick: the records sorted by (item, begin, distance, width); the first of every item survives
    c.tm.begin();
    growTo(b->trimKeysA, nText), growTo(b->trimKeysB, nText);
    growTo(b->trimPickOcc, nItems), growTo(b->trimPickRead, nItems), growTo(b->trimPickDst, nItems);
    const uint32_t kBlocks = capBlocks(std::min<uint32_t>((nText + 255) / 256, 4096u));
    gridLine(verbose, "k_trim_keys", nText, 256ull * kBlocks);
    hipLaunchKernelGGL(k_trim_keys, dim3(kBlocks), dim3(256), 0, s, b->trimText.p, nText, b->trimItems.p, nItems, b->trimKeysA.p, b->trimCnt.p + 3);
    uint32_t itemBits = 1; // (nItems < 2^itemBits: the all-ones key of a hole sorts behind every item)
    while ((1ull << itemBits) <= nItems) itemBits++;
    sortKeys(b->sortTmp, b->trimKeysA.p, b->trimKeysB.p, nText, 0, TRIM_KEY_ITEM + itemBits, s);
    gridLine(verbose, "k_trim_pick", nText, 256ull * kBlocks);
    hipLaunchKernelGGL(k_trim_pick, dim3(kBlocks), dim3(256), 0, s, b->trimKeysB.p, nText, b->trimItems.p, b->trimItemOcc.p, b->trimPickOcc.p,
                       b->trimPickRead.p, b->trimPickDst.p, b->trimCnt.p + 10);
    HIPCHK(hipGetLastError());
    uint32_t nPick = 0;
    HIPCHK(hipMemcpyAsync(&nPick, b->trimCnt.p + 10, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    c.tm.end("k_trim_pick");
    if (!nPick) return CMB_OK;
    // ---- commit: the survivors' CIGARs from the matrix family of the batch's other occurrences (runCigar), then everything into place
    c.tm.begin();
    growTo(b->trimAln, nPick), growTo(b->trimOps, (size_t)nPick * b->alnStride);
    const uint32_t cSlots = capSlots((uint32_t)std::min<uint64_t>(((nPick + 255ull) / 256) * 256, 512u * 1024u));
    const CigarJob job{b->offs.p, b->G.p, b->gw, b->maxLen, c.mf, b->trimPickOcc.p, b->trimPickRead.p, (uint64_t)nPick, b->trimOps.p, b->alnStride,
                       b->trimAln.p, b->trimCnt.p + 3, 0u};
    launchCigar(ix, s, job, b->k > CIGAR_BLOCK_WORDS_MAX_ED, b->k <= TBN_MAX_ED && !getenv("CMB_TRACE_WIDE"), vRows(b->maxLen), cSlots, b->vW, b->dpSlab, verbose);
    const uint32_t cBlocks = capBlocks(std::min<uint32_t>((nPick + 255) / 256, 4096u));
    gridLine(verbose, "k_trim_commit", nPick, 256ull * cBlocks);
    hipLaunchKernelGGL(k_trim_commit, dim3(cBlocks), dim3(256), 0, s, b->trimPickOcc.p, b->trimPickDst.p, b->trimAln.p, b->trimOps.p, nPick, b->alnStride,
                       b->fout.p, b->alnRec.p, b->alnOps.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hc, b->trimCnt.p, sizeof(hc), hipMemcpyDeviceToHost, s));
    c.tm.end("k_trim_commit");
    if (hc[3] & (FLAG_CAPACITY | FLAG_TRACE_RULE))
        return fail(CMB_ERR_INTERNAL, "a trimmed occurrence does not fit its key or the CIGAR traceback of one left the band");
    b->trimStats[1] = nPick, b->trimStats[2] = b->trimStats[0] - nPick;
    return CMB_OK;
}

// the final occurrences, their offsets per group and (on request) their alignments in the page-locked buffers of the batch
static int downloadResults(RunCtx& c, uint64_t total) {
    cmb_batch* b = c.b;
    hipStream_t s = c.s;
    const uint32_t nGroups = filterGroups(b);
    b->occs.resize(total);
    b->occOffs.resize((size_t)nGroups + 1);
    if (total) HIPCHK(hipMemcpyAsync(b->occs.data(), b->fout.p, (size_t)total * sizeof(cmb_occ), hipMemcpyDeviceToHost, s));
    if (b->wantAln) {
        b->hAlnRec.resize(total);
        b->hAlnOps.resize((size_t)total * b->alnStride);
        if (total) {
            HIPCHK(hipMemcpyAsync(b->hAlnRec.data(), b->alnRec.p, (size_t)total * sizeof(AlnRec), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(b->hAlnOps.data(), b->alnOps.p, (size_t)total * b->alnStride * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipMemcpyAsync(c.hcnt, b->cnt.p, sizeof(c.hcnt), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(b->occOffs.data(), b->foffs.p, ((size_t)nGroups + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (b->wantAln && (c.hcnt[3] & FLAG_CAPACITY))
        return fail(CMB_ERR_INTERNAL, "a CIGAR traceback left the band or an occurrence is not an alignment within its distance");
    lap(c, "results to the host");
    if (c.verbose) {
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        fprintf(stderr, "[mem] device memory in use: %.1f GB of %.1f GB\n", (tot - fr) / 1e9, tot / 1e9);
    }
    return CMB_OK;
}

static int batchRunOne(cmb_batch* b) {
    try {
        useDevice(b->ix->device);
        Timer tm(b->stream, b->times);
        RunCtx c{b, b->stream, tm};
        int rc = adoptStagedChunk(c);
        if (rc != CMB_OK) return rc;
        b->times.clear();
        b->done = false;
        b->hasNaive = false;
        if (b->nReads == 0) {
            b->occs.resize(0);
            b->occOffs.resize(1);
            b->occOffs.p[0] = 0;
            memset(b->cnts, 0, sizeof(b->cnts));
            b->done = true;
            return CMB_OK;
        }
        c.verboseEnv = getenv("CMB_VERBOSE");
        c.verbose = c.verboseEnv != nullptr, c.smallPools = getenv("CMB_TEST_SMALL_POOLS") != nullptr;
        c.geoX = b->wideEdit && frontierGeoOf(b) == FrontierGeo::X;
        c.preset = !b->presetItems.empty();
        c.t0 = std::chrono::steady_clock::now();
        c.q.cnt = b->cnt.p;
        c.q.counters = b->counters.p;

        if ((rc = runPrep(c)) != CMB_OK) return rc;
        if (c.preset && (rc = adoptPreset(c)) != CMB_OK) return rc;
        // ---- prologue + search (re-run with larger queues and pools if they overflow: nothing is truncated)
        // (a stage that asks for another attempt has already grown its pool when the limit is tested here: the sizes of a batch
        // whose run fails on a limit are one step larger than they would be had the test come first)
        const bool edit = b->metric == CMB_METRIC_EDIT;
        int poolAttempts = 0;
        for (int attempt = 0; !c.preset; attempt++) {
            Step step = Step::GoOn;
            if ((rc = searchAttempt(c, attempt, step)) != CMB_OK) return rc;
            if (step == Step::AgainNaiveQueue && attempt >= 60) return fail(CMB_ERR_INTERNAL, "the naive search's frontier keeps overflowing");
            if (step == Step::AgainPools && ++poolAttempts >= (edit ? 48 : 24))
                return fail(CMB_ERR_INTERNAL, edit ? "frontier pools keep overflowing" : "frontier keeps overflowing");
            if (step != Step::GoOn) continue;
            if (c.hcnt[3] & FLAG_CAPACITY) return fail(CMB_ERR_INTERNAL, "device search capacity exceeded (band width / descendants / stack)");
            if (!(c.hcnt[3] & (FLAG_ITEM_OVERFLOW | FLAG_FMOCC_OVERFLOW | FLAG_DFS_OVERFLOW | FLAG_EXACT_OVERFLOW))) break;
            if (attempt >= 60) return fail(CMB_ERR_INTERNAL, "work queues keep overflowing");
            const uint32_t dfsCap = cap32(b->dfs.n), exCap = cap32(b->exq.n);
            if (c.verbose)
                fprintf(stderr, "[retry] queues too small:%s%s%s%s\n", c.hcnt[0] > c.q.itemCap ? " items" : "", c.hcnt[1] > c.q.fmCap ? " occurrences" : "",
                        c.hcnt[5] > dfsCap ? " tasks" : "", c.hcnt[4] > exCap ? " exact" : "");
            // (a search that stopped at the overflow has only counted what it needed up to there: the naive search of very
            // short reads, which match all over the text, asks for orders of magnitude more than the first guess)
            const size_t grow = b->hasNaive ? 8 : 2;
            if (c.hcnt[0] > c.q.itemCap) b->items.alloc((size_t)c.hcnt[0] * grow + 1024);
            if (c.hcnt[1] > c.q.fmCap) b->fm.alloc((size_t)c.hcnt[1] * grow + 1024);
            if (c.hcnt[5] > dfsCap) b->dfs.alloc((size_t)c.hcnt[5] + c.hcnt[5] / 8 + 1024);
            if (c.hcnt[4] > exCap) b->exq.alloc((size_t)c.hcnt[4] + c.hcnt[4] / 8 + 1024);
        }
        c.nItems = c.hcnt[0], c.nFm = c.hcnt[1];
        lap(c, "prep + search");
        if ((rc = dedupFmOccurrences(c)) != CMB_OK) return rc;
        lap(c, "fm occurrences");
        if ((rc = locateAndVerify(c)) != CMB_OK) return rc;
        lap(c, "verify + traceback + fmocc");
        if (c.preset) return finishPreset(c);

        if ((rc = filterNaive(c)) != CMB_OK) return rc;
        // TOTAL_REPORTED_POSITIONS (indexinterface.cpp:1378,1390 / :1333,1352)
        // (the device counter holds the records k_verify / k_traceback wrote; queue holes are not records)
        downloadCounters(b);
        b->cnts[1] += c.naiveSurvivors; // reported once more, as text occurrences of the read (indexinterface.cpp:1333, :1378)
        uint64_t total = 0;
        if ((rc = filterFinal(c, total)) != CMB_OK) return rc;
        lap(c, "filter");
        if ((rc = runCigar(c, total)) != CMB_OK) return rc;
        if ((rc = trimSpanning(c, total)) != CMB_OK) return rc;
        if ((rc = downloadResults(c, total)) != CMB_OK) return rc;
        b->done = true;
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

// ---- what the b-move translation unit borrows from this one (move_backend.hip: cmb_move_attach_text, alignments) -------------
// The b-move index holds no text (the reference builds the CIGAR of that flavour from a matched string that travels with the search,
// indexinterface.h:294-303).  With 288 GB of HBM a 2-bit copy of the text fits beside the index (a quarter byte per character: 50 GB for
// 64 human haplotypes next to ~130 GB of tables), and the matched string of an occurrence IS text[begin, end): findCIGAR on that
// window (k_cigar) gives the reference's CIGAR without carrying anything through the frontier.
namespace cmb {
int deviceOfIndex(const cmb_index* ix) { return ix->device; }
bool indexIsTextOnly(const cmb_index* ix) { return ix->textOnly; }
const std::vector<uint32_t>& seqStartsOfIndex(const cmb_index* textIndex) { return textIndex->seqStarts; }
// The final lists of a batch that has run with alignments, one view per part, for the SAM and pair drivers and the strata of BEST mode
int batchListViews(cmb_batch* b, bool perStrand, std::vector<ListView>& out) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    if (perStrand && b->ix == nullptr) return fail(CMB_ERR_INVALID, "a batch without an index");
    if (!b->done) return fail(CMB_ERR_INVALID, "batch has not been run");
    if (!b->wantAln) return fail(CMB_ERR_INVALID, "alignments were not requested (cmb_batch_want_alignments)");
    if (perStrand && !b->perStrand) return fail(CMB_ERR_INVALID, "the strands were not filtered each by itself (cmb_batch_filter_per_strand)");
    std::vector<cmb_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    out.clear();
    for (cmb_batch* c : parts) {
        ListView v;
        v.nReads = c->nReads, v.k = c->k, v.metric = c->metric, v.textIndex = c->ix;
        v.reads = c->reads.p, v.offs = c->offs.p;
        v.goffs = c->foffs.p, v.groupStride = c->perStrand ? 2u : 1u;
        v.occ = c->fout.p, v.aln = c->alnRec.p, v.ops = c->alnOps.p, v.stride = c->alnStride;
        v.stream = c->stream;
        v.hostOffs = c->hostOffs.data();
        v.hOcc = c->occs.data(), v.hOccBytes = sizeof(cmb_occ), v.hOccOffs = c->occOffs.data(), v.hOffsPerGroup = true;
        v.hAln = c->hAlnRec.data(), v.hOps = c->hAlnOps.data();
        v.cnts = c->cnts, v.times = &c->times;
        v.bufs = &c->samBufs, v.scanTmp = &c->scanTmp;
        v.trimOnDevice = c->trimOn, v.trimDropped = c->trimStats[2];
        out.push_back(v);
    }
    return CMB_OK;
}
// (declared in units.hpp; the k_cigar launch of runCigar)
int moveCigarsOnText(cmb_index* textIndex, hipStream_t s, const uint64_t* offs, const uint32_t* G, uint32_t gw, uint32_t nReads, uint32_t maxLen,
                     uint32_t k, int gapless, const uint4* occs, const uint32_t* occRead, uint64_t nOcc, AlnRec* aln, uint16_t* ops, uint32_t stride,
                     uint32_t* flagWord) {
    try {
        HIPCHK(hipSetDevice(textIndex->device));
        if (!nOcc) return CMB_OK;
        DevBuf<uint4> mfull;
        MFull mf{nullptr, 0};
        if (!gapless) {
            mf.nBlk = mfullBlocks(maxLen);
            const uint64_t nW = (uint64_t)2 * nReads * mf.nBlk;
            mfull.alloc(2 * nW);
            hipLaunchKernelGGL(k_match_words, dim3((unsigned)((nW + 255) / 256)), dim3(256), 0, s, G, gw, offs, 2 * nReads, mf.nBlk, mfull.p);
            mf.p = mfull.p;
        }
        const uint32_t cSlots = capSlots((uint32_t)std::min<uint64_t>(((nOcc + 255) / 256) * 256, 512u * 1024u));
        // (beyond 9 errors the matrix with the wide left margin, as for the FM-index batches; match words straight from the read's bit-strings)
        DevBuf<uint64_t> vW;
        DevBuf<uint8_t> slab;
        const CigarJob job{offs, G, gw, maxLen, mf, occs, occRead, nOcc, ops, stride, aln, flagWord, gapless ? 1u : 0u};
        launchCigar(textIndex, s, job, !gapless && k > CIGAR_BLOCK_WORDS_MAX_ED, k <= TBN_MAX_ED, vRows(maxLen), cSlots, vW, slab,
                    getenv("CMB_VERBOSE") != nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s)); // (the temporaries above go out of scope)
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}
} // namespace cmb

extern "C" int cmb_batch_result_size(const cmb_batch* b, uint64_t* n_occ) {
    if (!b || !n_occ) return fail(CMB_ERR_INVALID, "null argument");
    if (!b->done) return fail(CMB_ERR_INVALID, "batch has not been run");
    uint64_t n = b->occs.size();
    for (const cmb_batch* c : b->subs) n += c->occs.size();
    *n_occ = n;
    return CMB_OK;
}
extern "C" int cmb_batch_results(const cmb_batch* b, cmb_occ* out, uint64_t out_cap, uint64_t* out_offs,
                                 uint64_t* counters) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    if (!b->done) return fail(CMB_ERR_INVALID, "batch has not been run");
    if (!b->subs.empty()) { // composite: the sub-batches' lists one after the other, offsets rebased
        uint64_t total = 0;
        for (const cmb_batch* c : b->subs) total += c->occs.size();
        if (out_cap < total) return fail(CMB_ERR_OVERFLOW, "output buffer too small");
        uint64_t base = 0, read = 0;
        for (const cmb_batch* c : b->subs) {
            if (out && !c->occs.empty()) memcpy(out + base, c->occs.data(), c->occs.size() * sizeof(cmb_occ));
            if (out_offs)
                for (uint32_t i = 0; i < c->nReads; i++) out_offs[read + i] = base + c->occOffs.data()[c->perStrand ? 2 * (size_t)i : i];
            read += c->nReads;
            base += c->occs.size();
        }
        if (out_offs) out_offs[read] = base;
        if (counters) memcpy(counters, b->cnts, sizeof(b->cnts));
        return CMB_OK;
    }
    if (out_cap < b->occs.size()) return fail(CMB_ERR_OVERFLOW, "output buffer too small");
    if (out && !b->occs.empty()) memcpy(out, b->occs.data(), b->occs.size() * sizeof(cmb_occ));
    if (out_offs) {
        if (b->perStrand)
            for (uint32_t i = 0; i <= b->nReads; i++) out_offs[i] = b->occOffs.data()[2 * (size_t)i];
        else memcpy(out_offs, b->occOffs.data(), b->occOffs.size() * sizeof(uint64_t));
    }
    if (counters) memcpy(counters, b->cnts, sizeof(b->cnts));
    return CMB_OK;
}
extern "C" int cmb_batch_filter_per_strand(cmb_batch* b, int on) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    // the group of a key becomes read x strand: a sub-batch of more than 2^(group bits - 1) reads (only reachable
    // through CMB_SUBBATCH_SPLIT) would overflow it in k_pack_keys after the search — refused before any work instead
    if (on)
        for (const cmb_batch* c : b->subs.empty() ? std::vector<const cmb_batch*>{b} : std::vector<const cmb_batch*>(b->subs.begin(), b->subs.end()))
            if ((uint64_t)c->nReads > (1ull << (groupBits(c) - 1)))
                return fail(CMB_ERR_UNSUPPORTED, "a sub-batch of more than 2^" + std::to_string(groupBits(c) - 1) +
                                                     " reads cannot filter every strand by itself (read x strand does not fit the filter key)");
    b->perStrand = on != 0;
    for (cmb_batch* c : b->subs) c->perStrand = on != 0;
    b->done = false;
    return CMB_OK;
}
extern "C" int cmb_batch_want_alignments(cmb_batch* b, int on) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    b->wantAln = on != 0;
    for (cmb_batch* c : b->subs) c->wantAln = on != 0;
    b->done = false;
    return CMB_OK;
}
// the occurrences over the end of their sequence are trimmed or dropped by the run itself (trimSpanning); FM-index batches in ALL mode
extern "C" int cmb_batch_trim_on_device(cmb_batch* b, int on) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    if (on && !b->wantAln) return fail(CMB_ERR_INVALID, "trimming on the device needs the alignments (cmb_batch_want_alignments)");
    b->trimOn = on != 0;
    for (cmb_batch* c : b->subs) c->trimOn = on != 0;
    b->done = false;
    return CMB_OK;
}
extern "C" int cmb_batch_trim_stats(const cmb_batch* b, uint64_t* spanning, uint64_t* trimmed, uint64_t* dropped) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    if (!b->done) return fail(CMB_ERR_INVALID, "batch has not been run");
    uint64_t t[3] = {b->trimStats[0], b->trimStats[1], b->trimStats[2]};
    for (const cmb_batch* c : b->subs)
        for (int i = 0; i < 3; i++) t[i] += c->trimStats[i];
    if (spanning) *spanning = t[0];
    if (trimmed) *trimmed = t[1];
    if (dropped) *dropped = t[2];
    return CMB_OK;
}
extern "C" int cmb_batch_alignments(const cmb_batch* b, cmb_aln* out, uint64_t cap, uint16_t* cigar_ops, uint64_t ops_cap,
                                    uint64_t* n_ops) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    if (!b->done) return fail(CMB_ERR_INVALID, "batch has not been run");
    if (!b->wantAln) return fail(CMB_ERR_INVALID, "alignments were not requested (cmb_batch_want_alignments)");
    std::vector<const cmb_batch*> parts;
    if (b->subs.empty()) parts.push_back(b);
    else
        for (const cmb_batch* c : b->subs) parts.push_back(c);
    uint64_t total = 0, ops = 0;
    for (const cmb_batch* c : parts) {
        total += c->hAlnRec.size();
        for (size_t i = 0; i < c->hAlnRec.size(); i++) ops += c->hAlnRec.data()[i].nOps;
    }
    if (n_ops) *n_ops = ops;
    if (cap < total || ops_cap < ops) return fail(CMB_ERR_OVERFLOW, "output buffer too small");
    uint64_t o = 0, po = 0;
    for (const cmb_batch* c : parts)
        for (size_t i = 0; i < c->hAlnRec.size(); i++) {
            const AlnRec& r = c->hAlnRec.data()[i];
            out[o] = cmb_aln{r.seqId, r.seqBegin, po, (uint16_t)r.nOps, (uint16_t)r.spans};
            const uint16_t* src = c->hAlnOps.data() + i * c->alnStride;
            for (uint32_t j = 0; j < r.nOps; j++) cigar_ops[po + j] = src[r.nOps - 1 - j]; // (stored end to begin)
            po += r.nOps;
            o++;
        }
    return CMB_OK;
}
extern "C" int cmb_batch_timings(const cmb_batch* b, const char** names, float* ms, uint32_t cap) {
    if (!b) return 0;
    uint32_t n = 0;
    for (const auto& t : b->times) {
        if (n >= cap) break;
        if (names) names[n] = t.name;
        if (ms) ms[n] = t.ms;
        n++;
    }
    return (int)n;
}
// Reads not longer than the number of parts of the search scheme (and every read of a one-part strategy) are matched by naive
// backtracking, as in the reference (searchstrategy.cpp:148-152, :442-459; indexinterface.cpp:1055-1210 -> dev_bfs_naive.hpp).
// cmb_batch_read_status says which reads took that path; cmb_batch_allow_unsupported is kept for older callers and has no effect.
extern "C" int cmb_batch_allow_unsupported(cmb_batch* b, int on) {
    (void)on;
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    return CMB_OK;
}
static uint32_t readStatusOne(const cmb_batch* b, uint8_t* status) {
    uint32_t n = 0;
    const uint32_t P = b->k ? b->sNumParts : 0;
    for (uint32_t i = 0; i < b->nReads; i++) {
        const uint64_t len = b->hostOffs[i + 1] - b->hostOffs[i];
        const bool naive = b->k > 0 && (P >= len || P == 1);
        if (status) status[i] = naive ? CMB_READ_NAIVE_FALLBACK : 0;
        n += naive;
    }
    return n;
}
extern "C" int cmb_batch_read_status(const cmb_batch* b, uint8_t* status, uint32_t* n_flagged) {
    if (!b) return fail(CMB_ERR_INVALID, "null argument");
    uint32_t n = 0;
    if (b->subs.empty()) n = readStatusOne(b, status);
    else
        for (size_t j = 0; j < b->subs.size(); j++) n += readStatusOne(b->subs[j], status ? status + b->subBound[j] : nullptr);
    if (n_flagged) *n_flagged = n;
    return CMB_OK;
}

extern "C" void cmb_batch_destroy(cmb_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ix->device);
    delete b;
}

extern "C" int cmb_match_batch(cmb_index* idx, const cmb_strategy* st, uint32_t max_distance, const char* seqs,
                               const uint64_t* offs, uint32_t n_reads, cmb_occ* out, uint64_t out_cap,
                               uint64_t* out_offs, uint64_t* counters, uint64_t* needed) {
    cmb_batch* b = nullptr;
    int rc = cmb_batch_create(idx, st, max_distance, seqs, offs, n_reads, &b);
    if (rc) return rc;
    rc = cmb_batch_run(b);
    if (rc == CMB_OK) {
        uint64_t n = 0;
        cmb_batch_result_size(b, &n);
        if (needed) *needed = n;
        rc = cmb_batch_results(b, out, out_cap, out_offs, counters);
    }
    cmb_batch_destroy(b);
    return rc;
}

// ------------------------------------------------------------------------- fine-grained hooks
extern "C" int cmb_rank_batch(cmb_index* idx, int rev, const uint32_t* c, const uint64_t* p, uint64_t n,
                              uint64_t* out) {
    if (!idx || (n && (!c || !p || !out))) return fail(CMB_ERR_INVALID, "null argument");
    try {
        useDevice(idx->device);
        for (uint64_t i = 0; i < n; i++)
            if (c[i] > 3 || p[i] > idx->d.n) return fail(CMB_ERR_INVALID, "rank argument out of range");
        DevBuf<uint32_t> dc;
        DevBuf<uint64_t> dp, dout;
        dc.upload(c, n);
        dp.upload(p, n);
        dout.alloc(n);
        if (n) hipLaunchKernelGGL(k_rank, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, idx->d, rev, dc.p, dp.p, n, dout.p);
        HIPCHK(hipGetLastError());
        if (n) HIPCHK(hipMemcpy(out, dout.p, n * 8, hipMemcpyDeviceToHost));
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

static int checkRanges(const cmb_index* idx, const uint32_t* in, uint64_t n) {
    for (uint64_t i = 0; i < 4 * n; i++)
        if (in[i] > idx->d.n) return fail(CMB_ERR_INVALID, "range bound beyond the text length");
    return CMB_OK;
}

extern "C" int cmb_extend_batch(cmb_index* idx, int mode, const uint32_t* in, uint64_t n, uint32_t* out,
                                uint8_t* ok) {
    if (!idx || mode < 0 || mode > 2 || (n && (!in || !out || !ok))) return fail(CMB_ERR_INVALID, "bad argument");
    if (checkRanges(idx, in, n)) return CMB_ERR_INVALID;
    try {
        useDevice(idx->device);
        DevBuf<uint4> din, dout;
        DevBuf<uint8_t> dok;
        din.upload((const uint4*)in, n);
        dout.alloc(4 * n);
        dok.alloc(4 * n);
        if (n) {
            const unsigned nb = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 32);
            hipLaunchKernelGGL(k_extend, dim3(nb), dim3(256), 0, 0, idx->d, mode, din.p, n, dout.p, dok.p);
        }
        HIPCHK(hipGetLastError());
        if (n) {
            HIPCHK(hipMemcpy(out, dout.p, n * 64, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(ok, dok.p, n * 4, hipMemcpyDeviceToHost));
        }
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

extern "C" int cmb_extend_bench(cmb_index* idx, int mode, const void* d_in, uint64_t n, void* d_out, void* d_ok,
                                uint32_t iters, float* avg_ms) {
    if (!idx || mode < 0 || mode > 2 || !d_in || !d_out || !d_ok || !avg_ms || !iters)
        return fail(CMB_ERR_INVALID, "bad argument");
    try {
        useDevice(idx->device);
        hipStream_t s;
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        const unsigned nb = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 32);
        auto kern = k_extend;
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, idx->d, mode, (const uint4*)d_in, n, (uint4*)d_out,
                           (uint8_t*)d_ok); // warm-up
        HIPCHK(hipEventRecord(a, s));
        for (uint32_t i = 0; i < iters; i++)
            hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, idx->d, mode, (const uint4*)d_in, n,
                               (uint4*)d_out, (uint8_t*)d_ok);
        HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, a, b));
        *avg_ms = ms / iters;
        HIPCHK(hipGetLastError());
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        (void)hipStreamDestroy(s);
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

extern "C" int cmb_locate_batch(cmb_index* idx, const uint32_t* rows, uint64_t n, uint32_t* out,
                                uint64_t* lf_steps) {
    if (!idx || (n && (!rows || !out))) return fail(CMB_ERR_INVALID, "null argument");
    for (uint64_t i = 0; i < n; i++)
        if (rows[i] >= idx->d.n) return fail(CMB_ERR_INVALID, "suffix array row out of range");
    try {
        useDevice(idx->device);
        DevBuf<uint32_t> dr, dout;
        DevBuf<unsigned long long> dlf;
        dr.upload(rows, n);
        dout.alloc(n);
        dlf.alloc(1);
        HIPCHK(hipMemset(dlf.p, 0, 8));
        if (n) hipLaunchKernelGGL(k_locate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, idx->d, dr.p, n, dout.p, dlf.p);
        HIPCHK(hipGetLastError());
        if (n) HIPCHK(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
        unsigned long long lf = 0;
        HIPCHK(hipMemcpy(&lf, dlf.p, 8, hipMemcpyDeviceToHost));
        if (lf_steps) *lf_steps = lf;
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

// The PRODUCTION edit-distance verification path for one pattern and n start positions: k_verify<KEYS> (one key per
// candidate) -> radix sort + run-length encode (identical candidates are verified once, counters scaled by the
// multiplicity) -> k_verify_stage x stages -> k_traceback (beyond 7 errors: -> k_wide_filter -> k_verify_wide), exactly as cmb_batch_run
// runs it (it IS cmb_batch_run on a one-read batch whose in-text items are given).  Same contract as cmb_verify_batch, incl. duplicates in `starts`.
extern "C" int cmb_verify_batch_staged(cmb_index* idx, const char* pattern, uint32_t plen, const uint32_t* starts,
                                       uint64_t n, uint32_t max_ed, uint32_t min_ed, int fixed_start, cmb_occ* out,
                                       uint64_t out_cap, uint64_t* n_out, uint64_t* counters) {
    if (!idx || !pattern || (n && !starts) || !n_out) return fail(CMB_ERR_INVALID, "null argument");
    if (plen == 0 || plen > (uint32_t)MAX_READ) return fail(CMB_ERR_UNSUPPORTED, "pattern length not supported");
    if (max_ed == 0 || max_ed > MXN_MAX_ED || min_ed > 15) return fail(CMB_ERR_UNSUPPORTED, "more than 13 errors"); // (8 ... 13: k_wide_filter + k_verify_wide)
    if (n >= (1ull << 31)) return fail(CMB_ERR_INVALID, "too many start positions");
    for (uint64_t i = 0; i < n; i++)
        if (starts[i] > idx->d.n) return fail(CMB_ERR_INVALID, "start position beyond the text");
    *n_out = 0;
    if (n == 0) {
        if (counters) memset(counters, 0, CMB_CNT_MAX * sizeof(uint64_t));
        return CMB_OK;
    }
    cmb_strategy* st = nullptr;
    int rc = cmb_strategy_create_named("columba", CMB_METRIC_EDIT, CMB_PARTITION_UNIFORM, &st); // (schemes for 1..7 errors; unused)
    if (rc) return rc;
    cmb_batch* b = nullptr;
    const uint64_t ho[2] = {0, plen};
    rc = batchCreateOne(idx, st, max_ed, pattern, ho, 1, &b);
    cmb_strategy_destroy(st);
    if (rc) return rc;
    const uint32_t meta = (max_ed << 12) | (min_ed << 16) | ((fixed_start ? 1u : 0u) << 20) | ((uint32_t)ITEM_EDIT << 21) | (1u << 23);
    b->presetItems.resize(n);
    for (uint64_t i = 0; i < n; i++) b->presetItems[i] = make_uint4(0, starts[i], 0, meta); // (bit 23: nothing to locate)
    rc = batchRunOne(b);
    if (rc == CMB_OK) {
        std::vector<TextOccRec> t = b->presetOut;
        t.erase(std::remove_if(t.begin(), t.end(), [](const TextOccRec& x) { return x.rsId == 0xFFFFFFFFu; }), t.end());
        std::sort(t.begin(), t.end(), [](const TextOccRec& x, const TextOccRec& y) {
            if (x.begin != y.begin) return x.begin < y.begin;
            if (x.end != y.end) return x.end < y.end;
            return x.dist < y.dist;
        });
        *n_out = t.size();
        if (t.size() > out_cap) rc = fail(CMB_ERR_OVERFLOW, "output buffer too small");
        else
            for (size_t i = 0; i < t.size(); i++) out[i] = cmb_occ{t[i].begin, t[i].end, t[i].dist, 0};
        if (counters) memcpy(counters, b->cnts, sizeof(b->cnts));
    }
    cmb_batch_destroy(b);
    return rc;
}

// in-text verification hook: FMIndex::inTextVerification(startPos, maxED, minED, ..., pattern,
// fixedStartPos) (fmindex.cpp:267-310) for one pattern.  Runs the production k_prep + k_verify on a
// one-read batch whose items carry the start positions directly (meta bit 23: nothing to locate).
static int verifyDirect(cmb_index* idx, const char* pattern, uint32_t plen, const uint32_t* starts, const uint32_t* ends,
                        uint64_t n, uint32_t max_ed, uint32_t min_ed, int fixed_start, cmb_occ* out, uint64_t out_cap,
                        uint64_t* n_out, uint64_t* counters);
extern "C" int cmb_verify_batch(cmb_index* idx, const char* pattern, uint32_t plen, const uint32_t* starts,
                                uint64_t n, uint32_t max_ed, uint32_t min_ed, int fixed_start, cmb_occ* out,
                                uint64_t out_cap, uint64_t* n_out, uint64_t* counters) {
    return verifyDirect(idx, pattern, plen, starts, nullptr, n, max_ed, min_ed, fixed_start, out, out_cap, n_out, counters);
}
// FMIndex::inTextVerificationOneString (fmindex.cpp:312-342): the pattern against ONE text window [start, end) with a
// fixed start (one zero in the first column) — what IndexInterface::findSeqName runs on an occurrence it has trimmed
// to the sequence it lies in (indexinterface.cpp:850-866)
extern "C" int cmb_verify_window(cmb_index* idx, const char* pattern, uint32_t plen, uint32_t start, uint32_t end,
                                 uint32_t max_ed, uint32_t min_ed, cmb_occ* out, uint64_t out_cap, uint64_t* n_out,
                                 uint64_t* counters) {
    if (end <= start) return fail(CMB_ERR_INVALID, "empty text window");
    return verifyDirect(idx, pattern, plen, &start, &end, 1, max_ed, min_ed, 1, out, out_cap, n_out, counters);
}
static int verifyDirect(cmb_index* idx, const char* pattern, uint32_t plen, const uint32_t* starts, const uint32_t* ends,
                        uint64_t n, uint32_t max_ed, uint32_t min_ed, int fixed_start, cmb_occ* out, uint64_t out_cap,
                        uint64_t* n_out, uint64_t* counters) {
    if (!idx || !pattern || (n && !starts) || !n_out) return fail(CMB_ERR_INVALID, "null argument");
    if (plen == 0 || plen > (uint32_t)MAX_READ) return fail(CMB_ERR_UNSUPPORTED, "pattern length not supported");
    const bool dp = 3 * max_ed + 1 > MXW_LEFT; // beyond 7 errors: k_verify_wide (the band does not fit the bit-parallel in-text matrices)
    if (max_ed > MXN_MAX_ED || min_ed > 15) return fail(CMB_ERR_UNSUPPORTED, "more than 13 errors");
    for (uint64_t i = 0; i < n; i++)
        if (starts[i] > idx->d.n) return fail(CMB_ERR_INVALID, "start position beyond the text");
    try {
        useDevice(idx->device);
        const uint32_t mlen = (plen + 15u) & ~15u; // row stride of the per-read arrays (k_prep stores 16 bytes)
        const uint32_t gw = gWords(mlen);
        DevBuf<uint8_t> reads, seq;
        DevBuf<uint64_t> offs;
        DevBuf<uint32_t> G, cnt;
        DevBuf<uint4> items;
        DevBuf<TextOccRec> text;
        DevBuf<uint64_t> vW;
        DevBuf<uint4> tbq;
        DevBuf<unsigned long long> ctr;
        const uint64_t ho[2] = {0, plen};
        reads.uploadPadded((const uint8_t*)pattern, plen, 64);
        offs.upload(ho, 2);
        seq.alloc(2 * (size_t)mlen);
        G.alloc(8 * (size_t)gw);
        std::vector<uint4> hi(n);
        const uint32_t meta = (max_ed << 12) | (min_ed << 16) | ((fixed_start ? 1u : 0u) << 20) |
                              ((uint32_t)ITEM_EDIT << 21) | (1u << 23);
        for (uint64_t i = 0; i < n; i++) hi[i] = make_uint4(0, starts[i], ends ? ends[i] : 0u, meta);
        items.upload(hi.data(), n);
        // (every wavefront of k_verify / k_traceback may leave one partly used chunk of 256 records)
        const size_t cap = n * 32 + 64 + 2 * (std::min<uint64_t>(std::max<uint64_t>(((n + 255) / 256) * 256, 256), 65536) / 64 + 1) * 256;
        text.alloc(cap);
        cnt.alloc(8);
        ctr.alloc(CMB_CNT_MAX);
        HIPCHK(hipMemset(cnt.p, 0, 32));
        HIPCHK(hipMemset(ctr.p, 0, CMB_CNT_MAX * 8));
        const uint32_t slots = capSlots((uint32_t)std::min<uint64_t>(std::max<uint64_t>(((n + 255) / 256) * 256, 256), 65536));
        const bool verbose = getenv("CMB_VERBOSE") != nullptr;
        const bool narrow = max_ed <= TBN_MAX_ED && !getenv("CMB_TRACE_WIDE");
        const uint32_t tLines = traceLines(narrow, (uint32_t)VROWS);
        vW.alloc((size_t)tLines * 8 * slots);
        tbq.alloc(n + (size_t)(slots / 64 + 1) * 256);
        VPlanes vp{vW.p, slots, tLines};
        Queues q{};
        q.text = text.p;
        q.textCap = (uint32_t)cap;
        q.cnt = cnt.p;
        q.counters = ctr.p;
        DevBuf<uint4> mfull;
        MFull mf{nullptr, mfullBlocks(mlen)};
        mfull.alloc((size_t)2 * 2 * mf.nBlk);
        launchPrep(0, reads.p, offs.p, 1u, mlen, gw, seq.p, G.p, nullptr, 0u, mfull.p, mf.nBlk, verbose);
        mf.p = mfull.p;
        uint32_t hc[8];
        if (n && dp) {
            DevBuf<uint8_t> slab;
            const uint32_t slotBytes = (vwRows(mlen) + 1u) * VW_ROW_BYTES;
            const uint32_t dSlots = capSlots((uint32_t)std::min<uint64_t>(((n + 255) / 256) * 256, 256u * 64u));
            slab.alloc((size_t)slotBytes * dSlots);
            gridLine(verbose, "k_verify_wide", n, dSlots);
            auto kWide = k_verify_wide<false, WxTen>;
            if (max_ed > MX_MAX_ED) kWide = k_verify_wide<false, WxThirteen>;
            hipLaunchKernelGGL(kWide, dim3(dSlots / 256), dim3(256), 0, 0, idx->d, offs.p, mlen, seq.p, G.p, gw, items.p, (uint32_t)n,
                               (const unsigned long long*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, slab.p,
                               slotBytes, q);
            HIPCHK(hipDeviceSynchronize());
        } else if (n) {
            gridLine(verbose, "k_verify", n, slots);
            hipLaunchKernelGGL(k_verify<false>, dim3(slots / 256), dim3(256), 0, 0, idx->d, offs.p, mlen, gw, seq.p, mf,
                               items.p, (uint32_t)n, tbq.p, (uint32_t)tbq.n, (unsigned long long*)nullptr, q);
            HIPCHK(hipMemcpy(hc, cnt.p, 32, hipMemcpyDeviceToHost));
            if (hc[7]) {
                gridLine(verbose, "k_traceback", hc[7], slots);
                launchTraceback(0, idx->d, narrow, offs.p, mf, tbq.p, hc[7], vp, q, 0u);
            }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(hc, cnt.p, 32, hipMemcpyDeviceToHost));
        if (hc[3] & FLAG_TEXT_OVERFLOW) return fail(CMB_ERR_INTERNAL, "verification output overflow");
        if (hc[3] & (FLAG_CAPACITY | FLAG_TRACE_RULE)) return fail(CMB_ERR_INTERNAL, "a traceback left the band");
        std::vector<TextOccRec> t(hc[2]);
        if (hc[2]) HIPCHK(hipMemcpy(t.data(), text.p, hc[2] * sizeof(TextOccRec), hipMemcpyDeviceToHost));
        t.erase(std::remove_if(t.begin(), t.end(), [](const TextOccRec& x) { return x.rsId == 0xFFFFFFFFu; }),
                t.end()); // holes of the wavefronts' queue chunks
        *n_out = t.size();
        if (t.size() > out_cap) return fail(CMB_ERR_OVERFLOW, "output buffer too small");
        std::sort(t.begin(), t.end(), [](const TextOccRec& x, const TextOccRec& y) {
            if (x.begin != y.begin) return x.begin < y.begin;
            if (x.end != y.end) return x.end < y.end;
            return x.dist < y.dist;
        });
        for (size_t i = 0; i < t.size(); i++) out[i] = cmb_occ{t[i].begin, t[i].end, t[i].dist, 0};
        if (counters) {
            unsigned long long c2[CMB_CNT_MAX];
            HIPCHK(hipMemcpy(c2, ctr.p, sizeof(c2), hipMemcpyDeviceToHost));
            for (int i = 0; i < CMB_CNT_MAX; i++) counters[i] = c2[i];
        }
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

// CIGAR of one pattern against n text windows [begin, end) with given distances (IBitParallelED::findCIGAR,
// bitparallelmatrix.h:460-527) on the device: k_cigar over a one-read batch.  ops_out: n x stride run-length
// operations (length << 2 | op) from the begin of the alignment, n_ops_out[i] of them for window i.
extern "C" int cmb_cigar_windows(cmb_index* idx, const char* pattern, uint32_t plen, const uint32_t* begins,
                                 const uint32_t* ends, const uint32_t* distances, uint64_t n, uint16_t* ops_out,
                                 uint32_t stride, uint32_t* n_ops_out) {
    if (!idx || !pattern || (n && (!begins || !ends || !distances || !ops_out || !n_ops_out))) return fail(CMB_ERR_INVALID, "null argument");
    if (plen == 0 || plen > (uint32_t)MAX_READ) return fail(CMB_ERR_UNSUPPORTED, "pattern length not supported");
    uint32_t maxD = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (ends[i] < begins[i] || ends[i] > idx->d.n) return fail(CMB_ERR_INVALID, "text window out of range");
        if (ends[i] - begins[i] > plen + distances[i]) return fail(CMB_ERR_INVALID, "text window longer than an alignment within the distance");
        maxD = std::max(maxD, distances[i]);
    }
    if (maxD > MXN_MAX_ED) return fail(CMB_ERR_UNSUPPORTED, "more than 13 errors"); // (fixed start: the band of 2 maxD + 1 <= 27 columns fits the in-text matrix)
    if (stride < 2 * maxD + 3) return fail(CMB_ERR_INVALID, "stride must be at least 2 * distance + 3");
    if (n == 0) return CMB_OK;
    try {
        useDevice(idx->device);
        const uint32_t mlen = (plen + 15u) & ~15u, gw = gWords(mlen);
        DevBuf<uint8_t> reads, seq;
        DevBuf<uint64_t> offs, vW;
        DevBuf<uint32_t> G, occRead, flag;
        DevBuf<uint4> occs, mfull;
        DevBuf<uint16_t> ops;
        DevBuf<AlnRec> aln;
        const uint64_t ho[2] = {0, plen};
        reads.uploadPadded((const uint8_t*)pattern, plen, 64);
        offs.upload(ho, 2);
        seq.alloc(2 * (size_t)mlen);
        G.alloc(8 * (size_t)gw);
        MFull mf{nullptr, mfullBlocks(mlen)};
        mfull.alloc((size_t)2 * 2 * mf.nBlk);
        launchPrep(0, reads.p, offs.p, 1u, mlen, gw, seq.p, G.p, nullptr, 0u, mfull.p, mf.nBlk, getenv("CMB_VERBOSE") != nullptr);
        mf.p = mfull.p;
        std::vector<uint4> ho4(n);
        for (uint64_t i = 0; i < n; i++) ho4[i] = make_uint4(begins[i], ends[i], distances[i], 0u);
        occs.upload(ho4.data(), n);
        std::vector<uint32_t> zeros(n, 0u);
        occRead.upload(zeros.data(), n);
        flag.alloc(1);
        HIPCHK(hipMemset(flag.p, 0, sizeof(uint32_t)));
        const uint32_t slots = (uint32_t)std::min<uint64_t>(((n + 255) / 256) * 256, 65536);
        ops.alloc(n * stride);
        aln.alloc(n);
        DevBuf<uint8_t> slab;
        const CigarJob job{offs.p, G.p, gw, mlen, mf, occs.p, occRead.p, n, ops.p, stride, aln.p, flag.p, 0u};
        launchCigar(idx, 0, job, maxD > CIGAR_BLOCK_WORDS_MAX_ED, maxD <= TBN_MAX_ED, (uint32_t)VROWS, slots, vW, slab, false);
        HIPCHK(hipGetLastError());
        uint32_t hf = 0;
        HIPCHK(hipMemcpy(&hf, flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (hf) return fail(CMB_ERR_INTERNAL, "a CIGAR traceback left the band or a window is not an alignment within its distance");
        std::vector<AlnRec> ha(n);
        std::vector<uint16_t> hops(n * stride);
        HIPCHK(hipMemcpy(ha.data(), aln.p, n * sizeof(AlnRec), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hops.data(), ops.p, n * stride * sizeof(uint16_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; i++) {
            n_ops_out[i] = ha[i].nOps;
            for (uint32_t j = 0; j < ha[i].nOps; j++) ops_out[i * stride + j] = hops[i * stride + ha[i].nOps - 1 - j];
        }
        return CMB_OK;
    } catch (const std::exception& e) {
        return fail(CMB_ERR_DEVICE, e.what());
    }
}

