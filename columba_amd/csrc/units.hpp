// What crosses the library's translation units: every function one unit defines and another calls is declared here, once, and the
// definer includes this header as its users do (pair_sam.hip and pair_best.hip are host code and share host_error.hpp alone).
#pragma once
#include "../../include/columba_amd.h"
#include "host_best.hpp"
#include "host_error.hpp"
#include "host_sam.hpp"
#include "host_util.hpp"

namespace cmb {
// ---- columba_amd.hip (the index, the strategy, the FM batch, the fine-grained hooks; the only unit with kernels.hpp)
int deviceOfIndex(const cmb_index* ix);
bool indexIsTextOnly(const cmb_index* ix);
const std::vector<uint32_t>& seqStartsOfIndex(const cmb_index* textIndex);
inline void useDeviceOf(const cmb_index* ix) { HIPCHK(hipSetDevice(deviceOfIndex(ix))); }
// one view per part of a batch that has run with alignments (perStrand: and with every strand filtered by itself, as the pair path needs)
int batchListViews(cmb_batch* b, bool perStrand, std::vector<ListView>& out);
// CIGAR and sequence assignment of nOcc occurrences {begin, end, distance, strand} of the reads `occRead` on a text: the k_cigar launch
// of an FM batch for a caller that has the pieces (device pointers throughout; ops: nOcc x stride, stored end to begin)
int moveCigarsOnText(cmb_index* textIndex, hipStream_t s, const uint64_t* offs, const uint32_t* G, uint32_t gw, uint32_t nReads, uint32_t maxLen,
                     uint32_t k, int gapless, const uint4* occs, const uint32_t* occRead, uint64_t nOcc, AlnRec* aln, uint16_t* ops, uint32_t stride,
                     uint32_t* flagWord);
// The arrays of cmb_index_desc in the reference's layouts, already in HBM on the index's device (seqStarts alone is a host array).
// cmb_index_create uploads a description into this form; cmb_build_index (build.hip) hands over the arrays the device builder made.
struct IndexDeviceArrays {
    uint64_t n;          // text length with the final '$'
    const uint8_t* text; // ASCII
    uint64_t counts[5], dollarFwd, dollarRev;
    const uint64_t *bvFwd, *cntFwd, *bvRev, *cntRev, *saBv, *saBvCounts;
    const uint32_t* saSamples;
    uint64_t nSamples;
    uint32_t saSparseness;
    const uint32_t* seqStarts;
    uint32_t nSeqs, kmerSize, inTextSwitch;
};
// everything cmb_index_create does behind its upload: the re-laid-out rank blocks, text codes and 2-bit text, the k-mer table, the
// consistency probe, the dense suffix array and the sequence starts.  The arguments have been checked; the arrays stay the caller's.
int indexFromDeviceArrays(const IndexDeviceArrays& a, int device, cmb_index** out);
// ---- move_backend.hip
// The arrays of a b-move index in the DEVICE layout, already in HBM on the index's device: per direction the 16-byte rows 0 .. runs (the
// terminating row among them; room for runs + 2 rows, the gap fields not yet filled) and the samples; the locate arrays as
// cmb_move_desc names them.  cmb_move_create uploads and unpacks a description into this form; cmb_build_move_index (build.hip) hands
// over what the device builder made.
struct MoveDeviceArrays {
    uint64_t n = 0; // text length with the final '$'
    struct Side {
        DevBuf<uint4> rows;
        DevBuf<uint64_t> smpF, smpL;
        uint64_t runs = 0, zeroCharPos = 0;
    } side[2]; // the text, the reversed text
    bool hasLocate = false;
    DevBuf<uint64_t> predFirst, firstToRun, predLast, lastToRun, plcpPos, plcpSum; // (plcpPos.n: the number of PLCP runs)
};
// everything cmb_move_create does behind its upload: the gap fields, the directories of the position sets and every consistency check
// (CMB_ERR_INVALID for arrays that are not a consistent index).  The index takes the buffers over: `a` is left empty.
int moveIndexFromDeviceArrays(MoveDeviceArrays& a, int device, cmb_move_index** out);
// one view per part of a batch that has run with its lists kept (cmb_move_batch_keep_device_lists)
int moveBatchListViews(cmb_move_batch* b, std::vector<ListView>& out);

// ---- sam.hip
// IndexInterface::findSeqName for an occurrence that runs over the end of its sequence (indexinterface.cpp:833-899):
// trim to the sequence it mostly lies in and verify again inside that window (edit distance only)
bool trimOccurrence(cmb_index* idx, const std::string& seq, uint32_t largestStratum, int metric, BestOcc& o, uint64_t* counters);
// a record of the lists in HBM as the host containers hold it (CIGAR runs are stored end to begin)
inline BestOcc bestOccOf(const uint4& o, const AlnRec& a, const uint16_t* ops) {
    BestOcc b;
    b.occ = cmb_occ{o.x, o.y, o.z, o.w};
    const uint32_t nOps = std::min<uint32_t>(a.nOps, BEST_OPS_STRIDE);
    b.aln = cmb_aln{a.seqId, a.seqBegin, 0, (uint16_t)nOps, (uint16_t)a.spans, 0};
    for (uint32_t j = 0; j < nOps; j++) b.ops.push_back(ops[nOps - 1 - j]);
    return b;
}
} // namespace cmb

// The result of BEST mode (best.hip fills it; sam.hip writes the SAM text of a device-resident one): plain data
struct cmb_best {
    std::vector<cmb_occ> occ;
    std::vector<cmb_aln> aln;
    std::vector<uint16_t> ops;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> best, nHits;
    uint64_t cnts[CMB_CNT_MAX];
    // cmb_match_best_device: the final lists in HBM, in the layout k_sam_write reads (SamCtx: occurrences as uint4, AlnRec, CIGAR runs
    // at BEST_OPS_STRIDE stored end to begin, 64-bit offsets per read); occ / aln / ops above are filled from them on first use
    bool onDevice = false, fetched = false;
    cmb_index* ix = nullptr;
    int metric = 1;
    uint32_t nReads = 0, x = 0;
    uint64_t nOcc = 0;
    cmb::DevBuf<uint4> dOcc;
    cmb::DevBuf<cmb::AlnRec> dAln;
    cmb::DevBuf<uint16_t> dOps;
    cmb::DevBuf<uint64_t> dOffs;
    cmb::DevBuf<uint32_t> dBest, dHits;
    std::vector<uint8_t> hostRead; // reads whose bookkeeping went through the host (an occurrence over a sequence end, edit distance)
    uint32_t nHostReads = 0;
    // cmb_best_sam_device: the SAM driver's buffers, the chunk's raw reads (the batches of the strata are gone), the reads the host
    // formats as a flag per read (k_sam_plan_best), the finished text
    cmb::SamDeviceBufs sam;
    cmb::DevBuf<uint8_t> samReads, samHostFlag, scanTmp;
    cmb::DevBuf<uint64_t> samReadOffs;
    cmb::PinnedBuf<char> samOut;
    std::vector<uint64_t> readOffs; // the chunk's read offsets, as given to cmb_match_best_device
    // cmb_best_timings: host time per phase of the call (every phase ends in a synchronise) and, summed over the strata, the
    // device time of the batches' kernels as cmb_batch_timings names them
    std::vector<std::pair<std::string, double>> times;
    void addTime(const std::string& name, double ms) {
        for (auto& t : times)
            if (t.first == name) {
                t.second += ms;
                return;
            }
        times.push_back({name, ms});
    }
    bool readsUp = false;
};
