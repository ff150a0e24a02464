// BEST (+x strata) mode (include/columba_amd.h): the strata loop over batches of either backend, with the bookkeeping on the host or
// on the device (dev_best.hpp), and the result's accessors.  Of a batch this unit sees the C-ABI and its list views (units.hpp).
#include "units.hpp"
#include "dev_best.hpp"

#include <chrono>
#include <functional>
#include <memory>

using namespace cmb;

// SearchStrategy::matchApproxBestPlusX / findBestAlignments / processSeq / mapRead / checkAlignments /
// combineOccVectors (reference src/searchstrategy.cpp:623-760, :791-812, :536-620; src/searchstrategy.h:490-523).
// The reference walks every read through its strata on its own: exact matches, then k = 1, 3, 5, 9, 13 (k + x + 2 below
// 5, + 4 above) up to the identity cut-off, until a stratum holds an alignment; every stratum is one ALL-mode search
// of ONE strand (mapRead) whose occurrences below the first unprocessed distance are dropped.  Here a stratum is one
// device batch over all reads that are still looking at that distance: both strands at once, each strand filtered
// by itself (cmb_batch_filter_per_strand), CIGARs and sequence assignment from the device (k_cigar); the per-read
// bookkeeping below is the reference's.
namespace {
// what one stratum returns: the ALL-mode lists of a set of reads at distance k, both strands, every strand filtered by itself
struct StratumOut {
    std::vector<cmb_occ> oc;
    std::vector<cmb_aln> al;
    std::vector<uint16_t> ops;
    std::vector<uint64_t> oo, cnt;
};
typedef std::function<int(const char* cat, const uint64_t* o, uint32_t n, uint32_t k, StratumOut& r)> StratumRunner;

// The strata loop's store (host_best.hpp) with every read's occurrences in host vectors.
// idx: the index whose text and sequence starts serve the trimming (the FM-index itself, or the text beside a b-move index);
// trimCounters: the in-text counters of a trimming count (FM-index flavour: inTextVerificationOneString; the b-move flavour's
// checkTrimmedMatch counts nothing, indexinterface.cpp:722-796)
struct BestHostStore {
    cmb_index* idx;
    const cmb_strategy* st;
    bool trimCounters;
    const StratumRunner& runOn;
    const char* seqs;
    const uint64_t* offs;
    cmb_best* R;
    std::vector<BestCursor> cur;
    std::vector<BestHostRead> rd;

    BestCursor& cursor(uint32_t i) { return cur[i]; }
    bool nonEmpty(uint32_t i, int s2, uint32_t d) const { return rd[i].nonEmpty(s2, d); }
    void check(uint32_t i, int s2, uint32_t l, uint32_t cutOffTrim) {
        bestCheckHost(rd[i], cur[i].best, s2, l, cutOffTrim, [&](const std::string& seq, BestOcc& o, uint32_t cutOff) {
            return trimOccurrence(idx, seq, cutOff, st->metric, o, trimCounters ? R->cnts : nullptr);
        });
    }
    // one stratum for a set of reads: ALL-mode search of both strands at distance k, every strand filtered by itself
    int run(const std::vector<uint32_t>& ids, uint32_t k) {
        std::string cat;
        std::vector<uint64_t> o;
        bestGatherReads(seqs, offs, ids, cat, o);
        StratumOut so;
        if (const int rcode = runOn(cat.data(), o.data(), (uint32_t)ids.size(), k, so)) return rcode;
        for (int i = 0; i < CMB_CNT_MAX; i++) R->cnts[i] += so.cnt[i];
        for (size_t j = 0; j < ids.size(); j++) {
            const uint32_t minD = std::min<uint32_t>(cur[ids[j]].proc, k); // processSeq (:791-812): the first distance not processed yet
            for (uint64_t q2 = so.oo[j]; q2 < so.oo[j + 1]; q2++) {
                const cmb_aln& a = so.al[q2];
                if (so.oc[q2].distance >= minD)
                    rd[ids[j]].add(BestOcc{so.oc[q2], a, std::vector<uint16_t>(so.ops.begin() + a.cigar_off, so.ops.begin() + a.cigar_off + a.cigar_len)});
            }
        }
        return CMB_OK;
    }
};

// deviceCap: the largest distance the flavour's device path runs
int matchBestWith(cmb_index* idx, const cmb_strategy* st, uint32_t deviceCap, bool trimCounters, const StratumRunner& runOn, uint32_t x,
                  uint32_t min_identity, const char* seqs, const uint64_t* offs, uint32_t n_reads, cmb_best** out) {
    if (!idx || !st || !offs || !out || (!seqs && n_reads)) return failWith(CMB_ERR_INVALID, "null argument");
    if (min_identity < 50 || min_identity > 100) return failWith(CMB_ERR_INVALID, "the minimal identity lies between 50 and 100");
    try {
        const uint32_t maxSupported = bestMaxSupported(st->schemes, deviceCap);
        std::unique_ptr<cmb_best> R(new cmb_best());
        memset(R->cnts, 0, sizeof(R->cnts));
        BestHostStore S{idx, st, trimCounters, runOn, seqs, offs, R.get(), std::vector<BestCursor>(n_reads), std::vector<BestHostRead>(n_reads)};
        for (uint32_t i = 0; i < n_reads; i++) {
            S.cur[i] = bestCursor(bestMaxED(maxSupported, (uint32_t)(offs[i + 1] - offs[i]), min_identity));
            S.rd[i].fw = cleanReadSeq(std::string(seqs + offs[i], seqs + offs[i + 1]));
            S.rd[i].rc = revComplWithN(S.rd[i].fw);
            S.rd[i].start(S.cur[i].cutOff);
        }
        if (const int rcode = bestStrataLoop(S, n_reads, x)) return rcode;
        // ---- results: combineOccVectors (:573-620) per read
        R->offs.assign(n_reads + 1, 0);
        R->best.assign(n_reads, 0xFFFFFFFFu);
        R->nHits.assign(n_reads, 0);
        for (uint32_t i = 0; i < n_reads; i++) {
            const BestCursor& r = S.cur[i];
            R->offs[i] = R->occ.size();
            if (!r.bestFound) continue;
            R->best[i] = r.best;
            R->nHits[i] = S.rd[i].hitsAt(r.best);
            bestCombineHost(S.rd[i], r.best, std::min<uint32_t>(r.best + x, r.cutOff), [&](const BestOcc& o) {
                cmb_aln a = o.aln;
                a.cigar_off = R->ops.size();
                a.cigar_len = (uint16_t)o.ops.size();
                a.spans = o.aln.spans == 2 ? 2 : 0;
                R->ops.insert(R->ops.end(), o.ops.begin(), o.ops.end());
                R->occ.push_back(o.occ);
                R->aln.push_back(a);
            });
        }
        R->offs[n_reads] = R->occ.size();
        *out = R.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}
} // namespace

extern "C" int cmb_match_best(cmb_index* idx, const cmb_strategy* st, uint32_t x, uint32_t min_identity, const char* seqs,
                              const uint64_t* offs, uint32_t n_reads, cmb_best** out) {
    if (!idx || !st) return failWith(CMB_ERR_INVALID, "null argument");
    const StratumRunner run = [&](const char* cat, const uint64_t* o, uint32_t n, uint32_t k, StratumOut& r) -> int {
        cmb_batch* b = nullptr;
        int rcode = cmb_batch_create(idx, st, k, cat, o, n, &b);
        if (rcode) return rcode;
        struct Guard {
            cmb_batch* b;
            ~Guard() { cmb_batch_destroy(b); }
        } guard{b};
        cmb_batch_filter_per_strand(b, 1);
        cmb_batch_want_alignments(b, 1);
        if ((rcode = cmb_batch_run(b))) return rcode;
        uint64_t nOcc = 0, nOps = 0;
        cmb_batch_result_size(b, &nOcc);
        r.oc.resize(nOcc ? nOcc : 1);
        r.al.resize(nOcc ? nOcc : 1);
        r.oo.resize((size_t)n + 1);
        r.cnt.assign(CMB_CNT_MAX, 0);
        if ((rcode = cmb_batch_results(b, r.oc.data(), r.oc.size(), r.oo.data(), r.cnt.data()))) return rcode;
        (void)cmb_batch_alignments(b, r.al.data(), 0, nullptr, 0, &nOps);
        r.ops.resize(nOps ? nOps : 1);
        return cmb_batch_alignments(b, r.al.data(), r.al.size(), r.ops.data(), r.ops.size(), &nOps);
    };
    // (MAX_K, definitions.h:50)
    return matchBestWith(idx, st, 13u, true, run, x, min_identity, seqs, offs, n_reads, out);
}
// ---- BEST mode with the bookkeeping on the device (dev_best.hpp) ------------------------------------------------------------------
// The strata loop and every per-read decision are the ones matchBestWith runs (host_best.hpp; searchstrategy.cpp:623-712); what that
// keeps in vectors per read, strand and distance is here a pool of records in HBM plus, per read, a few words on the host: which
// distances hold an occurrence / an occurrence inside one sequence (from k_best_scan), which went through checkAlignments, and the
// cursor.  The host touches those words once per read and stratum and no occurrence — except for the reads that keep an occurrence over a sequence end
// under edit distance: trimming verifies again and moves the occurrence to another distance (checkAlignments, :536-571), so from that
// stratum on such a read's lists live in host vectors as in matchBestWith, and its final records are spliced into the device lists.
namespace {
struct BestDevRead {
    BestCursor c;
    bool host = false; // its lists live in a BestHostRead
    uint16_t any[2] = {0, 0}, asg[2] = {0, 0}, chk[2] = {0, 0};
};
struct BestPoolBufs {
    DevBuf<uint4> occ;
    DevBuf<AlnRec> aln;
    DevBuf<uint16_t> ops;
    DevBuf<uint32_t> read;
    uint64_t n = 0, cap = 0;
    BestPool at(uint64_t i) { return BestPool{occ.p + i, aln.p + i, ops.p + i * BEST_OPS_STRIDE, read.p + i}; }
    void reserve(uint64_t want) { // (the exact size is known before a record is written: the pool never overflows)
        if (want <= cap) return;
        const uint64_t c = want + want / 2 + 4096;
        BestPoolBufs f;
        f.occ.alloc(c), f.aln.alloc(c), f.ops.alloc(c * BEST_OPS_STRIDE), f.read.alloc(c);
        if (n) {
            HIPCHK(hipMemcpy(f.occ.p, occ.p, n * sizeof(uint4), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(f.aln.p, aln.p, n * sizeof(AlnRec), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(f.ops.p, ops.p, n * BEST_OPS_STRIDE * sizeof(uint16_t), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(f.read.p, read.p, n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        }
        std::swap(occ.p, f.occ.p), std::swap(occ.n, f.occ.n);
        std::swap(aln.p, f.aln.p), std::swap(aln.n, f.aln.n);
        std::swap(ops.p, f.ops.p), std::swap(ops.n, f.ops.n);
        std::swap(read.p, f.read.p), std::swap(read.n, f.read.n);
        cap = c;
    }
};
// What one stratum leaves in HBM, whichever flavour matched it: per part the lists k_best_scan / k_best_append read (two filter groups
// per read), the counters and kernel times of its run, and how to let go of the batch that owns the lists.
struct StratumLists {
    uint32_t nReads;
    const uint64_t* foffs;
    const uint4* fout;
    const AlnRec* aln;
    const uint16_t* ops;
    uint32_t stride;
};
struct DevStratum {
    std::vector<StratumLists> parts;
    uint64_t cnts[CMB_CNT_MAX] = {};
    std::vector<KernelTime> times;
    std::function<void()> destroy;
    ~DevStratum() {
        if (destroy) destroy();
    }
    void adopt(const std::vector<ListView>& views) { // the lists, counters and kernel times of a batch that has run
        for (const ListView& v : views) {
            for (int i = 0; i < CMB_CNT_MAX; i++) cnts[i] += v.cnts[i];
            parts.push_back(StratumLists{v.nReads, v.goffs, v.occ, v.aln, v.ops, v.stride});
            times.insert(times.end(), v.times->begin(), v.times->end());
        }
    }
};
// create, per-strand filter, alignments, run: an ALL-mode search of both strands of `n` reads at distance k whose lists stay on the device
typedef std::function<int(const char* cat, const uint64_t* o, uint32_t n, uint32_t k, DevStratum& r, const std::function<void(const char*)>& lap)>
    DevStratumRunner;

// The strata loop's store (host_best.hpp) with the occurrences in a pool in HBM and, per read, masks of the distances that hold one;
// the reads that trimming takes to the host keep theirs in a BestHostRead.
// idx: the index whose text and sequence starts serve the trimming (the FM-index itself, or the text beside a b-move index);
// trimCounters: as for BestHostStore
struct BestDevStore {
    cmb_index* idx;
    const cmb_strategy* st;
    bool trimCounters;
    const DevStratumRunner& runOn;
    const char* seqs;
    const uint64_t* offs;
    uint32_t nReads;
    cmb_best* R;
    bool edit;
    std::vector<BestDevRead> rd;
    std::map<uint32_t, BestHostRead> hr;
    BestPoolBufs pool, stage;
    DevBuf<uint8_t> dMinD, dMode, tmp;
    DevBuf<uint32_t> dIds, dList;
    DevBuf<unsigned long long> dMasks;
    DevBuf<uint64_t> dCnt, dPoff;
    std::vector<uint8_t> hMinD, hMode;
    std::vector<unsigned long long> hMasks;

    BestCursor& cursor(uint32_t i) { return rd[i].c; }
    bool nonEmpty(uint32_t i, int s2, uint32_t d) { return rd[i].host ? hr[i].nonEmpty(s2, d) : ((rd[i].any[s2] >> d) & 1u) != 0; }
    // checkAlignments (:536-571).  On the device's side an occurrence is assigned (it lies inside one sequence) or dropped
    // (Hamming distance never trims); on the host's side it is BestHostStore's.
    void check(uint32_t i, int s2, uint32_t l, uint32_t cutOffTrim) {
        BestDevRead& r = rd[i];
        if (l > r.c.cutOff) return;
        if (r.host) {
            bestCheckHost(hr[i], r.c.best, s2, l, cutOffTrim, [&](const std::string& seq, BestOcc& o, uint32_t cutOff) {
                return trimOccurrence(idx, seq, cutOff, st->metric, o, trimCounters ? R->cnts : nullptr);
            });
            return;
        }
        const uint16_t bit = (uint16_t)(1u << l);
        r.any[s2] = (uint16_t)((r.any[s2] & ~bit) | (r.asg[s2] & bit));
        r.chk[s2] |= bit;
        if ((r.asg[s2] & bit) && l < r.c.best) r.c.best = (uint8_t)l;
    }
    // one stratum for a set of reads: ALL-mode search of both strands at distance k, every strand filtered by itself; the batch's
    // lists stay where they are
    int run(const std::vector<uint32_t>& ids, uint32_t k) {
        const uint32_t n = (uint32_t)ids.size();
        auto t0 = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) {
            auto t1 = std::chrono::steady_clock::now();
            R->addTime(what, std::chrono::duration<double, std::milli>(t1 - t0).count());
            t0 = t1;
        };
        std::string cat;
        std::vector<uint64_t> o;
        bestGatherReads(seqs, offs, ids, cat, o);
        lap("host: gather of the stratum's reads");
        DevStratum ds;
        if (const int rcode = runOn(cat.data(), o.data(), n, k, ds, lap)) return rcode;
        for (int i = 0; i < CMB_CNT_MAX; i++) R->cnts[i] += ds.cnts[i];
        const std::vector<StratumLists>& parts = ds.parts;
        for (const KernelTime& t : ds.times) R->addTime(std::string("strata: ") + t.name, t.ms);
        // processSeq (:791-812): what lies below the first distance not processed yet is dropped
        hMinD.resize(n);
        for (uint32_t j = 0; j < n; j++) hMinD[j] = (uint8_t)std::min<uint32_t>(rd[ids[j]].c.proc, k);
        growTo(dMinD, n), growTo(dIds, n), growTo(dMasks, n), growTo(dCnt, (size_t)n + 1), growTo(dPoff, (size_t)n + 1);
        HIPCHK(hipMemcpy(dMinD.p, hMinD.data(), n, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dIds.p, ids.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dCnt.p + n, 0, sizeof(uint64_t)));
        uint32_t base = 0;
        for (const StratumLists& c : parts) {
            if (c.nReads)
                hipLaunchKernelGGL(k_best_scan, dim3((c.nReads + 3u) / 4u), dim3(256), 0, 0, c.foffs, c.fout, c.aln, c.nReads, dMinD.p + base,
                                   dMasks.p + base, dCnt.p + base);
            base += c.nReads;
        }
        HIPCHK(hipGetLastError());
        scanExclusive(tmp, dCnt.p, dPoff.p, (size_t)n + 1, (hipStream_t)0);
        uint64_t kept = 0;
        hMasks.resize(n);
        HIPCHK(hipMemcpy(&kept, dPoff.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hMasks.data(), dMasks.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const uint64_t poolBase = pool.n;
        if (poolBase + kept >= 0xFFFFFFFFull) return failWith(CMB_ERR_UNSUPPORTED, "more than 2^32 occurrences in the strata of one chunk");
        pool.reserve(poolBase + kept);
        base = 0;
        for (const StratumLists& c : parts) {
            if (c.nReads && kept)
                hipLaunchKernelGGL(k_best_append, dim3((c.nReads + 3u) / 4u), dim3(256), 0, 0, c.foffs, c.fout, c.aln, c.ops, c.stride, c.nReads,
                                   dMinD.p + base, dIds.p + base, dPoff.p + base, pool.at(poolBase));
            base += c.nReads;
        }
        HIPCHK(hipGetLastError());
        pool.n = poolBase + kept;
        // the words of every read; the reads that go to, or are with, the host
        bool anyHost = false, anyNew = false;
        for (uint32_t j = 0; j < n; j++) {
            BestDevRead& r = rd[ids[j]];
            const unsigned long long m = hMasks[j];
            if (r.host) {
                hMode[ids[j]] = 1, anyHost = true;
                continue;
            }
            r.any[0] |= (uint16_t)((m >> BEST_ANY0) & 0x3FFFu), r.any[1] |= (uint16_t)((m >> BEST_ANY1) & 0x3FFFu);
            r.asg[0] |= (uint16_t)((m >> BEST_ASG0) & 0x3FFFu), r.asg[1] |= (uint16_t)((m >> BEST_ASG1) & 0x3FFFu);
            if (edit && ((m >> BEST_SPAN) & 1ull)) hMode[ids[j]] = 2, anyHost = anyNew = true;
        }
        if (anyHost) {
            const uint64_t from = anyNew ? 0 : poolBase, span = pool.n - from;
            growTo(dMode, nReads);
            growTo(dList, (size_t)span + 1);
            HIPCHK(hipMemcpy(dMode.p, hMode.data(), nReads, hipMemcpyHostToDevice));
            HIPCHK(hipMemset(dList.p, 0, sizeof(uint32_t)));
            uint32_t nList = 0;
            if (span) {
                hipLaunchKernelGGL(k_best_collect, dim3((uint32_t)((span + 255u) / 256u)), dim3(256), 0, 0, pool.read.p, from, pool.n, poolBase,
                                   dMode.p, dList.p);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpy(&nList, dList.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
            }
            std::vector<uint32_t> list(nList);
            std::vector<uint4> go(nList);
            std::vector<AlnRec> ga(nList);
            std::vector<uint16_t> gp((size_t)nList * BEST_OPS_STRIDE);
            std::vector<uint32_t> gr(nList);
            if (nList) {
                HIPCHK(hipMemcpy(list.data(), dList.p + 1, (size_t)nList * sizeof(uint32_t), hipMemcpyDeviceToHost));
                std::sort(list.begin(), list.end()); // (the order in which the records were found)
                HIPCHK(hipMemcpy(dList.p + 1, list.data(), (size_t)nList * sizeof(uint32_t), hipMemcpyHostToDevice));
                growTo(stage.occ, nList), growTo(stage.aln, nList), growTo(stage.ops, (size_t)nList * BEST_OPS_STRIDE), growTo(stage.read, nList);
                hipLaunchKernelGGL(k_best_gather, dim3((nList + 255u) / 256u), dim3(256), 0, 0, dList.p + 1, nList, pool.at(0), stage.at(0));
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpy(go.data(), stage.occ.p, (size_t)nList * sizeof(uint4), hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(ga.data(), stage.aln.p, (size_t)nList * sizeof(AlnRec), hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(gp.data(), stage.ops.p, gp.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(gr.data(), stage.read.p, (size_t)nList * sizeof(uint32_t), hipMemcpyDeviceToHost));
            }
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t i = ids[j];
                if (hMode[i] == 2) {
                    BestHostRead& h = hr[i];
                    h.fw = cleanReadSeq(std::string(seqs + offs[i], seqs + offs[i + 1]));
                    h.rc = revComplWithN(h.fw);
                    h.start(rd[i].c.cutOff);
                    rd[i].host = true;
                }
                hMode[i] = 0;
            }
            for (uint32_t t = 0; t < nList; t++) hr[gr[t]].add(bestOccOf(go[t], ga[t], gp.data() + (size_t)t * BEST_OPS_STRIDE));
        }
        HIPCHK(hipDeviceSynchronize()); // (the batch and its lists go away)
        lap("host: strata bookkeeping (k_best_scan, k_best_append, host reads)");
        ds.destroy();
        ds.destroy = nullptr;
        lap("host: cmb_batch_destroy");
        return CMB_OK;
    }
};

int matchBestDeviceWith(cmb_index* idx, const cmb_strategy* st, bool trimCounters, const DevStratumRunner& runOn, uint32_t x, uint32_t min_identity,
                        const char* seqs, const uint64_t* offs, uint32_t n_reads, cmb_best** out) {
    if (!idx || !st || !offs || !out || (!seqs && n_reads)) return failWith(CMB_ERR_INVALID, "null argument");
    if (min_identity < 50 || min_identity > 100) return failWith(CMB_ERR_INVALID, "the minimal identity lies between 50 and 100");
    try {
        useDeviceOf(idx);
        const uint32_t maxSupported = bestMaxSupported(st->schemes, 13u); // (MAX_K, definitions.h:50)
        std::unique_ptr<cmb_best> R(new cmb_best());
        memset(R->cnts, 0, sizeof(R->cnts));
        R->onDevice = true, R->ix = idx, R->metric = st->metric, R->nReads = n_reads, R->x = x;
        R->readOffs.assign(offs, offs + n_reads + 1);
        BestDevStore S{idx, st, trimCounters, runOn, seqs, offs, n_reads, R.get(), st->metric != CMB_METRIC_HAMMING};
        S.rd.resize(n_reads), S.hMode.assign(n_reads, 0);
        for (uint32_t i = 0; i < n_reads; i++) S.rd[i].c = bestCursor(bestMaxED(maxSupported, (uint32_t)(offs[i + 1] - offs[i]), min_identity));
        if (const int rcode = bestStrataLoop(S, n_reads, x)) return rcode;
        BestPoolBufs& pool = S.pool;
        DevBuf<uint8_t>& tmp = S.tmp;
        const auto tFinal = std::chrono::steady_clock::now();
        // ---- results: combineOccVectors (:573-620).  Pool reads on the device; host reads as matchBestWith does
        std::vector<unsigned long long> hState(n_reads, 0);
        R->best.assign(n_reads, 0xFFFFFFFFu);
        R->hostRead.assign(n_reads, 0);
        for (uint32_t i = 0; i < n_reads; i++) {
            const BestDevRead& r = S.rd[i];
            if (r.host) R->hostRead[i] = 1, R->nHostReads++;
            if (!r.c.bestFound) continue;
            R->best[i] = r.c.best;
            const unsigned long long hi = std::min<uint32_t>(r.c.best + x, r.c.cutOff);
            if (!r.host)
                hState[i] = (unsigned long long)r.c.best | (hi << 8) | (1ull << 16) | ((unsigned long long)(r.chk[0] & 0x3FFFu) << 32) |
                            ((unsigned long long)(r.chk[1] & 0x3FFFu) << 46);
        }
        std::vector<uint4> sOcc; // the final records of the host reads, one read after the other
        std::vector<AlnRec> sAln;
        std::vector<uint16_t> sOps;
        std::vector<uint32_t> hostHits;
        std::vector<std::pair<uint32_t, uint64_t>> hostAt; // (read, its first record in sOcc)
        for (auto& kv : S.hr) {
            const uint32_t i = kv.first;
            const BestCursor& r = S.rd[i].c;
            BestHostRead& h = kv.second;
            hostAt.push_back({i, sOcc.size()});
            hostHits.push_back(0);
            if (!r.bestFound) continue;
            hostHits.back() = h.hitsAt(r.best);
            bestCombineHost(h, r.best, std::min<uint32_t>(r.best + x, r.cutOff), [&](const BestOcc& o) {
                const uint32_t nOps = (uint32_t)std::min<size_t>(o.ops.size(), BEST_OPS_STRIDE);
                sOcc.push_back(uint4{o.occ.begin, o.occ.end, o.occ.distance, o.occ.strand});
                sAln.push_back(AlnRec{o.aln.seq_id, o.aln.seq_begin, nOps, o.aln.spans == 2 ? 2u : 0u});
                const size_t at = sOps.size();
                sOps.resize(at + BEST_OPS_STRIDE, 0);
                for (uint32_t j = 0; j < nOps; j++) sOps[at + j] = o.ops[nOps - 1 - j]; // (CIGAR runs are stored end to begin)
            });
        }
        hostAt.push_back({n_reads, sOcc.size()});
        DevBuf<unsigned long long> dState;
        DevBuf<uint32_t> dFlag, dPerRead;
        DevBuf<uint64_t> dPos, dUflag, dUpos, dDevBase;
        DevBuf<BestKey> keysA, keysB;
        const uint64_t nPool = pool.n;
        growTo(dState, n_reads), growTo(R->dHits, n_reads), growTo(R->dBest, n_reads), growTo(dPerRead, n_reads);
        growTo(dFlag, (size_t)nPool + 1), growTo(dPos, (size_t)nPool + 1);
        if (n_reads) {
            HIPCHK(hipMemcpy(dState.p, hState.data(), (size_t)n_reads * sizeof(unsigned long long), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(R->dBest.p, R->best.data(), (size_t)n_reads * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIPCHK(hipMemset(R->dHits.p, 0, (size_t)n_reads * sizeof(uint32_t)));
            HIPCHK(hipMemset(dPerRead.p, 0, (size_t)n_reads * sizeof(uint32_t)));
        }
        HIPCHK(hipMemset(dFlag.p + nPool, 0, sizeof(uint32_t)));
        uint64_t nSel = 0, nDev = 0;
        if (nPool) {
            hipLaunchKernelGGL(k_best_flag, dim3((uint32_t)((nPool + 255u) / 256u)), dim3(256), 0, 0, pool.at(0), nPool, dState.p, dFlag.p, R->dHits.p);
            HIPCHK(hipGetLastError());
            scanExclusive(tmp, dFlag.p, dPos.p, (size_t)nPool + 1, (hipStream_t)0);
            HIPCHK(hipMemcpy(&nSel, dPos.p + nPool, sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
        growTo(dUflag, (size_t)nSel + 1), growTo(dUpos, (size_t)nSel + 1);
        if (nSel) {
            keysA.alloc(nSel), keysB.alloc(nSel);
            hipLaunchKernelGGL(k_best_keys, dim3((uint32_t)((nPool + 255u) / 256u)), dim3(256), 0, 0, pool.at(0), nPool, dFlag.p, dPos.p, keysA.p);
            HIPCHK(hipGetLastError());
            // order: distance, strand, (sequence, begin inside it), the order in which the records were found — the last key makes the
            // order total, so the (stable) merge sort has no ties to keep
            withScratch(tmp, [&](void* p, size_t& bytes) {
                return rocprim::merge_sort(p, bytes, keysA.p, keysB.p, (size_t)nSel, BestKeyLess(), (hipStream_t)0);
            });
            HIPCHK(hipMemset(dUflag.p + nSel, 0, sizeof(uint64_t)));
            hipLaunchKernelGGL(k_best_uniq, dim3((uint32_t)((nSel + 255u) / 256u)), dim3(256), 0, 0, keysB.p, nSel, dUflag.p, dPerRead.p);
            HIPCHK(hipGetLastError());
            scanExclusive(tmp, dUflag.p, dUpos.p, (size_t)nSel + 1, (hipStream_t)0);
            HIPCHK(hipMemcpy(&nDev, dUpos.p + nSel, sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
        // every read's place in the final lists: a running sum over one word per read
        std::vector<uint32_t> perRead(n_reads, 0);
        R->nHits.assign(n_reads, 0);
        if (n_reads) {
            HIPCHK(hipMemcpy(perRead.data(), dPerRead.p, (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(R->nHits.data(), R->dHits.p, (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        std::vector<uint64_t> devBase((size_t)n_reads + 1, 0);
        R->offs.assign((size_t)n_reads + 1, 0);
        {
            size_t h = 0;
            for (uint32_t i = 0; i < n_reads; i++) {
                uint64_t mine = perRead[i];
                if (h + 1 < hostAt.size() && hostAt[h].first == i) {
                    mine = hostAt[h + 1].second - hostAt[h].second;
                    R->nHits[i] = hostHits[h];
                    HIPCHK(hipMemcpy(R->dHits.p + i, &hostHits[h], sizeof(uint32_t), hipMemcpyHostToDevice));
                    h++;
                }
                devBase[i + 1] = devBase[i] + perRead[i];
                R->offs[i + 1] = R->offs[i] + mine;
            }
        }
        const uint64_t total = R->offs[n_reads];
        R->nOcc = total;
        growTo(R->dOffs, (size_t)n_reads + 1), growTo(dDevBase, (size_t)n_reads + 1);
        HIPCHK(hipMemcpy(R->dOffs.p, R->offs.data(), ((size_t)n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dDevBase.p, devBase.data(), ((size_t)n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        R->dOcc.alloc(total), R->dAln.alloc(total), R->dOps.alloc(total * BEST_OPS_STRIDE);
        const BestPool fin{R->dOcc.p, R->dAln.p, R->dOps.p, nullptr};
        if (nSel) {
            hipLaunchKernelGGL(k_best_emit, dim3((uint32_t)((nSel + 255u) / 256u)), dim3(256), 0, 0, keysB.p, nSel, dUflag.p, dUpos.p, dDevBase.p,
                               R->dOffs.p, pool.at(0), fin);
            HIPCHK(hipGetLastError());
        }
        for (size_t h = 0; h + 1 < hostAt.size(); h++) { // the host reads' records at their place
            const uint64_t s0 = hostAt[h].second, cnt = hostAt[h + 1].second - s0, at = R->offs[hostAt[h].first];
            if (!cnt) continue;
            HIPCHK(hipMemcpy(R->dOcc.p + at, sOcc.data() + s0, cnt * sizeof(uint4), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(R->dAln.p + at, sAln.data() + s0, cnt * sizeof(AlnRec), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(R->dOps.p + at * BEST_OPS_STRIDE, sOps.data() + s0 * BEST_OPS_STRIDE, cnt * BEST_OPS_STRIDE * sizeof(uint16_t),
                             hipMemcpyHostToDevice));
        }
        HIPCHK(hipDeviceSynchronize());
        R->addTime("host: final selection, sort, lists", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tFinal).count());
        *out = R.release();
        return CMB_OK;
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}
} // namespace

extern "C" int cmb_match_best_device(cmb_index* idx, const cmb_strategy* st, uint32_t x, uint32_t min_identity, const char* seqs,
                                     const uint64_t* offs, uint32_t n_reads, cmb_best** out) {
    if (!idx || !st || !offs || !out || (!seqs && n_reads)) return failWith(CMB_ERR_INVALID, "null argument");
    if (min_identity < 50 || min_identity > 100) return failWith(CMB_ERR_INVALID, "the minimal identity lies between 50 and 100");
    if (indexIsTextOnly(idx)) return failWith(CMB_ERR_INVALID, "this index holds only the text (cmb_index_create_text_only): nothing can be matched on it");
    const DevStratumRunner run = [&](const char* cat, const uint64_t* o, uint32_t n, uint32_t k, DevStratum& r,
                                     const std::function<void(const char*)>& lap) -> int {
        cmb_batch* b = nullptr;
        int rcode = cmb_batch_create(idx, st, k, cat, o, n, &b);
        if (rcode) return rcode;
        r.destroy = [b] { cmb_batch_destroy(b); };
        cmb_batch_filter_per_strand(b, 1);
        cmb_batch_want_alignments(b, 1);
        lap("host: cmb_batch_create");
        if ((rcode = cmb_batch_run(b))) return rcode;
        lap("host: cmb_batch_run");
        std::vector<ListView> views;
        if ((rcode = batchListViews(b, true, views))) return rcode;
        r.adopt(views);
        return CMB_OK;
    };
    return matchBestDeviceWith(idx, st, true, run, x, min_identity, seqs, offs, n_reads, out);
}
// The same on the b-move index: the strata are b-move batches whose final lists stay in HBM (cmb_move_batch_keep_device_lists), the
// trimming of the host reads uses the text beside the index and counts nothing, as cmb_move_match_best; the result carries the text-only
// index, so cmb_best_results, cmb_best_host_reads, cmb_best_timings and cmb_best_sam_device work on it as on an FM-index result.
extern "C" int cmb_move_match_best_device(cmb_move_index* idx, const cmb_strategy* st, uint32_t x, uint32_t min_identity, uint32_t kmer_size,
                                          const char* seqs, const uint64_t* offs, uint32_t n_reads, cmb_best** out) {
    if (!idx || !st || !offs || !out || (!seqs && n_reads)) return failWith(CMB_ERR_INVALID, "null argument");
    cmb_index* text = cmb_move_text_index(idx);
    if (!text) return failWith(CMB_ERR_INVALID, "BEST mode on the b-move index needs the text beside it (cmb_move_attach_text)");
    const DevStratumRunner run = [&](const char* cat, const uint64_t* o, uint32_t n, uint32_t k, DevStratum& r,
                                     const std::function<void(const char*)>& lap) -> int {
        cmb_move_batch* b = nullptr;
        int rcode = cmb_move_batch_create(idx, st, k, kmer_size, cat, o, n, &b);
        if (rcode) return rcode;
        r.destroy = [b] { cmb_move_batch_destroy(b); };
        cmb_move_batch_filter_per_strand(b, 1);
        if ((rcode = cmb_move_batch_want_alignments(b, 1))) return rcode;
        if ((rcode = cmb_move_batch_keep_device_lists(b, 1))) return rcode;
        lap("host: cmb_batch_create");
        if ((rcode = cmb_move_batch_run(b))) return rcode;
        lap("host: cmb_batch_run");
        std::vector<ListView> views;
        if ((rcode = moveBatchListViews(b, views))) return rcode;
        r.adopt(views);
        return CMB_OK;
    };
    return matchBestDeviceWith(text, st, false, run, x, min_identity, seqs, offs, n_reads, out);
}
// The same on the b-move index (the reference's RUN_LENGTH_COMPRESSION build runs the same matchApproxBestPlusX): the strata are
// b-move batches, CIGARs and trimming read the matched string of an occurrence from the text beside the index (cmb_move_attach_text).
extern "C" int cmb_move_match_best(cmb_move_index* idx, const cmb_strategy* st, uint32_t x, uint32_t min_identity, uint32_t kmer_size,
                                   const char* seqs, const uint64_t* offs, uint32_t n_reads, cmb_best** out) {
    if (!idx || !st) return failWith(CMB_ERR_INVALID, "null argument");
    cmb_index* text = cmb_move_text_index(idx);
    if (!text) return failWith(CMB_ERR_INVALID, "BEST mode on the b-move index needs the text beside it (cmb_move_attach_text)");
    const StratumRunner run = [&](const char* cat, const uint64_t* o, uint32_t n, uint32_t k, StratumOut& r) -> int {
        cmb_move_batch* b = nullptr;
        int rcode = cmb_move_batch_create(idx, st, k, kmer_size, cat, o, n, &b);
        if (rcode) return rcode;
        struct Guard {
            cmb_move_batch* b;
            ~Guard() { cmb_move_batch_destroy(b); }
        } guard{b};
        cmb_move_batch_filter_per_strand(b, 1);
        if ((rcode = cmb_move_batch_want_alignments(b, 1))) return rcode;
        if ((rcode = cmb_move_batch_run(b))) return rcode;
        uint64_t nOcc = 0, nOps = 0;
        cmb_move_batch_result_size(b, &nOcc);
        std::vector<cmb_move_occ> mo(nOcc ? nOcc : 1);
        r.al.resize(nOcc ? nOcc : 1);
        r.oo.resize((size_t)n + 1);
        r.cnt.assign(CMB_CNT_MAX, 0);
        if ((rcode = cmb_move_batch_results(b, mo.data(), mo.size(), r.oo.data(), r.cnt.data()))) return rcode;
        r.oc.resize(nOcc ? nOcc : 1);
        for (uint64_t i = 0; i < nOcc; i++) {
            r.oc[i].begin = (uint32_t)mo[i].begin, r.oc[i].end = (uint32_t)mo[i].end; // (texts below 2^32: cmb_move_attach_text)
            r.oc[i].distance = mo[i].distance, r.oc[i].strand = mo[i].strand;
        }
        (void)cmb_move_batch_alignments(b, r.al.data(), 0, nullptr, 0, &nOps);
        r.ops.resize(nOps ? nOps : 1);
        return cmb_move_batch_alignments(b, r.al.data(), r.al.size(), r.ops.data(), r.ops.size(), &nOps);
    };
    // (strata up to 13 errors, the reference's MAX_K, as on the FM-index: the b-move search runs that far since round 3, its alignments since round 4)
    return matchBestWith(text, st, 13u, false, run, x, min_identity, seqs, offs, n_reads, out);
}
// the lists of a device-resident result on the host, packed as cmb_match_best packs them (CIGAR runs from the begin, one after the other)
static void fetchBest(cmb_best* r) {
    if (!r->onDevice || r->fetched) return;
    useDeviceOf(r->ix);
    const uint64_t n = r->nOcc;
    r->occ.resize(n);
    r->aln.resize(n);
    std::vector<AlnRec> ar(n);
    std::vector<uint16_t> raw((size_t)n * BEST_OPS_STRIDE);
    if (n) {
        static_assert(sizeof(cmb_occ) == sizeof(uint4), "cmb_occ is the device's occurrence record");
        HIPCHK(hipMemcpy(r->occ.data(), r->dOcc.p, n * sizeof(cmb_occ), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ar.data(), r->dAln.p, n * sizeof(AlnRec), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(raw.data(), r->dOps.p, raw.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    uint64_t nOps = 0;
    for (uint64_t i = 0; i < n; i++) nOps += ar[i].nOps;
    r->ops.resize(nOps);
    uint64_t po = 0;
    for (uint64_t i = 0; i < n; i++) {
        r->aln[i] = cmb_aln{ar[i].seqId, ar[i].seqBegin, po, (uint16_t)ar[i].nOps, (uint16_t)ar[i].spans, 0};
        const uint16_t* src = raw.data() + i * BEST_OPS_STRIDE;
        for (uint32_t j = 0; j < ar[i].nOps; j++) r->ops[po + j] = src[ar[i].nOps - 1 - j]; // (stored end to begin)
        po += ar[i].nOps;
    }
    r->fetched = true;
}
extern "C" int cmb_best_sizes(const cmb_best* r, uint64_t* n_occ, uint64_t* n_ops) {
    if (!r) return failWith(CMB_ERR_INVALID, "null argument");
    try {
        fetchBest(const_cast<cmb_best*>(r));
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
    if (n_occ) *n_occ = r->occ.size();
    if (n_ops) *n_ops = r->ops.size();
    return CMB_OK;
}
extern "C" int cmb_best_results(const cmb_best* r, cmb_occ* occ, cmb_aln* aln, uint64_t cap, uint16_t* cigar_ops, uint64_t ops_cap,
                                uint64_t* offs, uint32_t* best, uint32_t* n_hits, uint64_t* counters) {
    if (!r) return failWith(CMB_ERR_INVALID, "null argument");
    const bool lists = occ || aln || cigar_ops; // (a device-resident result downloads its lists only when they are asked for)
    try {
        if (lists) fetchBest(const_cast<cmb_best*>(r));
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
    if ((lists || !r->onDevice) && (cap < r->occ.size() || ops_cap < r->ops.size())) return failWith(CMB_ERR_OVERFLOW, "output buffer too small");
    if (occ && !r->occ.empty()) memcpy(occ, r->occ.data(), r->occ.size() * sizeof(cmb_occ));
    if (aln && !r->aln.empty()) memcpy(aln, r->aln.data(), r->aln.size() * sizeof(cmb_aln));
    if (cigar_ops && !r->ops.empty()) memcpy(cigar_ops, r->ops.data(), r->ops.size() * sizeof(uint16_t));
    if (offs) memcpy(offs, r->offs.data(), r->offs.size() * sizeof(uint64_t));
    if (best) memcpy(best, r->best.data(), r->best.size() * sizeof(uint32_t));
    if (n_hits) memcpy(n_hits, r->nHits.data(), r->nHits.size() * sizeof(uint32_t));
    if (counters) memcpy(counters, r->cnts, sizeof(r->cnts));
    return CMB_OK;
}
extern "C" int cmb_best_timings(const cmb_best* r, const char** names, float* ms, uint32_t cap) {
    if (!r) return 0;
    uint32_t n = 0;
    for (const auto& t : r->times) {
        if (n >= cap) break;
        if (names) names[n] = t.first.c_str();
        if (ms) ms[n] = (float)t.second;
        n++;
    }
    return (int)n;
}
extern "C" int cmb_best_host_reads(const cmb_best* r, uint8_t* status, uint32_t* n) {
    if (!r) return failWith(CMB_ERR_INVALID, "null argument");
    if (status)
        for (size_t i = 0; i < r->offs.size() - 1; i++) status[i] = i < r->hostRead.size() ? r->hostRead[i] : 0;
    if (n) *n = r->nHostReads;
    return CMB_OK;
}
extern "C" void cmb_best_destroy(cmb_best* r) { delete r; }
