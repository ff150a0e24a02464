// BEST (+x strata) mode, the host side, once: the rule that decides which distance a read looks at next (findBestAlignments,
// reference src/searchstrategy.cpp:623-712), the loop that walks a chunk of reads through their strata as batches, and the containers
// of the reads whose occurrences live in host vectors (checkAlignments :536-568, combineOccVectors :570-621).  Plain C++17: no HIP, no
// batch; best.hip puts a host store and a device store under the loop, pair_best.hip steps the rule for one read.
#pragma once
#include "../../include/columba_amd.h"

#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace cmb {

// ---- the rule -----------------------------------------------------------------------------------------------------------------------
// Where one read stands.  proc: the distances below it have been searched (a stratum searches both strands and everything from the
// first distance not searched yet up to k, processSeq :777-811, so what has been searched is always a prefix).  A byte each: distances
// end at 13 (MAX_K), and a chunk keeps 10^6 cursors that the loop and the stores pass over several times.
struct BestCursor {
    uint8_t cutOff = 0, best = 0, k = 0, prevK = 0, maxED = 0, proc = 0;
    bool bestFound = false, finished = false;
};

// getMaxSupportedDistanceForBestMapping (searchstrategy.h:1864, :2744): the largest k such that 1..k all have a scheme, up to `cap`
template <class Schemes> inline uint32_t bestMaxSupported(const Schemes& schemes, uint32_t cap) {
    uint32_t k = 0;
    while (k < cap && schemes.count(k + 1) && !schemes.at(k + 1).empty()) k++;
    return k;
}
// getMaxED (searchstrategy.h:1797): the cut-off of a read from its length and the minimal identity (13: MAX_K, definitions.h:50)
inline uint32_t bestMaxED(uint32_t maxSupported, uint32_t len, uint32_t minIdentity) {
    return std::min<uint32_t>(std::min<uint32_t>(13u, maxSupported), (len * (100 - minIdentity)) / 100);
}
inline BestCursor bestCursor(uint32_t cutOff) { // (:628-630); cutOff: bestMaxED's, at most 13
    BestCursor c;
    c.cutOff = (uint8_t)cutOff, c.best = (uint8_t)(cutOff + 1);
    return c;
}
// the exact stratum (x == 0) has been checked: the first stratum to look at (:657-665, :676)
inline void bestAfterExact(BestCursor& c, uint32_t x) {
    const uint8_t x8 = (uint8_t)std::min(x, 255u); // (any x beyond the cut-off starts above it: the read is finished)
    if (c.best == 0) c.bestFound = true;
    c.maxED = c.best == 0 ? x8 : c.cutOff;
    c.prevK = 0;
    c.k = std::max<uint8_t>(x8, 1);
    c.finished = c.k > c.maxED;
}
// the strata that stratum k sends through checkAlignments (:686): check(l) may lower c.best, which the bound follows
template <class Check> inline void bestSweep(const BestCursor& c, uint32_t k, uint32_t x, Check&& check) {
    for (uint32_t l = c.prevK + 1u; l <= std::min(k, c.best + x); l++) check(l);
}
// stratum k has answered (update: hasUpdate :668-681) and been swept: finished, or the next k (:691-708)
inline void bestAdvance(BestCursor& c, uint32_t k, bool update, uint32_t x) {
    if (c.bestFound) { // this was the last iteration
        c.finished = true;
    } else if (update && c.best <= c.cutOff) {
        c.bestFound = true;
        c.finished = x == 0;
        c.prevK = (uint8_t)k;
        c.k = (uint8_t)std::min<uint32_t>(c.best + x, c.maxED); // check the final x strata
    } else if (k == c.maxED) {
        c.finished = true;
    } else {
        c.prevK = (uint8_t)k;
        c.k = (uint8_t)std::min<uint32_t>(k + x + (k < 5 ? 2u : 4u), c.maxED);
    }
}

// ---- the strata loop ----------------------------------------------------------------------------------------------------------------
// The reference walks one read at a time; here a stratum is one batch over all reads that look at the same distance.  The store holds
// the occurrences, however it likes:
//   BestCursor& cursor(i)                    read i's cursor
//   bool nonEmpty(i, strand, d)              does read i hold an occurrence of that strand at distance d
//   void check(i, strand, l, cutOffTrim)     checkAlignments on stratum l; lowers cursor(i).best when an occurrence stays
//   int run(ids, k)                          search those reads at distance k and keep what lies at min(proc, k) .. k; 0 or an error code
template <class Store> int bestStrataLoop(Store& S, uint32_t nReads, uint32_t x) {
    std::vector<uint32_t> need(nReads);
    if (x == 0 && nReads) { // exact matches first (:636-661)
        for (uint32_t i = 0; i < nReads; i++) need[i] = i;
        if (const int rc = S.run(need, 0)) return rc;
        for (uint32_t i = 0; i < nReads; i++) {
            BestCursor& c = S.cursor(i);
            c.proc = 1;
            if (S.nonEmpty(i, 0, 0) || S.nonEmpty(i, 1, 0)) {
                S.check(i, 0, 0, c.cutOff);
                S.check(i, 1, 0, c.cutOff);
            }
        }
    }
    std::vector<uint32_t> active; // the reads that are not finished, in ascending order
    for (uint32_t i = 0; i < nReads; i++) {
        bestAfterExact(S.cursor(i), x);
        if (!S.cursor(i).finished) active.push_back(i);
    }
    std::vector<uint8_t> isFresh(nReads, 0);
    while (!active.empty()) {
        // the reads that look at a stratum now, grouped by its distance
        std::map<uint32_t, std::vector<uint32_t>> byK;
        for (uint32_t i : active) byK[S.cursor(i).k].push_back(i);
        for (const auto& kv : byK) {
            const uint32_t k = kv.first;
            need.clear(); // (a stratum that has been searched needs no new search: the final x strata after a late find)
            for (uint32_t i : kv.second)
                if ((isFresh[i] = S.cursor(i).proc <= k)) need.push_back(i);
            if (!need.empty()) {
                if (const int rc = S.run(need, k)) return rc;
                for (uint32_t i : need) S.cursor(i).proc = (uint8_t)(k + 1);
            }
            for (uint32_t i : kv.second) {
                BestCursor& c = S.cursor(i);
                // hasUpdate: a stratum looked at before answers with ITS occurrences only; a new one (processSeq) with any
                // occurrence at distance 0..k.  (Here a read returns to a searched stratum only once its best is found, with k below
                // prevK: the sweep is empty and the read finishes whatever the answer.  The reference's form is kept because the
                // pairing's strata are filled by other walks too, where the difference shows.)
                bool update = false;
                for (int s = 0; s < 2; s++)
                    for (uint32_t d = isFresh[i] ? 0 : k; d <= k; d++) update |= S.nonEmpty(i, s, d);
                if (update)
                    bestSweep(c, k, x, [&](uint32_t l) {
                        S.check(i, 0, l, c.maxED);
                        S.check(i, 1, l, c.maxED);
                    });
                bestAdvance(c, k, update, x);
            }
        }
        active.erase(std::remove_if(active.begin(), active.end(), [&](uint32_t i) { return S.cursor(i).finished; }), active.end());
    }
    return 0;
}

// the reads of one stratum, one after the other, as a batch takes them
inline void bestGatherReads(const char* seqs, const uint64_t* offs, const std::vector<uint32_t>& ids, std::string& cat, std::vector<uint64_t>& o) {
    cat.clear();
    o.assign(ids.size() + 1, 0);
    for (size_t j = 0; j < ids.size(); j++) {
        cat.append(seqs + offs[ids[j]], seqs + offs[ids[j] + 1]);
        o[j + 1] = cat.size();
    }
}

// ---- a read whose occurrences live on the host ----------------------------------------------------------------------------------------
struct BestOcc {
    cmb_occ occ;
    cmb_aln aln; // spans: 0 inside one sequence, 1 over a sequence end, 2 found with trimming, 3 assigned (checkAlignments has seen it)
    std::vector<uint16_t> ops;
};
struct BestHostRead {
    std::vector<std::vector<BestOcc>> ov[2]; // [strand][distance 0 .. cut-off]
    std::string fw, rc;                      // the cleaned read and its reverse complement (trimming verifies against them)
    void start(uint32_t cutOff) {
        for (int s = 0; s < 2; s++) ov[s].assign((size_t)cutOff + 1, {});
    }
    void add(BestOcc&& o) {
        if (o.occ.distance < ov[0].size()) ov[o.occ.strand ? 1 : 0][o.occ.distance].push_back(std::move(o));
    }
    bool nonEmpty(int s, uint32_t d) const { return !ov[s][d].empty(); }
    uint32_t hitsAt(uint32_t d) const { return (uint32_t)(ov[0][d].size() + ov[1][d].size()); }
};
// checkAlignments (:536-568): keep what lies inside one sequence; trim(sequence, occurrence, cutOffTrim) is findSeqName on an occurrence
// that runs over a sequence end — true: found, at the distance it has now, and it moves to that stratum
template <class Trim> void bestCheckHost(BestHostRead& h, uint8_t& best, int s, uint32_t l, uint32_t cutOffTrim, Trim&& trim) {
    if (l >= h.ov[s].size()) return;
    std::vector<BestOcc> assigned, trimmed;
    for (BestOcc& o : h.ov[s][l]) {
        if (o.aln.spans == 0 || o.aln.spans == 3) { // FOUND
            o.aln.spans = 3;
            assigned.push_back(std::move(o));
            if (l < best) best = (uint8_t)l;
        } else if (o.aln.spans == 1) {
            if (trim(s ? h.rc : h.fw, o, cutOffTrim) && o.occ.distance > l && o.occ.distance < h.ov[s].size()) trimmed.push_back(std::move(o));
        }
    }
    h.ov[s][l] = std::move(assigned);
    for (BestOcc& o : trimmed) {
        o.aln.spans = 3; // (removeTrimmingLabel: it is an ordinary assigned occurrence of its new stratum)
        const uint32_t d = o.occ.distance;
        h.ov[s][d].push_back(std::move(o));
    }
}
// combineOccVectors (:570-621): strata best .. hi, forward before reverse complement, ordered by (sequence, begin), one record per place
template <class Emit> void bestCombineHost(BestHostRead& h, uint32_t best, uint32_t hi, Emit&& emit) {
    for (uint32_t d = best; d <= hi; d++)
        for (int s = 0; s < 2; s++) {
            std::vector<BestOcc>& v = h.ov[s][d];
            std::stable_sort(v.begin(), v.end(), [](const BestOcc& a, const BestOcc& b) {
                return a.aln.seq_id < b.aln.seq_id || (a.aln.seq_id == b.aln.seq_id && a.aln.seq_begin < b.aln.seq_begin);
            });
            v.erase(std::unique(v.begin(), v.end(), [](const BestOcc& a, const BestOcc& b) {
                        return a.aln.seq_id == b.aln.seq_id && a.aln.seq_begin == b.aln.seq_begin;
                    }), v.end());
            for (BestOcc& o : v) emit(o);
        }
}

} // namespace cmb
