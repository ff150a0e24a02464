// SAM text (include/columba_amd.h): the host-only record builders, the text of a chunk formatted on the host, and the device driver
// (dev_sam.hpp, dev_pair.hpp) for single-end chunks of either backend, read pairs in ALL mode and device-resident BEST results.  Of a
// batch this unit sees its list views (units.hpp) and nothing else; the fine-grained hooks it needs are called through the C-ABI.
#include "units.hpp"
#include "dev_sam.hpp"
#include "dev_pair.hpp"

#include <array>
#include <chrono>

using namespace cmb;

// ------------------------------------------------------------------------- output records (host-only)
static int64_t putString(const std::string& s, char* out, uint64_t cap) {
    if (out && cap > s.size()) memcpy(out, s.c_str(), s.size() + 1);
    return (int64_t)s.size();
}
static SamHit toHit(const cmb_sam_hit& h) {
    SamHit r;
    r.seqName = h.seq_name ? h.seq_name : "*";
    r.cigar = cigarString(h.cigar_ops, h.n_ops);
    r.pos0 = h.pos0;
    r.distance = h.distance;
    r.revCompl = h.revcomp != 0;
    return r;
}
extern "C" int64_t cmb_sam_se(const char* read_id, const cmb_sam_hit* hit, int primary, uint32_t n_hits, uint32_t min_score,
                              const char* print_seq, const char* print_qual, char* out, uint64_t cap) {
    if (!read_id || !hit || !print_seq || !print_qual) return failWith(CMB_ERR_INVALID, "null argument");
    return putString(samLineSE(read_id, toHit(*hit), primary != 0, n_hits, min_score, print_seq, print_qual), out, cap);
}
extern "C" int64_t cmb_sam_se_xa(const char* read_id, const cmb_sam_hit* hits, uint32_t n, uint32_t n_hits, const char* print_seq,
                                 const char* print_qual, char* out, uint64_t cap) {
    if (!read_id || !hits || n == 0 || !print_seq || !print_qual) return failWith(CMB_ERR_INVALID, "null argument");
    std::vector<SamHit> v;
    for (uint32_t i = 0; i < n; i++) v.push_back(toHit(hits[i]));
    return putString(samLineSEWithXA(read_id, v, n_hits, print_seq, print_qual), out, cap);
}
extern "C" int64_t cmb_sam_unmapped_se(const char* read_id, const char* seq, const char* qual, char* out, uint64_t cap) {
    if (!read_id || !seq || !qual) return failWith(CMB_ERR_INVALID, "null argument");
    return putString(samLineUnmappedSE(read_id, seq, qual), out, cap);
}
extern "C" int cmb_read_prepare(const char* id, const char* seq, const char* qual, char* id_out, char* seq_out, char* revcomp_out,
                                char* revqual_out) {
    if (!id || !seq) return failWith(CMB_ERR_INVALID, "null argument");
    const std::string cid = cleanSeqID(id), cs = cleanReadSeq(seq), rc = revComplWithN(cs);
    std::string rq = qual ? qual : "";
    std::reverse(rq.begin(), rq.end());
    if (id_out) memcpy(id_out, cid.c_str(), cid.size() + 1);
    if (seq_out) memcpy(seq_out, cs.c_str(), cs.size() + 1);
    if (revcomp_out) memcpy(revcomp_out, rc.c_str(), rc.size() + 1);
    if (revqual_out) memcpy(revqual_out, rq.c_str(), rq.size() + 1);
    return CMB_OK;
}

// (declared in units.hpp: best.hip trims the occurrences of its host reads with it)
bool cmb::trimOccurrence(cmb_index* idx, const std::string& seq, uint32_t largestStratum, int metric, BestOcc& o, uint64_t* counters) {
    if (metric == CMB_METRIC_HAMMING) return false;
    const std::vector<uint32_t>& sp = seqStartsOfIndex(idx);
    const uint32_t index = o.aln.seq_id;
    if (sp.size() < 2 || index + 1 >= sp.size()) return false;
    uint32_t b = o.occ.begin, e = o.occ.end, seqId = index;
    if (sp[index + 1] - b <= largestStratum) { // option 1: begin is just before the end of the sequence
        seqId = index + 1;
        if (seqId + 1 >= sp.size()) return false;
        b = sp[seqId];
        e = std::min(e, sp[seqId + 1]);
    } else if (e - sp[index + 1] <= largestStratum) { // option 2: end is just over the start of the next sequence
        e = sp[index + 1];
    } else {
        return false;
    }
    if (e <= b) return false;
    cmb_occ res[64];
    uint64_t n = 0, cnt[CMB_CNT_MAX];
    if (cmb_verify_window(idx, seq.data(), (uint32_t)seq.size(), b, e, largestStratum, 0, res, 64, &n, cnt) != CMB_OK) return false;
    for (int i = 0; counters && i < CMB_CNT_MAX; i++) counters[i] += cnt[i];
    if (n == 0) return false;
    // the minimal occurrence under TextOcc::operator< (begin, distance, width; indexhelpers.h:779-795)
    const cmb_occ* bestO = &res[0];
    for (uint64_t i = 1; i < n; i++) {
        const cmb_occ& c = res[i];
        const uint32_t wc = c.end - c.begin, wb = bestO->end - bestO->begin;
        if (c.begin != bestO->begin ? c.begin < bestO->begin
                                    : c.distance != bestO->distance ? c.distance < bestO->distance : wc < wb)
            bestO = &c;
    }
    o.occ.begin = bestO->begin;
    o.occ.end = bestO->end;
    o.occ.distance = bestO->distance;
    o.aln.seq_id = seqId;
    o.aln.seq_begin = bestO->begin - sp[seqId];
    o.aln.spans = 2; // found with trimming
    uint16_t opsBuf[2 * 13 + 3];
    uint32_t nOps = 0;
    o.ops.clear();
    if (cmb_cigar_windows(idx, seq.data(), (uint32_t)seq.size(), &o.occ.begin, &o.occ.end, &o.occ.distance, 1, opsBuf, 2 * 13 + 3,
                          &nOps) != CMB_OK)
        return false;
    o.ops.assign(opsBuf, opsBuf + nOps);
    return true;
}

// IndexInterface::findSeqName for ONE occurrence that runs over the end of its sequence (cmb_aln.spans == 1), for host layers
// that build their own records (paired reads): FOUND_WITH_TRIMMING -> *found = 1 and occ / aln / CIGAR updated; NOT_FOUND -> 0.
extern "C" int cmb_trim_occurrence(cmb_index* idx, const char* pattern, uint32_t plen, uint32_t largest_stratum, int metric, cmb_occ* occ,
                                   cmb_aln* aln, uint16_t* cigar_ops, uint32_t ops_cap, uint32_t* n_ops, int* found) {
    if (!idx || !pattern || !occ || !aln || !found) return failWith(CMB_ERR_INVALID, "null argument");
    try {
        BestOcc o;
        o.occ = *occ;
        o.aln = *aln;
        const bool ok = trimOccurrence(idx, std::string(pattern, plen), largest_stratum, metric, o, nullptr);
        *found = ok ? 1 : 0;
        if (ok) {
            if (o.ops.size() > ops_cap) return failWith(CMB_ERR_OVERFLOW, "room for the CIGAR operations of the trimmed occurrence");
            *occ = o.occ;
            *aln = o.aln;
            aln->cigar_len = (uint16_t)o.ops.size();
            for (size_t i = 0; i < o.ops.size() && cigar_ops; i++) cigar_ops[i] = o.ops[i];
            if (n_ops) *n_ops = (uint32_t)o.ops.size();
        }
        return CMB_OK;
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}

// SAM text of a whole chunk in ALL mode: matchApproxAllMap D) -> SearchStrategy::generateOutputSingleEnd
// (searchstrategy.cpp:530-533, :1824-1902) -> generateSE_SAM / generateSE_SAM_XATag (searchstrategy.h:1612-1641), from the
// occurrences, CIGARs and sequence assignments the device produced (cmb_batch_want_alignments before cmb_batch_run).
// Occurrences that run over the end of their sequence are trimmed and verified again (findSeqName,
// indexinterface.cpp:833-899) through the device hooks.
static SamHit samHitOf(const BestOcc& o, const std::string& seqName) { // an occurrence as the record builders take it
    SamHit h;
    h.seqName = seqName, h.cigar = cigarString(o.ops.data(), (uint32_t)o.ops.size());
    h.pos0 = o.aln.seq_begin, h.distance = o.occ.distance, h.revCompl = o.occ.strand != 0;
    return h;
}
// the SAM records of one read from its occurrences with alignments (generateOutputSingleEnd, searchstrategy.cpp:1824-1902)
static void samOfRead(std::string& text, cmb_index* idx, uint32_t k, int metric, const std::string& read, const std::string& revC,
                      const std::string& sid, const std::string& qual, std::vector<BestOcc>& occs, const char* const* seq_names,
                      int unmapped_records, int xa_tag) {
    std::string revQ = qual;
    std::reverse(revQ.begin(), revQ.end());
    std::vector<SamHit> hits;
    for (BestOcc& o : occs) {
        if (o.aln.spans == CMB_SPANS_DROPPED) continue; // NOT_FOUND, decided by the run (cmb_batch_trim_on_device)
        if (o.aln.spans == 1 && !trimOccurrence(idx, o.occ.strand ? revC : read, k, metric, o, nullptr)) continue; // NOT_FOUND
        hits.push_back(samHitOf(o, seq_names[o.aln.seq_id]));
    }
    if (hits.empty()) {
        if (unmapped_records) text += samLineUnmappedSE(sid, read, qual);
        return;
    }
    // primary = the first occurrence of minimal distance, swapped to the front (:1883-1899)
    size_t mi = 0;
    for (size_t j = 1; j < hits.size(); j++)
        if (hits[j].distance < hits[mi].distance) mi = j;
    const uint32_t minScore = hits[mi].distance;
    uint32_t nHits = 0;
    for (const SamHit& h : hits) nHits += h.distance == minScore;
    if (mi != 0) std::swap(hits[0], hits[mi]);
    const bool rcFirst = hits[0].revCompl;
    if (xa_tag) {
        text += samLineSEWithXA(sid, hits, nHits, rcFirst ? revC : read, rcFirst ? revQ : qual);
    } else {
        text += samLineSE(sid, hits[0], true, nHits, minScore, rcFirst ? revC : read, rcFirst ? revQ : qual);
        for (size_t j = 1; j < hits.size(); j++) text += samLineSE(sid, hits[j], false, nHits, minScore, "*", "*");
    }
}

// the occurrences of read i of a part with their alignments, as the run left them on the host (a b-move text lies below 2^32 characters
// when it has alignments: cmb_move_attach_text)
static std::vector<BestOcc> occsOfViewRead(const ListView& v, uint32_t i) {
    std::vector<BestOcc> occs;
    const size_t g = v.hOffsPerGroup ? v.groupStride : 1u;
    for (uint64_t q = v.hOccOffs[g * i]; q < v.hOccOffs[g * i + g]; q++) {
        const uint8_t* rec = (const uint8_t*)v.hOcc + q * v.hOccBytes;
        const cmb_occ* o = (const cmb_occ*)rec;
        const cmb_move_occ* m = (const cmb_move_occ*)rec;
        const uint4 o4 = v.hOccBytes == sizeof(cmb_occ) ? make_uint4(o->begin, o->end, o->distance, o->strand)
                                                        : make_uint4((uint32_t)m->begin, (uint32_t)m->end, m->distance, m->strand);
        occs.push_back(bestOccOf(o4, v.hAln[q], v.hOps + q * v.stride)); // (a stride is 2 k + 3 <= BEST_OPS_STRIDE)
    }
    return occs;
}

extern "C" int64_t cmb_batch_sam(const cmb_batch* b, const char* seqs, const char* const* read_ids, const char* const* quals,
                                 const char* const* seq_names, int unmapped_records, int xa_tag, char* out, uint64_t cap) {
    if (!b || !seqs || !read_ids || !seq_names) return failWith(CMB_ERR_INVALID, "null argument");
    try {
        std::vector<ListView> views;
        // (a view also hands out the part's driver buffers, so batchListViews takes a mutable batch; here only its host copies are read)
        if (int rc = batchListViews(const_cast<cmb_batch*>(b), false, views)) return rc;
        std::string text;
        uint64_t readBase = 0, charBase = 0;
        for (const ListView& c : views) {
            for (uint32_t i = 0; i < c.nReads; i++) {
                const uint64_t gi = readBase + i;
                const uint64_t o0 = charBase + c.hostOffs[i], o1 = charBase + c.hostOffs[i + 1];
                const std::string read = cleanReadSeq(std::string(seqs + o0, seqs + o1)), revC = revComplWithN(read);
                const std::string sid = cleanSeqID(read_ids[gi]);
                const std::string qual = quals && quals[gi] ? quals[gi] : "*";
                std::vector<BestOcc> occs = occsOfViewRead(c, i);
                samOfRead(text, c.textIndex, c.k, c.metric, read, revC, sid, qual, occs, seq_names, unmapped_records, xa_tag);
            }
            readBase += c.nReads;
            charBase += c.hostOffs[c.nReads];
        }
        return putString(text, out, cap);
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}

// The same text written on the device (dev_sam.hpp): plan -> lengths of the host-formatted reads -> scan -> write, every sub-batch on
// its own stream, the finished text in one page-locked buffer of the batch.  Reads with an occurrence that runs over the end of its
// sequence (AlnRec::spans == 1) go through samOfRead on the host — findSeqName trims them and may drop them — and their bytes are
// copied into place by the write kernel; nothing else is formatted on the host.
// The driver's steps, shared with cmb_best_sam_device; every one works on the stream it is given.
// 1. The slice [r0, r0 + n) of the packed inputs goes up, the plan's arrays are sized and the length behind the last read is cleared;
//    cx gets the input fields of the context (the packed bytes stay where they are: idBase / qualBase are subtracted on the device).
static int samUpload(SamDeviceBufs& d, const cmb_sam_inputs* in, uint64_t r0, uint32_t n, hipStream_t s, SamCtx& cx) {
    const size_t offBytes = ((size_t)n + 1) * sizeof(uint64_t);
    const uint64_t idLo = in->id_offs[r0], idHi = in->id_offs[r0 + n];
    if (idHi < idLo) return failWith(CMB_ERR_INVALID, "identifier offsets must be non-decreasing");
    growTo(d.ids, idHi - idLo + 1); // (+ 1: the cleaned identifier starts at byte 1, also of an empty line)
    growTo(d.idOffs, (size_t)n + 1);
    if (idHi > idLo) HIPCHK(hipMemcpyAsync(d.ids.p, in->ids + idLo, idHi - idLo, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.idOffs.p, in->id_offs + r0, offBytes, hipMemcpyHostToDevice, s));
    uint64_t qLo = 0;
    if (in->quals) {
        qLo = in->qual_offs[r0];
        const uint64_t qHi = in->qual_offs[r0 + n];
        if (qHi < qLo) return failWith(CMB_ERR_INVALID, "quality offsets must be non-decreasing");
        growTo(d.quals, qHi - qLo);
        growTo(d.qualOffs, (size_t)n + 1);
        if (qHi > qLo) HIPCHK(hipMemcpyAsync(d.quals.p, in->quals + qLo, qHi - qLo, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.qualOffs.p, in->qual_offs + r0, offBytes, hipMemcpyHostToDevice, s));
    }
    const uint64_t nameBytes = in->n_seqs ? in->seq_name_offs[in->n_seqs] : 0;
    growTo(d.names, nameBytes);
    growTo(d.nameOffs, (size_t)in->n_seqs + 1);
    if (nameBytes) HIPCHK(hipMemcpyAsync(d.names.p, in->seq_names, nameBytes, hipMemcpyHostToDevice, s));
    if (in->n_seqs) HIPCHK(hipMemcpyAsync(d.nameOffs.p, in->seq_name_offs, ((size_t)in->n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    growTo(d.plan, n);
    growTo(d.len, (size_t)n + 1);
    growTo(d.offs, (size_t)n + 1);
    HIPCHK(hipMemsetAsync(d.len.p + n, 0, sizeof(uint64_t), s));
    cx.ids = d.ids.p, cx.idOffs = d.idOffs.p, cx.idBase = idLo;
    cx.quals = in->quals ? d.quals.p : nullptr, cx.qualOffs = d.qualOffs.p, cx.qualBase = qLo;
    cx.names = d.names.p, cx.nameOffs = d.nameOffs.p, cx.nSeqs = in->n_seqs, cx.nReads = n;
    return CMB_OK;
}
// 2. The reads of `list` (ascending) are formatted on the host — format(i, text) appends the records of read i — and spliced in: their
//    text goes up and k_sam_override puts their lengths over the plan's.  The stream must have been waited for if `list` came from it.
//    -> the bytes of the host's text; roomBehind: bytes the side buffer must hold behind them (the pairs of k_pair_class_write)
template <class F> static uint64_t samSplice(SamDeviceBufs& d, const std::vector<uint32_t>& list, hipStream_t s, F format, uint64_t roomBehind = 0) {
    std::string side;
    std::vector<uint64_t> sideOffs(list.size() + 1, 0);
    for (size_t q = 0; q < list.size(); q++) {
        format(list[q], side);
        sideOffs[q + 1] = side.size();
    }
    growTo(d.side, side.size() + roomBehind);
    growTo(d.sideOffs, sideOffs.size());
    growTo(d.sideReads, list.size());
    if (!side.empty()) HIPCHK(hipMemcpy(d.side.p, side.data(), side.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.sideOffs.p, sideOffs.data(), sideOffs.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.sideReads.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sam_override, dim3(((uint32_t)list.size() + 255u) / 256u), dim3(256), 0, s, d.sideReads.p, d.sideOffs.p, (uint32_t)list.size(),
                       d.plan.p, d.len.p);
    HIPCHK(hipGetLastError());
    return side.size();
}
// 3. The position of every read in the text; *total (the text's length) is valid once the stream has been waited for ...
static void samScan(SamDeviceBufs& d, DevBuf<uint8_t>& scanTmp, uint32_t n, uint64_t* total, hipStream_t s) {
    scanExclusive(scanTmp, d.len.p, d.offs.p, (size_t)n + 1, s);
    HIPCHK(hipMemcpyAsync(total, d.offs.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
}
//    ... and then the text is written and copied to dst (page-locked); the caller waits for the stream once more.
static void samWrite(SamDeviceBufs& d, const SamCtx& cx, uint64_t total, char* dst, hipStream_t s) {
    growTo(d.text, (size_t)total + 16);
    hipLaunchKernelGGL(k_sam_write, dim3((cx.nReads + SAM_READS_PER_WAVE - 1u) / SAM_READS_PER_WAVE), dim3(64), 0, s, cx, d.plan.p, d.offs.p, d.side.p,
                       d.text.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst, d.text.p, (size_t)total, hipMemcpyDeviceToHost, s));
}
// the sequence names of packed inputs as the host formatters take them
static std::vector<std::string> samNamesOf(const cmb_sam_inputs* in) {
    std::vector<std::string> names;
    for (uint32_t q = 0; q < in->n_seqs; q++) names.emplace_back(in->seq_names + in->seq_name_offs[q], in->seq_names + in->seq_name_offs[q + 1]);
    return names;
}

// the list fields of the context of one part
static SamCtx samCtxOf(const ListView& v) { return SamCtx{v.reads, v.offs, v.goffs, v.groupStride, v.occ, v.aln, v.ops, v.stride}; }
// ... of a part whose run dropped occurrences (AlnRec::spans == 4): the lists without those, in the part's driver buffers (k_sam_keep_*)
static void samKeepLists(const ListView& v, SamCtx& cx, hipStream_t s) {
    SamBufs& B = *v.bufs;
    const uint64_t nGroups = (uint64_t)v.nReads * v.groupStride;
    const uint64_t n = v.hOccOffs[nGroups]; // (a view of an FM-index batch: offsets per group)
    growTo(B.keepFlag, n + 1), growTo(B.keepPos, n + 1), growTo(B.keepOffs, nGroups + 1);
    growTo(B.keepOcc, n), growTo(B.keepAln, n), growTo(B.keepOps, n * v.stride);
    const bool verbose = getenv("CMB_VERBOSE") != nullptr;
    const dim3 perOcc(capBlocks((uint32_t)std::min<uint64_t>((n + 256) / 256, 4096))), perGroup(capBlocks((uint32_t)std::min<uint64_t>((nGroups + 256) / 256, 4096)));
    gridLine(verbose, "k_sam_keep_copy", n, 256ull * perOcc.x);
    gridLine(verbose, "k_sam_keep_offs", nGroups + 1, 256ull * perGroup.x);
    hipLaunchKernelGGL(k_sam_keep_flags, perOcc, dim3(256), 0, s, v.aln, n, B.keepFlag.p);
    scanExclusive(*v.scanTmp, B.keepFlag.p, B.keepPos.p, (size_t)n + 1, s);
    hipLaunchKernelGGL(k_sam_keep_copy, perOcc, dim3(256), 0, s, v.occ, v.aln, v.ops, v.stride, n, B.keepPos.p, B.keepOcc.p, B.keepAln.p, B.keepOps.p);
    hipLaunchKernelGGL(k_sam_keep_offs, perGroup, dim3(256), 0, s, v.goffs, nGroups, B.keepPos.p, B.keepOffs.p);
    HIPCHK(hipGetLastError());
    cx.foffs = B.keepOffs.p, cx.occ = B.keepOcc.p, cx.aln = B.keepAln.p, cx.ops = B.keepOps.p;
}
static bool samInputsOk(const cmb_sam_inputs* in) {
    return in && in->seqs && in->ids && in->id_offs && (!in->quals || in->qual_offs) && (!in->n_seqs || (in->seq_names && in->seq_name_offs));
}
// The driver over the parts of a chunk, whichever backend matched it: every part's lists in HBM, the buffers it keeps for the driver, and
// its occurrences on the host for the reads the host formats; the text and the sequence starts of the parts' index serve their trimming
static int samDeviceOver(const std::vector<ListView>& parts, const cmb_sam_inputs* in, int unmapped_records, int xa_tag, const char** text,
                         uint64_t* length, uint64_t* host_reads) {
    cmb_index* idx = parts[0].textIndex;
    useDeviceOf(idx);
    const size_t P = parts.size();
    const bool verbose = getenv("CMB_VERBOSE") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!verbose) return;
        auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[host] sam: %-28s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    };
    std::vector<uint64_t> readBase(P + 1, 0), charBase(P + 1, 0), partBytes(P, 0);
    std::vector<uint32_t> nHost(P, 0);
    std::vector<SamCtx> ctx(P);
    for (size_t j = 0; j < P; j++) {
        readBase[j + 1] = readBase[j] + parts[j].nReads;
        charBase[j + 1] = charBase[j] + (parts[j].nReads ? parts[j].hostOffs[parts[j].nReads] : 0);
    }
    // ---- plan: inputs up, one wavefront per read
    for (size_t j = 0; j < P; j++) {
        const ListView& c = parts[j];
        const uint32_t n = c.nReads;
        if (!n) continue;
        hipStream_t s = c.stream;
        SamCtx& cx = ctx[j] = samCtxOf(c);
        if (c.trimOnDevice && c.trimDropped) samKeepLists(c, cx, s);
        cx.unmapped = unmapped_records ? 1u : 0u, cx.xa = xa_tag ? 1u : 0u;
        if (int rc = samUpload(c.bufs->sam, in, readBase[j], n, s, cx)) return rc;
        growTo(c.bufs->hostList, (size_t)n + 1);
        HIPCHK(hipMemsetAsync(c.bufs->hostList.p, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_sam_plan, dim3((n + 3u) / 4u), dim3(256), 0, s, cx, c.bufs->sam.plan.p, c.bufs->sam.len.p, c.bufs->hostList.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&nHost[j], c.bufs->hostList.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    lap("inputs up, plan started");
    // ---- the reads the host formats (k_sam_plan listed them), then the position of every read in its sub-batch's text
    std::vector<std::string> names;
    std::vector<const char*> namePtrs;
    uint64_t nHostAll = 0;
    for (size_t j = 0; j < P; j++) {
        const ListView& c = parts[j];
        const uint32_t n = c.nReads;
        if (!n) continue;
        hipStream_t s = c.stream;
        HIPCHK(hipStreamSynchronize(s));
        if (nHost[j]) {
            if (names.empty()) names = samNamesOf(in);
            if (namePtrs.empty())
                for (const std::string& nm : names) namePtrs.push_back(nm.c_str());
            std::vector<uint32_t> list(nHost[j]);
            HIPCHK(hipMemcpy(list.data(), c.bufs->hostList.p + 1, (size_t)nHost[j] * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::sort(list.begin(), list.end());
            samSplice(c.bufs->sam, list, s, [&](uint32_t i, std::string& side) {
                const uint64_t gi = readBase[j] + i;
                const uint64_t o0 = charBase[j] + c.hostOffs[i], o1 = charBase[j] + c.hostOffs[i + 1];
                const std::string read = cleanReadSeq(std::string(in->seqs + o0, in->seqs + o1)), revC = revComplWithN(read);
                const std::string sid = cleanSeqID(std::string(in->ids + in->id_offs[gi], in->ids + in->id_offs[gi + 1]));
                const std::string qual = in->quals ? std::string(in->quals + in->qual_offs[gi], in->quals + in->qual_offs[gi + 1]) : "*";
                std::vector<BestOcc> occs = occsOfViewRead(c, i);
                samOfRead(side, idx, c.k, c.metric, read, revC, sid, qual, occs, namePtrs.data(), unmapped_records, xa_tag);
            });
            nHostAll += nHost[j];
        }
        samScan(c.bufs->sam, *c.scanTmp, n, &partBytes[j], s);
    }
    uint64_t total = 0;
    for (size_t j = 0; j < P; j++) {
        if (parts[j].nReads) HIPCHK(hipStreamSynchronize(parts[j].stream));
        total += partBytes[j];
    }
    lap("plan, host reads, scan");
    // ---- write: every sub-batch its piece, copied to its place in the batch's text (page-locked, kept with the first part)
    PinnedBuf<char>& samOut = parts[0].bufs->samOut;
    samOut.resize((size_t)total + 1);
    samOut.p[total] = '\0';
    uint64_t at = 0;
    for (size_t j = 0; j < P; j++) {
        if (!parts[j].nReads || !partBytes[j]) continue;
        samWrite(parts[j].bufs->sam, ctx[j], partBytes[j], samOut.p + at, parts[j].stream);
        at += partBytes[j];
    }
    for (size_t j = 0; j < P; j++)
        if (parts[j].nReads && partBytes[j]) HIPCHK(hipStreamSynchronize(parts[j].stream));
    lap("write, text down");
    *text = samOut.p;
    *length = total;
    if (host_reads) *host_reads = nHostAll;
    return CMB_OK;
}

extern "C" int cmb_batch_sam_device(cmb_batch* b, const cmb_sam_inputs* in, int unmapped_records, int xa_tag, const char** text,
                                    uint64_t* length, uint64_t* host_reads) {
    if (!b || !text || !length || !samInputsOk(in)) return failWith(CMB_ERR_INVALID, "null argument");
    try {
        std::vector<ListView> views;
        if (int rc = batchListViews(b, false, views)) return rc;
        return samDeviceOver(views, in, unmapped_records, xa_tag, text, length, host_reads);
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}
// the same on a b-move batch whose final lists stayed in HBM (cmb_move_batch_keep_device_lists)
extern "C" int cmb_move_batch_sam_device(cmb_move_batch* b, const cmb_sam_inputs* in, int unmapped_records, int xa_tag, const char** text,
                                         uint64_t* length, uint64_t* host_reads) {
    if (!b || !text || !length || !samInputsOk(in)) return failWith(CMB_ERR_INVALID, "null argument");
    try {
        std::vector<ListView> views;
        if (int rc = moveBatchListViews(b, views)) return rc;
        if (!views[0].textIndex) return failWith(CMB_ERR_INVALID, "the batch's index has no text beside it (cmb_move_attach_text)");
        return samDeviceOver(views, in, unmapped_records, xa_tag, text, length, host_reads);
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}

// ---- read pairs in ALL mode: both mates' lists stay in HBM, the pairs are formed and their records written there (dev_pair.hpp).  The
// driver is the single-end one — inputs up (samUpload, once per mate), plan, the host's pairs spliced in (samSplice), scan (samScan),
// write — with sub-batch j of the two batches on the stream of read 1's.  A pair the device does not handle (an occurrence over the
// end of its sequence or without a sequence, or lists without a concordant pair) is formatted by cmb_pair_sam from the batches' host
// copies, trimmed as the host adapters do (cmb_trim_occurrence with edit distance).
namespace {
struct PairHostRead { // one mate as cmb_pair_sam takes it
    std::string id, seq, rc, qual, rq;
    std::vector<BestOcc> occs;
    std::vector<cmb_pair_occ> po;
    cmb_pair_read view() const { return cmb_pair_read{id.c_str(), seq.c_str(), rc.c_str(), qual.c_str(), rq.c_str(), po.data(), (uint32_t)po.size()}; }
};
void pairHostRead(PairHostRead& h, const ListView& c, uint32_t i, const cmb_sam_inputs* in, uint64_t gi, uint64_t charBase) {
    const uint64_t o0 = charBase + c.hostOffs[i], o1 = charBase + c.hostOffs[i + 1];
    h.seq = cleanReadSeq(std::string(in->seqs + o0, in->seqs + o1));
    h.rc = revComplWithN(h.seq);
    h.id = cleanSeqID(std::string(in->ids + in->id_offs[gi], in->ids + in->id_offs[gi + 1]));
    h.qual = in->quals ? std::string(in->quals + in->qual_offs[gi], in->quals + in->qual_offs[gi + 1]) : std::string();
    h.rq = h.qual;
    std::reverse(h.rq.begin(), h.rq.end());
    h.occs = occsOfViewRead(c, i);
    h.po.clear();
    for (BestOcc& o : h.occs) {
        if (o.aln.spans == 1 && !trimOccurrence(c.textIndex, o.occ.strand ? h.rc : h.seq, c.k, CMB_METRIC_EDIT, o, nullptr)) continue; // NOT_FOUND
        h.po.push_back(cmb_pair_occ{o.aln.seq_id, o.aln.seq_begin, o.aln.seq_begin + (o.occ.end - o.occ.begin), o.occ.begin, o.occ.distance,
                                    o.occ.strand, o.ops.data(), (uint32_t)o.ops.size()});
    }
}
// the argument checks of the pair drivers that need no batch
int pairArgsCheck(const void* mates1, const void* mates2, const cmb_pair_params* params, const cmb_sam_inputs* in1, const cmb_sam_inputs* in2,
                  uint32_t classes, const char** text, uint64_t* length) {
    if (!mates1 || !mates2 || !params || !text || !length || !samInputsOk(in1) || !samInputsOk(in2)) return failWith(CMB_ERR_INVALID, "null argument");
    if (mates1 == mates2) return failWith(CMB_ERR_INVALID, "the two mates need a batch each");
    if (params->orientation > 2) return failWith(CMB_ERR_INVALID, "orientation must be one of CMB_ORIENTATION_*");
    if (classes > CMB_PAIR_CLASS_ALL) return failWith(CMB_ERR_INVALID, "classes must be a combination of CMB_PAIR_CLASS_*");
    return CMB_OK;
}
// The driver over the parts of the two mates' batches, whichever backend matched them (subs1 / subs2: sub-batch j of the two).  classes:
// the CMB_PAIR_CLASS_* that k_pair_class_write formats; the pairs of the others go to the host
int pairDeviceOver(const std::vector<ListView>& subs1, const std::vector<ListView>& subs2, const cmb_pair_params* params, const cmb_sam_inputs* in1,
                   const cmb_sam_inputs* in2, uint32_t classes, const char** text, uint64_t* length, cmb_pair_class_stats* stats) {
    {
        for (const std::vector<ListView>* subs : {&subs1, &subs2})
            for (const ListView& v : *subs)
                if (v.trimOnDevice)
                    return failWith(CMB_ERR_INVALID, "a batch that trims on the device (cmb_batch_trim_on_device) cannot be paired: the pair drivers trim on the host");
        if (subs1[0].textIndex != subs2[0].textIndex || subs1[0].k != subs2[0].k || subs1[0].metric != subs2[0].metric)
            return failWith(CMB_ERR_INVALID, "the mates' batches differ in index, metric or maximal distance");
        uint64_t total1 = 0, total2 = 0;
        for (const ListView& v : subs1) total1 += v.nReads;
        for (const ListView& v : subs2) total2 += v.nReads;
        if (total1 != total2) return failWith(CMB_ERR_INVALID, "the mates' batches do not hold the same number of reads");
        if (subs1.size() != subs2.size()) return failWith(CMB_ERR_INVALID, "the mates' batches are split into different sub-batches");
        const size_t P = subs1.size();
        for (size_t j = 0; j < P; j++)
            if (subs1[j].nReads != subs2[j].nReads) return failWith(CMB_ERR_INVALID, "the mates' batches are split into different sub-batches");
        if (in1->n_seqs != in2->n_seqs) return failWith(CMB_ERR_INVALID, "the mates' inputs name different numbers of sequences");
        useDeviceOf(subs1[0].textIndex);
        const cmb_sam_inputs* in[2] = {in1, in2};
        std::vector<uint64_t> readBase(P + 1, 0), charBase1(P + 1, 0), charBase2(P + 1, 0), partBytes(P, 0), partRecords(P, 0), partMapped(P, 0);
        std::vector<uint32_t> nHost(P, 0), nCls(P, 0);
        std::vector<std::array<uint32_t, PAIR_CLS_COUNTERS>> clsCount(P);
        std::vector<PairCtx> ctx(P);
        for (size_t j = 0; j < P; j++) {
            const uint32_t n = subs1[j].nReads;
            readBase[j + 1] = readBase[j] + n;
            charBase1[j + 1] = charBase1[j] + (n ? subs1[j].hostOffs[n] : 0);
            charBase2[j + 1] = charBase2[j] + (n ? subs2[j].hostOffs[n] : 0);
        }
        // ---- plan: inputs of both mates up, one wavefront per pair
        for (size_t j = 0; j < P; j++) {
            const ListView* c[2] = {&subs1[j], &subs2[j]};
            const uint32_t n = c[0]->nReads;
            if (!n) continue;
            hipStream_t s = c[0]->stream;
            SamBufs& B = *c[0]->bufs;
            PairCtx& pc = ctx[j];
            pc.orientation = params->orientation, pc.maxFrag = params->max_frag, pc.minFrag = params->min_frag;
            for (int m = 0; m < 2; m++) {
                pc.m[m] = samCtxOf(*c[m]);
                if (int rc = samUpload(c[m]->bufs->sam, in[m], readBase[j], n, s, pc.m[m])) return rc;
            }
            growTo(B.pairPlan, n);
            growTo(B.pairRecords, (size_t)n + 1);
            growTo(B.pairMapped, (size_t)n + 1);
            growTo(B.pairSums, (size_t)n + 1);
            growTo(B.hostList, (size_t)n + 1);
            HIPCHK(hipMemsetAsync(B.hostList.p, 0, sizeof(uint32_t), s));
            HIPCHK(hipMemsetAsync(B.pairRecords.p + n, 0, sizeof(uint64_t), s));
            HIPCHK(hipMemsetAsync(B.pairMapped.p + n, 0, sizeof(uint32_t), s));
            growTo(B.clsList, (size_t)n + 1);
            growTo(B.clsLen, (size_t)n + 1);
            growTo(B.clsOffs, (size_t)n + 1);
            growTo(B.clsCount, PAIR_CLS_COUNTERS);
            HIPCHK(hipMemsetAsync(B.clsList.p, 0, sizeof(uint32_t), s));
            HIPCHK(hipMemsetAsync(B.clsLen.p + n, 0, sizeof(uint64_t), s));
            HIPCHK(hipMemsetAsync(B.clsCount.p, 0, PAIR_CLS_COUNTERS * sizeof(uint32_t), s));
            hipLaunchKernelGGL(k_pair_plan, dim3((n + 3u) / 4u), dim3(256), 0, s, pc, params->unmapped_records ? 1u : 0u, B.sam.plan.p,
                               B.pairPlan.p, B.sam.len.p, B.pairRecords.p, B.pairMapped.p, B.hostList.p, classes,
                               params->discordant_allowed ? 1u : 0u, B.clsList.p, B.clsLen.p, B.clsCount.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&nHost[j], B.hostList.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(&nCls[j], B.clsList.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(clsCount[j].data(), B.clsCount.p, PAIR_CLS_COUNTERS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        }
        // ---- the pairs the host formats, then the position of every pair in its sub-batch's text
        std::vector<std::string> names;
        std::vector<const char*> namePtrs;
        uint64_t nHostAll = 0, hostMapped = 0, clsAll[PAIR_CLS_COUNTERS] = {};
        for (size_t j = 0; j < P; j++) {
            const ListView* c[2] = {&subs1[j], &subs2[j]};
            const uint32_t n = c[0]->nReads;
            if (!n) continue;
            hipStream_t s = c[0]->stream;
            SamBufs& B = *c[0]->bufs;
            HIPCHK(hipStreamSynchronize(s));
            uint64_t clsBytes = 0, hostBytes = 0; // the side buffer: the host's text, then the text of k_pair_class_write's pairs
            if (nCls[j]) {
                scanExclusive(*c[0]->scanTmp, B.clsLen.p, B.clsOffs.p, (size_t)n + 1, s);
                HIPCHK(hipMemcpyAsync(&clsBytes, B.clsOffs.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (!nHost[j]) growTo(B.sam.side, (size_t)clsBytes + 16);
            }
            if (nHost[j]) {
                if (names.empty()) {
                    names = samNamesOf(in1);
                    for (const std::string& nm : names) namePtrs.push_back(nm.c_str());
                }
                std::vector<uint32_t> list(nHost[j]);
                HIPCHK(hipMemcpy(list.data(), B.hostList.p + 1, (size_t)nHost[j] * sizeof(uint32_t), hipMemcpyDeviceToHost));
                std::sort(list.begin(), list.end());
                PairHostRead h[2];
                std::vector<char> buf;
                hostBytes = samSplice(B.sam, list, s, [&](uint32_t i, std::string& side) {
                    pairHostRead(h[0], *c[0], i, in1, readBase[j] + i, charBase1[j]);
                    pairHostRead(h[1], *c[1], i, in2, readBase[j] + i, charBase2[j]);
                    const cmb_pair_read r1 = h[0].view(), r2 = h[1].view();
                    uint32_t nPairs = 0;
                    const int64_t len = cmb_pair_sam(params, &r1, &r2, namePtrs.data(), nullptr, 0, &nPairs);
                    if (len < 0) throw std::runtime_error(cmb_last_error());
                    buf.resize((size_t)len + 1);
                    cmb_pair_sam(params, &r1, &r2, namePtrs.data(), buf.data(), (uint64_t)len + 1, &nPairs);
                    side.append(buf.data(), (size_t)len);
                    hostMapped += nPairs > 0;
                }, clsBytes ? clsBytes + 16 : 0);
                nHostAll += nHost[j];
            }
            if (nCls[j]) {
                hipLaunchKernelGGL(k_pair_class_write, dim3(nCls[j]), dim3(64), 0, s, ctx[j], B.sam.plan.p, B.pairPlan.p, B.clsList.p, B.clsOffs.p,
                                   hostBytes, B.sam.side.p);
                HIPCHK(hipGetLastError());
            }
            for (uint32_t q = 0; q < PAIR_CLS_COUNTERS; q++) clsAll[q] += clsCount[j][q];
            samScan(B.sam, *c[0]->scanTmp, n, &partBytes[j], s);
            // the records the device writes and the pairs it maps: a 64-bit sum each, through the same scan buffer one after the other
            scanExclusive(*c[0]->scanTmp, B.pairRecords.p, B.pairSums.p, (size_t)n + 1, s);
            HIPCHK(hipMemcpyAsync(&partRecords[j], B.pairSums.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            scanExclusive(*c[0]->scanTmp, B.pairMapped.p, B.pairSums.p, (size_t)n + 1, s);
            HIPCHK(hipMemcpyAsync(&partMapped[j], B.pairSums.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        }
        uint64_t total = 0, deviceRecords = 0, deviceMapped = 0;
        for (size_t j = 0; j < P; j++) {
            if (subs1[j].nReads) HIPCHK(hipStreamSynchronize(subs1[j].stream));
            total += partBytes[j];
            deviceRecords += partRecords[j];
            deviceMapped += partMapped[j];
        }
        // ---- write: every sub-batch its piece, copied to its place in the text of read 1's batch
        PinnedBuf<char>& samOut = subs1[0].bufs->samOut;
        samOut.resize((size_t)total + 1);
        samOut.p[total] = '\0';
        uint64_t at = 0;
        for (size_t j = 0; j < P; j++) {
            const uint32_t n = subs1[j].nReads;
            if (!n || !partBytes[j]) continue;
            SamDeviceBufs& d = subs1[j].bufs->sam;
            hipStream_t s = subs1[j].stream;
            growTo(d.text, (size_t)partBytes[j] + 16);
            hipLaunchKernelGGL(k_pair_write, dim3((n + PAIR_PER_WAVE - 1u) / PAIR_PER_WAVE), dim3(64), 0, s, ctx[j], d.plan.p, subs1[j].bufs->pairPlan.p,
                               d.offs.p, d.side.p, d.text.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(samOut.p + at, d.text.p, (size_t)partBytes[j], hipMemcpyDeviceToHost, s));
            at += partBytes[j];
        }
        for (size_t j = 0; j < P; j++)
            if (subs1[j].nReads && partBytes[j]) HIPCHK(hipStreamSynchronize(subs1[j].stream));
        *text = samOut.p;
        *length = total;
        if (getenv("CMB_VERBOSE"))
            fprintf(stderr,
                    "[host] pair sam: %llu pairs, %llu of them formatted on the host, %llu records from the device; device pairs: %llu both "
                    "unmapped, %llu concordant, %llu one unmapped, %llu discordant, %llu unpaired, %llu over the limit (classes %u)\n",
                    (unsigned long long)readBase[P], (unsigned long long)nHostAll, (unsigned long long)deviceRecords,
                    (unsigned long long)clsAll[PAIR_CLS_BOTH_UNMAPPED], (unsigned long long)clsAll[PAIR_CLS_CONCORDANT],
                    (unsigned long long)clsAll[PAIR_CLS_ONE_UNMAPPED], (unsigned long long)clsAll[PAIR_CLS_DISCORDANT],
                    (unsigned long long)clsAll[PAIR_CLS_UNPAIRED], (unsigned long long)clsAll[PAIR_CLS_OVER_LIMIT], classes);
        if (stats) {
            stats->host_pairs = nHostAll;
            stats->mapped_pairs = hostMapped + deviceMapped;
            stats->device_records = deviceRecords;
            stats->both_unmapped = clsAll[PAIR_CLS_BOTH_UNMAPPED], stats->concordant = clsAll[PAIR_CLS_CONCORDANT];
            stats->one_unmapped = clsAll[PAIR_CLS_ONE_UNMAPPED], stats->discordant = clsAll[PAIR_CLS_DISCORDANT];
            stats->unpaired = clsAll[PAIR_CLS_UNPAIRED], stats->over_limit = clsAll[PAIR_CLS_OVER_LIMIT];
        }
        return CMB_OK;
    }
}
} // namespace

extern "C" int cmb_pair_sam_device_classes(cmb_batch* mates1, cmb_batch* mates2, const cmb_pair_params* params, const cmb_sam_inputs* in1,
                                           const cmb_sam_inputs* in2, uint32_t classes, const char** text, uint64_t* length,
                                           cmb_pair_class_stats* stats) {
    if (int rc = pairArgsCheck(mates1, mates2, params, in1, in2, classes, text, length)) return rc;
    try {
        std::vector<ListView> subs1, subs2; // (sub-batch j of the two batches)
        if (int rc = batchListViews(mates1, true, subs1)) return rc;
        if (int rc = batchListViews(mates2, true, subs2)) return rc;
        return pairDeviceOver(subs1, subs2, params, in1, in2, classes, text, length, stats);
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}
extern "C" int cmb_pair_sam_device(cmb_batch* mates1, cmb_batch* mates2, const cmb_pair_params* params, const cmb_sam_inputs* in1,
                                   const cmb_sam_inputs* in2, const char** text, uint64_t* length, cmb_pair_device_stats* stats) {
    cmb_pair_class_stats cs{};
    const int rc = cmb_pair_sam_device_classes(mates1, mates2, params, in1, in2, 0u, text, length, &cs);
    if (rc == CMB_OK && stats) stats->host_pairs = cs.host_pairs, stats->mapped_pairs = cs.mapped_pairs, stats->device_records = cs.device_records;
    return rc;
}
// the same on two b-move batches whose final lists stayed in HBM, every strand filtered by itself, on an index with its text beside it
extern "C" int cmb_move_pair_sam_device(cmb_move_batch* mates1, cmb_move_batch* mates2, const cmb_pair_params* params, const cmb_sam_inputs* in1,
                                        const cmb_sam_inputs* in2, uint32_t classes, const char** text, uint64_t* length,
                                        cmb_pair_class_stats* stats) {
    if (int rc = pairArgsCheck(mates1, mates2, params, in1, in2, classes, text, length)) return rc;
    try {
        std::vector<ListView> subs1, subs2;
        if (int rc = moveBatchListViews(mates1, subs1)) return rc;
        if (int rc = moveBatchListViews(mates2, subs2)) return rc;
        for (const std::vector<ListView>* subs : {&subs1, &subs2})
            for (const ListView& v : *subs) {
                if (!v.textIndex) return failWith(CMB_ERR_INVALID, "the batch's index has no text beside it (cmb_move_attach_text)");
                if (v.groupStride != 2u)
                    return failWith(CMB_ERR_INVALID, "the strands were not filtered each by itself (cmb_move_batch_filter_per_strand)");
            }
        return pairDeviceOver(subs1, subs2, params, in1, in2, classes, text, length, stats);
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}

// test hook: the MAPQ the device path prints for 1 ... n occurrences of minimal distance (dev_sam.hpp: samMapQ)
extern "C" int cmb_sam_device_mapq(uint32_t n, uint32_t* out) {
    if (!out && n) return failWith(CMB_ERR_INVALID, "null argument");
    try {
        if (!n) return CMB_OK;
        DevBuf<uint32_t> d;
        d.alloc(n);
        hipLaunchKernelGGL(k_sam_mapq, dim3((n + 255u) / 256u), dim3(256), 0, 0, n, d.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(out, d.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return CMB_OK;
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}

// The same for occurrences and alignments the caller holds (cmb_batch_results + cmb_batch_alignments, or their b-move
// counterparts with the text-only index of cmb_move_text_index): occ_offs[n_reads + 1], aln[i].cigar_off into cigar_ops.
extern "C" int64_t cmb_sam_chunk(cmb_index* idx, uint32_t max_distance, int metric, const char* seqs, const uint64_t* offs, uint32_t n_reads,
                                 const char* const* read_ids, const char* const* quals, const char* const* seq_names, const cmb_occ* occ,
                                 const uint64_t* occ_offs, const cmb_aln* aln, const uint16_t* cigar_ops, int unmapped_records, int xa_tag,
                                 char* out, uint64_t cap) {
    if (!idx || !seqs || !offs || !read_ids || !seq_names || !occ_offs || (occ_offs[n_reads] && (!occ || !aln || !cigar_ops)))
        return failWith(CMB_ERR_INVALID, "null argument");
    try {
        std::string text;
        for (uint32_t i = 0; i < n_reads; i++) {
            const std::string read = cleanReadSeq(std::string(seqs + offs[i], seqs + offs[i + 1])), revC = revComplWithN(read);
            const std::string sid = cleanSeqID(read_ids[i]);
            const std::string qual = quals && quals[i] ? quals[i] : "*";
            std::vector<BestOcc> occs;
            for (uint64_t q2 = occ_offs[i]; q2 < occ_offs[i + 1]; q2++) {
                BestOcc o;
                o.occ = occ[q2];
                o.aln = aln[q2];
                o.ops.assign(cigar_ops + aln[q2].cigar_off, cigar_ops + aln[q2].cigar_off + aln[q2].cigar_len);
                occs.push_back(std::move(o));
            }
            samOfRead(text, idx, max_distance, metric, read, revC, sid, qual, occs, seq_names, unmapped_records, xa_tag);
        }
        return putString(text, out, cap);
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}
// SAM text of a chunk from a device-resident BEST result, written on the device: the text samOfBest (include/columba_amd_best.hpp) puts
// together from cmb_best_results with the record builders, byte for byte.  The final lists have the layout k_sam_write reads, so only
// the plan differs (k_sam_plan_best); the reads whose bookkeeping went through the host are formatted by the record builders and
// spliced in as cmb_batch_sam_device does.
extern "C" int cmb_best_sam_device(cmb_best* r, const cmb_sam_inputs* in, int unmapped_records, int xa_tag, const char** text,
                                   uint64_t* length, uint64_t* host_reads) {
    if (!r || !in || !text || !length) return failWith(CMB_ERR_INVALID, "null argument");
    if (!r->onDevice) return failWith(CMB_ERR_INVALID, "the result does not live on the device (cmb_match_best_device)");
    const uint32_t n = r->nReads;
    if (!in->id_offs || (!in->seqs && n && r->readOffs[n]) || (!in->ids && in->id_offs[n]) || (in->quals && !in->qual_offs) ||
        (in->n_seqs && (!in->seq_names || !in->seq_name_offs)))
        return failWith(CMB_ERR_INVALID, "null argument");
    try {
        cmb_index* idx = r->ix;
        useDeviceOf(idx);
        *text = "";
        *length = 0;
        if (host_reads) *host_reads = r->nHostReads;
        if (!n) return CMB_OK;
        hipStream_t s = 0;
        if (!r->readsUp) { // the chunk's raw reads: once per handle
            const uint64_t chars = r->readOffs[n];
            growTo(r->samReads, chars + 1);
            growTo(r->samReadOffs, (size_t)n + 1);
            if (chars) HIPCHK(hipMemcpy(r->samReads.p, in->seqs, chars, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(r->samReadOffs.p, r->readOffs.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
            growTo(r->samHostFlag, n);
            HIPCHK(hipMemcpy(r->samHostFlag.p, r->hostRead.data(), n, hipMemcpyHostToDevice));
            r->readsUp = true;
        }
        SamCtx cx{r->samReads.p, r->samReadOffs.p, r->dOffs.p, 1u, r->dOcc.p, r->dAln.p, r->dOps.p, BEST_OPS_STRIDE};
        cx.unmapped = unmapped_records ? 1u : 0u, cx.xa = xa_tag ? 1u : 0u;
        if (int rc = samUpload(r->sam, in, 0, n, s, cx)) return rc;
        hipLaunchKernelGGL(k_sam_plan_best, dim3((n + 3u) / 4u), dim3(256), 0, s, cx, r->dBest.p, r->dHits.p, r->samHostFlag.p, r->sam.plan.p,
                           r->sam.len.p);
        HIPCHK(hipGetLastError());
        // ---- the host reads (known from the strata bookkeeping) through the record builders: samOfBest's lines
        if (r->nHostReads) {
            const std::vector<std::string> nameStr = samNamesOf(in);
            std::vector<uint32_t> list;
            for (uint32_t i = 0; i < n; i++)
                if (r->hostRead[i]) list.push_back(i);
            samSplice(r->sam, list, s, [&](uint32_t i, std::string& side) {
                const std::string read = cleanReadSeq(std::string(in->seqs + r->readOffs[i], in->seqs + r->readOffs[i + 1])), revC = revComplWithN(read);
                const std::string sid = cleanSeqID(std::string(in->ids + in->id_offs[i], in->ids + in->id_offs[i + 1]));
                const std::string qual = in->quals ? std::string(in->quals + in->qual_offs[i], in->quals + in->qual_offs[i + 1]) : "*";
                const uint64_t o0 = r->offs[i], cnt = r->offs[i + 1] - o0;
                if (!cnt) {
                    if (unmapped_records) side += samLineUnmappedSE(sid, read, qual);
                    return;
                }
                std::vector<uint4> oc(cnt);
                std::vector<AlnRec> al(cnt);
                std::vector<uint16_t> op(cnt * BEST_OPS_STRIDE);
                HIPCHK(hipMemcpy(oc.data(), r->dOcc.p + o0, cnt * sizeof(uint4), hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(al.data(), r->dAln.p + o0, cnt * sizeof(AlnRec), hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(op.data(), r->dOps.p + o0 * BEST_OPS_STRIDE, op.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
                std::vector<SamHit> hits;
                for (uint64_t t = 0; t < cnt; t++) {
                    const BestOcc bo = bestOccOf(oc[t], al[t], op.data() + t * BEST_OPS_STRIDE);
                    hits.push_back(samHitOf(bo, bo.aln.seq_id < nameStr.size() ? nameStr[bo.aln.seq_id] : std::string()));
                }
                std::string revQ = qual;
                std::reverse(revQ.begin(), revQ.end());
                const bool rcFirst = hits[0].revCompl;
                if (xa_tag) {
                    side += samLineSEWithXA(sid, hits, r->nHits[i], rcFirst ? revC : read, rcFirst ? revQ : qual);
                } else {
                    side += samLineSE(sid, hits[0], true, r->nHits[i], r->best[i], rcFirst ? revC : read, rcFirst ? revQ : qual);
                    for (size_t j = 1; j < hits.size(); j++) side += samLineSE(sid, hits[j], false, r->nHits[i], r->best[i], "*", "*");
                }
            });
        }
        uint64_t total = 0;
        samScan(r->sam, r->scanTmp, n, &total, s);
        HIPCHK(hipStreamSynchronize(s));
        r->samOut.resize((size_t)total + 1);
        r->samOut.p[total] = '\0';
        if (total) {
            samWrite(r->sam, cx, total, r->samOut.p, s);
            HIPCHK(hipStreamSynchronize(s));
        }
        *text = r->samOut.p;
        *length = total;
        return CMB_OK;
    } catch (const std::exception& e) {
        return failWith(CMB_ERR_DEVICE, e.what());
    }
}
