// Index construction on the device, for a host that links libcolumba_amd.so: the preprocessing and the file writer of
// include/columba_amd_build.hpp around the arrays of cmb_build_* (include/columba_amd.h) instead of the host's SA-IS and scalar loops.
// The files are the host builder's byte for byte (tests/test_gpu_cpp_device_builder.py, tests/test_gpu_cpp_device_move_builder.py): the
// Vanilla flavour with its 32-bit length_t (buildIndexDevice) and the run-length compressed flavour (buildMoveIndexDevice).
//   g++ -std=c++17 -O2 -DCOLUMBA_AMD_DEVICE_BUILD -I include examples/columba_build.cpp -o columba_build -L columba_amd -lcolumba_amd -lz
// Also here: an FMIndex or a BMove straight from FASTA files, with no index files in between (fmIndexFromFasta, bmoveFromFasta).
#pragma once
#include "columba_amd.h"
#include "columba_amd.hpp"
#include "columba_amd_bmove.hpp"
#include "columba_amd_build.hpp"

#include <memory>

namespace columba_amd {
namespace build {

// the producer writeIndexFiles asks (as HostArrays): every array comes from one cmb_build handle
class DeviceArrays {
  public:
    DeviceArrays(const std::string& text, int device) {
        if (cmb_build_create(text.data(), text.size(), device, &b) != CMB_OK) throw std::runtime_error(cmb_last_error());
        cmb_build_sizes z;
        cmb_build_sizes_of(b, &z);
        N = z.text_length + 1;
        bvF.resize(z.bv_words), bvR.resize(z.bv_words), cntF.resize(z.cnt_words), cntR.resize(z.cnt_words), bwt.resize(z.bwt_words);
        a.bv_fwd = bvF.data(), a.cnt_fwd = cntF.data(), a.bv_rev = bvR.data(), a.cnt_rev = cntR.data(), a.bwt_words = bwt.data();
        a.bv_cap = z.bv_words, a.cnt_cap = z.cnt_words, a.bwt_cap = z.bwt_words;
        check(cmb_build_bwt_arrays(b, &a, nullptr));
    }
    DeviceArrays(const DeviceArrays&) = delete;
    DeviceArrays& operator=(const DeviceArrays&) = delete;
    ~DeviceArrays() { cmb_build_destroy(b); }
    cmb_build* handle() const { return b; }
    std::vector<uint32_t> charCounts() const { return std::vector<uint32_t>(a.char_counts, a.char_counts + 256); }
    SparseSA sparse(uint32_t sf) {
        uint64_t nb = 0, nc = 0, ns = 0;
        check(cmb_build_sparse_sa_sizes(b, sf, &nb, &nc, &ns));
        SparseSA r;
        r.bv.resize(nb), r.counts.resize(nc), r.samples.resize(ns);
        check(cmb_build_sparse_sa(b, sf, r.bv.data(), nb, r.counts.data(), nc, r.samples.data(), ns, &ns));
        return r;
    }
    std::vector<uint64_t> bwtWords() { return std::move(bwt); }
    BwtBitvectors bitvectors(bool reversed) { // (each is asked for once)
        BwtBitvectors r;
        r.dollarPos = reversed ? a.dollar_pos_rev : a.dollar_pos_fwd;
        r.N = N;
        r.bv = std::move(reversed ? bvR : bvF);
        r.counts = std::move(reversed ? cntR : cntF);
        return r;
    }

  private:
    static void check(int rc) {
        if (rc != CMB_OK) throw std::runtime_error(cmb_last_error());
    }
    cmb_build* b = nullptr;
    cmb_build_arrays a{};
    uint64_t N = 0;
    std::vector<uint64_t> bvF, cntF, bvR, cntR, bwt;
};

// buildIndex with the arrays from the device: the same preprocessing, the same writer, the same files
inline void buildIndexDevice(const std::vector<std::string>& fastaFiles, const std::string& base, uint32_t sparseness = 4, uint32_t seedLength = 0,
                             bool allSparsenessFactors = false, int device = 0) {
    if (sparseness == 0 || (sparseness & (sparseness - 1)) != 0) throw std::runtime_error("the sparseness factor must be a power of two");
    const Text tx = preprocessFastaFiles(fastaFiles, seedLength);
    DeviceArrays arrays(tx.T, device);
    writeIndexFiles(tx, base, sparseness, allSparsenessFactors, arrays);
}

// FASTA files -> a resident FMIndex (FMIndex::FromText) and what the SAM header and the records need of the text: sequence names,
// positions, first sequence of every file (Text::T is released)
inline std::unique_ptr<FMIndex> fmIndexFromFasta(const std::vector<std::string>& fastaFiles, Text& tx, length_t inTextSwitch, int sa_sparse = 4,
                                                 length_t wordSize = 10, uint32_t seedLength = 0, int device = 0) {
    tx = preprocessFastaFiles(fastaFiles, seedLength);
    std::unique_ptr<FMIndex> ix(new FMIndex(FMIndex::FromText{}, tx.T, tx.positions, inTextSwitch, sa_sparse, wordSize, device));
    std::string().swap(tx.T);
    return ix;
}

// the producer writeMoveIndexFiles asks (as hostMoveParts): every part comes from one cmb_build handle (cmb_build_move_arrays)
inline MoveParts deviceMoveParts(const std::string& text, int device) {
    cmb_build* b = nullptr;
    if (cmb_build_create(text.data(), text.size(), device, &b) != CMB_OK) throw std::runtime_error(cmb_last_error());
    std::unique_ptr<cmb_build, void (*)(cmb_build*)> owner(b, cmb_build_destroy);
    auto check = [](int rc) {
        if (rc != CMB_OK) throw std::runtime_error(cmb_last_error());
    };
    cmb_build_move_sizes z;
    check(cmb_build_move_sizes_of(b, 64, &z));
    MoveParts p;
    p.lfbp.resize(z.lfbp_bytes), p.revLfbp.resize(z.rev_lfbp_bytes);
    for (auto* v : {&p.smpf, &p.smpl, &p.prdf, &p.ftr, &p.prdl, &p.ltr}) v->resize(z.runs);
    p.revSmpf.resize(z.rev_runs), p.revSmpl.resize(z.rev_runs), p.plcpPos.resize(z.n_plcp), p.plcpSum.resize(z.n_plcp);
    cmb_build_move_arrays_io io{};
    io.length_bits = 64;
    io.lfbp = p.lfbp.data(), io.rev_lfbp = p.revLfbp.data(), io.lfbp_cap = z.lfbp_bytes, io.rev_lfbp_cap = z.rev_lfbp_bytes;
    io.samples_first = p.smpf.data(), io.samples_last = p.smpl.data(), io.pred_first = p.prdf.data(), io.first_to_run = p.ftr.data();
    io.pred_last = p.prdl.data(), io.last_to_run = p.ltr.data(), io.runs_cap = z.runs;
    io.rev_samples_first = p.revSmpf.data(), io.rev_samples_last = p.revSmpl.data(), io.rev_runs_cap = z.rev_runs;
    io.plcp_pos = p.plcpPos.data(), io.plcp_sum = p.plcpSum.data(), io.plcp_cap = z.n_plcp;
    check(cmb_build_move_arrays(b, &io, nullptr));
    return p;
}

// buildMoveIndex with the parts from the device: the same preprocessing, the same writer, the same files
inline void buildMoveIndexDevice(const std::vector<std::string>& fastaFiles, const std::string& base, uint32_t seedLength = 100,
                                 bool keepText = false, int device = 0) {
    const Text tx = preprocessFastaFiles(fastaFiles, seedLength);
    writeMoveIndexFiles(tx, base, keepText, deviceMoveParts(tx.T, device));
}

// FASTA files -> a resident BMove (BMove::FromText) and what the SAM header and the records need of the text, as fmIndexFromFasta;
// attachText: with the text beside the index, for alignments
inline std::unique_ptr<rlc::BMove> bmoveFromFasta(const std::vector<std::string>& fastaFiles, Text& tx, uint32_t seedLength = 100,
                                                  bool attachText = false, int device = 0) {
    tx = preprocessFastaFiles(fastaFiles, seedLength);
    std::unique_ptr<rlc::BMove> ix(new rlc::BMove(rlc::BMove::FromText{}, tx.T, device, true, attachText, tx.positions));
    std::string().swap(tx.T);
    return ix;
}

} // namespace build
} // namespace columba_amd
