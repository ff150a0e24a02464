// Index construction on the device, for a host that links libcolumba_amd.so: the preprocessing and the file writer of
// include/columba_amd_build.hpp around the arrays of cmb_build_* (include/columba_amd.h) instead of the host's SA-IS and scalar loops.
// The files are the host builder's byte for byte (tests/test_gpu_cpp_device_builder.py).  Vanilla flavour, 32-bit length_t.
//   g++ -std=c++17 -O2 -DCOLUMBA_AMD_DEVICE_BUILD -I include examples/columba_build.cpp -o columba_build -L columba_amd -lcolumba_amd -lz
// Also here: an FMIndex straight from FASTA files, with no index files in between (fmIndexFromFasta).
#pragma once
#include "columba_amd.h"
#include "columba_amd.hpp"
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

} // namespace build
} // namespace columba_amd
