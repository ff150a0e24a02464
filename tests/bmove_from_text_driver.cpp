// BMove built from text on the device (BMove::FromText, bmoveFromFasta) against BMove loaded from the index files of the same FASTA
// files (tests/test_gpu_cpp_device_move_builder.py): cmb_move_info and the exact matches of the reads in <reads file>, one per line.
//   bmove_from_text_driver <index base> <reads file> <fasta> [<fasta> ...]     prints "OK <text length> <runs> <matches>" or the difference
#include "columba_amd_build_device.hpp"

#include <cstdio>
#include <fstream>

using namespace columba_amd;

static bool sameMatches(const std::vector<std::vector<rlc::TextOcc>>& a, const std::vector<std::vector<rlc::TextOcc>>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].size() != b[i].size()) return false;
        for (size_t j = 0; j < a[i].size(); j++)
            if (a[i][j].getBegin() != b[i][j].getBegin() || a[i][j].getEnd() != b[i][j].getEnd() || a[i][j].getDistance() != b[i][j].getDistance() ||
                a[i][j].getStrand() != b[i][j].getStrand())
                return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    try {
        std::vector<std::string> reads, fasta(argv + 3, argv + argc);
        std::ifstream rf(argv[2]);
        for (std::string line; std::getline(rf, line);)
            if (!line.empty()) reads.push_back(line);
        rlc::BMove fromFiles(argv[1]);
        build::Text tx;
        std::unique_ptr<rlc::BMove> fromFasta = build::bmoveFromFasta(fasta, tx, 100, true);
        const build::Text tx2 = build::preprocessFastaFiles(fasta, 100);
        rlc::BMove fromText(rlc::BMove::FromText{}, tx2.T);
        uint64_t info[3][3];
        const rlc::BMove* all[3] = {&fromFiles, fromFasta.get(), &fromText};
        for (int k = 0; k < 3; k++)
            if (cmb_move_info(all[k]->handle(), &info[k][0], &info[k][1], &info[k][2]) != CMB_OK) throw std::runtime_error(cmb_last_error());
        for (int k = 1; k < 3; k++)
            for (int f = 0; f < 3; f++)
                if (info[k][f] != info[0][f]) {
                    std::printf("cmb_move_info differs: index %d field %d: %llu, %llu from the files\n", k, f, (unsigned long long)info[k][f],
                                (unsigned long long)info[0][f]);
                    return 1;
                }
        if (fromFasta->getTextSize() != fromFiles.getTextSize() || fromFasta->getNumberOfRuns() != fromFiles.getNumberOfRuns() || !tx.T.empty() ||
            tx.positions != tx2.positions || !cmb_move_text_index(fromFasta->handle()) || cmb_move_text_index(fromText.handle())) {
            std::printf("the adapter's own fields differ\n");
            return 1;
        }
        std::vector<std::vector<rlc::TextOcc>> want, got;
        const uint64_t total = fromFiles.exactMatchesOutput(reads, want);
        for (int k = 1; k < 3; k++) {
            if (all[k]->exactMatchesOutput(reads, got) != total || !sameMatches(want, got)) {
                std::printf("exact matches differ: index %d\n", k);
                return 1;
            }
        }
        uint64_t matches = 0;
        for (const auto& m : want) matches += m.size();
        std::printf("OK %llu %llu %llu\n", (unsigned long long)info[0][0], (unsigned long long)info[0][1], (unsigned long long)matches);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "bmove_from_text_driver: %s\n", e.what());
        return 3;
    }
}
