// The driver of tools/reader_rate.py: what a chunk costs from the file to the packed arrays, on the host and on the device, in one process.
//   reader_rate <fastq file> <records per chunk> <chunks>
// The file holds <chunks> chunks.  Chunk by chunk, alternating:
//   A  Reader::getNextChunk and the packing loop columba_align runs on its records (seqs, offs, one char* per identifier and quality)
//   B  DeviceReader::getNextChunk (window read, upload, kernels, download: the chunk is packed when it returns)
// and prints "A <ms>" / "B <ms>" per chunk and "EQUAL <0|1>" (the read characters and offsets of both are the same bytes).  Then the
// file is read once more through a second DeviceReader with CMB_VERBOSE set: the library prints the parts of every parse to stderr.
#include "columba_amd_io.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

using namespace columba_amd;

static double msSince(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <fastq file> <records per chunk> <chunks>\n", argv[0]);
        return 2;
    }
    const size_t n = (size_t)strtoull(argv[2], nullptr, 10), chunks = (size_t)strtoull(argv[3], nullptr, 10);
    try {
        {
            Reader host(argv[1]);
            DeviceReader device(argv[1]);
            std::vector<SequenceRecord> chunk;
            ParsedChunk packed;
            for (size_t c = 0; c < chunks; c++) {
                auto t0 = std::chrono::steady_clock::now();
                const bool any = host.getNextChunk(chunk, n);
                std::string seqs;
                std::vector<uint64_t> offs(chunk.size() + 1, 0);
                std::vector<const char*> ids, quals;
                for (size_t i = 0; i < chunk.size(); i++) {
                    seqs += chunk[i].read;
                    offs[i + 1] = seqs.size();
                    ids.push_back(chunk[i].seqID.c_str());
                    quals.push_back(chunk[i].qual.c_str());
                }
                printf("A %.3f\n", msSince(t0));
                t0 = std::chrono::steady_clock::now();
                const bool anyDevice = device.getNextChunk(packed, n);
                printf("B %.3f\n", msSince(t0));
                const bool equal = any == anyDevice && packed.size() == chunk.size() && ids.size() == chunk.size() && quals.size() == chunk.size() &&
                                   memcmp(packed.offs, offs.data(), offs.size() * sizeof(uint64_t)) == 0 && memcmp(packed.seqs, seqs.data(), seqs.size()) == 0;
                printf("EQUAL %d %zu\n", equal ? 1 : 0, chunk.size());
                fflush(stdout);
            }
        }
        setenv("CMB_VERBOSE", "1", 1);
        DeviceReader device(argv[1]);
        ParsedChunk packed;
        for (size_t c = 0; c < chunks; c++) device.getNextChunk(packed, n);
    } catch (const std::exception& e) {
        fprintf(stderr, "Fatal error: %s\n", e.what());
        return 1;
    }
    return 0;
}
