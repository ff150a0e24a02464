// What Reader (include/columba_amd_io.hpp) returns for a read file, for the tests of the device parser to compare against:
//   reader_driver <file> <records per chunk> <calls>
// makes <calls> calls of getNextChunk and prints, per call, "C <return value> <records>\n" and per record
// "R <identifier bytes> <read bytes> <quality bytes>\n" followed by the three fields as they are and a newline.  An exception ends the
// output with "E <message>\n" (exit status 3).  Built with -DREADER_DEVICE (and linked with the library) the same calls go to DeviceReader.
#include "columba_amd_io.hpp"

#include <cstdio>
#include <cstdlib>

using namespace columba_amd;

static void print(bool any, const std::vector<SequenceRecord>& chunk) {
    printf("C %d %zu\n", any ? 1 : 0, chunk.size());
    for (const auto& r : chunk) {
        printf("R %zu %zu %zu\n", r.seqID.size(), r.read.size(), r.qual.size());
        fwrite(r.seqID.data(), 1, r.seqID.size(), stdout);
        fwrite(r.read.data(), 1, r.read.size(), stdout);
        fwrite(r.qual.data(), 1, r.qual.size(), stdout);
        fputc('\n', stdout);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <file> <records per chunk> <calls>\n", argv[0]);
        return 2;
    }
    const size_t n = (size_t)strtoull(argv[2], nullptr, 10), calls = (size_t)strtoull(argv[3], nullptr, 10);
    try {
#ifdef READER_DEVICE
        DeviceReader reader(argv[1]);
        ParsedChunk chunk;
        for (size_t c = 0; c < calls; c++) {
            const bool any = reader.getNextChunk(chunk, n);
            print(any, chunk.records());
        }
#else
        Reader reader(argv[1]);
        std::vector<SequenceRecord> chunk;
        for (size_t c = 0; c < calls; c++) {
            const bool any = reader.getNextChunk(chunk, n);
            print(any, chunk);
        }
#endif
    } catch (const std::exception& e) {
        printf("E %s\n", e.what());
        return 3;
    }
    return 0;
}
