// A Columba-style aligner (single-end and paired-end reads, ALL and BEST mode) over the C-ABI (the counterpart of `columba` for the hot path this library
// accelerates: reference src/parallel.cpp main / threadEntrySingleEnd / processChunk):
//   columba_align (-r <index base> | -G <fasta> [<fasta> ...]) -f <reads.fq|fa> -o <out.sam> [-e <max distance>] [-a all|best] [-x <strata>]
//                 [-I <min identity>] [-S <strategy>] [-m edit|hamming] [-p uniform|static|dynamic]
//                 [-s <SA sparseness>] [-K <k-mer size>] [-i <in-text switch>] [-b <reads per chunk>] [-XA] [-nU]
//                 [-F <mates.fq> -O fr|rf|ff -X <max insert> -N <min insert> -nD -nI]  (read pairs)
// Read pairs: unless -nI or one of -O / -X / -N is given, orientation and insert-size bounds are inferred from the first pairs of
// the files as the reference does (parallel.cpp:468-655, :862-935: up to 10 000 reads matched single-end, the pairs whose mates both map
// unambiguously are the sample) and that first chunk is paired from its single-end results.
// FASTQ / FASTA in, SAM out (header of <base>.headerSN.bin, records in input order).
// -G <fasta> [<fasta> ...] instead of -r <index base>: no index files — the reference sequences are preprocessed as columba_build does
// (seed length 0) and their index is built on the GPU, where it stays (include/columba_amd_build_device.hpp: fmIndexFromFasta).  The
// records are those of a run with -r on the files columba_build writes for the same FASTA files.
#include "columba_amd.hpp"
#include "columba_amd_build_device.hpp"
#include "columba_amd_io.hpp"

#include <cstring>
#include <iostream>
#include <memory>

using namespace columba_amd;

// The chunks of a read file: the packed chunks of DeviceReader (the records of a FASTQ file found on the device; FASTA files fall back
// to Reader inside it) with their records made only where a path wants them, or with CMB_READER_HOST=1 Reader's records.
struct ChunkSource {
    std::unique_ptr<Reader> host;
    std::unique_ptr<DeviceReader> device;
    ParsedChunk packed;
    std::vector<SequenceRecord> records;
    static constexpr bool READER_DEVICE_DEFAULT = true; // 30 against 208 ms per 10^6 reads of 150 bp
    static bool onDevice() { // CMB_READER_HOST=1 keeps the host reader, CMB_READER_DEVICE=1 asks for the device reader
        if (const char* e = getenv("CMB_READER_HOST"); e && atoi(e) != 0) return false;
        if (const char* e = getenv("CMB_READER_DEVICE"); e && atoi(e) != 0) return true;
        return READER_DEVICE_DEFAULT;
    }
    explicit ChunkSource(const std::string& file) {
        if (onDevice()) device.reset(new DeviceReader(file));
        else host.reset(new Reader(file));
    }
    bool next(size_t n, bool wantRecords) {
        if (host) return host->getNextChunk(records, n);
        const bool any = device->getNextChunk(packed, n);
        if (wantRecords) records = packed.records();
        return any;
    }
    size_t size() const { return host ? records.size() : packed.size(); }
};

int main(int argc, char** argv) {
    std::string base, readsFile, matesFile, orientation = "fr", outFile, strategyName = "columba", mode = "best", metric = "edit", part = "dynamic", cmdline;
    int k = 0, x = 0, identity = 95, sparse = 4, kmer = 10, inTextSwitch = 4;
    size_t chunkReads = 1000000;
    std::vector<std::string> fastaFiles; // -G
    bool xa = false, unmapped = true, discordant = true, noInfer = false, pairParamsGiven = false;
    unsigned maxInsert = 500, minInsert = 0;
    for (int i = 0; i < argc; i++) cmdline += std::string(i ? " " : "") + argv[i];
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= argc) throw std::runtime_error("missing value for " + a);
            return argv[++i];
        };
        try {
            if (a == "-r") base = val();
            else if (a == "-f") readsFile = val();
            else if (a == "-G") {
                while (i + 1 < argc && argv[i + 1][0] != '-') fastaFiles.push_back(argv[++i]);
                if (fastaFiles.empty()) throw std::runtime_error("missing value for -G");
            }
            else if (a == "-o") outFile = val();
            else if (a == "-e") k = std::stoi(val());
            else if (a == "-a") mode = val();
            else if (a == "-x") x = std::stoi(val());
            else if (a == "-I") identity = std::stoi(val());
            else if (a == "-S") strategyName = val();
            else if (a == "-m") metric = val();
            else if (a == "-p") part = val();
            else if (a == "-s") sparse = std::stoi(val());
            else if (a == "-K") kmer = std::stoi(val());
            else if (a == "-i") inTextSwitch = std::stoi(val()); // (in-text verification switch point, the reference's -i; default 4)
            else if (a == "-b") chunkReads = (size_t)std::stoul(val());
            else if (a == "-XA") xa = true;
            else if (a == "-nU") unmapped = false;
            else if (a == "-F") matesFile = val();
            else if (a == "-O") orientation = val(), pairParamsGiven = true;
            else if (a == "-X") maxInsert = (unsigned)std::stoul(val()), pairParamsGiven = true;
            else if (a == "-N") minInsert = (unsigned)std::stoul(val()), pairParamsGiven = true;
            else if (a == "-nI") noInfer = true;
            else if (a == "-nD") discordant = false;
            else throw std::runtime_error("unknown option " + a);
        } catch (const std::exception& e) {
            std::cerr << "Fatal error: " << e.what() << "\n";
            return 2;
        }
    }
    if (base.empty() == fastaFiles.empty() || readsFile.empty() || outFile.empty()) {
        std::cerr << "usage: " << argv[0] << " (-r <index base> | -G <fasta> [<fasta> ...]) -f <reads> -o <out.sam> [-e k] [-a all|best] [-x strata] [-I identity] "
                     "[-S strategy] [-m edit|hamming] [-p uniform|static|dynamic] [-s sparseness] [-K kmer] [-i in-text switch] [-b chunk] [-XA] [-nU] "
                     "[-F mates -O fr|rf|ff -X max insert -N min insert -nD -nI]\n";
        return 2;
    }
    try {
        build::Text refText; // -G: names, positions and first sequences per file of the reference, as the index files hold them
        std::unique_ptr<FMIndex> indexPtr(fastaFiles.empty() ? new FMIndex(base, (length_t)inTextSwitch, false, sparse, false, (length_t)kmer)
                                                             : build::fmIndexFromFasta(fastaFiles, refText, (length_t)inTextSwitch, sparse, (length_t)kmer).release());
        FMIndex& index = *indexPtr;
        const PartitionStrategy ps = part == "uniform" ? UNIFORM : part == "static" ? STATIC : DYNAMIC;
        const DistanceMetric dm = metric == "hamming" ? HAMMING : EDIT;
        NamedStrategy strategy(index, strategyName.c_str(), ps, dm);
        const std::vector<std::string> seqNames = fastaFiles.empty() ? readSequenceNames(base) : refText.seqNames;
        std::string headerLines; // (-G: what columba_build writes to .headerSN.bin)
        for (size_t i = 0; i < refText.seqNames.size(); i++)
            headerLines += "@SQ\tSN:" + refText.seqNames[i] + "\tLN:" + std::to_string(refText.positions[i + 1] - refText.positions[i]) + "\n";
        std::vector<const char*> seqNamePtrs;
        for (const auto& s : seqNames) seqNamePtrs.push_back(s.c_str());
        uint32_t ori = orientation == "rf" ? CMB_ORIENTATION_RF : orientation == "ff" ? CMB_ORIENTATION_FF : CMB_ORIENTATION_FR;
        ChunkSource reader(readsFile);
        std::unique_ptr<ChunkSource> mateReader(matesFile.empty() ? nullptr : new ChunkSource(matesFile));
        OutputWriter writer(outFile, fastaFiles.empty() ? base + ".headerSN.bin" : headerLines, cmdline, !fastaFiles.empty());
        const std::vector<SequenceRecord>& chunk = reader.records;
        size_t chunkID = 0, nReads = 0, nMapped = 0;
        if (mateReader && !noInfer && !pairParamsGiven) {
            // PE_MAX_READS_FOR_INFERENCE = 10 000 reads (definitions.h:58): the first 5 000 pairs at most
            const size_t want = std::min<size_t>(chunkReads, 5000);
            if (reader.next(want, true)) {
                mateReader->next(want, true);
                const std::vector<SequenceRecord>& mates = mateReader->records;
                uint32_t seqsInFirstFile = (uint32_t)seqNames.size();
                if (!fastaFiles.empty()) {
                    if (refText.firstSeqIDPerFile.size() > 1) seqsInFirstFile = refText.firstSeqIDPerFile[1];
                } else {
                    std::ifstream fs(base + ".fsid", std::ios::binary);
                    uint32_t v[2] = {0, 0};
                    if (fs.read(reinterpret_cast<char*>(v), sizeof(v))) seqsInFirstFile = v[1]; // (a second file starts at sequence v[1])
                }
                auto report = [&](const cmb_pair_inferred& got, size_t unambiguousPairs, size_t readsGiven) {
                    std::cerr << "Found " << unambiguousPairs << " unambiguous pairs while processing " << readsGiven
                              << " reads for inferring paired-end parameters\n";
                    if (got.inferred) {
                        ori = got.orientation, maxInsert = got.max_insert, minInsert = got.min_insert;
                        std::cerr << "Inferred paired-end parameters: orientation " << (ori == CMB_ORIENTATION_FR ? "FR" : ori == CMB_ORIENTATION_RF ? "RF" : "FF")
                                  << ", insert size " << got.mean_insert << " +- " << got.stddev_insert << ", bounds [" << minInsert << ", " << maxInsert << "]\n";
                    } else
                        std::cerr << "No pairs mapped unambiguously. Using default values!\n";
                };
                std::string text;
                if (mode == "all") {
                    auto inf = strategy.inferPairedEndParametersAll(chunk, mates, (length_t)k, seqsInFirstFile);
                    report(inf.inferred, inf.unambiguousPairs, inf.readsGiven);
                    text = strategy.samOfChunkPairedAll(chunk, mates, seqNamePtrs, (length_t)k, ori, maxInsert, minInsert, discordant, unmapped, nMapped, &inf);
                } else {
                    auto inf = strategy.inferPairedEndParameters(chunk, mates, (uint32_t)identity, seqsInFirstFile);
                    report(inf.inferred, inf.unambiguousPairs, inf.readsGiven);
                    text = strategy.samOfChunkPairedBest(chunk, mates, seqNamePtrs, 0, (uint32_t)identity, ori, maxInsert, minInsert, discordant, unmapped, nMapped,
                                                         nullptr, &inf);
                }
                nReads += chunk.size();
                writer.commitChunk(chunkID++, std::move(text));
            }
        }
        while (reader.next(chunkReads, mateReader != nullptr)) {
            if (reader.device && !mateReader) { // the chunk is packed already
                std::string text = mode == "all" ? strategy.samOfChunkAll(reader.packed, seqNamePtrs, (length_t)k, unmapped, xa)
                                                 : strategy.samOfChunkBest(reader.packed, seqNames, (uint32_t)x, (uint32_t)identity, unmapped, xa, nMapped);
                nReads += reader.size();
                writer.commitChunk(chunkID++, std::move(text));
                continue;
            }
            std::string seqs;
            std::vector<uint64_t> offs(chunk.size() + 1, 0);
            std::vector<const char*> ids, quals;
            for (size_t i = 0; i < chunk.size(); i++) {
                seqs += chunk[i].read;
                offs[i + 1] = seqs.size();
                ids.push_back(chunk[i].seqID.c_str());
                quals.push_back(chunk[i].qual.c_str());
            }
            std::string text;
            if (mateReader) {
                mateReader->next(chunkReads, true);
                const std::vector<SequenceRecord>& mates = mateReader->records;
                if (mode == "all")
                    text = strategy.samOfChunkPairedAll(chunk, mates, seqNamePtrs, (length_t)k, ori, maxInsert, minInsert, discordant, unmapped, nMapped);
                else
                    text = strategy.samOfChunkPairedBest(chunk, mates, seqNamePtrs, (uint32_t)x, (uint32_t)identity, ori, maxInsert, minInsert, discordant,
                                                         unmapped, nMapped);
            } else if (mode == "all") {
                text = strategy.samOfChunkAll(seqs, offs, ids, quals, seqNamePtrs, (length_t)k, unmapped, xa);
            } else {
                text = strategy.samOfChunkBest(seqs, offs, chunk, seqNames, (uint32_t)x, (uint32_t)identity, unmapped, xa, nMapped);
            }
            nReads += chunk.size();
            writer.commitChunk(chunkID++, std::move(text));
        }
        writer.flush();
        std::cerr << "aligned " << nReads << " reads in " << chunkID << " chunk(s)\n";
    } catch (const std::exception& e) {
        std::cerr << "Fatal error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
