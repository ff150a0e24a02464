// Host-side I/O around the C-ABI: a FASTA / FASTQ chunk reader, an ordered SAM writer and the chunk loop of a
// Columba-style aligner.  Host C++ only; all matching happens behind include/columba_amd.h, and so does the
// record splitting of DeviceReader (cmb_reads_*), which hands FASTQ chunks over packed.
//
// Mirrors (reference, src/):
//   SequenceRecord::readFromFileFASTQ / readFromFileFASTA   fastq.cpp:43-146 (records; multi-line FASTA; "*" quality)
//   Reader::getNextChunk                                    fastq.cpp:395      (chunks of records)
//   OutputWriter::writerThread (header + ordered chunks)    fastq.cpp:567-660  (@HD, @PG, the @SQ lines of <base>.headerSN.bin)
//   processChunk / threadEntrySingleEnd                     parallel.cpp:67-111
#pragma once
#include "columba_amd.h"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#if defined(__has_include)
#if __has_include(<zlib.h>)
#include <zlib.h> // gz-compressed read files (the reference: HAVE_ZLIB, seqfile.cpp); link with -lz
#define COLUMBA_AMD_HAVE_ZLIB 1
#endif
#endif

namespace columba_amd {

// A read file as a stream of lines, plain or gz-compressed by its extension (SeqFile, seqfile.{h,cpp}: ".gz" selects zlib)
class LineSource {
    std::ifstream in;
#ifdef COLUMBA_AMD_HAVE_ZLIB
    gzFile gz = nullptr;
#endif
    bool compressed = false;
    std::string buf;
    size_t pos = 0;
    bool exhausted = false;

    bool fill() { // more bytes into buf; false at the end of the file
        if (exhausted) return false;
        buf.erase(0, pos);
        pos = 0;
        char tmp[1 << 16];
        long n = 0;
        if (compressed) {
#ifdef COLUMBA_AMD_HAVE_ZLIB
            n = gzread(gz, tmp, sizeof(tmp));
            if (n < 0) throw std::ios::failure("error while reading a gz-compressed file");
#endif
        } else {
            in.read(tmp, sizeof(tmp));
            n = (long)in.gcount();
        }
        if (n <= 0) {
            exhausted = true;
            return false;
        }
        buf.append(tmp, (size_t)n);
        return true;
    }

  public:
    explicit LineSource(const std::string& file) {
        compressed = file.size() > 3 && file.compare(file.size() - 3, 3, ".gz") == 0;
        if (compressed) {
#ifdef COLUMBA_AMD_HAVE_ZLIB
            gz = gzopen(file.c_str(), "rb");
            if (!gz) throw std::runtime_error("Cannot open file: " + file);
#else
            throw std::runtime_error("gz-compressed input needs zlib (built without it): " + file);
#endif
        } else {
            in.open(file, std::ios::binary);
            if (!in) throw std::runtime_error("Cannot open file: " + file);
        }
    }
    LineSource(const LineSource&) = delete;
    ~LineSource() {
#ifdef COLUMBA_AMD_HAVE_ZLIB
        if (gz) gzclose(gz);
#endif
    }
    int peek() { // the next character, EOF at the end
        if (pos >= buf.size() && !fill()) return EOF;
        return (unsigned char)buf[pos];
    }
    bool getline(std::string& line) { // without the newline; false at the end of the file
        line.clear();
        for (;;) {
            const size_t nl = buf.find('\n', pos);
            if (nl != std::string::npos) {
                line.append(buf, pos, nl - pos);
                pos = nl + 1;
                return true;
            }
            line.append(buf, pos, std::string::npos);
            pos = buf.size();
            if (!fill()) return !line.empty();
        }
    }
    bool good() { return peek() != EOF; }
};

struct SequenceRecord { // fastq.h SequenceRecord: identifier line as read (with @ or >), sequence, quality ("*" for FASTA)
    std::string seqID, read, qual;
};

class Reader { // fastq.h Reader (single-end; plain text or .gz)
    LineSource in;
    std::string fileName;
    bool fastq = false;
    bool typeKnown = false;

    static void chomp(std::string& s) {
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    }
    bool skipBlankLines() {
        for (;;) {
            const int c = in.peek();
            if (c == EOF) return false;
            if (c != '\n' && c != '\r') return true;
            std::string dummy;
            in.getline(dummy);
        }
    }

  public:
    explicit Reader(const std::string& file) : in(file), fileName(file) {}
    // one record; false at the end of the file
    bool next(SequenceRecord& r) {
        r.seqID.clear();
        r.read.clear();
        r.qual.clear();
        if (!skipBlankLines()) return false;
        const int c = in.peek();
        if (!typeKnown) {
            fastq = c == '@';
            typeKnown = true;
        }
        if (fastq) { // fastq.cpp:43-99
            if (c != '@') throw std::ios::failure("File " + fileName + " doesn't appear to be in FastQ format");
            std::string plus;
            in.getline(r.seqID);
            in.getline(r.read);
            in.getline(plus);
            in.getline(r.qual);
            chomp(r.seqID);
            chomp(r.read);
            chomp(r.qual);
            return !r.read.empty();
        }
        if (c != '>') throw std::ios::failure("File " + fileName + " doesn't appear to be in Fasta format");
        in.getline(r.seqID); // fastq.cpp:101-146
        chomp(r.seqID);
        std::string line;
        while (in.good() && in.peek() != '>' && in.peek() != EOF) {
            in.getline(line);
            chomp(line);
            r.read += line;
        }
        r.qual = "*";
        return !r.read.empty();
    }
    // up to n records; false when the file is exhausted and nothing was read
    bool getNextChunk(std::vector<SequenceRecord>& chunk, size_t n) {
        chunk.clear();
        SequenceRecord r;
        while (chunk.size() < n && next(r)) chunk.push_back(r);
        return !chunk.empty();
    }
};

// A chunk of records in the packed form cmb_batch_create, cmb_match_best_device and cmb_sam_inputs take: read i is
// seqs[offs[i], offs[i + 1]), its raw identifier line ids[idOffs[i], idOffs[i + 1]), its quality quals[qualOffs[i], qualOffs[i + 1]).
// From DeviceReader the arrays are those of the reader's parser (page-locked, valid until its next chunk); from a FASTA file the
// chunk owns them.
struct ParsedChunk {
    const char *seqs = "", *ids = "", *quals = "";
    const uint64_t *offs = nullptr, *idOffs = nullptr, *qualOffs = nullptr;
    size_t n = 0;
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    std::vector<SequenceRecord> records() const {
        std::vector<SequenceRecord> out(n);
        for (size_t i = 0; i < n; i++) {
            out[i].seqID.assign(ids + idOffs[i], (size_t)(idOffs[i + 1] - idOffs[i]));
            out[i].read.assign(seqs + offs[i], (size_t)(offs[i + 1] - offs[i]));
            out[i].qual.assign(quals + qualOffs[i], (size_t)(qualOffs[i + 1] - qualOffs[i]));
        }
        return out;
    }
    void view(const cmb_reads_view& v) {
        seqs = v.seqs, ids = v.ids, quals = v.quals, offs = v.offs, idOffs = v.id_offs, qualOffs = v.qual_offs, n = v.n_records;
    }
    void pack(const std::vector<SequenceRecord>& recs) { // (the host reader's records: a FASTA file)
        own[0].clear(), own[1].clear(), own[2].clear();
        for (auto& o : ownOffs) o.assign(1, 0);
        for (const auto& r : recs) {
            own[0] += r.read, own[1] += r.seqID, own[2] += r.qual;
            for (int f = 0; f < 3; f++) ownOffs[f].push_back(own[f].size());
        }
        seqs = own[0].data(), ids = own[1].data(), quals = own[2].data();
        offs = ownOffs[0].data(), idOffs = ownOffs[1].data(), qualOffs = ownOffs[2].data(), n = recs.size();
    }

  private:
    std::string own[3];
    std::vector<uint64_t> ownOffs[3];
};

// Reader for FASTQ files with the records found on the device: the file is read in windows of raw bytes (plain, or inflated with zlib
// for ".gz"), cmb_reads_parse_fastq splits a window into records and returns the chunk packed.  Chunk for chunk and record for record
// what Reader returns (its behaviour is the parser's specification), the return value and the exception for a file that is not FASTQ
// included.  A file whose first record does not begin with '@' (FASTA among them) is read by Reader.  One limit Reader does not have:
// a chunk is cut where CMB_READS_MAX_WINDOW bytes of the file end, and a single record longer than that is an error.
class DeviceReader {
    std::string fileName;
    std::ifstream in;
#ifdef COLUMBA_AMD_HAVE_ZLIB
    gzFile gz = nullptr;
#endif
    bool compressed = false, eof = false;
    std::unique_ptr<Reader> host; // FASTA, or whatever Reader is to complain about
    cmb_reads* parser = nullptr;
    std::unique_ptr<char[]> win; // the window is win[begin, end)
    size_t cap = 0, begin = 0, end = 0;
    double bytesPerRecord = 512; // the estimate the window is sized from; the first chunk corrects it

    size_t readRaw(char* dst, size_t n) {
        if (compressed) {
#ifdef COLUMBA_AMD_HAVE_ZLIB
            size_t got = 0;
            while (got < n) { // (gzread takes an unsigned count)
                const int k = gzread(gz, dst + got, (unsigned)std::min<size_t>(n - got, 1u << 30));
                if (k < 0) throw std::ios::failure("error while reading a gz-compressed file");
                if (k == 0) break;
                got += (size_t)k;
            }
            return got;
#else
            return 0;
#endif
        }
        in.read(dst, (std::streamsize)n);
        return (size_t)in.gcount();
    }
    // the window holds `want` bytes, or everything up to the end of the file
    void fill(size_t want) {
        if (eof || end - begin >= want) return;
        if (want > cap || begin) { // the unconsumed tail moves to the front (of a larger buffer if need be)
            const size_t newCap = std::max(cap, want);
            std::unique_ptr<char[]> grown(newCap > cap ? new char[newCap] : nullptr);
            char* to = grown ? grown.get() : win.get();
            if (end > begin) memmove(to, win.get() + begin, end - begin);
            if (grown) win = std::move(grown), cap = newCap;
            end -= begin, begin = 0;
        }
        const size_t got = readRaw(win.get() + end, want - end);
        end += got;
        if (end < want) eof = true;
    }

  public:
    explicit DeviceReader(const std::string& file, int device = 0) : fileName(file) {
        int first;
        { // what the first record begins with (blank lines skipped, as Reader does)
            LineSource peek(file);
            std::string dummy;
            while ((first = peek.peek()) == '\n' || first == '\r') peek.getline(dummy);
        }
        if (first != '@' && first != EOF) {
            host.reset(new Reader(file));
            return;
        }
        compressed = file.size() > 3 && file.compare(file.size() - 3, 3, ".gz") == 0;
        if (compressed) {
#ifdef COLUMBA_AMD_HAVE_ZLIB
            gz = gzopen(file.c_str(), "rb");
            if (!gz) throw std::runtime_error("Cannot open file: " + file);
#endif
        } else {
            in.open(file, std::ios::binary);
            if (!in) throw std::runtime_error("Cannot open file: " + file);
        }
        if (cmb_reads_create(device, &parser) != CMB_OK) throw std::runtime_error(cmb_last_error());
    }
    DeviceReader(const DeviceReader&) = delete;
    ~DeviceReader() {
        cmb_reads_destroy(parser);
#ifdef COLUMBA_AMD_HAVE_ZLIB
        if (gz) gzclose(gz);
#endif
    }
    bool onDevice() const { return !host; }
    // up to n records; false when Reader::getNextChunk would return false
    bool getNextChunk(ParsedChunk& chunk, size_t n) {
        if (host) {
            std::vector<SequenceRecord> recs;
            const bool any = host->getNextChunk(recs, n);
            chunk.pack(recs);
            return any;
        }
        const uint32_t maxRecords = (uint32_t)std::min<size_t>(std::max<size_t>(n, 1), 0xFFFFFFFFu);
        size_t want = (size_t)std::min<double>((double)CMB_READS_MAX_WINDOW, std::max(65536.0, bytesPerRecord * (double)maxRecords));
        for (;;) {
            fill(want);
            cmb_reads_info info;
            const int rc = cmb_reads_parse_fastq(parser, win.get() + begin, end - begin, maxRecords, eof, &info);
            // (CMB_ERR_UNSUPPORTED: a window that begins with '>' — in a file that began with '@' that is a bad record as well)
            if (rc == CMB_ERR_INVALID || rc == CMB_ERR_UNSUPPORTED) throw std::ios::failure("File " + fileName + " doesn't appear to be in FastQ format");
            if (rc != CMB_OK) throw std::runtime_error(cmb_last_error());
            if (info.stop == CMB_READS_STOP_WINDOW && !eof) { // the window ended before the chunk did
                if (want < CMB_READS_MAX_WINDOW) {
                    want = (size_t)std::min<uint64_t>(CMB_READS_MAX_WINDOW, 2 * (uint64_t)want);
                    continue;
                }
                if (!info.n_records) throw std::runtime_error("File " + fileName + ": a record is longer than the largest window of the device parser");
            }
            begin += (size_t)info.consumed;
            cmb_reads_view v;
            if (cmb_reads_arrays(parser, &v) != CMB_OK) throw std::runtime_error(cmb_last_error());
            chunk.view(v);
            if (info.n_records) bytesPerRecord = 1.05 * (double)info.consumed / (double)info.n_records + 64.0 / (double)info.n_records;
            return info.n_records != 0;
        }
    }
};

class OutputWriter { // fastq.h OutputWriter: SAM header, then the chunks in the order of their ids; ".sam" or ".sam.gz" (fastq.cpp:466-493)
    std::ofstream out;
#ifdef COLUMBA_AMD_HAVE_ZLIB
    gzFile gz = nullptr;
#endif
    std::map<size_t, std::string> pending;
    size_t nextChunkID = 0;
    void put(const std::string& s) {
#ifdef COLUMBA_AMD_HAVE_ZLIB
        if (gz) {
            for (size_t o = 0; o < s.size();) { // (gzwrite takes an unsigned count)
                const unsigned n = (unsigned)(s.size() - o < (1u << 30) ? s.size() - o : (1u << 30));
                if (gzwrite(gz, s.data() + o, n) != (int)n) throw std::ios::failure("error while writing a gz-compressed file");
                o += n;
            }
            return;
        }
#endif
        out << s;
    }

  public:
    // headerIsText: `headerFile` holds the @SQ lines themselves instead of the name of the file with them (an index without files)
    OutputWriter(const std::string& file, const std::string& headerFile, const std::string& commandLine, bool headerIsText = false) {
        std::string ext = file.size() >= 7 ? file.substr(file.size() - 7) : std::string();
        for (auto& c : ext) c = (char)toupper((unsigned char)c);
        if (ext == ".SAM.GZ") {
#ifdef COLUMBA_AMD_HAVE_ZLIB
            gz = gzopen(file.c_str(), "wb");
            if (!gz) throw std::runtime_error("Cannot open file: " + file);
#else
            throw std::runtime_error("gz-compressed output needs zlib (built without it): " + file);
#endif
        } else {
            out.open(file);
            if (!out) throw std::runtime_error("Cannot open file: " + file);
        }
        put("@HD\tVN:1.6\tSO:queryname\n"); // fastq.cpp:579-583
        put("@PG\tID:Columba-amd\tPN:Columba\tCL:" + commandLine + "\n");
        if (headerIsText) {
            put(headerFile);
            return;
        }
        std::ifstream hs(headerFile, std::ios::binary);
        std::string line;
        while (hs && std::getline(hs, line)) put(line + "\n");
    }
    OutputWriter(const OutputWriter&) = delete;
    ~OutputWriter() {
#ifdef COLUMBA_AMD_HAVE_ZLIB
        if (gz) gzclose(gz);
#endif
    }
    void commitChunk(size_t id, std::string&& text) { // chunks may arrive out of order; they leave in order
        pending.emplace(id, std::move(text));
        for (auto it = pending.begin(); it != pending.end() && it->first == nextChunkID; it = pending.erase(it), nextChunkID++)
            put(it->second);
    }
    void flush() {
#ifdef COLUMBA_AMD_HAVE_ZLIB
        if (gz) {
            gzflush(gz, Z_SYNC_FLUSH);
            return;
        }
#endif
        out.flush();
    }
};

// sequence names of an index: <base>.sna (size_t length + bytes per name, indexinterface.cpp:175-195)
inline std::vector<std::string> readSequenceNames(const std::string& base) {
    std::vector<std::string> names;
    std::ifstream f(base + ".sna", std::ios::binary);
    while (f) {
        size_t len = 0;
        f.read(reinterpret_cast<char*>(&len), sizeof(len));
        if (!f) break;
        std::string s(len, '\0');
        f.read(&s[0], (std::streamsize)len);
        if (!f) break;
        names.push_back(s);
    }
    return names;
}

} // namespace columba_amd
