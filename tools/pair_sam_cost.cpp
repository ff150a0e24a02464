// What the SAM text of a chunk of read pairs in ALL mode costs behind the matching, on the host path (cmb_pair_sam per pair) or the device
// path (cmb_pair_sam_device) of the C++ adapter.  Per repetition samOfChunkPairedAll is timed as a whole, and then the matching alone as
// that path does it (two batches with alignments, every strand filtered by itself; one after the other on the host path, both alive on
// the device path); the cost behind the matching is the difference of the two sums.
//   usage: pair_sam_cost <index base> <reads1.txt> <reads2.txt> <number of sequences> <k> <max fragment> <min fragment> <repetitions>
// The path is the environment's (CMB_PAIR_DEVICE); tools/pair_sam_cost.py builds the inputs and runs this once per path.  Prints one JSON line.
#include "columba_amd.hpp"

#include <chrono>
#include <iostream>

using namespace columba_amd;

struct Rec {
    std::string seqID, read, qual;
};
typedef std::chrono::steady_clock Clock;
static double msSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct Strategy : NamedStrategy {
    using NamedStrategy::NamedStrategy;
    // the matching of both mates; bothAlive: the second batch is created and run while the first one lives (the device path), and
    // *stats then gets what one cmb_pair_sam_device_classes call on the two reports (outside the clock)
    double matchMs(const std::vector<Rec>* mates[2], const std::vector<const char*>& seqNames, length_t k, const cmb_pair_params& prm, bool bothAlive,
                   uint32_t classes, cmb_pair_class_stats* stats) {
        cmb_batch* b[2] = {nullptr, nullptr};
        std::string seqs[2];
        double ms = 0;
        for (int m = 0; m < 2; m++) {
            const Clock::time_point t0 = Clock::now();
            const std::vector<Rec>& recs = *mates[m];
            std::vector<uint64_t> offs(recs.size() + 1, 0);
            for (size_t j = 0; j < recs.size(); j++) seqs[m] += recs[j].read, offs[j + 1] = seqs[m].size();
            check(cmb_batch_create(index.handle(), h, k, seqs[m].data(), offs.data(), (uint32_t)recs.size(), &b[m]));
            check(cmb_batch_want_alignments(b[m], 1));
            check(cmb_batch_filter_per_strand(b[m], 1));
            check(cmb_batch_run(b[m]));
            ms += msSince(t0);
            if (!bothAlive) cmb_batch_destroy(b[m]), b[m] = nullptr;
        }
        if (bothAlive) {
            cmb_sam_inputs in[2];
            std::unique_ptr<SamPacked> packed[2];
            for (int m = 0; m < 2; m++) {
                const std::vector<Rec>& recs = *mates[m];
                packed[m].reset(new SamPacked(recs.size(), seqNames, [&](size_t i) -> const std::string& { return recs[i].seqID; }, false,
                                              [&](size_t i) -> const std::string& { return recs[i].qual; }));
                in[m] = packed[m]->inputs(seqs[m]);
            }
            const char* text = nullptr;
            uint64_t length = 0;
            const int rc = cmb_pair_sam_device_classes(b[0], b[1], &prm, &in[0], &in[1], classes, &text, &length, stats);
            cmb_batch_destroy(b[0]);
            cmb_batch_destroy(b[1]);
            check(rc);
        }
        return ms;
    }
};

static std::vector<Rec> readsOf(const char* file, int mate) {
    std::vector<Rec> v;
    std::ifstream f(file);
    std::string line;
    while (std::getline(f, line))
        if (!line.empty()) v.push_back(Rec{"@p" + std::to_string(v.size()) + "/" + std::to_string(mate) + " x", line, std::string(line.size(), 'I')});
    return v;
}

int main(int argc, char** argv) {
    if (argc < 9) {
        std::cerr << "usage: " << argv[0] << " <index base> <reads1.txt> <reads2.txt> <sequences> <k> <max fragment> <min fragment> <repetitions>\n";
        return 2;
    }
    try {
        FMIndex index(argv[1], 4, true, 4, false, 10);
        Strategy strategy(index, "multiple_opt", DYNAMIC, EDIT);
        const std::vector<Rec> m1 = readsOf(argv[2], 1), m2 = readsOf(argv[3], 2);
        const std::vector<Rec>* mates[2] = {&m1, &m2};
        std::vector<std::string> names;
        for (int i = 0; i < atoi(argv[4]); i++) names.push_back("chr" + std::to_string(i));
        std::vector<const char*> namePtrs;
        for (const auto& s : names) namePtrs.push_back(s.c_str());
        const length_t k = (length_t)atoi(argv[5]);
        const cmb_pair_params prm = {CMB_ORIENTATION_FR, (uint32_t)atoi(argv[6]), (uint32_t)atoi(argv[7]), 1, 1};
        const int reps = atoi(argv[8]);
        const char* e = getenv("CMB_PAIR_DEVICE");
        const bool device = e && atoi(e) != 0;
        uint32_t classes = CMB_PAIR_CLASS_ALL; // (as samOfChunkPairedAll chooses them)
        if (const char* c = getenv("CMB_PAIR_DEVICE_CLASSES")) classes = (uint32_t)strtoul(c, nullptr, 0);
        size_t mapped = 0, bytes = 0;
        uint64_t sum = 0;
        double totalMs = 0, matchMs = 0;
        std::string each; // the cost behind the matching of every repetition, so that their spread shows
        cmb_pair_class_stats stats{};
        for (int r = -1; r < reps; r++) { // (the first round warms up: buffers, page-locked memory)
            if (r == 0) totalMs = matchMs = 0, mapped = 0;
            const Clock::time_point t0 = Clock::now();
            const std::string text = strategy.samOfChunkPairedAll(m1, m2, namePtrs, k, prm.orientation, prm.max_frag, prm.min_frag, true, true, mapped);
            const double callMs = msSince(t0), callMatchMs = strategy.matchMs(mates, namePtrs, k, prm, device, classes, &stats);
            totalMs += callMs, matchMs += callMatchMs;
            if (r >= 0) each += (each.empty() ? "" : ", ") + std::to_string((callMs - callMatchMs) * 1e6 / (double)m1.size());
            bytes = text.size();
            sum = 0;
            for (unsigned char c : text) sum = sum * 1099511628211ull + c;
        }
        const double perM = 1e6 / ((double)m1.size() * reps);
        printf("{\"path\": \"%s\", \"pairs\": %zu, \"repetitions\": %d, \"total_ms_per_1e6_pairs\": %.1f, \"match_ms_per_1e6_pairs\": %.1f, "
               "\"after_ms_per_1e6_pairs\": %.1f, \"after_ms_per_1e6_pairs_each\": [%s], \"classes\": %u, \"one_unmapped\": %llu, \"discordant\": %llu, "
               "\"over_limit\": %llu, \"host_pair_share\": %.4f, \"mapped_pairs\": %zu, \"text_bytes\": %zu, \"text_hash\": \"%016llx\"}\n",
               device ? "device" : "host", m1.size(), reps, totalMs * perM, matchMs * perM, (totalMs - matchMs) * perM, each.c_str(), device ? classes : 0u,
               (unsigned long long)stats.one_unmapped, (unsigned long long)stats.discordant, (unsigned long long)stats.over_limit,
               (double)stats.host_pairs / (double)m1.size(), mapped / (size_t)reps, bytes, (unsigned long long)sum);
    } catch (const std::exception& e) {
        std::cerr << "Fatal error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
