// Drives the BEST-mode strata loop of columba_amd/csrc/host_best.hpp over a scripted store (tests/test_best_loop.py).
// stdin:  x n, then per read: cutOff maskFw maskRc (bit d: the read has an occurrence at distance d on that strand, inside one sequence)
// stdout: "run k id id ..." per stratum batch in the order they ran, then per read
//         "read i found best | k k ... | strand:l strand:l ... | strand:d strand:d ..." — the distances it was searched at, the
//         checkAlignments calls it got, the records combineOccVectors kept
#include "host_best.hpp"

#include <cstdio>
#include <cstdlib>

using namespace cmb;

struct Scripted {
    std::vector<BestCursor> cur;
    std::vector<BestHostRead> rd;
    std::vector<uint32_t> mask[2];
    std::vector<std::vector<uint32_t>> searched;
    std::vector<std::vector<std::pair<int, uint32_t>>> checked;

    BestCursor& cursor(uint32_t i) { return cur[i]; }
    bool nonEmpty(uint32_t i, int s, uint32_t d) const { return rd[i].nonEmpty(s, d); }
    void check(uint32_t i, int s, uint32_t l, uint32_t cutOffTrim) {
        checked[i].push_back({s, l});
        bestCheckHost(rd[i], cur[i].best, s, l, cutOffTrim, [](const std::string&, BestOcc&, uint32_t) -> bool {
            std::fprintf(stderr, "no scripted occurrence runs over a sequence end\n");
            std::abort();
        });
    }
    int run(const std::vector<uint32_t>& ids, uint32_t k) {
        std::printf("run %u", k);
        for (uint32_t i : ids) {
            std::printf(" %u", i);
            searched[i].push_back(k);
            for (uint32_t d = std::min<uint32_t>(cur[i].proc, k); d <= k; d++) // what a stratum keeps: min(proc, k) .. k
                for (uint32_t s = 0; s < 2; s++)
                    if ((mask[s][i] >> d) & 1u) {
                        BestOcc o{};
                        o.occ.distance = d, o.occ.strand = s;
                        o.aln.seq_begin = 2 * d + s;
                        rd[i].add(std::move(o));
                    }
        }
        std::printf("\n");
        return 0;
    }
};

int main() {
    uint32_t x = 0, n = 0;
    if (std::scanf("%u %u", &x, &n) != 2) return 2;
    Scripted S;
    S.cur.resize(n), S.rd.resize(n), S.mask[0].resize(n), S.mask[1].resize(n), S.searched.resize(n), S.checked.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t cutOff = 0;
        if (std::scanf("%u %u %u", &cutOff, &S.mask[0][i], &S.mask[1][i]) != 3) return 2;
        S.cur[i] = bestCursor(cutOff);
        S.rd[i].start(cutOff);
    }
    if (bestStrataLoop(S, n, x)) return 3;
    for (uint32_t i = 0; i < n; i++) {
        const BestCursor& c = S.cur[i];
        std::printf("read %u %d %u |", i, c.bestFound ? 1 : 0, c.best);
        for (uint32_t k : S.searched[i]) std::printf(" %u", k);
        std::printf(" |");
        for (const auto& sl : S.checked[i]) std::printf(" %d:%u", sl.first, sl.second);
        std::printf(" |");
        if (c.bestFound)
            bestCombineHost(S.rd[i], c.best, std::min<uint32_t>(c.best + x, c.cutOff), [](const BestOcc& o) { std::printf(" %u:%u", o.occ.strand, o.occ.distance); });
        std::printf("\n");
    }
    return 0;
}
