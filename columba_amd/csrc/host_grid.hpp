// Launch geometry knobs of the batch pipeline (host_util.hpp includes this; no HIP here, so that a CPU program can call it:
// tests/grid_cap_driver.cpp).  Most launches are capped at a fixed number of lanes and let every lane loop over the items beyond the
// cap; the environment may lower a cap, never to a launch of 0 blocks nor to a slot count that is no positive multiple of the block.
//   CMB_TEST_GRID_CAP=<blocks>   every capped launch takes min(its own cap, <blocks>): tests run the second trip of each loop at a few
//                                hundred items (tests/test_gpu_grid_trips.py).  Unset: no cap, the geometry is the default's.
// Zero, negative and non-numeric values of any knob count as 1 block.  All are read per run.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace cmb {

constexpr uint32_t GRID_UNCAPPED = 0xFFFFFFFFu;

// the value of a knob that counts blocks, lanes or slots: at least 1, at most 2^31 - 1
inline uint32_t knobValue(const char* v) {
    const long long x = v ? strtoll(v, nullptr, 10) : 0;
    return (uint32_t)std::min<long long>(std::max<long long>(x, 1), 0x7FFFFFFF);
}
// a knob in blocks: `dflt` when unset
inline uint32_t envBlocks(const char* name, uint32_t dflt) {
    const char* v = getenv(name);
    return v ? knobValue(v) : dflt;
}
// a knob in lanes / slots: `dflt` when unset, otherwise rounded down to a multiple of the block, one block at least, `most` at most
inline uint32_t envSlots(const char* name, uint32_t dflt, uint32_t most = 0x7FFFFF00u, uint32_t block = 256u) {
    const char* v = getenv(name);
    if (!v) return dflt;
    return std::max(block, std::min(most, knobValue(v)) / block * block);
}
inline uint32_t testGridCap() { return envBlocks("CMB_TEST_GRID_CAP", GRID_UNCAPPED); }
// blocks / slots of a launch under the test cap (0 blocks stay 0: the caller launches nothing then)
inline uint32_t capBlocks(uint32_t blocks) { return std::min(blocks, testGridCap()); }
inline uint32_t capSlots(uint32_t slots, uint32_t block = 256u) { return capBlocks(slots / block) * block; }

// CMB_VERBOSE: what a capped launch was given
inline void gridLine(bool verbose, const char* kernel, uint64_t items, uint64_t lanes) {
    if (verbose) fprintf(stderr, "[grid] %s %llu items, %llu lanes\n", kernel, (unsigned long long)items, (unsigned long long)lanes);
}

} // namespace cmb
