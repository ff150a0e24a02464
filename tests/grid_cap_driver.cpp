// Stand-alone driver of tests/test_grid_cap.py: the launch-geometry knobs of columba_amd/csrc/host_grid.hpp as the environment of this
// process sets them.  One line per question, `name value`.
#include "host_grid.hpp"

#include <cstdio>

using namespace cmb;

int main() {
    printf("cap %u\n", testGridCap());
    // blocks of launches whose own cap is 1, 4, 128, 1024, 8192 and 16384 blocks, and of a launch with nothing to do
    const uint32_t own[] = {0u, 1u, 4u, 128u, 1024u, 8192u, 16384u};
    for (uint32_t b : own) printf("blocks_%u %u\n", b, capBlocks(b));
    // lanes of launches counted in slots of 256 (k_parts' 8 M, k_verify's 256 k, one block) and in wavefronts of 64 (b-move prologue)
    printf("slots_8M %u\n", capSlots(256u * 32768u));
    printf("slots_256k %u\n", capSlots(256u * 1024u));
    printf("slots_256 %u\n", capSlots(256u));
    printf("slots_0 %u\n", capSlots(0u));
    printf("lanes64_16384 %u\n", 64u * capBlocks(16384u));
    // the knobs beside it, each under the name the library reads: GRID_KNOB in blocks, SLOT_KNOB in slots
    printf("knob_blocks %u\n", envBlocks("GRID_KNOB", 8192u));
    printf("knob_slots %u\n", envSlots("SLOT_KNOB", 256u * 1536u));
    printf("knob_slots_most %u\n", envSlots("SLOT_KNOB", 256u * 1024u, 256u * 2048u));
    // a knob and the cap together: the smaller wins
    printf("both_blocks %u\n", capBlocks(envBlocks("GRID_KNOB", 8192u)));
    printf("both_slots %u\n", capSlots(envSlots("SLOT_KNOB", 256u * 1536u)));
    gridLine(false, "quiet", 1, 1);
    gridLine(true, "k_test", 769, 256);
    return 0;
}
