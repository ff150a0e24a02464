// The 16-byte row of a move table in HBM (layout: move_dev.hpp), by itself: the device builder (dev_move_build.hpp) writes rows and the
// b-move backend reads them, in two translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmb {

constexpr uint64_t MV_M40 = (1ull << 40) - 1;

struct MoveRow {
    uint32_t head;
    uint64_t in, out, outRun;
};

__host__ __device__ inline uint4 packMoveRow(uint32_t head, uint64_t in, uint64_t out, uint64_t outRun) {
    const uint64_t lo = (uint64_t)(head & 7u) | (in & MV_M40) << 3 | (out & MV_M40) << 43;
    const uint64_t hi = (out & MV_M40) >> 21 | (outRun & MV_M40) << 19;
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
__host__ __device__ inline MoveRow unpackMoveRow(const uint4 v) {
    const uint64_t lo = (uint64_t)v.x | (uint64_t)v.y << 32, hi = (uint64_t)v.z | (uint64_t)v.w << 32;
    MoveRow r;
    r.head = (uint32_t)lo & 7u;
    r.in = (lo >> 3) & MV_M40;
    r.out = (lo >> 43 | hi << 21) & MV_M40;
    r.outRun = (hi >> 19) & MV_M40;
    return r;
}

} // namespace cmb
