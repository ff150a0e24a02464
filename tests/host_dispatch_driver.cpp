// What the selectors of columba_amd/csrc/host_dispatch.hpp hand their functors (tests/test_host_dispatch.py; no GPU, no HIP).
// One line per call: the name of the case, then the constants the functor received, in the order it received them.
#include "host_dispatch.hpp"

#include <cstdio>
#include <cstdlib>

using namespace cmb;

// the functor returns a function pointer, as the selectors of the library do: every instance has the same type
template <bool A, bool B, bool C, bool D> void four() { printf(" %d %d %d %d\n", (int)A, (int)B, (int)C, (int)D); }
template <int V> int theInt() { return V; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const uint32_t mxMaxEd = (uint32_t)atoi(argv[1]), mxsMaxEd = (uint32_t)atoi(argv[2]);
    for (int m = 0; m < 16; m++) {
        const bool a = m & 8, b = m & 4, c = m & 2, d = m & 1;
        printf("four_%d", m);
        withBools([](auto w, auto x, auto y, auto z) { return four<w(), x(), y(), z()>; }, a, b, c, d)();
    }
    for (int m = 0; m < 4; m++) {
        printf("two_%d", m);
        withBools([](auto x, auto y) { printf(" %d %d\n", (int)decltype(x)::value, (int)decltype(y)::value); }, (m & 2) != 0, (m & 1) != 0);
    }
    printf("zero %d\n", withBools([] { return 7; }));
    for (int v = -1; v <= 5; v++) printf("int3_%d %d\n", v, withInt<3>(v, [](auto i) { return theInt<i()>; })());
    printf("int1_4 %d\n", withInt<1>(4, [](auto i) { return (int)decltype(i)::value; }));
    // the geometry of the frontier over distance x width x noSmallMatrix x forced 64-bit words; the limits (dev_matrix.hpp: MX_MAX_ED,
    // MXS_MAX_ED) are the test's to give
    for (int k = 0; k <= 13; k++)
        for (int m = 0; m < 8; m++)
            printf("geo_%d_%d %d\n", k, m, (int)frontierGeo((m & 4) != 0, (uint32_t)k, (m & 2) != 0, (m & 1) != 0, mxMaxEd, mxsMaxEd));
    return 0;
}
