// Runtime values to template arguments, in one place (host_util.hpp includes this; no HIP here, so that a CPU program can call it:
// tests/host_dispatch_driver.cpp).  A selector calls its functor with compile-time constants; the functor names the kernel instance.
#pragma once
#include <cstdint>
#include <type_traits>
#include <utility>

namespace cmb {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): one constant per flag, in the order given
template <typename F> decltype(auto) withBools(F&& f) { return std::forward<F>(f)(); }
template <typename F, typename... Bs> decltype(auto) withBools(F&& f, bool b0, Bs... bs) {
    auto next = [&](auto... cs) -> decltype(auto) { return b0 ? f(std::true_type{}, cs...) : f(std::false_type{}, cs...); };
    return withBools(next, bs...);
}

// f(std::integral_constant<int, v>{}) for v in [0, N); a value beyond the range takes the last instance
template <int N, typename F> decltype(auto) withInt(int v, F&& f) {
    if constexpr (N <= 1) return f(std::integral_constant<int, 0>{});
    else if (v >= N - 1) return f(std::integral_constant<int, N - 1>{});
    else return withInt<N - 1>(v, std::forward<F>(f));
}

// Which record geometry the frontier of an edit-distance batch runs on (dev_bfs_edit.hpp: GeoX, GeoW, GeoN32, GeoN).  The wide tables
// beyond mxMaxEd errors (the reach of the reference's 64-bit in-index matrix): GeoX with its 16-row blocks, otherwise GeoW.  The narrow
// tables up to mxsMaxEd errors: the in-index matrix on 32-bit words (GeoN32), unless a phase of an earlier run did not fit it or
// CMB_MATRIX64 keeps the reference's 64-bit words (GeoN)
enum class FrontierGeo { X, W, N32, N };
inline FrontierGeo frontierGeo(bool wide, uint32_t k, bool noSmallMatrix, bool matrix64, uint32_t mxMaxEd, uint32_t mxsMaxEd) {
    if (wide) return k > mxMaxEd ? FrontierGeo::X : FrontierGeo::W;
    return k <= mxsMaxEd && !noSmallMatrix && !matrix64 ? FrontierGeo::N32 : FrontierGeo::N;
}

} // namespace cmb
