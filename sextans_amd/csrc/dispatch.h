// dispatch.h -- run-time values as compile-time constants: the one place where a kernel variant is picked from an option or a width.
//   with_bool(h->opt_exact, [&](auto EX) { go(kern<..., decltype(EX)::value>); });
//   with_value<8, 4, 2>(width / 4, [&](auto L) { constexpr int LPR = decltype(L)::value; ... });
// Every call instantiates f for ALL its values; nested calls instantiate the full cross product -- nest only where every combination
// is a kernel that is meant to exist.  Not a public header.
#pragma once
#include <type_traits>

namespace sxe {

template <class F>
decltype(auto) with_bool(bool b, F &&f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the V that equals v; the LAST value also takes every v that matches none
template <int V, int... Vs, class F>
decltype(auto) with_value(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
    else return v == V ? f(std::integral_constant<int, V>{}) : with_value<Vs...>(v, f);
}

// f(LPR) with the lanes per row of a tile width as a compile-time constant.  fp32 kernels, 4 columns per lane: 32 / 16 / 8 columns ->
// 8 / 4 / 2 lanes; bf16 kernels, 8 columns per lane: 64 / 32 / 16 / 8 columns -> 8 / 4 / 2 / 1 lanes
template <class F>
decltype(auto) by_width(int width, F &&f) { return with_value<8, 4, 2>(width / 4, f); }
template <class F>
decltype(auto) by_width_bf16(int width, F &&f) { return with_value<8, 4, 2, 1>(width / 8, f); }

}  // namespace sxe
