// omc_dispatch.h -- a run-time value as a compile-time constant: the one way a host launcher picks a kernel's template
// arguments.  Every helper calls f with a std::integral_constant / std::bool_constant and returns what f returns; nested,
// they spell a kernel's whole selection:
//   for_vec4(v4, [&](auto vec) { for_put(is_put, [&](auto put) { launch kernel<vec(), put()> }); });
// A helper instantiates f for EVERY value it lists, so a launcher must use the one that lists exactly the instantiations its
// kernel is meant to have (a kernel built for widths 4 and 1 takes for_vec4, never for_vec).
#pragma once
#include <type_traits>

namespace omc {

// one of the listed ints; a value that is not listed takes the LAST one
template <int V, int... Rest, class F>
inline auto for_int(int v, F&& f)
{
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
    else if (v == V) return f(std::integral_constant<int, V>{});
    else return for_int<Rest...>(v, f);
}

template <class F>
inline auto for_flag(bool on, F&& f)
{
    if (on) return f(std::bool_constant<true>{});
    else return f(std::bool_constant<false>{});
}

// the payoff side, as the kernels' PUT argument: 1 put, 0 call
template <class F>
inline auto for_put(int is_put, F&& f)
{
    return for_int<1, 0>(is_put ? 1 : 0, f);
}

// columns (or pairs) per thread: 4, 2 or 1 -- and 4 or 1 for the kernels that have no 8-byte form
template <class F>
inline auto for_vec(int vec, F&& f)
{
    return for_int<4, 2, 1>(vec, f);
}
template <class F>
inline auto for_vec4(bool v4, F&& f)
{
    return for_int<4, 1>(v4 ? 4 : 1, f);
}

// the path model: 0 GBM, 1 / 2 / 3 / 4 Heston scheme 0 / 1 / 2 / 3 (the entry points refuse every other scheme before a launcher
// is reached)
template <class F>
inline auto for_model(int model, int scheme, F&& f)
{
    return for_int<0, 1, 2, 3, 4>(model == 0 ? 0 : scheme == 0 ? 1 : scheme == 1 ? 2 : scheme == 2 ? 3 : 4, f);
}

// a Heston scheme alone: 0 .. 3
template <class F>
inline auto for_scheme(int scheme, F&& f)
{
    return for_int<0, 1, 2, 3>(scheme, f);
}

}  // namespace omc
