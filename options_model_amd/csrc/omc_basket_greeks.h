// omc_basket_greeks.h -- host interface of the frozen-policy pathwise Greeks of the multi-asset options
// (omc_basket_greeks.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omc_basket.h"

namespace omc {

// Sums the sweep leaves in its result buffer, float64, in groups of 8 (one block reduction each):
//   group 0              0 cf  1 cf^2  2 n_exercised  3 n_zero  4 rho  5 rho^2  6 theta  7 theta^2
//   group 1 + i          asset i: 0 delta  1 delta^2  2 vega  3 vega^2  4 gamma  5 gamma^2  6 price_up  7 price_down
//   groups 1 + d ..      slot 2 i + e of them: asset i's n_exercised_up (e = 0) / n_exercised_down (e = 1)
// 10 d + 8 sums, padded to whole groups with zeros.  Without gamma the gamma, price and scenario-count sums are zeros.
constexpr int basket_greeks_groups(int d) { return 1 + d + (2 * d + 7) / 8; }
constexpr int kBasketGreeksMaxQ = 8 * basket_greeks_groups(kBasketMax);

struct BasketGreeksArgs {
    int64_t P;  // antithetic pairs: one lane each
    int N, d, is_put, want_gamma;
    uint32_t k0, k1, stream;  // the generator's Philox coordinates
    uint64_t pair_offset;
    double K, invK, r, T, h, lup, ldn;  // lup = 1 + h, ldn = 1 - h
    // per asset, float64: spot, volatility, yield; hw = h (double)wf_i (the arithmetic scenario's step), cup / cdn =
    // pow(1 +- h, (double)wf_i) (the geometric scenario's factor)
    double S0[kBasketMax], sigma[kBasketMax], q[kBasketMax], hw[kBasketMax], cup[kBasketMax], cdn[kBasketMax];
    const double* D;      // [N+1] exp(-r dt k)
    const double* betas;  // [N+1][4] b0, b1, b2, n: frozen fits (n > 0.5 fits)
    double* part;         // [8 groups][basket_greeks_blocks(P)] per-workgroup partials
    double* result;       // [8 groups]
};

inline int64_t basket_greeks_blocks(int64_t P) { return (P + 255) / 256; }
// the sweep (events around it when given) + its finalize: sums -> a.result
hipError_t basket_greeks(hipStream_t st, const BasketGreeksArgs& a, const BasketLaw& law, hipEvent_t ev_begin,
                         hipEvent_t ev_end);

}  // namespace omc
