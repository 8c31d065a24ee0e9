// omc_greeks.h -- host interface of the pathwise-Greeks sweep (omc_greeks.hip) of the two-pass flow.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace omc {

// Sums the Greeks sweep leaves in its result buffer (kGreeksQ doubles, float64, fixed order):
//   0 cf  1 cf^2  2 n_exercised  3 n_zero  4 sum_nitm (from gmom; 0 when gmom is null)  5 price_up  6 price_down  7 -
//   8 delta  9 delta^2  10 gamma  11 gamma^2  12 vega  13 vega^2  14 rho  15 rho^2
//   16 theta  17 theta^2  18 n_exercised_up  19 n_exercised_down  20..23 -
constexpr int kGreeksQ = 24;

struct GreeksArgs {
    const float* S;      // [N+1][ld]: the full matrix, or the first partner of every pair when cK is set
    int64_t ld, cols;    // cols = columns swept (paths, or stored pairs when folded)
    int N, is_put, gbm;  // gbm: form vega / rho / theta (the spot -> Brownian map exists)
    double K, S0, r, sigma, T, h;
    const double* D;      // [N+1] exp(-r dt k)
    const double* betas;  // [N+1][4] b0, b1, b2, n: frozen fits (n > 0.5 fits, as omc_lsm_apply_frozen)
    const double* cK;     // folded storage: [N+1] C_t / K (omc_lsm_dev.h); null = full storage
    const double* gmom;   // [N+1][8] moment table whose row sizes give sum_nitm; null = 0
    double* part;         // [kGreeksQ][greeks_blocks(..)] per-workgroup partials
    double* result;       // [kGreeksQ]
};

// workgroups of the sweep (one thread per `greeks_vec(..)` columns, no grid-stride loop) and its column width
int greeks_vec(const GreeksArgs& a);
int64_t greeks_blocks(const GreeksArgs& a);
// the sweep (events around it when given) + its finalize: sums -> a.result
hipError_t lsm_greeks(hipStream_t st, const GreeksArgs& a, hipEvent_t ev_begin, hipEvent_t ev_end);

}  // namespace omc
