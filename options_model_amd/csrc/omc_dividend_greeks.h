// omc_dividend_greeks.h -- host interface of the frozen-policy Greeks sweep for a stock that pays discrete dividends
// (omc_dividend_greeks.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omc_dividend.h"
#include "omc_greeks.h"
#include "omc_kernels.h"

namespace omc {

// Sums the sweep leaves in its result buffer: omc_greeks.h's kGreeksQ doubles in its order, with the two free slots
//   20 epsilon  21 epsilon^2
struct DivGreeksArgs {
    PathSpec paths;       // the generator's own spec (r is the DRIFT rate r - q); S / ld / vec_hint are not used
    const DivEntry* tab;  // device: the dividend steps in step order + the closing entry
    int is_put;
    double K, r, q, h;    // r: the discount rate; h: the relative bump of S0
    const double* D;      // [N+1] exp(-r dt k)
    const double* betas;  // [N+1][4] b0, b1, b2, n: frozen fits (n > 0.5 fits, as omc_lsm_apply_frozen)
    const double* gmom;   // [N+1][8] moment table whose row sizes give sum_nitm; null = 0
    double* part;         // [kGreeksQ][dividend_greeks_blocks(..)] per-workgroup partials
    double* result;       // [kGreeksQ]
};

// workgroups of the sweep: one lane per antithetic pair, no grid-stride loop
int64_t dividend_greeks_blocks(int64_t n_paths);
// the sweep (events around it when given) + its finalize: sums -> a.result
hipError_t dividend_greeks(hipStream_t st, const DivGreeksArgs& a, hipEvent_t ev_begin, hipEvent_t ev_end);

}  // namespace omc
