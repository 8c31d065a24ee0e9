// omc_jump_greeks.h -- host interface of the frozen-policy Greeks sweep under jump-diffusion (omc_jump_greeks.hip,
// DESIGN.md section 34).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omc_greeks.h"
#include "omc_jump.h"
#include "omc_kernels.h"

namespace omc {

// Sums the sweep leaves in its result buffer: omc_greeks.h's kGreeksQ doubles in its order, with
//   20 epsilon  21 epsilon^2  22 n_jumps (every pair's whole-path count, once per pair)
// and a fourth group of eight
//   24 dlambda  25 dlambda^2  26 dmu_j  27 dmu_j^2  28 dsigma_j  29 dsigma_j^2  30 theta_score  31 theta_score^2
constexpr int kJumpGreeksQ = kGreeksQ + 8;

struct JumpGreeksArgs {
    PathSpec paths;       // the generator's own spec (r is the DRIFT rate (r - q) - lambda kappa); S / ld / vec_hint unused
    JumpLaw law;
    int is_put;
    double K, r, h;       // r: the discount rate; h: the relative bump of S0
    double lambda, sigma_j, kappa;
    const double* D;      // [N+1] exp(-r dt k)
    const double* betas;  // [N+1][4] b0, b1, b2, n: frozen fits (n > 0.5 fits, as omc_lsm_apply_frozen)
    const double* gmom;   // [N+1][8] moment table whose row sizes give sum_nitm; null = 0
    double* part;         // [kJumpGreeksQ][jump_greeks_blocks(..)] per-workgroup partials
    double* result;       // [kJumpGreeksQ]
};

// workgroups of the sweep: one lane per antithetic pair, no grid-stride loop
int64_t jump_greeks_blocks(int64_t n_paths);
// the sweep (events around it when given) + its finalize: sums -> a.result
hipError_t jump_greeks(hipStream_t st, const JumpGreeksArgs& a, hipEvent_t ev_begin, hipEvent_t ev_end);

}  // namespace omc
