// omc_heston_bounds.h -- host interface of the Heston bound kernels and of the generator that keeps the variance
// (omc_heston_bounds.hip).
#pragma once
#include "omc_bounds.h"

namespace omc {

// the Heston law of a bounds call as the host knows it; the launchers turn it into the generator's float32 constants
// (make_heston), so every spot is the generator's
struct HestonBoundsLaw {
    double r, T, v0, kappa, theta, xi, rho;
    int scheme;       // 0 reference clamp, 1 full truncation
    const float* Vo;  // [N+1][n_outer] the variance state of the outer paths (launch_heston_paths_sv at stream_outer)
};

// omc_heston_paths_f32's S [n_steps+1][ld] with the variance state V [n_steps+1][ld] beside it: row 0 = (float)v0, row t
// = the state heston_pair_step<SCHEME> leaves after step t (scheme 0, 1, 2).  One pair per thread.
hipError_t launch_heston_paths_sv(hipStream_t st, float* S, float* V, int64_t ld, int64_t n_paths, int n_steps, double S0,
                                  double r, double T, double v0, double kappa, double theta, double xi, double rho,
                                  uint64_t seed, uint32_t stream, uint64_t pair_offset, int scheme);

// bounds_lower / bounds_inner (omc_bounds.h) under the Heston path law; scheme 0 or 1, anything else is hipErrorInvalidValue
hipError_t heston_bounds_lower(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, double* result);
hipError_t heston_bounds_inner(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, int64_t i0, int64_t ni);
// bounds_sched_inner (omc_bounds.h) under the Heston path law: Q^ at the scheduled dates only
hipError_t heston_bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, const BoundsSched& sc,
                                     int64_t i0, int64_t ni);
// bounds_check_inner (omc_bounds.h) under the Heston path law: Q^ at the listed items only
hipError_t heston_bounds_check_inner(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, const BoundsCheck& k,
                                     int64_t i0, int64_t ni);

}  // namespace omc
