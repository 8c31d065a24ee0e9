// omc_jump_bounds.h -- host interface of the jump-diffusion bound kernels and of the jump generator that keeps the
// variance (omc_jump_bounds.hip): Merton (GBM) and Bates (Heston scheme 0 / 1).
#pragma once
#include "omc_bounds.h"
#include "omc_jump.h"

namespace omc {

// the law of a jump-diffusion bounds call as the host knows it: the diffusion at the compensated drift rate
// (r - q) - lambda kappa_J, so every spot is the jump generator's, and the jumps
struct JumpBoundsLaw {
    DiffusionLaw d;
    JumpLaw law;
};

// launch_jump_paths' S (one pair per thread) with the variance state V [n_steps+1][ld] beside it, as
// launch_heston_paths_sv stores it; a.paths.model = 1, scheme 0 .. 3
hipError_t launch_jump_paths_sv(hipStream_t st, const JumpGen& a, float* V);

// bounds_lower / bounds_inner / bounds_sched_inner / bounds_check_inner (omc_bounds.h) under the jump law; a model or a
// scheme that has no kernels is hipErrorInvalidValue
hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, double* result);
hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, int64_t i0, int64_t ni);
hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, const BoundsSched& sc, int64_t i0,
                              int64_t ni);
hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, const BoundsCheck& k, int64_t i0,
                              int64_t ni);

}  // namespace omc
