// omc_heston_bounds.h -- host interface of the Heston bound kernels and of the generator that keeps the variance
// (omc_heston_bounds.hip).
#pragma once
#include "omc_bounds.h"
#include "omc_kernels.h"

namespace omc {

// omc_heston_paths_f32's S [n_steps+1][ld] with the variance state V [n_steps+1][ld] beside it: row 0 = (float)v0, row t
// = the state heston_pair_step<SCHEME> leaves after step t (scheme 0 .. 3); s.model = 1.  One pair per thread.
hipError_t launch_heston_paths_sv(hipStream_t st, const PathSpec& s, float* V);

// bounds_lower / bounds_inner / bounds_sched_inner / bounds_check_inner (omc_bounds.h) under the Heston path law: h.model =
// 1 with scheme 0 or 1, h.Vo the variance state of the outer paths (launch_heston_paths_sv at stream_outer); anything else is
// hipErrorInvalidValue
hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, double* result);
hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, int64_t i0, int64_t ni);
hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, const BoundsSched& sc, int64_t i0,
                              int64_t ni);
hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, const BoundsCheck& k, int64_t i0,
                              int64_t ni);

}  // namespace omc
