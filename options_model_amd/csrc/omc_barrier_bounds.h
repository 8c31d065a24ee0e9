// omc_barrier_bounds.h -- host interface of the barrier-law bound kernels and of the barrier generator that keeps the outer
// state (omc_barrier_bounds.hip): knock-in / knock-out options, discrete monitoring, on GBM and Heston
// scheme 0 / 1.
#pragma once
#include "omc_barrier.h"
#include "omc_bounds.h"

namespace omc {

// the contract as the kernels take it: a partner is hit at a step iff sg * s <= sthr (down: 1, thr; up: -1, -thr, thr the
// float32 threshold of barrier_threshold), and what is not live shows the policy `dead` (barrier_dead_spot)
struct BarrierTest {
    float sg, sthr, dead;
    int knock_out;  // 1: dead at the hit step and after it; 0 (knock-in): live from the hit step on
};
BarrierTest barrier_test(double K, int is_put, double H, int up, int knock_in);

// The generator that keeps the state of the outer paths (one pair per thread; paths.model 0, or 1 with scheme 0 / 1):
//   paths.S  the ENCODED matrix [N+1][ld], launch_barrier_paths' bits
//   Sr       the real spots [N+1][ld], the vanilla generator's bits
//   V        Heston: the variance state [N+1][ld] as launch_heston_paths_sv stores it (GBM: null)
//   hit      [n_paths] the first step at which the path is hit, 0 = never; start_hit != 0: the paths start hit, every
//            entry is -1 and row 0 is encoded as hit.  hit(t, i) is hit[i] != 0 && hit[i] <= t either way.
struct BarrierStateGen {
    PathSpec paths;
    BarrierTest test;
    int start_hit;
    float* Sr;
    float* V;
    int32_t* hit;
};
hipError_t launch_barrier_paths_state(hipStream_t st, const BarrierStateGen& a);

// the law of a barrier bounds call as the host knows it: the diffusion, the contract and the outer paths' state beside
// the encoded matrix BoundsArgs::So (which the walk and the keep mask read)
struct BarrierBoundsLaw {
    DiffusionLaw d;      // d.Vo: the outer variance state (Heston)
    BarrierTest test;
    const float* Sr;     // device [N+1][n_outer]: the outer paths' real spots
    const int32_t* hit;  // device [n_outer]: their first-hit steps
    int every;           // the schedule's k (BoundsSched::k) when the game has one, else 0: the lower sweep's exercise dates
};

// bounds_lower / bounds_inner / bounds_sched_inner / bounds_check_inner (omc_bounds.h) under the barrier law; a model or a
// scheme that has no kernels is hipErrorInvalidValue
hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, double* result);
hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, int64_t i0, int64_t ni);
hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, const BoundsSched& sc, int64_t i0,
                              int64_t ni);
hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, const BoundsCheck& k, int64_t i0,
                              int64_t ni);
// bounds_check_mark's keep mask and per-date counts with the rule "kept unless the knock-out is dead at (i, t)" (k.mode 0):
// the list-driven sweep then simulates the live items alone, a dead item's Q^ stays the 0.0 the flow cleared it to
hipError_t barrier_bounds_mark(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, const BoundsCheck& k);

}  // namespace omc
