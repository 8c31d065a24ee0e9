// omc_barrier.h -- host interface of the barrier path generator (omc_barrier.hip): knock-in / knock-out options priced
// on the path matrix itself.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omc_kernels.h"

namespace omc {

// Sums the generator leaves in its result buffer (kBarrierQ doubles, float64, fixed order), over both partners of
// every pair, payoffs discounted by exp(-r T) and taken from the REAL terminal spot:
//   0 knock-out payoff  1 its square  2 knock-in payoff  3 its square  4 partners that hit  5..7 -
constexpr int kBarrierQ = 8;

struct BarrierGen {
    // S = the encoded matrix [N+1][ld] (null: sums only, nothing stored); vec_hint is not read (barrier_vec)
    PathSpec paths;
    // the contract
    int is_put, up, knock_in, continuous;
    double K, H;
    // outputs: part = per-workgroup partials [kBarrierQ][barrier_blocks(..)], result = kBarrierQ doubles
    double* part;
    double* result;
};

// the float32 value stored where the option is not live: itm_threshold(K, is_put) (omc_lsm_dev.h), the float32 nearest
// to K on its out-of-the-money side -- payoff <= 0, fails the in-the-money test, u = s / K - 1 ~ 0
float barrier_dead_spot(double K, int is_put);
// the float32 knock threshold: down barriers hit iff s <= thr (thr the largest float32 with (double)thr <= H), up
// barriers iff s >= thr (the smallest float32 with (double)thr >= H) -- the float64 tests (double)s <= H / >= H
float barrier_threshold(double H, int up);
// workgroups of the generator (one thread per barrier_vec(..) pairs, no grid-stride loop)
int barrier_vec(const BarrierGen& a);
int64_t barrier_blocks(const BarrierGen& a);
// the generator (STORE when a.S is set) + its finalize: sums -> a.result
hipError_t launch_barrier_paths(hipStream_t st, const BarrierGen& a);

}  // namespace omc
