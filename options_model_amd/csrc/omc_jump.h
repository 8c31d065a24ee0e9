// omc_jump.h -- host interface of the jump-diffusion path generator (omc_jump.hip): Merton (GBM) and Bates (Heston)
// paths with compound-Poisson lognormal jumps, priced on the path matrix itself.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omc_kernels.h"

namespace omc {

constexpr int kJumpThr = 16;  // thresholds of the Poisson inversion: a step carries 0 .. 16 jumps

// What the kernel needs of the jump law, by value in its argument block (wave-uniform: scalar registers).
//   thr   the count of a step is #{k : w >= thr[k]}, w = the top 24 bits of the step's count word (omc_jump_table)
//   mj2   (float)(mu_j log2 e), sj2 = (float)(sigma_j log2 e): the log2 jump is fmaf(sqrtf(n) sj2, z_J, n mj2)
struct JumpLaw {
    uint32_t thr[kJumpThr];
    float mj2, sj2;
};

struct JumpGen {
    PathSpec paths;  // r is the DRIFT rate (r - q) - lambda kappa; S = the matrix [N+1][ld], full storage
    JumpLaw law;
};

// the generator: rows 0 .. N of both partners of every pair
hipError_t launch_jump_paths(hipStream_t st, const JumpGen& a);

}  // namespace omc
