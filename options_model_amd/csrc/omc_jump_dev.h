// omc_jump_dev.h -- device code the jump generator (omc_jump.hip) and the jump-diffusion bound kernels
// (omc_jump_bounds.hip) share: the size of a step's jump (include/omc.h, "jump-diffusion").
#pragma once
#include "omc_jump.h"
#include "omc_paths_dev.h"

namespace omc {

// the log2 jump of a step whose count word already passed thr[0]
__device__ __forceinline__ float jump_log2(const JumpLaw& j, uint32_t w, uint64_t pair, int t, uint32_t stream,
                                           uint32_t k0, uint32_t k1)
{
    int n = 1;
#pragma unroll
    for (int k = 1; k < kJumpThr; ++k) n += w >= j.thr[k] ? 1 : 0;
    const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0xC0000000u | (uint32_t)t, stream, k0, k1);
    float zc, zs;
    box_muller(o.x, o.y, zc, zs);
    const float fn = (float)n;
    return __builtin_fmaf(sqrtf(fn) * j.sj2, zc, fn * j.mj2);
}

}  // namespace omc
