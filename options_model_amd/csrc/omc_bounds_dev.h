// omc_bounds_dev.h -- device helpers the bound kernels share (omc_bounds.hip, omc_basket_bounds.hip; DESIGN.md sections 12
// and 17): the stopping rule from the exercise tables, the discounted payoff, the tables' LDS copy, the wave sum.
#pragma once
#include "omc_bounds.h"
#include "omc_lsm_dev.h"

namespace omc {

// does a path at spot s stop at date d?  iv = the date's table (lo0, lo1, len0, len1); an irregular date decides with
// the float64 rule of omc_lsm_apply_frozen
__device__ __forceinline__ bool bd_stop(float s, int d, uint4 iv, const BoundsArgs& a)
{
    if (d >= a.N) return true;
    if (iv.x == kCritIrregular) return exercises(pay_stored(s, a.K, a.invK, a.is_put), fit_given(a.betas, d, a.N));
    return crit_in(iv, __float_as_uint(s));
}

__device__ __forceinline__ double bd_value(float s, int d, const BoundsArgs& a)
{
    const double p = payoff_d(s, a.K, a.is_put);
    return a.D[d] * (p > 0.0 ? p : 0.0);
}

// the stored-path tables [N+1][8] -> LDS [N+1][4]
__device__ __forceinline__ void bd_load_tables(const BoundsArgs& a, uint4* sh)
{
    for (int t = threadIdx.x; t <= a.N; t += blockDim.x) sh[t] = *reinterpret_cast<const uint4*>(a.tab + (size_t)t * 8);
    __syncthreads();
}

__device__ __forceinline__ double wave_sum_f64(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

}  // namespace omc
