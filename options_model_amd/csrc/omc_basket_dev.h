// omc_basket_dev.h -- the device arithmetic of D correlated GBM assets, for the generator (omc_basket.hip) and the bound
// kernels (omc_basket_bounds.hip; DESIGN.md sections 16.1 and 17.1): the correlated normals of a Philox block, the step of
// both partners of an antithetic pair, the index of a path.  D is a template parameter and BasketLaw comes by value, so
// every loop over assets unrolls and every index of the constants is a compile-time one.
#pragma once
#include "omc_basket.h"
#include "omc_device.h"

#include "../../include/omc.h"

namespace omc {

// asset k's raw normals z of one Philox block join the correlated normals y[i][j] (asset i, step j of the block) of the
// assets i >= k: y_i = sum_{k <= i} Lf[i][k] z_k.  Called with k ascending -- the order include/omc.h fixes
template <int D>
__device__ __forceinline__ void basket_correlate(const BasketLaw& c, int k, const float (&z)[4], float (&y)[D][4])
{
#pragma unroll
    for (int i = k; i < D; ++i) {
        const float l = c.L[i * (i + 1) / 2 + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i == 0) y[i][j] = z[j];  // Lf[0][0] = 1.0f exactly
            else if (k == 0) y[i][j] = l * z[j];
            else y[i][j] = __builtin_fmaf(l, z[j], y[i][j]);
        }
    }
}

// the correlated normals of one pair's Philox block `blk`: asset k draws at the pair index pair + (k << 40)
template <int D>
__device__ __forceinline__ void basket_normals(const BasketLaw& c, uint64_t pair, uint32_t blk, uint32_t stream, uint32_t k0,
                                               uint32_t k1, float (&y)[D][4])
{
#pragma unroll
    for (int k = 0; k < D; ++k) {
        float z[4];
        normals4(pair + ((uint64_t)k << 40), blk, stream, k0, k1, z);
        basket_correlate<D>(c, k, z, y);
    }
}

// one step of both partners' assets with the block's normals of step u
template <int D>
__device__ __forceinline__ void basket_step(const BasketLaw& c, float (&sa)[D], float (&sb)[D], const float (&y)[D][4], int u)
{
#pragma unroll
    for (int k = 0; k < D; ++k) {
        sa[k] = sa[k] * fast_exp2(__builtin_fmaf(c.b[k], y[k][u], c.a[k]));
        sb[k] = sb[k] * fast_exp2(__builtin_fmaf(-c.b[k], y[k][u], c.a[k]));
    }
}

// the index of one path from its asset spots (KIND arithmetic, best-of or worst-of; the geometric kind has its own state)
template <int KIND, int D>
__device__ __forceinline__ float basket_index(const BasketLaw& c, const float (&s)[D])
{
    float x = c.w[0] * s[0];
#pragma unroll
    for (int k = 1; k < D; ++k) {
        if constexpr (KIND == OMC_BASKET_ARITHMETIC) x = __builtin_fmaf(c.w[k], s[k], x);
        else if constexpr (KIND == OMC_BASKET_BEST_OF) x = fmaxf(x, c.w[k] * s[k]);
        else x = fminf(x, c.w[k] * s[k]);
    }
    return x;
}

// the running sum of the Asian kinds (section 23): ONE float32 add.  With one asset B is a bare product, which the compiler
// would otherwise contract into the sum -- and the documented rule, restated in numpy by the tests, has two roundings
__device__ __forceinline__ float asian_add(float c, float B)
{
#pragma clang fp contract(off)
    return c + B;
}

// ... of the law's own kind (wave-uniform: a scalar branch)
template <int D>
__device__ __forceinline__ float basket_law_index(const BasketLaw& c, const float (&s)[D])
{
    if (c.kind == OMC_BASKET_ARITHMETIC) return basket_index<OMC_BASKET_ARITHMETIC, D>(c, s);
    if (c.kind == OMC_BASKET_BEST_OF) return basket_index<OMC_BASKET_BEST_OF, D>(c, s);
    return basket_index<OMC_BASKET_WORST_OF, D>(c, s);
}

}  // namespace omc
