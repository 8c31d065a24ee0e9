// omc_basket.h -- host interface of the multi-asset path generator (omc_basket.hip): d correlated GBM assets simulated in
// registers, the index of a basket / best-of / worst-of option stored as the path matrix the two-pass sweeps price
// (DESIGN.md section 16).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omc_dispatch.h"
#include "omc_kernels.h"

#include "../../include/omc.h"

namespace omc {

constexpr int kBasketMax = 8;                                  // assets at most
constexpr int kBasketTri = kBasketMax * (kBasketMax + 1) / 2;  // entries of the packed lower triangle

// the asset count as a compile-time constant: the one list of the counts the kernels are built for (callers check the range)
template <class F>
inline auto for_assets(int d, F&& f)
{
    static_assert(kBasketMax == 8, "one instantiation per asset count");
    return for_int<1, 2, 3, 4, 5, 6, 7, 8>(d, f);
}

// What the kernel needs of the basket, by value in its argument block (wave-uniform: scalar registers; no device table).
//   a, b    per asset: the exponent of a step is fmaf(b y, a)  (include/omc.h)
//   w, s0   (float)weight, (float)spot
//   L       (float) lower Cholesky factor of the correlation matrix, packed: row i at i (i + 1) / 2
//   g0      (float)prod S0_i^w_i, the geometric index of the initial spots
//   kind    OMC_BASKET_*
struct BasketLaw {
    float a[kBasketMax], b[kBasketMax], w[kBasketMax], s0[kBasketMax];
    float L[kBasketTri];
    float g0;
    int kind;
};

struct BasketGen {
    // geometry, Philox coordinates, vec_hint (pairs per thread at most, option "gbm_vec") and S = the index matrix
    // [N+1][ld], full storage; its single-asset model fields are not read: the assets are in `law`
    PathSpec paths;
    int d;              // assets, 1 .. kBasketMax
    BasketLaw law;
    float* assets;      // device, or null: the asset matrices [d][N+1][ld_assets]
    int64_t ld_assets;
    float* state;       // device, or null (read with `assets` only): the running state c_t / l_t of the Asian kinds,
                        // [N+1][ld_assets], row 0 = 0 -- what an inner path of the bounds starts from
};

// the running-average kinds: an index rule with a state of its own beside the asset spots
constexpr bool basket_kind_is_asian(int kind) { return kind == OMC_BASKET_ASIAN_ARITHMETIC || kind == OMC_BASKET_ASIAN_GEOMETRIC; }

// pairs per thread an instantiation for d assets holds at most (so that none spills: DESIGN.md 16.3)
constexpr int basket_vec_cap(int d) { return d <= 2 ? 4 : d <= 4 ? 2 : 1; }

// the generator: rows 0 .. N of both partners of every pair
hipError_t launch_basket_paths(hipStream_t st, const BasketGen& a);

}  // namespace omc
