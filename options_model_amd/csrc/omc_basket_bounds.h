// omc_basket_bounds.h -- host interface of the multi-asset Andersen-Broadie bound kernels (omc_basket_bounds.hip; DESIGN.md
// section 17): the lower sweep and the inner simulations with d correlated GBM assets per path.  The exercise tables, the
// outer walk and the sums are the single-asset ones (omc_bounds.h) on the INDEX matrix.
#pragma once
#include "omc_basket.h"
#include "omc_bounds.h"

namespace omc {

// BoundsArgs with the basket beside it.  Of `v` the kernels read everything but s0, a, b (the per-asset constants are in
// `law`); v.So is the outer INDEX matrix [N+1][n_outer], which bounds_walk takes as it is.
struct BasketBoundsArgs {
    BoundsArgs v;
    BasketLaw law;     // by value: wave-uniform scalars, as in the generator
    int d;             // assets, 1 .. kBasketMax
    const float* Ao;   // [d][N+1][n_outer] outer asset matrices (launch_basket_paths with `assets`, ld_assets = n_outer)
    const float* Co;   // the Asian kinds: [N+1][n_outer] outer running state (... with `state`); else not read
};

hipError_t basket_bounds_lower(hipStream_t st, const BasketBoundsArgs& a, double* result);
// Q^_t[i] for outer paths [i0, i0 + ni) and t = 0..N-1
hipError_t basket_bounds_inner(hipStream_t st, const BasketBoundsArgs& a, int64_t i0, int64_t ni);
// bounds_check_inner (omc_bounds.h) with d assets: Q^ at the listed items only
hipError_t basket_bounds_check_inner(hipStream_t st, const BasketBoundsArgs& a, const BoundsCheck& k, int64_t i0, int64_t ni);

}  // namespace omc
