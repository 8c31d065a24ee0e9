// omc_runnerup_bounds.h -- host interface of the bound kernels whose policy sees the index AND the runner-up of d correlated
// GBM assets (omc_runnerup_bounds.hip; the definitions are include/omc.h's).
#pragma once
#include "omc_basket_bounds.h"

namespace omc {

constexpr int kRunnerupCols = 8;        // doubles per date of the policy table: c0 .. c5, n, 0
constexpr int kRunnerupSums = 27;       // n, sum f [5], sum f f' [15, upper triangle by rows], sum y, sum f y [5]
constexpr int kRunnerupSlots = 32;      // ... reduced in four groups of eight
constexpr int kRunnerupFitBlocks = 256; // workgroups of a fit launch at most = partials per sum
constexpr int kRunnerupMaxSteps = 512;  // dates whose policy rows (64 bytes each) share the LDS with the lower sweep's sums

// for_assets for the kernels of this file: a runner-up needs two assets, so no instantiation for one is built (callers check
// the range)
template <class F>
inline auto for_runnerup_assets(int d, F&& f)
{
    static_assert(kBasketMax == 8, "one instantiation per asset count");
    return for_int<2, 3, 4, 5, 6, 7, 8>(d, f);
}

// BasketBoundsArgs with the two-regressor policy beside it.  Of g.v the kernels read neither betas nor tab.
struct RunnerupArgs {
    BasketBoundsArgs g;
    const double* pol;  // [N+1][8] device
};

// the Longstaff-Schwartz fit on the generator's paths: asset matrices in, policy rows 1 .. N-1 out
struct RunnerupFit {
    BasketLaw law;      // by value
    int d;              // assets, 2 .. kBasketMax
    const float* A;     // [d][N+1][ld] asset matrices of the fitting paths
    int64_t ld, M;
    int N, is_put;
    double K, invK;
    const double* D;    // [N+1] exp(-r dt k)
    float* x_ex;        // [M] the index at the path's exercise date
    int32_t* tex;       // [M] that date
    double* part;       // [kRunnerupSlots][kRunnerupFitBlocks] per-workgroup partial sums of one date
    double* pol;        // [N+1][8]: rows 0 and N cleared, rows N-1 .. 1 fitted
};

hipError_t runnerup_fit(hipStream_t st, const RunnerupFit& f);
// the one-workgroup solve of a date on its own, for a fit whose sums kernel is another file's (omc_heston_sv_bounds.hip): the
// partial sums part [kRunnerupSlots][kRunnerupFitBlocks] of nblk workgroups -> the policy row (c0 .. c5, n, 0)
hipError_t runnerup_fit_solve(hipStream_t st, const double* part, int nblk, double* row);
hipError_t runnerup_lower(hipStream_t st, const RunnerupArgs& a, double* result);
// Q^_t[i] for outer paths [i0, i0 + ni) and t = 0..N-1
hipError_t runnerup_inner(hipStream_t st, const RunnerupArgs& a, int64_t i0, int64_t ni);
hipError_t runnerup_walk(hipStream_t st, const RunnerupArgs& a, double* result);

}  // namespace omc
